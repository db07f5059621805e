"""Child process of tests/test_gpu_event_terms_encoded_train.py (a GPU fault
must not take the test runner down): two optimizer steps of ``training.train``
with Ranger at accumulation 2 on compact event batches (9 B/event, straight
from ``encoding.compact_events``), the contrast term on every scale with three
references and the polarities apart plus the average-timestamp term -- eagerly,
with ``capture=True, capture_event_terms=True``, and that through
``feed.DeviceFeeder`` -- and prints one JSON line.

6000 events per sample: the voxeliser takes its tiled, order-independent path,
so every kernel of the step is reproducible bit for bit."""
import contextlib
import io
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from dvs_of_training_framework_amd import encoding, synthetic, voxel  # noqa: E402
from tests.event_terms_capture_child import B, H, W, WEIGHTS, OURS, _family, _same, build, parse  # noqa: E402

PER_SAMPLE = 6000
STEPS, ACCUM = 2, 2
OPTS = {'contrast_weight': 0.25, 'contrast_scales': 'all', 'contrast_references': ('start', 'middle', 'end'),
        'contrast_polarity': True, 'avg_timestamp_weight': 0.5}


def compact_batch(seed):
    """synthetic.make_batch through encoding.encode_batch and encoding.compact_events: host tensors."""
    wire = synthetic.to_torch(synthetic.make_batch(seed, B, H, W, PER_SAMPLE))
    enc = encoding.encode_batch(wire['events'], wire['timestamps'], wire['sample_idx'], wire['images'], {}, B)
    events = encoding.compact_events(enc)
    assert voxel.is_compact(events) and events['x'].dtype == torch.short and events['polarity'].dtype == torch.bool
    assert 'sample_index' not in events and events['sample_event_offsets'].tolist() == [0, PER_SAMPLE, 2 * PER_SAMPLE]
    return {'events': events, 'timestamps': wire['timestamps'], 'sample_idx': wire['sample_idx'],
            'images': wire['images'], 'size': B}


def run_loop(args, data, seed, capture, feeder):
    from dvs_of_training_framework_amd import capture as cap_mod, feed
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import train
    model, optimizer, scheduler, ev = build(args, seed)
    rows = []
    info = {'replays': 0, 'roles': [], 'unheld': 0, 'ours_foreign': [], 'encoded_nodes': 0, 'wire_nodes': 0,
            'failed': None, 'recaptures': 0, 'loops': 0, 'bound': 0}

    class Log:
        def add_scalar(self, tag, value, x):
            rows.append((tag, float(value), x))
    orig_close = cap_mod.CapturedLoop.close

    def spy(self):
        torch.cuda.synchronize()
        info['loops'] += 1
        info['bound'] += len(self.bound)
        for key, step in list(self.steps.items()) + list(self.bound.items()):
            info['roles'].append(key if isinstance(key, str) else key[0])
            info['replays'] += step.replays
            a = step.audit()
            info['unheld'] += len(a['unheld'])
            info['ours_foreign'] += [n for n in a['foreign'] if any(o in n for o in OURS)]
            names = [n[3] for n in step.executor.nodes()]
            terms = [n for n in names if 'contrast_pyramid_' in n or 'avgts_' in n]
            info['encoded_nodes'] += sum('EncodedColumns' in n for n in terms)
            info['wire_nodes'] += sum('WireColumns' in n for n in terms)
        info['failed'] = str(self.failed) if self.failed else None
        info['recaptures'] = self.recaptures
        return orig_close(self)
    cap_mod.CapturedLoop.close = spy
    err = io.StringIO()
    loader = feed.DeviceFeeder(data, 'cuda') if feeder else data
    try:
        with contextlib.redirect_stderr(err):
            train(model, 'cuda', loader, optimizer, args.training_steps, scheduler, Log(), ev, weights=WEIGHTS,
                  timers=FakeTimer(), capture=capture, accumulation_steps=args.accum_step,
                  max_events_per_batch=10 ** 7, **({'capture_event_terms': True} if capture else {}), **OPTS)
    finally:
        cap_mod.CapturedLoop.close = orig_close
    torch.cuda.synchronize()
    return {'rows': rows, 'params': [p.detach().clone() for p in model.parameters()],
            'capture_lines': [ln for ln in err.getvalue().splitlines() if ln.startswith('capture:')],
            'stderr_tail': err.getvalue()[-600:], 'info': info}


def main():
    args = parse('RANGER', STEPS, ACCUM)
    data = [compact_batch(300 + i) for i in range(STEPS * ACCUM)]
    eager = run_loop(args, data, 21, False, False)
    legs = {'captured': run_loop(args, data, 21, True, False), 'fed': run_loop(args, data, 21, True, True),
            'fed_eager': run_loop(args, data, 21, False, True)}
    out = {'n_rows': len(eager['rows']), 'eager_capture_lines': eager['capture_lines']}
    fam = {name: _family(eager['rows'], tag, exact) for name, tag, exact in (
        ('loss', 'General/Train loss', True), ('contrast', 'Train/contrast', True),
        ('levels', 'Train/contrast/', False), ('avg_timestamp', 'Train/avg timestamp', True))}
    out['n'] = {k: len(v) for k, v in fam.items()}
    out['terms_move'] = len({r[1] for r in fam['contrast']}) > 1 and len({r[1] for r in fam['avg_timestamp']}) > 1
    out['finite'] = all(v == v and abs(v) < 1e30 for _, v, _ in eager['rows'])
    for name, leg in legs.items():
        i = leg['info']
        out[name] = {'rows_equal': leg['rows'] == eager['rows'], 'params_equal': _same(leg['params'], eager['params']),
                     'first_diff': next(((a, b) for a, b in zip(eager['rows'], leg['rows']) if a != b), None),
                     'capture_lines': leg['capture_lines'], 'replays': i['replays'], 'roles': sorted(set(i['roles'])),
                     'failed': i['failed'], 'recaptures': i['recaptures'], 'unheld': i['unheld'],
                     'ours_foreign': i['ours_foreign'], 'encoded_nodes': i['encoded_nodes'],
                     'wire_nodes': i['wire_nodes'], 'bound': i['bound'], 'stderr_tail': leg['stderr_tail']}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    os.environ.pop('DVSOF_LOOPBACK', None)
    main()
