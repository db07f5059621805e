"""Child process of tests/test_gpu_event_terms_capture.py (a GPU fault must
not take the test runner down): runs one scenario of the captured step that
carries the events-only terms and prints one JSON line.

  loop:<OPT>:<k>      train(capture=True, capture_event_terms=True) against
                      train(capture=False) of an identical model, 13 optimizer
                      steps of k micro-batches, contrast_weight 0.25
  wide[:<dtype>:<n>]  the widest option set (every scale, three references,
                      polarity, the average-timestamp term with polarity),
                      RANGER, 3 micro-batches per step, n steps (13)
  frameless:<k>       batches without frames through Losses.frameless
  padded              CapturedLoop at capacity 4096: a replay on 3000 events, a
                      re-recording for 5000, another batch size run eagerly
  loopback            the exchange under GradReducer(loopback=(2, 50))
  default             train(capture=True, contrast_weight=0.25) without the
                      keyword: the refusal line, no replay

Batches are ``capture_child.unique_pixel_batch``: one event per pixel and
sample keeps the voxeliser's small-input float atomics from reordering
anything -- the premise of every bitwise capture test, not a property of the
terms, whose sums are integers.
"""
import contextlib
import io
import json
import os
import sys
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from dvs_of_training_framework_amd import synthetic  # noqa: E402
from tests.capture_child import unique_pixel_batch  # noqa: E402

B, H, W, C = 2, 64, 64, 5
PER_SAMPLE = 2048
WEIGHTS = [0.5, 1, 1]
CONTRAST = {'contrast_weight': 0.25}
WIDE = {'contrast_weight': 0.25, 'contrast_scales': 'all',
        'contrast_references': ('start', 'middle', 'end'), 'contrast_polarity': True,
        'avg_timestamp_weight': 0.5, 'avg_timestamp_polarity': True}
# the library's kernels of the terms, by the option set that launches them
KERNELS = {
    'contrast': ('contrast_splat_kernel', 'contrast_close_kernel', 'contrast_bwd_events_kernel',
                 'contrast_bwd_close_kernel'),
    'pyramid': ('contrast_pyramid_splat_kernel', 'contrast_pyramid_close_kernel',
                'contrast_pyramid_bwd_events_kernel', 'contrast_pyramid_bwd_close_kernel'),
    'avg_timestamp': ('avgts_splat_kernel', 'avgts_close_kernel', 'avgts_bwd_events_kernel',
                      'avgts_bwd_close_kernel'),
    'frameless': ('frameless_sweep_kernel',),
}
OURS = ('contrast_', 'avgts_', 'frameless_', 'fill_u32', 'frame_final_kernel')


def frameless(batch):
    out = dict(batch, images=None)
    out['shape'] = (H, W)
    return out


def shares_level_pixels(batch, shift):
    """Per sample: do several events fall on one pixel of the level at ``shift``?"""
    ev = batch['events']
    out = []
    for s in range(int(batch['size'])):
        m = np.asarray(ev['sample_index']) == s
        key = (np.asarray(ev['y'])[m] >> shift) * W + (np.asarray(ev['x'])[m] >> shift)
        out.append(bool(np.unique(key).size < key.size))
    return all(out)


def has_horizontal_neighbours(batch):
    """Per sample: two events on horizontally adjacent pixels (they share splat
    corners for any non-integral flow)."""
    ev = batch['events']
    out = []
    for s in range(int(batch['size'])):
        m = np.asarray(ev['sample_index']) == s
        x, y = np.asarray(ev['x'])[m], np.asarray(ev['y'])[m]
        here = set(zip(y.tolist(), x.tolist()))
        out.append(any((yy, xx + 1) in here for yy, xx in here))
    return all(out)


def parse(opt_name, steps, accum, dtype='f32', lr='1e-2'):
    from dvs_of_training_framework_amd import options
    parser = options.add_train_arguments(ArgumentParser())
    return options.validate_train_args(parser.parse_args(
        ['-m', 'unused', '--flownet_path', 'dvs_of_training_framework_amd',
         '--height', str(H), '--width', str(W), '--event-representation-depth', str(C),
         '-bs', str(B * accum), '-mbs', str(B), '--optimizer', opt_name, '-ne', str(steps),
         '-lr', lr, '--half_life', '8', '--compute-dtype', dtype]))


def build(args, seed, red=None):
    """-> model, optimizer, scheduler, evaluator from one seed."""
    import train_flownet as tf
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.model import init_model
    torch.manual_seed(seed)
    model = init_model(args, torch.device('cuda'))
    model.train()
    model.predictor.reducer = red
    optimizer, scheduler = tf.construct_train_tools(args, model)
    ev = init_losses(args.shape, B, model, 'cuda', sequence_length=1)
    return model, optimizer, scheduler, ev


def run_loop(args, data, seed, capture, opts, red=None, event_terms=True):
    """training.train over ``data`` -> dict of what the comparison needs."""
    from dvs_of_training_framework_amd import capture as cap_mod
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import train
    model, optimizer, scheduler, ev = build(args, seed, red)
    rows = []
    info = {'replays': 0, 'roles': [], 'unheld': 0, 'foreign': [], 'ours_foreign': [], 'kernels': {},
            'marks': None, 'failed': None, 'recaptures': 0, 'loops': 0, 'violations': 0}

    class Log:
        def add_scalar(self, tag, value, x):
            rows.append((tag, float(value), x))
    orig_close = cap_mod.CapturedLoop.close

    def spy(self):
        torch.cuda.synchronize()
        info['loops'] += 1
        for role, step in self.steps.items():
            info['roles'].append(role)
            info['replays'] += step.replays
            a = step.audit()
            info['unheld'] += len(a['unheld'])
            info['foreign'] += [n for n in a['foreign'] if n not in info['foreign']]
            info['ours_foreign'] += [n for n in a['foreign'] if any(o in n for o in OURS)]
            names = [n[3] for n in step.executor.nodes()]
            # per micro-batch (one step is one): how often each kernel of the terms is a node
            # (no name of KERNELS is part of another)
            info['kernels'][role] = {k: sum(k in n for n in names)
                                     for group in KERNELS.values() for k in group}
            info['marks'] = step.executor.marks
            info['violations'] += len(getattr(step, 'exchange_audit', {}).get('violations', []))
        info['failed'] = str(self.failed) if self.failed else None
        info['recaptures'] = self.recaptures
        return orig_close(self)
    cap_mod.CapturedLoop.close = spy
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            train(model, 'cuda', (synthetic.to_torch(b) for b in data), optimizer,
                  args.training_steps, scheduler, Log(), ev, weights=WEIGHTS,
                  timers=FakeTimer(), capture=capture, accumulation_steps=args.accum_step,
                  max_events_per_batch=10 ** 7, reducer=red,
                  **({'capture_event_terms': True} if capture and event_terms else {}), **opts)
    finally:
        cap_mod.CapturedLoop.close = orig_close
    torch.cuda.synchronize()
    return {'rows': rows, 'params': [p.detach().clone() for p in model.parameters()],
            'capture_lines': [ln for ln in err.getvalue().splitlines() if ln.startswith('capture:')],
            'stderr_tail': err.getvalue()[-600:], 'info': info}


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def _family(rows, prefix, exact=False):
    return [r for r in rows if (r[0] == prefix if exact else r[0].startswith(prefix))]


def compare(args, data, opts, seed=21, red=None):
    eager = run_loop(args, data, seed, False, opts, red)
    cap = run_loop(args, data, seed, True, opts, red)
    i = cap['info']
    e_rows, c_rows = eager['rows'], cap['rows']
    fam = {name: (_family(e_rows, tag, exact), _family(c_rows, tag, exact)) for name, tag, exact in (
        ('loss', 'General/Train loss', True), ('contrast', 'Train/contrast', True),
        ('levels', 'Train/contrast/', False), ('avg_timestamp', 'Train/avg timestamp', True),
        ('photometric', 'Train/photometric loss/', False))}
    return {'rows_equal': e_rows == c_rows, 'n_rows': len(e_rows),
            'n': {k: len(v[0]) for k, v in fam.items()},
            'equal': {k: v[0] == v[1] for k, v in fam.items()},
            'level_tags': sorted({r[0] for r in fam['levels'][1]}),
            'photometric_values': sorted({r[1] for r in fam['photometric'][1]})[:3],
            'contrast_first': fam['contrast'][1][0][1] if fam['contrast'][1] else None,
            'contrast_moves': len({r[1] for r in fam['contrast'][1]}) > 1,
            'params_equal': _same(eager['params'], cap['params']),
            'capture_lines': cap['capture_lines'] + eager['capture_lines'],
            'replays': i['replays'], 'roles': sorted(set(i['roles'])), 'failed': i['failed'],
            'recaptures': i['recaptures'], 'unheld': i['unheld'], 'foreign': i['foreign'],
            'ours_foreign': i['ours_foreign'], 'kernels': i['kernels'], 'marks': i['marks'],
            'violations': i['violations'], 'stderr_tail': cap['stderr_tail'],
            'first_diff': next(((a, b) for a, b in zip(e_rows, c_rows) if a != b), None)}


def scenario_loop(opt_name, accum):
    steps = 13
    args = parse(opt_name, steps, accum)
    data = [unique_pixel_batch(4000 + i, B, H, W, PER_SAMPLE) for i in range(steps * accum)]
    assert all(b['events']['x'].size == B * PER_SAMPLE for b in data)
    out = compare(args, data, CONTRAST)
    out['neighbours'] = all(has_horizontal_neighbours(b) for b in data)
    return out


def scenario_wide(dtype, steps):
    accum = 3
    args = parse('RANGER', steps, accum, dtype)
    data = [unique_pixel_batch(5000 + i, B, H, W, PER_SAMPLE) for i in range(steps * accum)]
    out = compare(args, data, WIDE)
    # 2048 events of a sample on the 32x32 pixels of the level at shift 1: by counting
    out['collisions'] = all(shares_level_pixels(b, 1) for b in data)
    return out


def scenario_frameless(accum):
    steps = 13
    args = parse('RANGER', steps, accum)
    data = [frameless(unique_pixel_batch(6000 + i, B, H, W, PER_SAMPLE)) for i in range(steps * accum)]
    return compare(args, data, CONTRAST)


def scenario_padded():
    """One CapturedLoop in the role ``full`` against the eager steps on the
    same batches: recorded on 4096 events, replayed on 3000 (the padded slots
    leave the splat at its first test, and integer sums have no order), re-
    recorded for 5000, replayed on 4500, another batch size eagerly, a replay."""
    from dvs_of_training_framework_amd import predictor
    from dvs_of_training_framework_amd.capture import CapturedLoop
    from dvs_of_training_framework_amd.loss import unit_backward
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import TermReadback, process_minibatch
    opts = {'contrast_weight': 0.25, 'avg_timestamp_weight': 0.5}
    plan = [(B, 2048), (B, 1500), (B, 2500), (B, 2250), (1, 4000), (B, 1500)]
    data = [unique_pixel_batch(7000 + i, b, H, W, n) for i, (b, n) in enumerate(plan)]
    assert [b['events']['x'].size for b in data] == [4096, 3000, 5000, 4500, 4000, 3000]
    args = parse('ADAM', len(data), 1, lr='1e-4')
    seen = {}
    real = predictor._PredictorFn.backward

    def spy(ctx, *gflows):          # keeps the finest flow's gradient itself: no extra kernel
        seen.setdefault('new', []).append(gflows[-1])
        return real(ctx, *gflows)
    predictor._PredictorFn.backward = staticmethod(spy)

    def finest_gradient():
        """Of the micro-batch just run.  Two backward calls: the eager one of a
        step's constructor, then its recording, whose tensor is what later
        replays write; none: a replay."""
        new = seen.pop('new', [])
        if len(new) == 2:
            seen['recorded'] = new[1]
        return new[0] if new else seen['recorded']

    def record(loss, terms, model):
        torch.cuda.synchronize()
        return {'loss': float(loss.detach()), 'contrast': terms.contrast(), 'avg_timestamp': terms.avg_timestamp(),
                'table': terms.host(), 'g': finest_gradient().detach().clone(),
                'params': [p.detach().clone() for p in model.parameters()]}
    try:
        model, opt, sched, ev = build(args, 31)
        eager = []
        for b in data:
            opt.zero_grad(set_to_none=True)
            loss, terms, _ = process_minibatch(model, synthetic.to_torch(b, 'cuda'), FakeTimer(), 'cuda',
                                               True, ev, WEIGHTS, **opts)
            unit_backward(loss)
            model.strict = False
            opt.step()
            sched.step()
            eager.append(record(loss, terms, model))
        model, opt, sched, ev = build(args, 31)
        loop = CapturedLoop(model, ev, opt, WEIGHTS, 'cuda', 1, None, event_capacity=4096, loss_options=opts)
        cap, trace = [], []
        for b in data:
            before = loop.steps.get('full')
            loss, terms, _ = loop.run(synthetic.to_torch(b), 0)
            sched.step()
            step = loop.steps['full']
            trace.append({'capacity': step.capacity, 'replays': step.replays, 'recaptures': loop.recaptures,
                          'recorded_now': step is not before})
            assert isinstance(terms, TermReadback)
            cap.append(record(loss, terms, model))
        failed = str(loop.failed) if loop.failed else None
        loop.close()
    finally:
        predictor._PredictorFn.backward = staticmethod(real)
    per_step = [{k: (e[k] == c[k] if k not in ('g', 'params') else
                     (torch.equal(e[k], c[k]) if k == 'g' else _same(e[k], c[k])))
                 for k in e} for e, c in zip(eager, cap)]
    return {'per_step': per_step, 'trace': trace, 'failed': failed,
            'eager': [{k: e[k] for k in ('loss', 'contrast', 'avg_timestamp')} for e in eager],
            'captured': [{k: c[k] for k in ('loss', 'contrast', 'avg_timestamp')} for c in cap],
            'g_max': [float(e['g'].abs().max()) for e in eager]}


def scenario_loopback():
    from dvs_of_training_framework_amd import parallel
    from dvs_of_training_framework_amd.capture import CapturedTrainStep
    steps = 5
    data = [unique_pixel_batch(8000 + i, B, H, W, PER_SAMPLE) for i in range(steps)]
    red = parallel.GradReducer(loopback=(2, 50))
    assert red.active() and red.comm_info()['loopback']
    out = {}
    args = parse('ADAM', steps, 1)
    marks = {}
    for name, opts in (('plain', None), ('contrast', CONTRAST), ('wide', WIDE)):
        model, opt, _, ev = build(args, 41, red)
        step = CapturedTrainStep(model, ev, opt, WEIGHTS, 'cuda', synthetic.to_torch(data[0]),
                                 event_capacity=4096, reducer=red, loss_options=opts)
        marks[name] = step.executor.marks
        out['violations_' + name] = len(step.exchange_audit['violations'])
        out['window_kernels_' + name] = step.exchange_audit['window_kernels']
        step.close()
    out['marks'] = marks
    r = compare(args, data, WIDE, seed=51, red=red)
    none = run_loop(args, data, 51, False, WIDE, None)
    with_red = run_loop(args, data, 51, False, WIDE, red)
    out['exchange_changes_weights'] = not _same(none['params'], with_red['params'])
    out.update({k: r[k] for k in ('rows_equal', 'params_equal', 'replays', 'failed', 'capture_lines',
                                  'recaptures', 'violations', 'unheld', 'first_diff', 'stderr_tail')})
    out['loop_marks'] = r['marks']
    red.close()
    return out


def scenario_default():
    steps = 2
    args = parse('ADAM', steps, 1)
    data = [unique_pixel_batch(9000 + i, B, H, W, PER_SAMPLE) for i in range(steps)]
    eager = run_loop(args, data, 61, False, CONTRAST)
    cap = run_loop(args, data, 61, True, CONTRAST, event_terms=False)
    return {'capture_lines': cap['capture_lines'], 'loops': cap['info']['loops'],
            'replays': cap['info']['replays'], 'rows_equal': eager['rows'] == cap['rows'],
            'params_equal': _same(eager['params'], cap['params'])}


if __name__ == '__main__':
    os.environ.pop('DVSOF_LOOPBACK', None)      # the loopback scenario names its exchange itself
    name, _, arg = sys.argv[1].partition(':')
    if name == 'loop':
        opt_name, _, k = arg.partition(':')
        result = scenario_loop(opt_name, int(k))
    elif name == 'wide':
        dtype, _, n = arg.partition(':')
        result = scenario_wide(dtype or 'f32', int(n or 13))
    elif name == 'frameless':
        result = scenario_frameless(int(arg))
    else:
        result = {'padded': scenario_padded, 'loopback': scenario_loopback,
                  'default': scenario_default}[name]()
    print(json.dumps(result), flush=True)
