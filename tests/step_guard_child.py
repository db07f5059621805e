"""Child process of tests/test_gpu_step_guard.py: training.train under a step
guard, eagerly and with capture=True (one scenario per run, one JSON line; a
GPU fault here fails one test instead of killing the runner).

  <kind>:<accum>   kind adamw / ranger, accum micro-batches per optimizer step;
          8 optimizer steps at 64x64, B = 2: six good ones, one whose last
          micro-batch holds a NaN pixel, one more good one.  After every step a
          hook keeps the parameters, the optimizer state and the guard record.
          With DVSOF_LOOPBACK in the environment both legs exchange through
          the loopback communicator (capture_child._dist).
"""
import json
import math
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

import capture_child as cc  # noqa: E402
import optim_capture_child as occ  # noqa: E402
from dvs_of_training_framework_amd import synthetic  # noqa: E402

B, H, W, STEPS, POISONED = 2, 64, 64, 8, 7
MAX_NORM = 0.05


def batches(accum):
    counts = [4096, 3500, 4096, 2800]
    data = [cc.unique_pixel_batch(70 + i, B, H, W, counts[i % 4]) for i in range(STEPS * accum)]
    bad = data[POISONED * accum - 1]        # the micro-batch that closes step 7
    bad['images'] = bad['images'].copy()
    # a pixel the loss reads: the frame pyramid is a cascade whose coarsest level (8 x 8) takes
    # the frames at rows / columns 0, 9, ..., 63 (and their right / lower neighbours, weight
    # 0); every finer level resamples the level before it, so other pixels are never loaded
    bad['images'][1, 0, 18, 27] = float('nan')
    return data


def make(kind):
    if kind == 'adamw':
        return cc.make()
    return occ.make('ranger4')      # k = 4: steps 4 and 8 synchronise the slow weights


def leg(kind, accum, capture, red):
    from dvs_of_training_framework_amd import capture as cap_mod
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import train
    model, opt, sched, init_losses = make(kind)
    model.predictor.reducer = red
    opt.set_guard(MAX_NORM, True)
    ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
    rows, snaps = [], []

    class Log:
        def add_scalar(self, t, v, x):
            rows.append((t, float(v), x))

    def keep(step, samples):
        rec = opt.guard_state()
        flats = getattr(model.predictor, '_bucket_flat', [])
        bucket_norm = math.sqrt(sum(float((f.double() ** 2).sum()) for f in flats))
        snaps.append(dict(
            weights=[p.detach().clone() for p in model.parameters()],
            state=[v.detach().clone() for st in opt.state.values() for v in st.values()
                   if torch.is_tensor(v)],
            record=rec, raw=opt.guard_tensors()[0].cpu().numpy().tobytes().hex(),
            bucket_norm=bucket_norm))
    info = {}
    orig_close = cap_mod.CapturedLoop.close

    def spy(self):
        steps = dict(self.steps)
        info['roles'] = sorted(steps)
        info['failed'] = str(self.failed) if self.failed else None
        info['replays'] = sum(s.replays for s in steps.values())
        info['unheld'], info['audited'], info['violations'], info['marks'] = [], 0, [], 0
        info['guard_kernels'] = []
        for role, s in sorted(steps.items()):
            a = s.audit()
            info['unheld'] += [list(map(str, u)) for u in a['unheld']]
            info['audited'] += a['audited']
            x = getattr(s, 'exchange_audit', None)
            if x is not None:
                info['violations'] += [list(map(str, v)) for v in x['violations']]
            info['marks'] += s.executor.marks
            names = [n[3] for n in s.executor.nodes()]
            if s.closes:
                info['guard_kernels'] = [sum('guard_partials_kernel' in n for n in names),
                                         sum('guard_close_kernel' in n for n in names)]
            else:
                assert not any('guard_' in n for n in names), role
        return orig_close(self)
    cap_mod.CapturedLoop.close = spy
    try:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            loader = (synthetic.to_torch(b) for b in batches(accum))
            train(model, 'cuda', loader, opt, STEPS, sched, Log(), ev, timers=FakeTimer(),
                  capture=capture, max_events_per_batch=10 ** 7, accumulation_steps=accum,
                  reducer=red, hooks={'keep': keep})
    finally:
        cap_mod.CapturedLoop.close = orig_close
    torch.cuda.synchronize()
    return rows, snaps, info


def same(a, b):
    return len(a) == len(b) and all(torch.equal(u.view(torch.int32), v.view(torch.int32))
                                    for u, v in zip(a, b))


def summary(rows, snaps, first_weights, first_state):
    recs = [s['record'] for s in snaps]
    prev_w = [first_weights] + [s['weights'] for s in snaps[:-1]]
    prev_s = [first_state] + [s['state'] for s in snaps[:-1]]
    return dict(
        skipped=[r['skipped'] for r in recs], consecutive=[r['consecutive'] for r in recs],
        clipped=[r['clipped'] for r in recs], bad=[r['bad'] for r in recs],
        moved=[not same(s['weights'], p) for s, p in zip(snaps, prev_w)],
        # (step 1 creates the state: compared from step 2 on, step 1 counts as moved)
        state_moved=[True] + [not same(s['state'], p) for s, p in zip(snaps[1:], prev_s[1:])],
        logged_skipped=[int(v) for t, v, _ in rows if t == 'General/skipped steps'],
        norm_vs_buckets=[(r['norm'], s['bucket_norm']) for r, s in zip(recs, snaps)
                         if not math.isnan(r['norm'])])


def scenario(kind, accum):
    red = cc._dist()
    model0 = make(kind)[0]
    first = [p.detach().clone() for p in model0.parameters()]
    n_params = sum(p.numel() for p in model0.predictor.parameters())
    del model0
    r_e, s_e, _ = leg(kind, accum, False, red)
    r_c, s_c, info = leg(kind, accum, True, red)
    comm = red.comm_info() if red is not None else None
    if red is not None:
        red.close()
    out = dict(info)
    out.update(
        n_rows=len(r_e), rows_equal=[(t, v if v == v else 'nan', x) for t, v, x in r_e] ==
        [(t, v if v == v else 'nan', x) for t, v, x in r_c],
        weights_equal=[same(a['weights'], b['weights']) and same(a['state'], b['state'])
                       for a, b in zip(s_e, s_c)],
        records_equal=[a['raw'] == b['raw'] for a, b in zip(s_e, s_c)],
        eager=summary(r_e, s_e, first, []), captured=summary(r_c, s_c, first, []),
        comm=comm, n_params=n_params, exchange_violations=info.get('violations', []))
    return out


if __name__ == '__main__':
    kind, _, accum = sys.argv[1].partition(':')
    print(json.dumps(scenario(kind, int(accum or 1))), flush=True)
    cc._shutdown()
