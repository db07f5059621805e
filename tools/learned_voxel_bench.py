"""Learnable event representation at the benchmark shape (batch 8, 256 x 256 x 5,
65 536 events per sample), timed with HIP events: the learned forward against
voxel.voxelize on the same events, the table-gradient kernel, dvsof_first_dgrad,
and the eager training step with and without --learnable-representation;
``step_learnable_captured``: the RESIDENT model's step replayed by the step
executor against the eager loop of an identical model, in alternating blocks
(device time per step and host time to enqueue one).  With DVSOF_LOOPBACK=
"world:delay_us" in the environment that leg runs under the loopback gradient
exchange (``--captured-only`` runs nothing else).
``learned_fwd_deterministic``: the order-independent forward
(lv.voxelize(..., deterministic=True)) against the float-atomics forward and the
fixed voxeliser on the same events, in alternating blocks of one run
(``--forward-only`` runs nothing else).
One JSON line on stdout.  ``--default-step-only`` measures just the default
model's eager step: that part also runs on a checkout without the feature."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dvs_of_training_framework_amd import synthetic, voxel  # noqa: E402
from dvs_of_training_framework_amd.loss import init_losses  # noqa: E402
from dvs_of_training_framework_amd.net import Model  # noqa: E402
from dvs_of_training_framework_amd.optim import FusedRanger  # noqa: E402
from dvs_of_training_framework_amd.timer import FakeTimer  # noqa: E402
from dvs_of_training_framework_amd.training import process_minibatch  # noqa: E402

HBM = 8e12      # bytes/s


def timed(fn, reps, warmup=5, blocks=5):
    """-> (median us over blocks of reps calls, min, max)."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return dict(us=round(statistics.median(out), 2), min=round(min(out), 2), max=round(max(out), 2))


def share(row, nbytes):
    row['bytes'] = nbytes
    row['share_of_8TBs'] = round(nbytes / (row['us'] * 1e-6) / HBM, 4)
    return row


def alternating(legs, reps, warmup=5, blocks=5):
    """legs: [(name, fn)], timed in alternating blocks of ``reps`` calls.
    -> {name: median / min / max us per call over the blocks}."""
    for _ in range(warmup):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name, _ in legs}
    for _ in range(blocks):
        for name, fn in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / reps)
    return {name: dict(us=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
            for name, v in out.items()}


def forward_legs(B, H, W, C, n, reps):
    """The three forwards on the same events, one run, alternating blocks."""
    from dvs_of_training_framework_amd import learned_voxel as lv
    ev = synthetic.to_torch(synthetic.make_batch(1234, B, H, W, n), 'cuda')['events']
    t0 = torch.zeros(B, device='cuda')
    t1 = torch.full((B,), synthetic.WINDOW, device='cuda')
    R, S = 2, 8
    theta = lv.initial_kernel(R, S).cuda()
    return alternating([
        ('learned_fwd', lambda: lv.voxelize(ev, t0, t1, theta, R, S, B, C, H, W)),
        ('learned_fwd_deterministic',
         lambda: lv.voxelize(ev, t0, t1, theta, R, S, B, C, H, W, deterministic=True)),
        ('voxelize', lambda: voxel.voxelize(ev, t0, t1, B, C, H, W))], reps)


def step_time(B, H, W, C, n, learnable, reps):
    torch.manual_seed(0)
    kw = dict(learnable_representation=True) if learnable else {}
    model = Model('cuda', event_representation_depth=C, **kw)
    model.train()
    opt = FusedRanger(model.parameters(), lr=1e-3)
    ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
    batch = synthetic.to_torch(synthetic.make_batch(1234, B, H, W, n), 'cuda')

    def step():
        loss, _, _ = process_minibatch(model, batch, FakeTimer(), 'cuda', True, ev, [0.5, 1, 1])
        loss.backward()
        model.strict = False
        opt.step()
        opt.zero_grad(set_to_none=True)
    return timed(step, reps, warmup=8)


def captured_against_eager(B, H, W, C, n, reps, blocks=5):
    """The resident learnable model: executor replay against its own eager
    loop (two models from one seed, one resident batch), alternating blocks of
    ``reps`` steps.  -> {'eager': ..., 'captured': ...}: median / min / max
    device us per step and the host us it takes to enqueue a step."""
    from dvs_of_training_framework_amd import parallel
    from dvs_of_training_framework_amd.capture import CapturedTrainStep
    from dvs_of_training_framework_amd.loss import unit_backward
    red = parallel.GradReducer() if os.environ.get('DVSOF_LOOPBACK') else None
    batch = synthetic.to_torch(synthetic.make_batch(1234, B, H, W, n), 'cuda')

    def make():
        torch.manual_seed(0)
        model = Model('cuda', event_representation_depth=C, learnable_representation=True,
                      representation_resident=True)
        model.train()
        model.predictor.reducer = red
        return model, FusedRanger(model.parameters(), lr=1e-3), \
            init_losses((H, W), B, model, 'cuda', sequence_length=1)
    model_e, opt_e, ev_e = make()

    def eager():
        opt_e.zero_grad(set_to_none=True)
        loss, _, _ = process_minibatch(model_e, batch, FakeTimer(), 'cuda', True, ev_e, [0.5, 1, 1])
        unit_backward(loss)
        model_e.strict = False
        if red is not None:
            red.wait()
        opt_e.step()
    model_c, opt_c, ev_c = make()
    step = CapturedTrainStep(model_c, ev_c, opt_c, [0.5, 1, 1], 'cuda', batch, bind=True,
                             reducer=red)
    legs = (('eager', eager), ('captured', step))
    for _ in range(12):         # calibration, then the executor settles on a lane plan
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    dev, host = {k: [] for k, _ in legs}, {k: [] for k, _ in legs}
    for _ in range(blocks):
        for name, fn in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            host[name].append((time.perf_counter() - t) * 1e6 / reps)
            b.synchronize()
            dev[name].append(a.elapsed_time(b) * 1e3 / reps)
    out = {name: dict(us=round(statistics.median(dev[name]), 2), min=round(min(dev[name]), 2),
                      max=round(max(dev[name]), 2),
                      host_us=round(statistics.median(host[name]), 2)) for name, _ in legs}
    out['plan'] = step.executor.plan()[0]
    out['marks'] = step.executor.marks
    out['exchange'] = os.environ.get('DVSOF_LOOPBACK') or None
    step.close()
    if red is not None:
        red.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--depth', type=int, default=5)
    ap.add_argument('--events', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--default-step-only', action='store_true')
    ap.add_argument('--captured-only', action='store_true')
    ap.add_argument('--forward-only', action='store_true')
    a = ap.parse_args()
    B, H, W, C, n = a.batch, a.size, a.size, a.depth, a.events
    out = dict(shape=dict(B=B, H=H, W=W, C=C, events=B * n))
    if a.captured_only:
        out['step_learnable_captured'] = captured_against_eager(B, H, W, C, n, a.reps)
        print(json.dumps(out))
        return
    if a.forward_only:
        out['forward_alternating'] = forward_legs(B, H, W, C, n, a.reps)
        print(json.dumps(out))
        return
    out['step_default'] = step_time(B, H, W, C, n, False, a.reps)
    if not a.default_step_only:
        from dvs_of_training_framework_amd import conv, learned_voxel as lv
        out['step_learnable'] = step_time(B, H, W, C, n, True, a.reps)
        ev = synthetic.to_torch(synthetic.make_batch(1234, B, H, W, n), 'cuda')['events']
        t0 = torch.zeros(B, device='cuda')
        t1 = torch.full((B,), synthetic.WINDOW, device='cuda')
        R, S = 2, 8
        theta = lv.initial_kernel(R, S).cuda()
        N, grid_bytes = B * n, 4 * B * C * H * W
        out['voxelize'] = timed(lambda: voxel.voxelize(ev, t0, t1, B, C, H, W), a.reps)
        # wire columns 36 B/event; the grid is filled, then each event adds to <= 2R voxels
        out['learned_fwd'] = share(timed(
            lambda: lv.voxelize(ev, t0, t1, theta, R, S, B, C, H, W), a.reps),
            36 * N + grid_bytes + 2 * R * 4 * N)
        gV = torch.randn(B, C, H, W, device='cuda')
        out['learned_bwd'] = share(timed(
            lambda: lv.voxelize_bwd(ev, t0, t1, R, S, gV), a.reps), 36 * N + 2 * R * 4 * N)
        gz = torch.randn(B, H // 2, W // 2, 64, device='cuda')
        w = torch.randn(64, C, 3, 3, device='cuda').contiguous(memory_format=torch.channels_last)
        out['first_dgrad'] = share(timed(
            lambda: conv.first_dgrad(gz, w, B, C, H, W), a.reps), gz.numel() * 4 + grid_bytes)
        out['step_learnable_captured'] = captured_against_eager(B, H, W, C, n, a.reps)
        out['forward_alternating'] = forward_legs(B, H, W, C, n, a.reps)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
