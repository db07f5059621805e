"""Learnable event representation at the benchmark shape (batch 8, 256 x 256 x 5,
65 536 events per sample), timed with HIP events: the learned forward against
voxel.voxelize on the same events, the table-gradient kernel, dvsof_first_dgrad,
and the eager training step with and without --learnable-representation.
One JSON line on stdout.  ``--default-step-only`` measures just the default
model's eager step: that part also runs on a checkout without the feature."""
import argparse
import json
import statistics
import sys
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--depth', type=int, default=5)
    ap.add_argument('--events', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--default-step-only', action='store_true')
    a = ap.parse_args()
    B, H, W, C, n = a.batch, a.size, a.size, a.depth, a.events
    out = dict(shape=dict(B=B, H=H, W=W, C=C, events=B * n))
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
    print(json.dumps(out))


if __name__ == '__main__':
    main()
