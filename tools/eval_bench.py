#!/usr/bin/env python3
"""Throughput of testing.evaluate on a synthetic MVSEC-shaped sequence, one
JSON line (profiles/eval/README.md).

Sequence: 260x346 float64 ground-truth maps at 20 Hz, frames at 45 Hz
(--frames of them, each spanning --step image intervals: 1 = the direct-scale
branch, 4 = propagation over two to three maps), central 256x256 crop, about
--events events per frame, untrained OpticalFlow.  Reported:
  evaluate_fps        frames/s of testing.evaluate at batch_size 1 and 8
  host_fps            the same frames through the per-frame structure of the
                      reference: batch-1 inference, copy to the host, float64
                      restatement of propagation / count image / error
                      (tests/eval_cases.py) -- never the device path against itself
  kernels             the three kernels alone at F = 8, HIP-event timed,
                      bytes from the shapes
  sequence_fps        the same frames with the events resident on the device
                      (sequence.EventSequence): per batch a window table and one
                      dvsof_event_windows launch instead of numpy slicing,
                      cropping, collation and the upload of the columns; the
                      numpy-events figures of the same run are the comparison
  event_windows       that one C ABI call alone at F = 8 (13 B/event in,
                      44 B/event out, share of 8 TB/s)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dvs_of_training_framework_amd import _lib, eval as dev_eval, testing  # noqa: E402
from dvs_of_training_framework_amd.of import OpticalFlow  # noqa: E402
from dvs_of_training_framework_amd.sequence import EventSequence  # noqa: E402
from tests import eval_cases as ec  # noqa: E402

H, W, CROP = 260, 346, 256
GT_HZ, FRAME_HZ = 20.0, 45.0


def sequence(n_frames, step, per_frame, seed=0):
    rng = np.random.default_rng(seed)
    t0 = 100.0
    image_ts = t0 + 0.01 + np.arange(n_frames + step + 1) / FRAME_HZ
    frames = list(zip(image_ts[:n_frames], image_ts[step:step + n_frames]))
    K = int((image_ts[-1] - t0) * GT_HZ) + 3
    ts = t0 + np.arange(K) / GT_HZ
    x = rng.uniform(-3, 3, (K, H, W))
    y = rng.uniform(-3, 3, (K, H, W))
    x[rng.random(x.shape) < 0.1] = 0.0
    n = per_frame * (n_frames + step)
    t = np.sort(rng.uniform(image_ts[0], image_ts[-1], n))
    events = [rng.integers(0, W, n).astype(np.float64), rng.integers(0, H, n).astype(np.float64),
              t, rng.choice([-1.0, 1.0], n)]
    return events, frames, dict(timestamps=ts, x_flow_dist=x, y_flow_dist=y)


def timed(fn, reps=50):
    """us per call of fn, which only enqueues work (HIP events around reps calls)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels_alone(events, frames, gt, box, F=8):
    """The three C ABI calls alone: inputs, step table, outputs and scratch are
    made once; the timed loop holds nothing but the calls (back to back on one
    stream, so a call's launch overhead hides behind the kernel in front)."""
    dev = 'cuda'
    lib, stream = _lib.lib(), _lib.stream()
    y0, x0, h, w = box
    plans = [dev_eval.plan_gt_steps(gt['timestamps'], a, b) for a, b in frames[:F]]
    lo, hi = min(min(p[1]) for p in plans), max(max(p[1]) for p in plans) + 1
    xd = torch.from_numpy(gt['x_flow_dist'][lo:hi]).to(dev)
    yd = torch.from_numpy(gt['y_flow_dist'][lo:hi]).to(dev)
    table = dev_eval.StepTable(plans, lo, dev)
    u = torch.empty(F, h, w, device=dev)
    v = torch.empty_like(u)
    steps = sum(1 if p[0] else len(p[1]) for p in plans)
    out = {}

    def run_propagate():
        rc = lib.dvsof_gt_flow_propagate(
            xd.data_ptr(), yd.data_ptr(), dev_eval.F64, hi - lo, H, W, table.begin, table.maps,
            table.scales, table.mode, F, table.S, y0, x0, h, w, u.data_ptr(), v.data_ptr(), stream)
        assert rc == 0, rc
    us = timed(run_propagate)
    nbytes = steps * h * w * 2 * 8 + F * h * w * 2 * 4     # two f64 samples per step, u and v out
    out['propagate'] = dict(us=round(us, 2), steps=steps, bytes=nbytes, GBps=round(nbytes / us / 1e3, 1))

    idx = np.searchsorted(events[2], np.array(frames[:F]).ravel(), side='right').reshape(-1, 2)
    cols = [np.concatenate([events[c][i0:i1] for i0, i1 in idx]).astype(np.int64) for c in (0, 1)]
    begin = np.concatenate([[0], np.cumsum(idx[:, 1] - idx[:, 0])])
    n = int(begin[-1])
    xe, ye = torch.from_numpy(cols[0]).to(dev), torch.from_numpy(cols[1]).to(dev)
    bd = torch.from_numpy(begin).to(dev)
    count = torch.empty(F, h, w, dtype=torch.int32, device=dev)

    def run_count():
        rc = lib.dvsof_count_image_batched(xe.data_ptr(), ye.data_ptr(), n, bd.data_ptr(), F,
                                           y0, x0, h, w, count.data_ptr(), stream)
        assert rc == 0, rc
    us = timed(run_count)
    nbytes = n * 16 + F * h * w * 4 + n * 4                # columns in, zero fill, one atomic per event
    out['count_image'] = dict(us=round(us, 2), events=n, bytes=nbytes, GBps=round(nbytes / us / 1e3, 1))

    pred = torch.randn(F, 2, h, w, device=dev)
    rows = torch.empty(F, 32, dtype=torch.uint8, device=dev)
    need = lib.dvsof_flow_error_workspace_bytes(F, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def run_error():
        rc = lib.dvsof_flow_error(u.data_ptr(), v.data_ptr(), pred.data_ptr(), count.data_ptr(),
                                  F, h, w, h, rows.data_ptr(), ws.data_ptr(), need, stream)
        assert rc == 0, rc
    us = timed(run_error)
    nbytes = F * h * w * 5 * 4
    out['flow_error'] = dict(us=round(us, 2), bytes=nbytes, GBps=round(nbytes / us / 1e3, 1))
    return out


def window_kernel_alone(seq, frames, box, F=8):
    """dvsof_event_windows alone: table, inputs and outputs made once, the timed
    loop holds the call only.  Bytes from the shapes: 13 B per event read, 44 B
    per slot written (the table is noise)."""
    lib, stream = _lib.lib(), _lib.stream()
    starts, stops = [a for a, _ in frames[:F]], [b for _, b in frames[:F]]
    c = seq.collate_frames(starts, stops, box)
    ranges = seq.frame_ranges(np.stack([starts, stops], 1))
    cols, _, _, table = seq.windows(ranges[:, 0], ranges[:, 1], np.full(F, min(starts)),
                                    np.arange(F), np.zeros(F), box=box)
    for k in cols:
        assert torch.equal(cols[k], c.events[k]), k
    n = c.n_out
    tb, te, to, tor, tsa, tel = (t.data_ptr() for t in table)
    args = (seq.x.data_ptr(), seq.y.data_ptr(), seq.t_dev.data_ptr(), seq.p.data_ptr(), seq.n_events,
            tb, te, to, tor, tsa, tel, F, *box, cols['x'].data_ptr(), cols['y'].data_ptr(),
            cols['timestamp'].data_ptr(), cols['polarity'].data_ptr(), cols['sample_index'].data_ptr(),
            cols['element_index'].data_ptr(), n, n, stream)

    def run():
        rc = lib.dvsof_event_windows(*args)
        assert rc == 0, rc
    us = timed(run)
    nbytes = n * (13 + 44)
    return dict(us=round(us, 2), events=n, bytes=nbytes, GBps=round(nbytes / us / 1e3, 1),
                share_of_8TBps=round(nbytes / us / 1e3 / 8000, 3))


def host_reference_structure(of, events, frames, gt, box):
    """One frame at a time, off the device after the inference."""
    ev_crop, im_crop = ec.EventCrop(box), ec.ImageCrop(box)
    aee_sum = 0.0
    for e, start, stop in ec.frame_generator(events, frames):
        e = ev_crop(np.array(e).T).T
        flow = of([e], [start], [stop])[0]
        u, v = ec.propagate64(gt['x_flow_dist'], gt['y_flow_dist'], gt['timestamps'], start, stop)
        gt_flow = im_crop(np.dstack((u, v)))
        aee_sum += ec.flow_error64(gt_flow, flow, ec.get_count_image(e, gt_flow.shape[:2]))[0]
    return aee_sum / len(frames)


def panels_alone(F=8, side=CROP, per_frame=30000, seed=0):
    """--hook, first part: the polarity count and the panel launch pair alone at
    F frames of side x side (HIP events around the C ABI calls; bytes from the
    shapes), against visualization.eval_panels_numpy on the host."""
    from dvs_of_training_framework_amd import visualization as vis
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    rng = np.random.default_rng(seed)
    gt = rng.normal(0, 4, (F, 2, side, side)).astype(np.float32)
    gt[:, :, rng.random((side, side)) < 0.05] = 0.0
    pred = (gt + rng.normal(0, 2, gt.shape)).astype(np.float32)
    frames = rng.integers(0, 256, (F, side, side)).astype(np.uint8)
    n = F * per_frame
    cols = [torch.from_numpy(rng.integers(0, side, n)).to(dev) for _ in range(2)]
    pol = torch.from_numpy(rng.choice([-1, 1], n)).to(dev)
    begin = torch.arange(F + 1, device=dev) * per_frame
    count2 = torch.empty(F, 2, side, side, dtype=torch.int32, device=dev)
    out = {}

    def run_count():
        rc = lib.dvsof_count_image_polarity_batched(
            cols[0].data_ptr(), cols[1].data_ptr(), pol.data_ptr(), n, begin.data_ptr(), F, 0, 0,
            side, side, count2.data_ptr(), stream)
        assert rc == 0, rc
    us = timed(run_count)
    nbytes = n * 24 + F * 2 * side * side * 4 + n * 4      # columns in, zero fill, one atomic per event
    out['count_image_polarity'] = dict(us=round(us, 2), events=n, bytes=nbytes,
                                       GBps=round(nbytes / us / 1e3, 1))
    t = [torch.from_numpy(a).to(dev) for a in (pred, gt[:, 0].copy(), gt[:, 1].copy(), frames)]
    need = lib.dvsof_eval_panels_workspace_bytes(F)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    canvas = torch.empty(F, side, 4 * side, 3, dtype=torch.uint8, device=dev)
    stats = torch.empty(F, 32, dtype=torch.uint8, device=dev)

    def run_stats():
        rc = lib.dvsof_eval_panels_stats(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                         count2.data_ptr(), F, side, side, side, ws.data_ptr(), need, stream)
        assert rc == 0, rc

    def run_colour():
        rc = lib.dvsof_eval_panels(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), count2.data_ptr(),
                                   t[3].data_ptr(), F, side, side, side, 0.0, 6.0, 85, ws.data_ptr(), need,
                                   canvas.data_ptr(), canvas.numel(), side * 12 * side, 12 * side,
                                   stats.data_ptr(), stream)
        assert rc == 0, rc

    def run_pair():
        run_stats()
        run_colour()
    px = F * side * side
    for name, fn, nbytes in (('stats', run_stats, px * 24), ('colour', run_colour, px * (24 + 16 + 9 + 12)),
                             ('pair', run_pair, px * (48 + 16 + 9 + 12))):
        us = timed(fn)
        out[name] = dict(us=round(us, 2), bytes=nbytes, GBps=round(nbytes / us / 1e3, 1))
    host = [a.cpu().numpy() for a in (*t[:3], count2, t[3])]
    want = vis.eval_panels_numpy(*host)
    assert np.array_equal(canvas.cpu().numpy()[:, :, [0, 3 * side]], want[:, :, [0, 3 * side]])
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        vis.eval_panels_numpy(*host)
        times.append(round((time.perf_counter() - t0) * 1e3, 1))
    out['numpy_ms'] = times
    return out


def hook_leg(n_frames, per_frame):
    """--hook, second part: one EvaluationHook call over the synthetic sequence
    against the step time of the same run (eager steps of the same model at
    batch 8, 256 x 256, between which the hook runs)."""
    from dvs_of_training_framework_amd import hooks, synthetic
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.optim import FusedAdamW
    from dvs_of_training_framework_amd.sequence import FrameSequence
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    import tempfile
    dev = torch.device('cuda:0')
    events, frames, gt = sequence(n_frames, 1, per_frame)
    image_ts = np.array([a for a, _ in frames] + [frames[-1][1]])
    images = np.random.default_rng(1).integers(0, 256, (len(image_ts), H, W)).astype(np.uint8)
    keep = events[2] <= image_ts[-1]
    seq = FrameSequence([c[keep] for c in events], images, image_ts, device=dev)
    torch.manual_seed(0)
    model = Model(dev, event_representation_depth=5).train()
    opt = FusedAdamW(model.predictor.parameters(), lr=1e-4)
    B = 8
    losses = init_losses((CROP, CROP), B, model, dev, sequence_length=1)
    batches = [synthetic.to_torch(synthetic.make_batch(s, B, CROP, CROP, per_frame), dev) for s in range(4)]

    class Log:
        def add_scalar(self, tag, value, x):
            setattr(self, 'aee' if tag.endswith('mean AEE') else 'share', value)

    def steps(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(k):
            loss = process_minibatch(model, batches[i % 4], FakeTimer(), dev, True, losses, [0.5, 1, 1])[0]
            loss.backward()
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k
    out = dict(frames=None, step_ms=[], hook_ms=[])
    with tempfile.TemporaryDirectory() as tmp:
        hook = hooks.EvaluationHook(model, seq, gt, Log(), (CROP, CROP), tmp, pictures=4)
        out['frames'] = len(hook.frames)
        steps(10)
        hook(0, 0)                      # warm-up: every shape of the call
        for k in range(3):              # alternating: steps, a hook call, steps, ...
            out['step_ms'].append(round(steps(50), 3))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hook(k + 1, 0)
            torch.cuda.synchronize()
            out['hook_ms'].append(round((time.perf_counter() - t0) * 1e3, 1))
        out['mean_aee'] = hook.logger.aee
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--events', type=int, default=30000)
    ap.add_argument('--steps', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--host-frames', type=int, default=40)
    ap.add_argument('--hook', action='store_true',
                    help='the evaluation hook instead (profiles/evaluation_hook/README.md): the '
                         'polarity count and the panel launches alone at F = 8, then one hook '
                         'call over --frames frames against the step time of the same run')
    args = ap.parse_args()
    if args.hook:
        print(json.dumps(dict(panels_F8=panels_alone(per_frame=args.events),
                              hook=hook_leg(args.frames, args.events))))
        return
    box = [(H - CROP) // 2, (W - CROP) // 2, CROP, CROP]
    of = OpticalFlow((CROP, CROP), model=None, event_representation_depth=5)
    crops = dict(event_preproc_fun=ec.EventCrop(box), gt_proc_fun=ec.ImageCrop(box))
    result = dict(frames=args.frames, events_per_frame=args.events, shape=[H, W], crop=CROP, runs=[])
    for step in args.steps:
        events, frames, gt = sequence(args.frames, step, args.events)
        run = dict(step=step, direct_frames=sum(
            dev_eval.plan_gt_steps(gt['timestamps'], a, b)[0] for a, b in frames))
        for bs in (1, 8):
            testing.evaluate(of, events, frames[:2 * bs], gt, batch_size=bs, **crops)     # warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = testing.evaluate(of, events, frames, gt, batch_size=bs, **crops)
            torch.cuda.synchronize()
            run[f'evaluate_fps_batch{bs}'] = round(len(frames) / (time.perf_counter() - t), 1)
            run[f'mean_aee_batch{bs}'] = res[0]
        # the same frames, the events resident on the device (upload not timed: it happens once
        # per recording; reported on its own)
        t = time.perf_counter()
        seq = EventSequence(events, (H, W))
        torch.cuda.synchronize()
        run['sequence_upload_ms'] = round((time.perf_counter() - t) * 1e3, 1)
        for bs in (1, 8):
            testing.evaluate(of, seq, frames[:2 * bs], gt, batch_size=bs, **crops)        # warm-up
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = testing.evaluate(of, seq, frames, gt, batch_size=bs, **crops)
            torch.cuda.synchronize()
            run[f'sequence_fps_batch{bs}'] = round(len(frames) / (time.perf_counter() - t), 1)
            run[f'sequence_mean_aee_batch{bs}'] = res[0]
        run['event_windows_F8'] = window_kernel_alone(seq, frames, box)
        sub = frames[:args.host_frames]
        host_reference_structure(of, events, sub[:2], gt, box)
        t = time.perf_counter()
        run['host_mean_aee'] = host_reference_structure(of, events, sub, gt, box)
        run['host_fps'] = round(len(sub) / (time.perf_counter() - t), 1)
        run['host_frames'] = len(sub)
        run['kernels_F8'] = kernels_alone(events, frames, gt, box)
        result['runs'].append(run)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
