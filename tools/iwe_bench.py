#!/usr/bin/env python3
"""Cost of the label-free validation (docs/IWE_SPEC.md), one JSON line
(profiles/sharpness/README.md).

  kernels    dvsof_iwe_splat, dvsof_iwe_stats, dvsof_iwe_render and, beside
             them, dvsof_count_image_batched alone at 8 frames of 256x256 with
             30 000 and 120 000 events per frame: HIP events around blocks of
             launches, the kernels taking turns block by block within one run;
             the median block per kernel.  The splat's 64-bit integer atomics
             are counted on the host (corners inside the image with Q > 0) and
             reported as added bytes per second beside the chip-wide rate of
             FLOAT atomics, ~1.3 TB/s -- a yardstick only: nobody has measured
             64-bit integer atomics on this chip.
  multi      dvsof_iwe_splat_multi (docs/IWE_SPEC.md sections 8-13) on the
             same inputs with a polarity column, at the masks 1 (start), 5
             (start, end) and 7 (start, middle, end) without and with the
             polarities apart, and, at mask 1 without polarity, against the two
             calls it stands for there (dvsof_count_image_batched +
             dvsof_iwe_splat); all of them taking turns block by block within
             one run.  Every output is compared with the restatement once.
  metric     testing.flow_warp_loss over --frames frames of a synthetic
             MVSEC-shaped recording (260x346, central 256x256 crop, untrained
             network, batch 8) against the same frames' inference alone
             (of.flow_sequence), in alternating blocks of one run; with
             --references / --polarity also at those options.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dvs_of_training_framework_amd import _lib, eval as dev_eval, testing  # noqa: E402
from dvs_of_training_framework_amd.of import OpticalFlow  # noqa: E402
from dvs_of_training_framework_amd.sequence import EventSequence  # noqa: E402

H, W, CROP = 260, 346, 256
FRAME_HZ = 45.0
FLOAT_ATOMIC_TBPS = 1.3


def block_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels_alone(per_frame, F=8, side=CROP, rounds=7, reps=40, seed=0):
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    rng = np.random.default_rng(seed)
    n = F * per_frame
    x, y = rng.integers(0, side, n), rng.integers(0, side, n)
    t = np.sort(rng.random((F, per_frame)), 1).reshape(-1).astype(np.float32)
    begin = np.arange(F + 1, dtype=np.int64) * per_frame
    ts = np.tile(np.array([0, 1], np.float32), F)
    flow = rng.normal(0, 3, (F, 2, side, side)).astype(np.float32)
    d = {k: torch.from_numpy(v).to(dev) for k, v in dict(x=x, y=y, t=t, begin=begin, ts=ts, flow=flow).items()}
    q = torch.empty(F, side, side, dtype=torch.long, device=dev)
    count = torch.empty(F, side, side, dtype=torch.int32, device=dev)
    rows = torch.empty(F, 48, dtype=torch.uint8, device=dev)
    need = lib.dvsof_iwe_stats_workspace_bytes(F, side, side)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    canvas = torch.empty(F, side, 2 * side, 3, dtype=torch.uint8, device=dev)

    def check(rc):
        assert rc == 0, rc
    calls = {
        'count_image': lambda: check(lib.dvsof_count_image_batched(
            d['x'].data_ptr(), d['y'].data_ptr(), n, d['begin'].data_ptr(), F, 0, 0, side, side,
            count.data_ptr(), stream)),
        'splat': lambda: check(lib.dvsof_iwe_splat(
            d['x'].data_ptr(), d['y'].data_ptr(), d['t'].data_ptr(), n, d['begin'].data_ptr(),
            d['ts'].data_ptr(), d['flow'].data_ptr(), F, side, side, q.data_ptr(), stream)),
        'stats': lambda: check(lib.dvsof_iwe_stats(q.data_ptr(), count.data_ptr(), F, side, side,
                                                   rows.data_ptr(), ws.data_ptr(), need, stream)),
        'render': lambda: check(lib.dvsof_iwe_render(q.data_ptr(), count.data_ptr(), rows.data_ptr(), F, side,
                                                     side, canvas.data_ptr(), stream))}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the device against the restatement once, and the number of atomics from the same arithmetic
    want = dev_eval.iwe_splat_host(x, y, t, begin, ts, flow)
    assert np.array_equal(q.cpu().numpy(), want)
    atomics = count_atomics(x, y, t, flow, side)
    blocks = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            blocks[k].append(block_us(fn, reps))
    px = F * side * side
    nbytes = {'count_image': n * 16 + px * 4 + n * 4,
              'splat': n * 20 + n * 8 + px * 8 + atomics * 8,      # columns, two flow reads, zero fill, atomics
              'stats': px * 12, 'render': px * (12 + 6)}
    out = {}
    for k, v in blocks.items():
        us = statistics.median(v)
        out[k] = dict(us=round(us, 2), min_us=round(min(v), 2), max_us=round(max(v), 2), bytes=nbytes[k],
                      GBps=round(nbytes[k] / us / 1e3, 1))
    us = out['splat']['us']
    out['splat'].update(atomics=atomics, atomic_GBps=round(atomics * 8 / us / 1e3, 1),
                        share_of_float_atomic_rate=round(atomics * 8 / us / 1e3 / (FLOAT_ATOMIC_TBPS * 1e3), 3))
    return out


def multi_kernels(per_frame, F=8, side=CROP, rounds=7, reps=40, seed=0):
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    rng = np.random.default_rng(seed)
    n = F * per_frame
    x, y = rng.integers(0, side, n), rng.integers(0, side, n)
    t = np.sort(rng.random((F, per_frame)), 1).reshape(-1).astype(np.float32)
    p = rng.choice(np.array([-1, 1], np.int64), n)
    begin = np.arange(F + 1, dtype=np.int64) * per_frame
    ts = np.tile(np.array([0, 1], np.float32), F)
    flow = rng.normal(0, 3, (F, 2, side, side)).astype(np.float32)
    d = {k: torch.from_numpy(v).to(dev)
         for k, v in dict(x=x, y=y, t=t, p=p, begin=begin, ts=ts, flow=flow).items()}
    M = 6 * F
    q = torch.empty(M, side, side, dtype=torch.long, device=dev)
    count = torch.empty(M, side, side, dtype=torch.int32, device=dev)

    def check(rc):
        assert rc == 0, rc

    def multi(mask, pol):
        return lambda: check(lib.dvsof_iwe_splat_multi(
            d['x'].data_ptr(), d['y'].data_ptr(), d['t'].data_ptr(), d['p'].data_ptr(), n,
            d['begin'].data_ptr(), d['ts'].data_ptr(), d['flow'].data_ptr(), F, side, side, mask, pol,
            q.data_ptr(), count.data_ptr(), stream))

    def two_calls():
        check(lib.dvsof_count_image_batched(d['x'].data_ptr(), d['y'].data_ptr(), n, d['begin'].data_ptr(), F,
                                            0, 0, side, side, count.data_ptr(), stream))
        check(lib.dvsof_iwe_splat(d['x'].data_ptr(), d['y'].data_ptr(), d['t'].data_ptr(), n,
                                  d['begin'].data_ptr(), d['ts'].data_ptr(), d['flow'].data_ptr(), F, side,
                                  side, q.data_ptr(), stream))
    calls = {f'multi_mask{mask}_polarity{pol}': multi(mask, pol) for mask in (1, 5, 7) for pol in (0, 1)}
    calls['count_image_and_splat'] = two_calls
    images = {}
    for mask in (1, 5, 7):
        for pol in (0, 1):
            k = f'multi_mask{mask}_polarity{pol}'
            for _ in range(3):
                calls[k]()
            torch.cuda.synchronize()
            want_q, want_c = dev_eval.iwe_splat_multi_host(x, y, t, p, begin, ts, flow, mask, bool(pol))
            images[k] = len(want_q)
            assert np.array_equal(q[:images[k]].cpu().numpy(), want_q)
            assert np.array_equal(count[:images[k]].cpu().numpy().view(np.uint32), want_c)
    for _ in range(3):
        two_calls()
    images['count_image_and_splat'] = F
    blocks = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            blocks[k].append(block_us(fn, reps))
    out = {}
    for k, v in blocks.items():
        out[k] = dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2),
                      images=images[k], zero_fill_bytes=images[k] * side * side * 12)
    return out


def count_atomics(x, y, t, flow, side):
    """Corners inside the image with Q > 0 (tau = t: the window is [0, 1])."""
    f = np.repeat(np.arange(flow.shape[0]), x.size // flow.shape[0])
    xw = x.astype(np.float32) - t * flow[f, 0, y, x]
    yw = y.astype(np.float32) - t * flow[f, 1, y, x]
    ok = (xw > -1) & (xw < side) & (yw > -1) & (yw < side)
    xw, yw = xw[ok], yw[ok]
    fx, fy = xw - np.floor(xw), yw - np.floor(yw)
    cx, cy = np.floor(xw).astype(np.int64), np.floor(yw).astype(np.int64)
    total = 0
    for j, wy in enumerate((np.float32(1) - fy, fy)):
        for i, wx in enumerate((np.float32(1) - fx, fx)):
            inside = (cx + i >= 0) & (cx + i < side) & (cy + j >= 0) & (cy + j < side)
            total += int((inside & ((wy * wx * np.float32(2.0 ** 32)).astype(np.int64) > 0)).sum())
    return total


def metric_against_inference(n_frames, per_frame, rounds=3, seed=0, references=('start',), polarity=False):
    rng = np.random.default_rng(seed)
    image_ts = 100.01 + np.arange(n_frames + 1) / FRAME_HZ
    frames = list(zip(image_ts[:-1], image_ts[1:]))
    n = per_frame * n_frames
    events = [rng.integers(0, W, n).astype(np.float64), rng.integers(0, H, n).astype(np.float64),
              np.sort(rng.uniform(image_ts[0], image_ts[-1], n)), rng.choice([-1.0, 1.0], n)]
    seq = EventSequence(events, (H, W))
    box = ((H - CROP) // 2, (W - CROP) // 2, CROP, CROP)
    of = OpticalFlow((CROP, CROP), model=None, event_representation_depth=5)
    arr = np.array(frames)

    def inference():
        for b0 in range(0, n_frames, 8):
            of.flow_sequence(seq, list(arr[b0:b0 + 8, 0]), list(arr[b0:b0 + 8, 1]), box=box, return_events=True)

    def metric():
        return testing.flow_warp_loss(of, seq, frames, box, batch_size=8, references=references,
                                      polarity=polarity)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r
    wall(inference)
    _, rows = wall(metric)
    out = dict(frames=n_frames, events_per_frame=per_frame, references=list(references), polarity=polarity,
               inference_ms=[], flow_warp_loss_ms=[])
    for _ in range(rounds):
        out['inference_ms'].append(round(wall(inference)[0], 2))
        out['flow_warp_loss_ms'].append(round(wall(metric)[0], 2))
    a, b = statistics.median(out['inference_ms']), statistics.median(out['flow_warp_loss_ms'])
    out['metric_share_of_batch'] = round((b - a) / b, 4)
    fwl, kept = dev_eval.derive_fwl(rows, CROP * CROP)
    out['mean_fwl'], out['mean_kept_mass'] = float(np.nanmean(fwl)), float(np.nanmean(kept))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--events', type=int, nargs='+', default=[30000, 120000])
    ap.add_argument('--references', default='start',
                    help='reference times of a second metric measurement: comma-separated among start, middle, end')
    ap.add_argument('--polarity', action='store_true', help='ON and OFF events apart in that measurement')
    args = ap.parse_args()
    references = tuple(args.references.split(','))
    result = dict(kernels_F8_256={str(e): kernels_alone(e) for e in args.events},
                  multi_F8_256={str(e): multi_kernels(e) for e in args.events},
                  metric=[metric_against_inference(args.frames, e) for e in args.events])
    if references != ('start',) or args.polarity:
        result['metric_with_options'] = [
            metric_against_inference(args.frames, e, references=references, polarity=args.polarity)
            for e in args.events]
    print(json.dumps(result))


if __name__ == '__main__':
    main()
