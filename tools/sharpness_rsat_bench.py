#!/usr/bin/env python3
"""Cost of the ratio of squared average timestamps beside the flow warp loss
(docs/IWE_SPEC.md sections 14-21), one JSON line
(profiles/sharpness/README.md).

  launches   the metric launches of a batch of 8 frames of 256x256 with 30 000
             and 120 000 events per frame, at the references start and at
             start, middle, end with the polarities apart: with the flag off
             (dvsof_count_image_batched + dvsof_iwe_splat, or
             dvsof_iwe_splat_multi, then dvsof_iwe_stats) against on
             (dvsof_iwe_avg_timestamp, then dvsof_iwe_stats on its q and
             count), HIP events around blocks of launches, the two legs taking
             turns block by block within one run, after a bitwise comparison of
             the q and count they share.  Reported: the median block of either
             leg, the spread of the block means, the ratio.
  metric     testing.flow_warp_loss against testing.event_alignment over
             --frames frames of a synthetic MVSEC-shaped recording (260x346,
             central 256x256 crop, untrained network, batch 8) and against the
             same frames' inference alone, in alternating blocks of one run.
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
from tools.iwe_bench import CROP, FRAME_HZ, H, W, block_us  # noqa: E402

OPTIONS = ((1, 0), (7, 1))      # start; start, middle, end with the polarities apart


def launches(per_frame, mask, pol, F=8, side=CROP, rounds=7, reps=40, seed=0):
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
    M = lib.dvsof_iwe_multi_images(F, mask, pol)
    P = M * side * side
    q = torch.empty(M, side, side, dtype=torch.long, device=dev)
    count = torch.empty(M, side, side, dtype=torch.int32, device=dev)
    iwe_rows = torch.empty(M, 48, dtype=torch.uint8, device=dev)
    iwe_need = lib.dvsof_iwe_stats_workspace_bytes(M, side, side)
    iwe_ws = torch.empty(iwe_need, dtype=torch.uint8, device=dev)
    nbytes = lib.dvsof_iwe_avg_timestamp_image_bytes(F, side, side, mask, pol)
    region = torch.empty(nbytes // 8, dtype=torch.long, device=dev)
    avg_rows = torch.empty(M, 4, dtype=torch.long, device=dev)
    need = lib.dvsof_iwe_avg_timestamp_workspace_bytes(F, side, side, mask, pol)
    ws = torch.empty(need // 8, dtype=torch.long, device=dev)
    head = (d['begin'].data_ptr(), d['ts'].data_ptr(), d['flow'].data_ptr(), F, side, side)

    def check(rc):
        assert rc == 0, rc

    def off():
        if mask == 1 and not pol:       # the defaults: the two calls the hook makes
            check(lib.dvsof_count_image_batched(d['x'].data_ptr(), d['y'].data_ptr(), n, d['begin'].data_ptr(), F,
                                                0, 0, side, side, count.data_ptr(), stream))
            check(lib.dvsof_iwe_splat(d['x'].data_ptr(), d['y'].data_ptr(), d['t'].data_ptr(), n, *head,
                                      q.data_ptr(), stream))
        else:
            check(lib.dvsof_iwe_splat_multi(d['x'].data_ptr(), d['y'].data_ptr(), d['t'].data_ptr(),
                                            d['p'].data_ptr(), n, *head, mask, pol, q.data_ptr(), count.data_ptr(),
                                            stream))
        check(lib.dvsof_iwe_stats(q.data_ptr(), count.data_ptr(), M, side, side, iwe_rows.data_ptr(),
                                  iwe_ws.data_ptr(), iwe_need, stream))

    def on():
        check(lib.dvsof_iwe_avg_timestamp(d['x'].data_ptr(), d['y'].data_ptr(), d['t'].data_ptr(),
                                          d['p'].data_ptr(), n, *head, mask, pol, region.data_ptr(), nbytes,
                                          avg_rows.data_ptr(), ws.data_ptr(), need, stream))
        check(lib.dvsof_iwe_stats(region.data_ptr(), region.data_ptr() + 24 * P, M, side, side,
                                  iwe_rows.data_ptr(), iwe_ws.data_ptr(), iwe_need, stream))
    for fn in (off, on):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # what the two legs share, bit for bit
    raw = region.view(torch.uint8)
    assert torch.equal(raw[:8 * P], q.view(torch.uint8).reshape(-1)), 'q differs'
    assert torch.equal(raw[24 * P:28 * P], count.view(torch.uint8).reshape(-1)), 'count differs'
    blocks = {'off': [], 'on': []}
    for _ in range(rounds):
        blocks['off'].append(block_us(off, reps))
        blocks['on'].append(block_us(on, reps))
    out = dict(events_per_frame=per_frame, reference_mask=mask, polarity=pol, images=M)
    for k, v in blocks.items():
        out[k] = dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    out['on_over_off'] = round(out['on']['us'] / out['off']['us'], 3)
    rsat = dev_eval.derive_rsat(avg_rows.view(torch.uint8).view(M, 32))
    out['mean_rsat'] = float(np.nanmean(rsat))
    return out


def metric_against_inference(n_frames, per_frame, mask, pol, rounds=3, seed=0):
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

    def off():
        return testing.flow_warp_loss(of, seq, frames, box, batch_size=8, references=mask, polarity=bool(pol))

    def on():
        return testing.event_alignment(of, seq, frames, box, batch_size=8, references=mask, polarity=bool(pol))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r
    wall(inference)
    _, rows = wall(off)
    _, (rows_on, avg_rows) = wall(on)
    assert rows.tobytes() == rows_on.tobytes(), 'the rows of the flow warp loss differ'
    out = dict(frames=n_frames, events_per_frame=per_frame, reference_mask=mask, polarity=pol, inference_ms=[],
               off_ms=[], on_ms=[])
    for _ in range(rounds):
        out['inference_ms'].append(round(wall(inference)[0], 2))
        out['off_ms'].append(round(wall(off)[0], 2))
        out['on_ms'].append(round(wall(on)[0], 2))
    a = statistics.median(out['inference_ms'])
    for k in ('off', 'on'):
        b = statistics.median(out[f'{k}_ms'])
        out[f'{k}_share_of_batch'] = round((b - a) / b, 4)
    out['mean_rsat'] = float(np.nanmean(dev_eval.derive_rsat(avg_rows)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=96)
    ap.add_argument('--events', type=int, nargs='+', default=[30000, 120000])
    args = ap.parse_args()
    result = dict(launches_F8_256=[launches(e, mask, pol) for e in args.events for mask, pol in OPTIONS],
                  metric=[metric_against_inference(args.frames, e, mask, pol)
                          for e in args.events for mask, pol in OPTIONS])
    print(json.dumps(result))


if __name__ == '__main__':
    main()
