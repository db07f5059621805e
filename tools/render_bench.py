#!/usr/bin/env python3
"""What a picture of the predicted flow costs, at the benchmark shape.

    python tools/render_bench.py [--batch 8] [--size 256] [--reps 20] [--blocks 5]

One pyramid mosaic per sample (four levels, size/8 .. size), two legs in
alternating blocks of ONE run; one JSON line each:

  device  ``visualization.render_pyramid`` on device flows: HIP events around
          the call (the two launches and the upload of the item table) and
          the host clock around call + synchronise (what a training thread
          that waits for the picture pays)
  host    the reference's way on the same flows: copy every level to the
          host, then the numpy restatement of flow2img per sample and level
          and the slicing into the mosaic (``render_pyramid`` on numpy
          arrays).  cv2's two passes are compiled code where the restatement
          is numpy, so this leg is an upper bound of the reference's cost,
          not a measurement of it.

Both legs draw the same bytes wherever the float32 arctan2 of the two
libraries agrees; the share of differing pixels is printed.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from dvs_of_training_framework_amd import visualization as vis  # noqa: E402


def say(**row):
    print(json.dumps(row), flush=True)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def device_block(levels, reps):
    events, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        vis.render_pyramid(levels)
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        events.append(a.elapsed_time(b))
    return events, wall


def host_block(levels, reps):
    wall = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vis.render_pyramid([f.cpu().numpy() for f in levels])
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--batch', type=int, default=8)
    p.add_argument('--size', type=int, default=256)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--host-reps', type=int, default=3)
    p.add_argument('--blocks', type=int, default=5)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('render_bench.py measures on the GPU: none here')
    gen = torch.Generator().manual_seed(11)
    levels = [(torch.randn(a.batch, 2, a.size >> k, a.size >> k, generator=gen) * (4 - k)).cuda()
              for k in (3, 2, 1, 0)]
    device_block(levels, 5), host_block(levels, 1)              # set-up: code objects, allocator
    dev_events, dev_wall, host_wall = [], [], []
    for _ in range(a.blocks):
        e, w = device_block(levels, a.reps)
        dev_events += e
        dev_wall += w
        host_wall += host_block(levels, a.host_reps)
    got = vis.render_pyramid(levels).cpu().numpy()
    want = vis.render_pyramid([f.cpu().numpy() for f in levels])
    pixels = a.batch * sum((a.size >> k) ** 2 for k in range(4))
    shape = dict(batch=a.batch, size=a.size, levels=4, pixels=pixels,
                 canvas=list(got.shape))
    say(what='render', leg='device', **shape, event_ms=round(median(dev_events), 4),
        event_ms_min=round(min(dev_events), 4), event_ms_max=round(max(dev_events), 4),
        wall_ms=round(median(dev_wall), 4), calls=len(dev_events),
        bytes_read=8 * pixels, bytes_written=int(got.size))
    say(what='render', leg='host', **shape, wall_ms=round(median(host_wall), 3),
        wall_ms_min=round(min(host_wall), 3), wall_ms_max=round(max(host_wall), 3),
        calls=len(host_wall))
    say(what='render', leg='agreement',
        differing_pixel_share=float((got != want).any(-1).mean()))


if __name__ == '__main__':
    main()
