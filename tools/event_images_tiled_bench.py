#!/usr/bin/env python3
"""The tiled schedule of the splat into the images of warped events against
the per-event kernels (include/dvsof_event_images_tiled.h), one JSON line per
shape (profiles/event_images_tiled/README.md).

8 frames of 256x256 with 30 000 and 120 000 events per frame (the shapes of
profiles/sharpness/README.md), at the reference start without polarity and at
start, middle, end with the polarities apart:

  metric    dvsof_iwe_splat_multi against dvsof_iwe_splat_multi_tiled (mode 1)
  contrast  dvsof_contrast_multi_fwd against dvsof_contrast_multi_fwd_tiled
            (mode 1): the whole forward, of which only the splat differs

HIP events around blocks of launches, the two legs taking turns block by block
within one run, after a bitwise comparison of q and count.  Reported: the
median block of either leg, the spread of the block means, the ratio.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dvs_of_training_framework_amd import _lib, eval as dev_eval  # noqa: E402
from tools.iwe_bench import CROP, block_us  # noqa: E402

OPTIONS = ((1, 0), (7, 1))      # start; start, middle, end with the polarities apart


def legs(kind, per_frame, mask, pol, F=8, side=CROP, rounds=7, reps=40, seed=0):
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    rng = np.random.default_rng(seed)
    n = F * per_frame
    cols = dict(x=rng.integers(0, side, n), y=rng.integers(0, side, n),
                t=np.sort(rng.random((F, per_frame)), 1).reshape(-1).astype(np.float32),
                p=rng.choice(np.array([-1, 1], np.int64), n), s=np.repeat(np.arange(F, dtype=np.int64), per_frame),
                begin=np.arange(F + 1, dtype=np.int64) * per_frame, ts=np.tile(np.array([0, 1], np.float32), F),
                fs=np.arange(F, dtype=np.int64), flow=rng.normal(0, 3, (F, 2, side, side)).astype(np.float32))
    d = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
    M = lib.dvsof_iwe_multi_images(F, mask, pol)
    out = {leg: (torch.empty(M, side, side, dtype=torch.long, device=dev),
                 torch.empty(M, side, side, dtype=torch.int32, device=dev)) for leg in ('old', 'tiled')}
    tiles, tile_bytes = dev_eval.event_images_tiled_workspace(F, mask, pol, side, side, n, dev)
    assert tiles is not None, 'the plan is refused at this shape'
    plan = np.zeros(4, np.int32)
    assert lib.dvsof_event_images_tiled_plan(F, mask, pol, side, side, n, plan.ctypes.data) == 1
    tail = (tiles.data_ptr(), tile_bytes, 1)
    if kind == 'metric':
        head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p')] + [n] + \
            [d[k].data_ptr() for k in ('begin', 'ts', 'flow')] + [F, side, side, mask, pol]

        def call(leg):
            q, count = out[leg]
            args = (*head, q.data_ptr(), count.data_ptr(), stream)
            rc = lib.dvsof_iwe_splat_multi(*args) if leg == 'old' else lib.dvsof_iwe_splat_multi_tiled(*args, *tail)
            assert rc == 0, rc
    else:
        head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n] + \
            [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, side, side, mask, pol]
        rows = torch.empty(M, 48, dtype=torch.uint8, device=dev)
        term = torch.empty((), device=dev)
        need = lib.dvsof_contrast_multi_workspace_bytes(F, mask, pol, side, side)
        ws = torch.empty(need // 8, dtype=torch.long, device=dev)

        def call(leg):
            q, count = out[leg]
            args = (*head, q.data_ptr(), count.data_ptr(), rows.data_ptr(), term.data_ptr(), ws.data_ptr(), need,
                    stream)
            rc = lib.dvsof_contrast_multi_fwd(*args) if leg == 'old' else \
                lib.dvsof_contrast_multi_fwd_tiled(*args, *tail)
            assert rc == 0, rc
    for leg in out:
        for _ in range(3):
            call(leg)
    torch.cuda.synchronize()
    assert torch.equal(out['old'][0], out['tiled'][0]), 'q differs'
    assert torch.equal(out['old'][1], out['tiled'][1]), 'count differs'
    blocks = {leg: [] for leg in out}
    for _ in range(rounds):
        for leg in out:
            blocks[leg].append(block_us(lambda: call(leg), reps))
    res = dict(kind=kind, events_per_frame=per_frame, reference_mask=mask, polarity=pol, images=M,
               tile=[int(plan[0]), int(plan[1])], tiles=int(plan[2]), capacity=int(plan[3]),
               tile_workspace_mib=round(tile_bytes / 2 ** 20, 1))
    for leg, v in blocks.items():
        res[leg] = dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    res['tiled_over_old'] = round(res['tiled']['us'] / res['old']['us'], 3)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--events-per-frame', type=int, nargs='+', default=[30000, 120000])
    ap.add_argument('--kinds', nargs='+', default=['metric', 'contrast'], choices=('metric', 'contrast'))
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=40)
    args = ap.parse_args(argv)
    for kind in args.kinds:
        for per_frame in args.events_per_frame:
            for mask, pol in OPTIONS:
                print(json.dumps(legs(kind, per_frame, mask, pol, rounds=args.rounds, reps=args.reps)), flush=True)


if __name__ == '__main__':
    main()
