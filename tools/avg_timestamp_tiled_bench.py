#!/usr/bin/env python3
"""The tiled schedule of the splat into the average-timestamp images against
the per-event kernels (include/dvsof_avg_timestamp_tiled.h), one JSON line per
shape and one for the training step (profiles/avg_timestamp_tiled/README.md).

8 frames of 256x256 with 2 000, 8 000, 30 000, 65 536 (the benchmark batch)
and 120 000 events per frame, at the term's default start,end without polarity
and at start,middle,end with the polarities apart:

  term    dvsof_avg_timestamp_fwd against dvsof_avg_timestamp_fwd_tiled
          (mode 1): the whole forward, of which only the splat differs
  metric  dvsof_iwe_avg_timestamp against dvsof_iwe_avg_timestamp_tiled (mode 1)

HIP events around blocks of launches, the two legs taking turns block by block
within one run, after a bitwise comparison of q, s, base, count and the rows.
Reported: the median block of either leg, the spread of the block means, the
ratio, and whether the tiled leg wins by more than either spread.

  step    one eager Ranger step of the benchmark batch with
          --avg-timestamp-weight, the term per event against
          avg_timestamp_tiled='force', in alternating blocks of one run.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L  # noqa: E402
from tools.iwe_bench import CROP, block_us  # noqa: E402

OPTIONS = ((5, 0), (7, 1))      # start, end; start, middle, end with the polarities apart
EVENTS_PER_FRAME = (2000, 8000, 30000, 65536, 120000)


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
    P = M * side * side
    tiles, tile_bytes = dev_eval.avg_timestamp_tiled_workspace(F, mask, pol, side, side, n, dev)
    assert tiles is not None, 'the plan is refused at this shape'
    plan = np.zeros(4, np.int32)
    assert lib.dvsof_event_images_tiled_plan(F, mask, pol, side, side, n, plan.ctypes.data) == 1
    tail = (tiles.data_ptr(), tile_bytes, 1)
    if kind == 'metric':
        head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p')] + [n] + \
            [d[k].data_ptr() for k in ('begin', 'ts', 'flow')] + [F, side, side, mask, pol]
        image_bytes = lib.dvsof_iwe_avg_timestamp_image_bytes(F, side, side, mask, pol)
        need = lib.dvsof_iwe_avg_timestamp_workspace_bytes(F, side, side, mask, pol)
        ws = torch.empty(need // 8, dtype=torch.long, device=dev)
        out = {leg: (torch.empty(image_bytes // 8, dtype=torch.long, device=dev),
                     torch.empty(M * 4, dtype=torch.long, device=dev)) for leg in ('old', 'tiled')}

        def call(leg):
            images, rows = out[leg]
            args = (*head, images.data_ptr(), image_bytes, rows.data_ptr(), ws.data_ptr(), need, stream)
            rc = lib.dvsof_iwe_avg_timestamp(*args) if leg == 'old' else \
                lib.dvsof_iwe_avg_timestamp_tiled(*args, *tail)
            assert rc == 0, rc

        def compared(leg):          # q, s, base, count; the rows
            return out[leg][0][:(28 * P + 7) // 8], out[leg][1]
    else:
        head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n] + \
            [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, side, side, mask, pol]
        need = lib.dvsof_avg_timestamp_workspace_bytes(F, mask, pol, side, side)
        lay = L.avg_timestamp_layout(F, M, side, side)
        out = {leg: (torch.empty(need // 8, dtype=torch.long, device=dev), torch.empty((), device=dev))
               for leg in ('old', 'tiled')}

        def call(leg):
            ws, term = out[leg]
            args = (*head, term.data_ptr(), ws.data_ptr(), need, stream)
            rc = lib.dvsof_avg_timestamp_fwd(*args) if leg == 'old' else lib.dvsof_avg_timestamp_fwd_tiled(*args, *tail)
            assert rc == 0, rc

        def compared(leg):          # the zeroed region (q, s, base, sums, count); the records, units and rows; the term
            ws, term = out[leg]
            return ws[:lay['zeroed_bytes'] // 8], ws[lay['rec'] // 8:lay['part'] // 8], term
    for leg in out:
        for _ in range(3):
            call(leg)
    torch.cuda.synchronize()
    for a, b in zip(compared('old'), compared('tiled')):
        assert torch.equal(a, b), 'the tiled call\'s bytes differ'
    assert bool(compared('tiled')[0].any())
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
    spread = max(res[leg]['max_us'] - res[leg]['min_us'] for leg in out)
    res['wins_by_more_than_the_spread'] = bool(res['old']['us'] - res['tiled']['us'] > spread)
    return res


def step(weight, rounds, steps=30, warmup=15):
    from tools.avg_timestamp_bench import Leg
    legs_ = {'per_event': Leg(weight), 'tiled': Leg(weight)}
    legs_['tiled'].extra['avg_timestamp_tiled'] = 'force'
    for leg in legs_.values():
        leg.block(warmup)
    ms = {k: [] for k in legs_}
    for _ in range(rounds):
        for k, leg in legs_.items():
            ms[k].append(round(leg.block(steps), 4))
    old, new = statistics.median(ms['per_event']), statistics.median(ms['tiled'])
    return dict(kind='step', weight=weight, steps_per_block=steps, per_event_ms=ms['per_event'], tiled_ms=ms['tiled'],
                per_event_median_ms=old, tiled_median_ms=new, saved_ms=round(old - new, 4))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--events-per-frame', type=int, nargs='+', default=list(EVENTS_PER_FRAME))
    ap.add_argument('--kinds', nargs='+', default=['term', 'metric', 'step'], choices=('term', 'metric', 'step'))
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--weight', type=float, default=0.5)
    args = ap.parse_args(argv)
    for kind in args.kinds:
        if kind == 'step':
            print(json.dumps(step(args.weight, args.rounds)), flush=True)
            continue
        for per_frame in args.events_per_frame:
            for mask, pol in OPTIONS:
                print(json.dumps(legs(kind, per_frame, mask, pol, rounds=args.rounds, reps=args.reps)), flush=True)


if __name__ == '__main__':
    main()
