#!/usr/bin/env python3
"""The tiled schedule of the forward splat of the two events-only terms on every
flow scale against the per-event kernels (include/dvsof_event_pyramids_tiled.h),
one JSON line per shape and one per training step
(profiles/event_pyramids_tiled/README.md).

8 frames of 256x256 with the default network's four levels (32, 64, 128, 256
square) and 2 000, 8 000, 30 000, 65 536 (the benchmark batch) and 120 000
events per frame, at start without polarity and at start,middle,end with the
polarities apart:

  contrast       dvsof_contrast_pyramid_fwd against dvsof_contrast_pyramid_fwd_tiled
  avg_timestamp  dvsof_avg_timestamp_pyramid_fwd against its _tiled twin
                 (mode 1): the whole forward, of which only the splat differs

HIP events around blocks of launches, the two legs taking turns block by block
within one run, after a bitwise comparison of the whole workspace and the
outputs.  Reported: the median block of either leg, the spread of the block
means, the ratio, and whether the tiled leg wins by more than either spread.
The time of pass 1, the fold and pass 2 alone is read from a kernel trace of
this tool at one shape (--kinds contrast --events-per-frame 65536).

  step  one eager Ranger step of a frameless benchmark batch with
        --contrast-scales all, and with --avg-timestamp-scales all beside it,
        the splats per event against event_pyramids_tiled='force', in
        alternating blocks of one run.
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L  # noqa: E402
from tools.iwe_bench import CROP, block_us  # noqa: E402

OPTIONS = ((1, 0), (7, 1))      # start; start, middle, end with the polarities apart
EVENTS_PER_FRAME = (2000, 8000, 30000, 65536, 120000)
SHIFTS = (3, 2, 1, 0)           # the network's order: coarsest first


def legs(family, per_frame, mask, pol, F=8, side=CROP, rounds=7, reps=40, seed=0):
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    rng = np.random.default_rng(seed)
    n = F * per_frame
    shapes = [(-(-side // 2 ** s),) * 2 for s in SHIFTS]
    cols = dict(x=rng.integers(0, side, n), y=rng.integers(0, side, n),
                t=np.sort(rng.random((F, per_frame)), 1).reshape(-1).astype(np.float32),
                p=rng.choice(np.array([-1, 1], np.int64), n), s=np.repeat(np.arange(F, dtype=np.int64), per_frame),
                ts=np.tile(np.array([0, 1], np.float32), F), fs=np.arange(F, dtype=np.int64))
    d = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
    flows = [torch.from_numpy(rng.normal(0, 3 / 2 ** s, (F, 2) + shape).astype(np.float32)).to(dev)
             for s, shape in zip(SHIFTS, shapes)]
    M = lib.dvsof_iwe_multi_images(F, mask, pol)
    table = L.contrast_level_table((side, side), shapes, F, M, L.contrast_level_weights(0.5, len(shapes)),
                                   [f.data_ptr() for f in flows])
    tiles, tile_bytes = dev_eval.event_pyramids_tiled_workspace(family, F, mask, pol, side, side, table, n, dev)
    assert tiles is not None, 'the plan is refused at this shape'
    plan = (ctypes.c_int32 * (6 + 3 * len(shapes)))()
    assert lib.dvsof_event_pyramids_tiled_plan(F, mask, pol, side, side, table, n, plan) == 1
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n, d['ts'].data_ptr(), d['fs'].data_ptr(),
                                                                   F, side, side, mask, pol, table]
    name = f'dvsof_{family}_pyramid'
    need = getattr(lib, name + '_workspace_bytes')(F, mask, pol, side, side, table)
    out = {leg: (torch.empty(need // 8, dtype=torch.long, device=dev), torch.empty(len(shapes) * M * 6 + 8, device=dev,
                                                                                   dtype=torch.long))
           for leg in ('old', 'tiled')}
    fwd, fwd_tiled = getattr(lib, name + '_fwd'), getattr(lib, name + '_fwd_tiled')

    def call(leg):
        ws, rest = out[leg]     # rest: the result rows (contrast), then the terms and the value
        outputs = ([rest.data_ptr()] if family == 'contrast' else []) + \
            [rest[-8:].data_ptr(), rest[-4:].data_ptr(), ws.data_ptr(), need, stream]
        rc = fwd(*head, *outputs) if leg == 'old' else fwd_tiled(*head, *outputs, tiles.data_ptr(), tile_bytes, 1)
        assert rc == 0, rc

    for leg in out:
        out[leg][1].zero_()
        for _ in range(3):
            call(leg)
    torch.cuda.synchronize()
    lay = L.avg_timestamp_pyramid_layout(F, M, shapes)
    whole = lay['part'] // 8 if family == 'avg_timestamp' else need // 8    # behind `part`: scratch of the statistics
    assert torch.equal(out['old'][0][:whole], out['tiled'][0][:whole]), 'the tiled call\'s workspace differs'
    assert torch.equal(out['old'][1], out['tiled'][1]) and bool(out['tiled'][0][:8 * M].any())
    blocks = {leg: [] for leg in out}
    for _ in range(rounds):
        for leg in out:
            blocks[leg].append(block_us(lambda: call(leg), reps))
    res = dict(kind=family, events_per_frame=per_frame, reference_mask=mask, polarity=pol, images=M,
               tiles=int(plan[2]), slice=int(plan[3]), aggregate_tiles=int(plan[4]),
               levels=[[int(v) for v in plan[6 + 3 * k:9 + 3 * k]] for k in range(len(shapes))],
               tile_workspace_mib=round(tile_bytes / 2 ** 20, 1))
    for leg, v in blocks.items():
        res[leg] = dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    res['tiled_over_old'] = round(res['tiled']['us'] / res['old']['us'], 3)
    spread = max(res[leg]['max_us'] - res[leg]['min_us'] for leg in out)
    res['wins_by_more_than_the_spread'] = bool(res['old']['us'] - res['tiled']['us'] > spread)
    return res


def step(both, rounds, steps=30, warmup=15):
    from tools.avg_timestamp_bench import H, W, Leg
    extra = {'contrast_weight': 0.25, 'contrast_scales': 'all'}
    if both:
        extra.update(avg_timestamp_weight=0.5, avg_timestamp_scales='all')
    legs_ = {'per_event': Leg(0.0), 'tiled': Leg(0.0)}
    for k, leg in legs_.items():
        leg.batches = [dict(b, images=None, shape=(H, W)) for b in leg.batches]
        leg.extra = dict(extra, **({'event_pyramids_tiled': 'force'} if k == 'tiled' else {}))
        leg.block(warmup)
    ms = {k: [] for k in legs_}
    for _ in range(rounds):
        for k, leg in legs_.items():
            ms[k].append(round(leg.block(steps), 4))
    old, new = statistics.median(ms['per_event']), statistics.median(ms['tiled'])
    return dict(kind='step', terms='contrast+avg_timestamp' if both else 'contrast', steps_per_block=steps,
                per_event_ms=ms['per_event'], tiled_ms=ms['tiled'], per_event_median_ms=old, tiled_median_ms=new,
                saved_ms=round(old - new, 4))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--events-per-frame', type=int, nargs='+', default=list(EVENTS_PER_FRAME))
    ap.add_argument('--kinds', nargs='+', default=['contrast', 'avg_timestamp', 'step'],
                    choices=('contrast', 'avg_timestamp', 'step'))
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=40)
    args = ap.parse_args(argv)
    for kind in args.kinds:
        if kind == 'step':
            for both in (False, True):
                print(json.dumps(step(both, args.rounds)), flush=True)
            continue
        for per_frame in args.events_per_frame:
            for mask, pol in OPTIONS:
                print(json.dumps(legs(kind, per_frame, mask, pol, rounds=args.rounds, reps=args.reps)), flush=True)


if __name__ == '__main__':
    main()
