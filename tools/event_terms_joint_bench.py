#!/usr/bin/env python3
"""The joint calls of the two events-only terms (include/dvsof_event_terms_joint.h)
against the four calls they stand for, one JSON line per shape and one per
training step (profiles/event_terms_joint/README.md).

8 frames of 256x256 with the default network's four levels (32, 64, 128, 256
square) and with the finest level alone; 16 000, 64 000, 240 000, 524 288 (the
benchmark batch) and 960 000 events; the default options (contrast at start,
average timestamp at start,end) and start,middle,end with the polarities apart
for both; the splat per event and tiled (mode 1):

  twins  dvsof_contrast_pyramid_fwd, dvsof_avg_timestamp_pyramid_fwd (their
         _tiled twins in the tiled rows), dvsof_contrast_pyramid_bwd,
         dvsof_avg_timestamp_pyramid_bwd
  joint  dvsof_event_terms_joint_fwd, dvsof_event_terms_joint_bwd

HIP events around blocks of launches, the two legs taking turns block by block
within one run, after a bitwise comparison of the contrast rows, both terms'
terms and values and both sets of gradients.  Reported: the median block of
either leg with its smallest and largest block, the ratio, and whether the
joint leg wins by more than either spread.

  step  one eager Ranger step of a frameless benchmark batch with both terms on
        every flow scale, event_terms_joint off against on, per event and with
        event_pyramids_tiled='force', in alternating blocks of one run.
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

OPTIONS = ((1, 5, 0), (7, 7, 1))    # (contrast mask, average-timestamp mask, polarity)
EVENTS = (16000, 64000, 240000, 524288, 960000)
LEVELS = ((3, 2, 1, 0), (0,))       # the network's order, coarsest first; the finest level alone


def legs(n, shifts, cmask, amask, pol, tiled, F=8, side=CROP, rounds=7, reps=20, seed=0):
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    rng = np.random.default_rng(seed)
    per_frame = n // F
    shapes = [(-(-side // 2 ** s),) * 2 for s in shifts]
    K = len(shapes)
    cols = dict(x=rng.integers(0, side, n), y=rng.integers(0, side, n),
                t=np.sort(rng.random((F, per_frame)), 1).reshape(-1).astype(np.float32),
                p=rng.choice(np.array([-1, 1], np.int64), n), s=np.repeat(np.arange(F, dtype=np.int64), per_frame),
                ts=np.tile(np.array([0, 1], np.float32), F), fs=np.arange(F, dtype=np.int64))
    d = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
    flows = [torch.from_numpy(rng.normal(0, 3 / 2 ** s, (F, 2) + shape).astype(np.float32)).to(dev)
             for s, shape in zip(shifts, shapes)]
    ptrs = [f.data_ptr() for f in flows]
    Mc, Ma = lib.dvsof_iwe_multi_images(F, cmask, pol), lib.dvsof_iwe_multi_images(F, amask, pol)
    seed_one = torch.ones((), device=dev)
    mode = 1 if tiled else -1

    class Side:     # the buffers of one leg: gradients and tables of both terms, the outputs
        def __init__(self):
            self.grads = [torch.empty_like(f) for f in flows + flows]
            self.ctable = L.contrast_level_table((side, side), shapes, F, Mc, L.contrast_level_weights(0.25, K), ptrs,
                                                 [g.data_ptr() for g in self.grads[:K]])
            self.atable = L.contrast_level_table((side, side), shapes, F, Ma, L.contrast_level_weights(0.5, K), ptrs,
                                                 [g.data_ptr() for g in self.grads[K:]])
            self.rows = torch.zeros(K * Mc * 6, dtype=torch.long, device=dev)
            self.out = torch.zeros(2, K + 1, device=dev)

        def same(self, other):
            return torch.equal(self.rows, other.rows) and torch.equal(self.out, other.out) and \
                all(torch.equal(a, b) for a, b in zip(self.grads, other.grads))

    twins, joint = Side(), Side()
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n, d['ts'].data_ptr(), d['fs'].data_ptr(),
                                                                   F, side, side]
    need = {'contrast': lib.dvsof_contrast_pyramid_workspace_bytes(F, cmask, pol, side, side, twins.ctable),
            'avg_timestamp': lib.dvsof_avg_timestamp_pyramid_workspace_bytes(F, amask, pol, side, side, twins.atable),
            'joint': lib.dvsof_event_terms_joint_workspace_bytes(F, cmask, amask, pol, side, side, joint.ctable,
                                                                 joint.atable)}
    ws = {k: torch.empty(v // 8, dtype=torch.long, device=dev) for k, v in need.items()}
    tiles = {k: dev_eval.event_pyramids_tiled_workspace(k, F, mask, pol, side, side, table, n, dev)
             for k, mask, table in (('contrast', cmask, twins.ctable), ('avg_timestamp', amask, twins.atable))} \
        if tiled else {}
    assert all(t[0] is not None for t in tiles.values()), 'the plan is refused at this shape'
    tail = {k: [t[0].data_ptr(), t[1], 1] for k, t in tiles.items()}
    form = '_tiled' if tiled else ''

    def call_twins():
        o = twins
        rcs = [getattr(lib, 'dvsof_contrast_pyramid_fwd' + form)(
                   *head, cmask, pol, o.ctable, o.rows.data_ptr(), o.out[0].data_ptr(), o.out[0, K:].data_ptr(),
                   ws['contrast'].data_ptr(), need['contrast'], stream, *tail.get('contrast', [])),
               getattr(lib, 'dvsof_avg_timestamp_pyramid_fwd' + form)(
                   *head, amask, pol, o.atable, o.out[1].data_ptr(), o.out[1, K:].data_ptr(),
                   ws['avg_timestamp'].data_ptr(), need['avg_timestamp'], stream, *tail.get('avg_timestamp', [])),
               lib.dvsof_contrast_pyramid_bwd(*head, cmask, pol, o.ctable, ws['contrast'].data_ptr(),
                                              need['contrast'], seed_one.data_ptr(), stream),
               lib.dvsof_avg_timestamp_pyramid_bwd(*head, amask, pol, o.atable, ws['avg_timestamp'].data_ptr(),
                                                   need['avg_timestamp'], seed_one.data_ptr(), stream)]
        assert rcs == [0] * 4, rcs

    def call_joint():
        o = joint
        rcs = [lib.dvsof_event_terms_joint_fwd(
                   *head, cmask, amask, pol, o.ctable, o.atable, o.rows.data_ptr(), o.out[0].data_ptr(),
                   o.out[0, K:].data_ptr(), o.out[1].data_ptr(), o.out[1, K:].data_ptr(), ws['joint'].data_ptr(),
                   need['joint'], stream, *(tail['avg_timestamp'][:2] if tiled else [None, 0]), mode),
               lib.dvsof_event_terms_joint_bwd(*head, cmask, amask, pol, o.ctable, o.atable, ws['joint'].data_ptr(),
                                               need['joint'], seed_one.data_ptr(), seed_one.data_ptr(), stream)]
        assert rcs == [0] * 2, rcs

    calls = {'twins': call_twins, 'joint': call_joint}
    for call in calls.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    assert twins.same(joint), 'the joint calls\' outputs differ from the twins\''
    assert bool(joint.rows.any()) and all(bool(g.any()) for g in joint.grads)
    blocks = {leg: [] for leg in calls}
    for _ in range(rounds):
        for leg, call in calls.items():
            blocks[leg].append(block_us(call, reps))
    res = dict(kind='calls', events=n, levels=K, contrast_mask=cmask, avg_timestamp_mask=amask, polarity=pol,
               schedule='tiled' if tiled else 'per_event',
               workspace_mib={k: round(v / 2 ** 20, 1) for k, v in need.items()})
    for leg, v in blocks.items():
        res[leg] = dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    res['joint_over_twins'] = round(res['joint']['us'] / res['twins']['us'], 3)
    spread = max(res[leg]['max_us'] - res[leg]['min_us'] for leg in calls)
    res['wins_by_more_than_the_spread'] = bool(res['twins']['us'] - res['joint']['us'] > spread)
    res['loses_by_more_than_the_spread'] = bool(res['joint']['us'] - res['twins']['us'] > spread)
    return res


def step(tiled, rounds, steps=30, warmup=15):
    from tools.avg_timestamp_bench import H, W, Leg
    extra = dict(contrast_weight=0.25, contrast_scales='all', avg_timestamp_weight=0.5, avg_timestamp_scales='all',
                 **({'event_pyramids_tiled': 'force'} if tiled else {}))
    legs_ = {'off': Leg(0.0), 'on': Leg(0.0)}
    for k, leg in legs_.items():
        leg.batches = [dict(b, images=None, shape=(H, W)) for b in leg.batches]
        leg.extra = dict(extra, **({'event_terms_joint': True} if k == 'on' else {}))
        leg.block(warmup)
    ms = {k: [] for k in legs_}
    for _ in range(rounds):
        for k, leg in legs_.items():
            ms[k].append(round(leg.block(steps), 4))
    off, on = statistics.median(ms['off']), statistics.median(ms['on'])
    return dict(kind='step', schedule='tiled' if tiled else 'per_event', steps_per_block=steps, off_ms=ms['off'],
                on_ms=ms['on'], off_median_ms=off, on_median_ms=on, saved_ms=round(off - on, 4),
                on_over_off=round(on / off, 3))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--events', type=int, nargs='+', default=list(EVENTS))
    ap.add_argument('--kinds', nargs='+', default=['calls', 'step'], choices=('calls', 'step'))
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args(argv)
    if 'calls' in args.kinds:
        for shifts in LEVELS:
            for n in args.events:
                for cmask, amask, pol in OPTIONS:
                    for tiled in (False, True):
                        print(json.dumps(legs(n, shifts, cmask, amask, pol, tiled, rounds=args.rounds,
                                              reps=args.reps)), flush=True)
    if 'step' in args.kinds:
        for tiled in (False, True):
            print(json.dumps(step(tiled, args.rounds)), flush=True)


if __name__ == '__main__':
    main()
