#!/usr/bin/env python3
"""The gradient-magnitude objective of the contrast term
(include/dvsof_contrast_gradient.h) against the variance objective
(dvsof_contrast_multi_fwd / _bwd), one JSON line per option set and call
(profiles/contrast_gradient/README.md).

8 frames of 256x256 with 524 288 events; the default options (start, the
polarities together) and start,middle,end with the polarities apart.  HIP
events around blocks of launches, the two legs taking turns block by block
within one run.  Reported per call: the median block of either leg with its
smallest and largest block in microseconds, and the ratio.  The two objectives
compute different terms, so nothing is compared but the images q and count,
which are the same bytes.

  --sink  no device: the term of either objective on the sink flow of
          docs/CONTRAST_SPEC.md section 10 at start, middle and end, from the
          float64 definitions of the tests.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dvs_of_training_framework_amd import _lib  # noqa: E402

OPTIONS = ((1, 0), (7, 1))      # (reference mask, polarity)


def legs(n, mask, pol, F=8, side=256, rounds=7, reps=20, seed=0):
    from tools.iwe_bench import block_us
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    rng = np.random.default_rng(seed)
    per_frame = n // F
    cols = dict(x=rng.integers(0, side, n), y=rng.integers(0, side, n),
                t=np.sort(rng.random((F, per_frame)), 1).reshape(-1).astype(np.float32),
                p=rng.choice(np.array([-1, 1], np.int64), n), s=np.repeat(np.arange(F, dtype=np.int64), per_frame),
                ts=np.tile(np.array([0, 1], np.float32), F), fs=np.arange(F, dtype=np.int64),
                flow=rng.normal(0, 3, (F, 2, side, side)).astype(np.float32))
    d = {k: torch.from_numpy(v).to(dev) for k, v in cols.items()}
    M = lib.dvsof_iwe_multi_images(F, mask, pol)
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [
        n, d['ts'].data_ptr(), d['fs'].data_ptr(), d['flow'].data_ptr(), F, side, side, mask, pol]
    need = {'variance': lib.dvsof_contrast_multi_workspace_bytes(F, mask, pol, side, side),
            'gradient': lib.dvsof_contrast_gradient_workspace_bytes(F, mask, pol, side, side)}
    b = {leg: dict(q=torch.empty(M, side, side, dtype=torch.long, device=dev),
                   count=torch.empty(M, side, side, dtype=torch.int32, device=dev),
                   rows=torch.empty(M, 48, dtype=torch.uint8, device=dev), term=torch.empty((), device=dev),
                   ws=torch.empty(need[leg] // 8, dtype=torch.long, device=dev),
                   grad=torch.empty(F, 2, side, side, device=dev)) for leg in need}
    seed_one = torch.ones((), device=dev)

    def fwd(leg):
        o = b[leg]
        out = [o['q'].data_ptr(), o['count'].data_ptr()] + ([o['rows'].data_ptr()] if leg == 'variance' else [])
        name = 'dvsof_contrast_multi_fwd' if leg == 'variance' else 'dvsof_contrast_gradient_fwd'
        assert getattr(lib, name)(*head, *out, o['term'].data_ptr(), o['ws'].data_ptr(), need[leg], stream) == 0

    def bwd(leg):
        o = b[leg]
        name = 'dvsof_contrast_multi_bwd' if leg == 'variance' else 'dvsof_contrast_gradient_bwd'
        assert getattr(lib, name)(*head, o['q'].data_ptr(), o['ws'].data_ptr(), need[leg], seed_one.data_ptr(), 0.25,
                                  o['grad'].data_ptr(), stream) == 0

    calls = {(call.__name__, leg): (lambda call=call, leg=leg: call(leg)) for call in (fwd, bwd) for leg in need}
    for call in calls.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    assert torch.equal(b['variance']['q'], b['gradient']['q']) and torch.equal(b['variance']['count'],
                                                                               b['gradient']['count'])
    assert all(bool(o['grad'].any()) and bool(torch.isfinite(o['term'])) for o in b.values())
    blocks = {k: [] for k in calls}
    for _ in range(rounds):
        for k, call in calls.items():
            blocks[k].append(block_us(call, reps))
    res = dict(events=n, frames=F, side=side, mask=mask, polarity=pol, images=M,
               workspace_mib={k: round(v / 2 ** 20, 1) for k, v in need.items()},
               terms={k: float(o['term']) for k, o in b.items()})
    for (call, leg), v in blocks.items():
        res[f'{call}_{leg}'] = dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2),
                                    max_us=round(max(v), 2))
    for call in ('fwd', 'bwd'):
        res[f'{call}_gradient_over_variance'] = round(res[f'{call}_gradient']['us'] / res[f'{call}_variance']['us'], 3)
    return res


def sink():
    from tests import contrast_multi_cases as mc
    from tests.test_gpu_contrast_gradient import definition
    c = mc.sink_case()
    out = dict(kind='sink')
    for name, mask in (('start', 1), ('middle', 2), ('end', 4)):
        out[name] = dict(variance=round(mc.oracle64(c, mask, False)['term'], 4),
                         gradient=round(definition(c, mask, False)['term'], 4))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--events', type=int, default=524288)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sink', action='store_true')
    args = ap.parse_args(argv)
    if args.sink:
        print(json.dumps(sink()), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit('the timing needs the GPU; --sink runs without one')
    for mask, pol in OPTIONS:
        print(json.dumps(legs(args.events, mask, pol, rounds=args.rounds, reps=args.reps)), flush=True)


if __name__ == '__main__':
    main()
