#!/usr/bin/env python3
"""The census term (include/dvsof_census.h) at batch 8, 256x256, four scales,
one JSON line per leg (profiles/census/README.md).

  calls   dvsof_census_fwd and dvsof_census_bwd alone, beside dvsof_loss_fused
          (forward and gradient of the three reference terms in one sweep) and
          dvsof_loss_pyramid (the launch ``Losses.census`` adds beside the fused
          loss's own pyramid) on the same frames and flows: HIP events around
          blocks of calls, the legs taking turns block by block within one run;
          per leg the median block with its smallest and largest, microseconds.
  step    one eager training step (Ranger, f32, process_minibatch + backward +
          optimizer) with and without --census-weight, in alternating blocks
          timed by a host clock around a device synchronise.
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dvs_of_training_framework_amd import _lib, loss as L  # noqa: E402

B, D, SIDE = 8, 16, 256
SHAPES = ((32, 32), (64, 64), (128, 128), (256, 256))      # the network's order: coarsest first


def calls_alone(rounds=9, reps=40, seed=0):
    from tools.avg_timestamp_bench import block_us
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (D, SIDE, SIDE), generator=g).float().to(dev)
    flows = [(torch.randn(B, 2, h, w, generator=g) * 2 * h / SIDE).to(dev) for h, w in SHAPES]
    start = torch.arange(0, 2 * B, 2, dtype=torch.int32, device=dev)
    stop = start + 1
    losses = L.Losses(SHAPES, B, dev)
    frames = losses._pyramid(flows, images)
    grads = [torch.empty_like(f) for f in flows]
    arr, K = L._scale_array(frames, flows, grads), len(SHAPES)
    need = dict(census=lib.dvsof_census_workspace_bytes(arr, K, B), fused=lib.dvsof_loss_workspace_bytes(arr, K, B))
    ws = {k: torch.empty(v // 4, device=dev) for k, v in need.items()}
    terms, value, seed_one = torch.empty(K, device=dev), torch.empty((), device=dev), torch.ones((), device=dev)
    fused_terms, oob = torch.empty(3, K, device=dev), torch.empty(K * B, dtype=torch.int32, device=dev)
    weights = (ctypes.c_float * 3)(0.5, 1.0, 1.0)
    levels = (ctypes.c_void_p * K)(*[f.data_ptr() for f in frames])
    hs, wd = (ctypes.c_int * K)(*[s[0] for s in SHAPES]), (ctypes.c_int * K)(*[s[1] for s in SHAPES])

    def census_fwd():
        assert lib.dvsof_census_fwd(arr, K, B, start.data_ptr(), stop.data_ptr(), 0.25, terms.data_ptr(),
                                    value.data_ptr(), ws['census'].data_ptr(), need['census'], stream) == 0

    def census_bwd():
        assert lib.dvsof_census_bwd(arr, K, B, start.data_ptr(), stop.data_ptr(), seed_one.data_ptr(),
                                    ws['census'].data_ptr(), need['census'], stream) == 0

    def loss_fused():
        assert lib.dvsof_loss_fused(arr, K, B, start.data_ptr(), stop.data_ptr(), weights, 1.0,
                                    fused_terms.data_ptr(), value.data_ptr(), oob.data_ptr(),
                                    ws['fused'].data_ptr(), need['fused'], stream) == 0

    def loss_pyramid():
        assert lib.dvsof_loss_pyramid(images.data_ptr(), D, SIDE, SIDE, levels, hs, wd, K, stream) == 0

    calls = {f.__name__: f for f in (census_fwd, census_bwd, loss_fused, loss_pyramid)}
    for call in calls.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(terms).all()) and all(bool(g.any()) for g in grads)
    blocks = {k: [] for k in calls}
    for _ in range(rounds):
        for k, call in calls.items():
            blocks[k].append(block_us(call, reps))
    pixels = sum(B * h * w for h, w in SHAPES)
    out = dict(kind='calls', batch=B, shapes=SHAPES, pixels=pixels, pairs=48 * pixels,
               workspace_mib=round(need['census'] / 2 ** 20, 2), terms=[round(t, 4) for t in terms.tolist()])
    for k, v in blocks.items():
        out[k] = dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
    return out


def step_with_and_without(weight, rounds=7, steps=30, warmup=15):
    from tools import avg_timestamp_bench as ab

    class Leg(ab.Leg):
        def __init__(self, w):
            super().__init__(0.0)
            self.extra = {'census_weight': w} if w else {}
    legs = {'without': Leg(0.0), 'with': Leg(weight)}
    for leg in legs.values():
        leg.block(warmup)
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, leg in legs.items():
            ms[k].append(round(leg.block(steps), 4))
    off, on = statistics.median(ms['without']), statistics.median(ms['with'])
    return dict(kind='step', weight=weight, steps_per_block=steps, without_ms=ms['without'], with_ms=ms['with'],
                without_median_ms=off, with_median_ms=on, added_ms=round(on - off, 4),
                added_share=round((on - off) / off, 4))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--weight', type=float, default=0.25)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('the timing needs the GPU')
    print(json.dumps(calls_alone(args.rounds, args.reps)), flush=True)
    if not args.no_step:
        print(json.dumps(step_with_and_without(args.weight)), flush=True)


if __name__ == '__main__':
    main()
