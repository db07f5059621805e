#!/usr/bin/env python3
"""Cost of the loss that reads no frame (docs/FRAMELESS_SPEC.md), one JSON line
(profiles/frameless/README.md).  Batch 8, 256x256, four scales, 5 bins, 65 536
events per sample.

  calls   dvsof_loss_frameless against today's workaround for a recording
          without frames -- dvsof_loss_fused_pyramid on frames of zeros with
          the photometric weight 0 -- on random flows (sigma 3 pixels): HIP
          events around blocks of launches, the two calls taking turns block
          by block within one run; the median block per call and every block
          (the spread).  Smoothness and out-of-border terms, the counts and
          the flow gradients of the two are compared once (the workaround's
          gradient adds 0 x the photometric one: equal wherever that is
          finite).
  step    one eager training step (Ranger, f32, process_minibatch +
          unit_backward + step) with --weight times the contrast term:
          a frameless batch against the framed batch of the same events with
          images of zeros and the photometric weight 0, in alternating blocks
          of one run; ms per step, the median block of each and every block.
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dvs_of_training_framework_amd import _lib, optim, synthetic  # noqa: E402
from dvs_of_training_framework_amd.loss import init_losses, unit_backward  # noqa: E402
from dvs_of_training_framework_amd.net import Model  # noqa: E402
from dvs_of_training_framework_amd.timer import FakeTimer  # noqa: E402
from dvs_of_training_framework_amd.training import process_minibatch  # noqa: E402

B, H, W, BINS, EVENTS = 8, 256, 256, 5, 65536


def block_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def calls_alone(rounds=9, reps=40, seed=0):
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    shapes = synthetic.scale_shapes(H, W)
    K, N, D = len(shapes), B, 2 * B
    flows = [torch.from_numpy(f).to(dev) for f in synthetic.make_flows(seed, N, shapes, 3.0)]

    def side():
        grads = [torch.empty_like(f) for f in flows]
        frames = [torch.empty(D, h, w, device=dev) for h, w in shapes]
        arr = (_lib.LossScale * K)()
        for k, (f, g) in enumerate(zip(flows, grads)):
            arr[k].frames, arr[k].flow, arr[k].grad_flow = frames[k].data_ptr(), f.data_ptr(), g.data_ptr()
            arr[k].h, arr[k].w = f.shape[-2:]
        return dict(grads=grads, frames=frames, arr=arr, terms=torch.empty(3, K, device=dev),
                    loss=torch.empty((), device=dev), oob=torch.empty(K * N, dtype=torch.int32, device=dev))
    new, old = side(), side()
    for k in range(K):
        new['arr'][k].frames = None
    images = torch.zeros(D, H, W, device=dev)
    start = torch.arange(0, D, 2, dtype=torch.int32, device=dev)
    stop = start + 1
    need_new = lib.dvsof_loss_frameless_workspace_bytes(new['arr'], K, N)
    need_old = lib.dvsof_loss_workspace_bytes(old['arr'], K, N)
    ws_new = torch.empty(need_new // 4, device=dev)
    ws_old = torch.empty(need_old // 4, device=dev)
    w2, w3 = (ctypes.c_float * 2)(0.5, 1.0), (ctypes.c_float * 3)(0.5, 0.0, 1.0)

    def check(rc):
        assert rc == 0, rc
    calls = {
        'frameless': lambda: check(lib.dvsof_loss_frameless(
            new['arr'], K, N, w2, 1.0, new['terms'].data_ptr(), new['loss'].data_ptr(), new['oob'].data_ptr(),
            ws_new.data_ptr(), need_new, stream)),
        'workaround': lambda: check(lib.dvsof_loss_fused_pyramid(
            images.data_ptr(), D, H, W, old['arr'], K, N, start.data_ptr(), stop.data_ptr(), w3, 1.0,
            old['terms'].data_ptr(), old['loss'].data_ptr(), old['oob'].data_ptr(), ws_old.data_ptr(), need_old,
            stream))}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the two compute the same smoothness and out-of-border terms, counts and gradients
    same = dict(terms=bool(torch.equal(new['terms'][[0, 2]], old['terms'][[0, 2]])),
                oob=bool(torch.equal(new['oob'], old['oob'])),
                grads=all(bool(torch.equal(a, b)) for a, b in zip(new['grads'], old['grads'])))
    blocks = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            blocks[k].append(block_us(fn, reps))
    flow_bytes = sum(f.numel() * 4 for f in flows)
    out = dict(rounds=rounds, reps=reps, scales=[list(s) for s in shapes], same=same,
               flow_and_gradient_bytes=2 * flow_bytes, loss=float(new['loss']))
    for k, v in blocks.items():
        out[k] = dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2),
                      blocks=[round(u, 2) for u in v])
    return out


class Leg:
    def __init__(self, frameless, weight):
        torch.manual_seed(1234)
        self.model = Model('cuda', event_representation_depth=BINS).train()
        self.opt = optim.FusedRanger(self.model.predictor.parameters(), lr=1e-3, weight_decay=1e-4)
        self.losses = init_losses((H, W), B, self.model, 'cuda', sequence_length=1)
        self.batches = [synthetic.to_torch(synthetic.make_batch(1234 + 1000 * i, B, H, W, EVENTS), 'cuda')
                        for i in range(2)]
        for batch in self.batches:
            if frameless:
                batch['images'], batch['shape'] = None, (H, W)
            else:
                batch['images'] = torch.zeros_like(batch['images'])
        self.weights = [0.5, 1, 1] if frameless else [0.5, 0, 1]
        self.weight = weight
        self.i = 0

    def step(self):
        batch = self.batches[self.i % 2]
        self.i += 1
        loss, _, _ = process_minibatch(self.model, batch, FakeTimer(), 'cuda', True, self.losses, self.weights,
                                       contrast_weight=self.weight)
        unit_backward(loss)
        self.model.strict = False
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)

    def block(self, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3


def step_framed_against_frameless(weight, rounds=7, steps=30, warmup=15):
    legs = {'workaround': Leg(False, weight), 'frameless': Leg(True, weight)}
    for leg in legs.values():
        leg.block(warmup)
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, leg in legs.items():
            ms[k].append(round(leg.block(steps), 4))
    old, new = statistics.median(ms['workaround']), statistics.median(ms['frameless'])
    return dict(weight=weight, steps_per_block=steps, workaround_ms=ms['workaround'], frameless_ms=ms['frameless'],
                workaround_median_ms=old, frameless_median_ms=new, saved_ms=round(old - new, 4),
                saved_share=round((old - new) / old, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--weight', type=float, default=0.25)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls-only', action='store_true')
    args = ap.parse_args()
    out = dict(shape=dict(B=B, H=H, W=W, bins=BINS, events_per_sample=EVENTS), calls=calls_alone())
    if not args.calls_only:
        out['step'] = step_framed_against_frameless(args.weight, args.rounds)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
