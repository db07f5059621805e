#!/usr/bin/env python3
"""Cost of the contrast term on every flow scale (docs/CONTRAST_SPEC.md
sections 19-23), one JSON line (profiles/contrast_pyramid/README.md).  Batch
8, 256x256, the four levels 256, 128, 64, 32 of the network, 65 536 events
per sample; all three references with polarity, and the defaults (start,
no polarity).

  calls   dvsof_contrast_pyramid_fwd / _bwd against four calls of
          dvsof_contrast_multi_fwd / _bwd on columns shifted beforehand (the
          one-level code of the same library): HIP events around blocks of
          launches, the forms taking turns block by block within one run, the
          median block of each; beside the device time the host time spent
          issuing a call (the queue is empty when a block starts, twenty calls
          do not fill it).  The two forms are compared byte for byte
          once before anything is timed.
  levels  the pyramid forward with a table of ONE level, per level: what a
          level costs alone (its fill, splat, statistics and closing wave) and
          its share of the sum of the four.
  step    one eager training step (Ranger, f32, process_minibatch +
          unit_backward + step) of a frameless batch with contrast_scales
          'all' against 'finest', in alternating blocks of one run.
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
from dvs_of_training_framework_amd import _lib, loss as L, optim, synthetic  # noqa: E402
from dvs_of_training_framework_amd.loss import init_losses, unit_backward  # noqa: E402
from dvs_of_training_framework_amd.net import Model  # noqa: E402
from dvs_of_training_framework_amd.timer import FakeTimer  # noqa: E402
from dvs_of_training_framework_amd.training import process_minibatch  # noqa: E402

B, H, W, BINS, EVENTS = 8, 256, 256, 5, 65536
SHAPES = ((32, 32), (64, 64), (128, 128), (256, 256))      # the network's order: coarsest first


def block_us(fn, reps):
    """-> (device us per call between two HIP events, host us per call spent issuing it)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = time.perf_counter() - t0
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, host * 1e6 / reps


def check(rc):
    assert rc == 0, rc


class Pyramid:
    """The buffers and the two calls of one level table."""

    def __init__(self, d, flows, shapes, mask, pol, weights):
        dev, self.lib, self.stream = 'cuda', _lib.lib(), _lib.stream()
        F, K = B, len(shapes)
        self.M = M = F * bin(mask).count('1') * (1 + pol)
        self.grads = [torch.empty_like(f) for f in flows]
        self.table = L.contrast_level_table((H, W), shapes, F, M, weights, [f.data_ptr() for f in flows],
                                            [g.data_ptr() for g in self.grads])
        self.need = self.lib.dvsof_contrast_pyramid_workspace_bytes(F, mask, pol, H, W, self.table)
        assert self.need > 0
        self.ws = torch.empty(self.need // 8, dtype=torch.long, device=dev)
        self.rows = torch.empty(K * M, 48, dtype=torch.uint8, device=dev)
        self.terms, self.value = torch.empty(K, device=dev), torch.empty((), device=dev)
        self.seed = torch.ones((), device=dev)
        self.head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [d['x'].numel()] + \
            [d['ts'].data_ptr(), d['fs'].data_ptr(), F, H, W, mask, pol]
        self.pixels = sum(h * w for h, w in shapes)

    def fwd(self):
        check(self.lib.dvsof_contrast_pyramid_fwd(*self.head, self.table, self.rows.data_ptr(),
                                                  self.terms.data_ptr(), self.value.data_ptr(), self.ws.data_ptr(),
                                                  self.need, self.stream))

    def bwd(self):
        check(self.lib.dvsof_contrast_pyramid_bwd(*self.head, self.table, self.ws.data_ptr(), self.need,
                                                  self.seed.data_ptr(), self.stream))

    def q(self):
        return self.ws[:self.M * self.pixels]


class FourCalls:
    """dvsof_contrast_multi_fwd / _bwd once per level on columns shifted beforehand."""

    def __init__(self, d, flows, shapes, mask, pol, weights):
        dev, self.lib, self.stream = 'cuda', _lib.lib(), _lib.stream()
        F = B
        M = F * bin(mask).count('1') * (1 + pol)
        self.levels = []
        self.seed = torch.ones((), device=dev)
        inside = (d['x'] >= 0) & (d['x'] < W) & (d['y'] >= 0) & (d['y'] < H)
        for flow, (h, w), weight in zip(flows, shapes, weights):
            s = L.contrast_level_shift((H, W), (h, w))
            x = torch.where(inside, d['x'] >> s, torch.full_like(d['x'], -1)).contiguous()
            y = torch.where(inside, d['y'] >> s, torch.full_like(d['y'], -1)).contiguous()
            need = self.lib.dvsof_contrast_multi_workspace_bytes(F, mask, pol, h, w)
            lev = dict(x=x, y=y, q=torch.empty(M, h, w, dtype=torch.long, device=dev),
                       count=torch.empty(M, h, w, dtype=torch.int32, device=dev),
                       rows=torch.empty(M, 48, dtype=torch.uint8, device=dev), term=torch.empty((), device=dev),
                       ws=torch.empty(need // 8, dtype=torch.long, device=dev), need=need,
                       grad=torch.empty_like(flow), weight=float(weight))
            lev['head'] = [x.data_ptr(), y.data_ptr(), d['t'].data_ptr(), d['p'].data_ptr(), d['s'].data_ptr(),
                           x.numel(), d['ts'].data_ptr(), d['fs'].data_ptr(), flow.data_ptr(), F, h, w, mask, pol]
            self.levels.append(lev)

    def fwd(self):
        for v in self.levels:
            check(self.lib.dvsof_contrast_multi_fwd(*v['head'], v['q'].data_ptr(), v['count'].data_ptr(),
                                                    v['rows'].data_ptr(), v['term'].data_ptr(), v['ws'].data_ptr(),
                                                    v['need'], self.stream))

    def bwd(self):
        for v in self.levels:
            check(self.lib.dvsof_contrast_multi_bwd(*v['head'], v['q'].data_ptr(), v['ws'].data_ptr(), v['need'],
                                                    self.seed.data_ptr(), v['weight'], v['grad'].data_ptr(),
                                                    self.stream))


def calls(rounds, reps, seed=0):
    dev = 'cuda'
    batch = synthetic.make_batch(seed, B, H, W, EVENTS)
    ev = batch['events']
    rng = np.random.default_rng(seed)
    c = dict(x=ev['x'], y=ev['y'], t=ev['timestamp'], p=ev['polarity'], s=ev['sample_index'],
             ts=np.tile(np.array([0, synthetic.WINDOW], np.float32), B), fs=np.arange(B, dtype=np.int64))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.items()}
    # sigma 3 pixels at full size, halved with every level
    flows = [torch.from_numpy(rng.normal(0, 3.0 * h / H, (B, 2, h, w)).astype(np.float32)).to(dev)
             for h, w in SHAPES]
    weights = L.contrast_level_weights(0.25, len(SHAPES))
    out = dict(events=int(d['x'].numel()), rounds=rounds, reps=reps)
    for tag, mask, pol in (('all_polarity', 7, 1), ('default', 1, 0)):
        one, four = Pyramid(d, flows, SHAPES, mask, pol, weights), FourCalls(d, flows, SHAPES, mask, pol, weights)
        forms = {'pyramid_fwd': one.fwd, 'four_fwd': four.fwd, 'pyramid_bwd': one.bwd, 'four_bwd': four.bwd}
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # the same bytes from both forms, before anything is timed
        assert torch.equal(one.q(), torch.cat([v['q'].reshape(-1) for v in four.levels]))
        assert torch.equal(one.terms, torch.stack([v['term'] for v in four.levels]))
        for g, v in zip(one.grads, four.levels):
            assert torch.equal(g, v['grad']) and bool(g.any())
        singles = {}
        for k, shape in enumerate(SHAPES):
            singles[f'{shape[0]}x{shape[1]}'] = Pyramid(d, flows[k:k + 1], (shape,), mask, pol, weights[k:k + 1]).fwd
        for fn in singles.values():
            fn()
        blocks = {k: [] for k in list(forms) + list(singles)}
        for _ in range(rounds):
            for k, fn in {**forms, **singles}.items():
                blocks[k].append(block_us(fn, reps))
        med = {k: statistics.median(u for u, _ in v) for k, v in blocks.items()}
        leg = {k: dict(us=round(med[k], 2), min_us=round(min(u for u, _ in blocks[k]), 2),
                       max_us=round(max(u for u, _ in blocks[k]), 2),
                       host_us=round(statistics.median(h for _, h in blocks[k]), 2)) for k in forms}
        leg['fwd_ratio_to_four_calls'] = round(med['pyramid_fwd'] / med['four_fwd'], 4)
        leg['bwd_ratio_to_four_calls'] = round(med['pyramid_bwd'] / med['four_bwd'], 4)
        total = sum(med[k] for k in singles)
        leg['one_level_fwd'] = {k: dict(us=round(med[k], 2), share=round(med[k] / total, 4)) for k in singles}
        leg['terms'] = [float(v) for v in one.terms]
        out[tag] = leg
    return out


class Leg:
    def __init__(self, scales):
        torch.manual_seed(1234)
        self.model = Model('cuda', event_representation_depth=BINS).train()
        self.opt = optim.FusedRanger(self.model.predictor.parameters(), lr=1e-3, weight_decay=1e-4)
        self.losses = init_losses((H, W), B, self.model, 'cuda', sequence_length=1)
        self.batches = [dict(synthetic.to_torch(synthetic.make_batch(1234 + 1000 * i, B, H, W, EVENTS), 'cuda'),
                             images=None, shape=(H, W)) for i in range(2)]
        self.extra = {'contrast_weight': 0.25}
        if scales != 'finest':
            self.extra['contrast_scales'] = scales
        self.i = 0

    def step(self):
        batch = self.batches[self.i % 2]
        self.i += 1
        loss, _, _ = process_minibatch(self.model, batch, FakeTimer(), 'cuda', True, self.losses, [0.5, 1, 1],
                                       **self.extra)
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


def step_finest_against_all(rounds, steps=30, warmup=15):
    legs = {'finest': Leg('finest'), 'all': Leg('all')}
    for leg in legs.values():
        leg.block(warmup)
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, leg in legs.items():
            ms[k].append(round(leg.block(steps), 4))
    finest, every = statistics.median(ms['finest']), statistics.median(ms['all'])
    return dict(finest_ms=ms['finest'], all_ms=ms['all'], finest_median_ms=finest, all_median_ms=every,
                added_ms=round(every - finest, 4), added_share=round((every - finest) / finest, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-step', action='store_true', help='the calls alone')
    args = ap.parse_args()
    out = dict(shape=dict(B=B, H=H, W=W, bins=BINS, events_per_sample=EVENTS, levels=[list(s) for s in SHAPES]),
               calls=calls(args.rounds, args.reps))
    if not args.no_step:
        out['step'] = step_finest_against_all(args.rounds)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
