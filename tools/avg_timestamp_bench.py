#!/usr/bin/env python3
"""Cost of the average-timestamp term (docs/AVG_TIMESTAMP_SPEC.md), one JSON
line (profiles/avg_timestamp/README.md).  Batch 8, 256x256, 5 bins, 65 536
events per sample.

  calls   dvsof_avg_timestamp_fwd / _bwd alone on random flows (sigma 3
          pixels) against dvsof_contrast_multi_fwd / _bwd at the same options,
          for the default options (start,end without polarity) and for
          start,middle,end with polarity: HIP events around blocks of
          launches, the eight calls taking turns block by block within one
          run; the median block per call and every block (the spread).  q and
          count of the two are compared once, and the atomics of either
          forward counted from the restatement's arithmetic.
  step    one eager training step (Ranger, f32, process_minibatch +
          unit_backward + step) of a framed batch without the term against
          --weight times it, in alternating blocks of one run; ms per step,
          the median block of each and every block.

--scales all: the term on every flow scale (AVG_TIMESTAMP_SPEC sections 11-15;
profiles/avg_timestamp_pyramid/README.md), the four levels 32, 64, 128, 256 of
the network, at start,end without and with polarity:
  pyramid dvsof_avg_timestamp_pyramid_fwd / _bwd against four calls of
          dvsof_avg_timestamp_fwd / _bwd on columns shifted beforehand (the
          one-level entry points of the same library), compared bit for bit
          before anything is timed, then in alternating blocks of one run: the
          median block of each, the spread of the block means, the host time
          to issue a call, and the launches of either form counted from a
          capture of one forward and one backward.
  step    one eager Ranger step of a frameless batch (contrast term on the
          finest flow) with --avg-timestamp-scales finest against all.
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
OPTIONS = (('default', 5, 0), ('all_polarity', 7, 1))


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
    ev = synthetic.make_batch(seed, B, H, W, EVENTS)['events']
    rng = np.random.default_rng(seed)
    c = dict(x=ev['x'], y=ev['y'], t=ev['timestamp'], p=ev['polarity'], s=ev['sample_index'],
             ts=np.tile(np.array([0, synthetic.WINDOW], np.float32), B), fs=np.arange(B, dtype=np.int64),
             flow=rng.normal(0, 3, (B, 2, H, W)).astype(np.float32))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.items()}
    n, F = d['x'].numel(), B
    grad = torch.empty(F, 2, H, W, device=dev)
    seed_t = torch.ones((), device=dev)

    def check(rc):
        assert rc == 0, rc
    calls, held, counted = {}, {}, {}
    for tag, mask, pol in OPTIONS:
        M = F * bin(mask).count('1') * (1 + pol)
        head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n] + \
            [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, H, W, mask, pol]
        need = lib.dvsof_avg_timestamp_workspace_bytes(F, mask, pol, H, W)
        old_need = lib.dvsof_contrast_multi_workspace_bytes(F, mask, pol, H, W)
        b = held[tag] = dict(ws=torch.empty(need // 8, dtype=torch.long, device=dev), term=torch.empty((), device=dev),
                             q=torch.empty(M, H, W, dtype=torch.long, device=dev),
                             count=torch.empty(M, H, W, dtype=torch.int32, device=dev),
                             rows=torch.empty(M, 48, dtype=torch.uint8, device=dev),
                             old_term=torch.empty((), device=dev),
                             old_ws=torch.empty(old_need // 8, dtype=torch.long, device=dev), M=M)
        calls[f'{tag}_fwd'] = lambda head=head, b=b, need=need: check(lib.dvsof_avg_timestamp_fwd(
            *head, b['term'].data_ptr(), b['ws'].data_ptr(), need, stream))
        calls[f'{tag}_bwd'] = lambda head=head, b=b, need=need: check(lib.dvsof_avg_timestamp_bwd(
            *head, b['ws'].data_ptr(), need, seed_t.data_ptr(), 0.25, grad.data_ptr(), stream))
        calls[f'{tag}_contrast_fwd'] = lambda head=head, b=b, need=old_need: check(lib.dvsof_contrast_multi_fwd(
            *head, b['q'].data_ptr(), b['count'].data_ptr(), b['rows'].data_ptr(), b['old_term'].data_ptr(),
            b['old_ws'].data_ptr(), need, stream))
        calls[f'{tag}_contrast_bwd'] = lambda head=head, b=b, need=old_need: check(lib.dvsof_contrast_multi_bwd(
            *head, b['q'].data_ptr(), b['old_ws'].data_ptr(), need, seed_t.data_ptr(), 0.25, grad.data_ptr(), stream))
        # the atomics of either forward, from the restatement's arithmetic: per (event, image) one count, and
        # per corner inside the image with a positive addend one into q (both) and one into s (this term)
        fwd = L.avg_timestamp_fwd_host(c['x'], c['y'], c['t'], c['p'], c['s'], c['ts'], c['fs'], c['flow'], mask,
                                       bool(pol))
        pr = L._contrast_multi_pairs(c['x'], c['y'], c['t'], c['p'], c['s'], c['ts'], c['fs'], c['flow'], bool(pol))
        q_adds = s_adds = base_adds = 0
        for rho in L._contrast_rhos(mask):
            wp = L._contrast_warp_to(pr, rho, H, W)
            a, k = np.abs(wp['sig']), wp['inside']
            base_adds += int((a > 0).sum())
            for j in range(2):
                for i in range(2):
                    xx, yy = wp['cx'][k] + i, wp['cy'][k] + j
                    ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                    wgt = (wp['wy'][j][k] * wp['wx'][i][k]).astype(np.float32)
                    q_adds += int((ok & (wgt * np.float32(2 ** 32) >= 1)).sum())
                    s_adds += int((ok & ((wgt * a[k]).astype(np.float32) * np.float32(2 ** 32) >= 1)).sum())
        pairs = int(pr['f'].size) * bin(mask).count('1')
        counted[tag] = dict(images=M, term=float(fwd['term']), workspace_bytes=need,
                            contrast_workspace_and_image_bytes=old_need + 12 * M * H * W,
                            atomics_32bit=pairs, atomics_64bit=q_adds + s_adds + base_adds,
                            contrast_atomics_32bit=pairs, contrast_atomics_64bit=q_adds)
        held[tag]['fwd'] = fwd
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for tag, mask, pol in OPTIONS:              # the device against the restatement, and q against the contrast call
        b, lay = held[tag], L.avg_timestamp_layout(F, held[tag]['M'], H, W)
        q = b['ws'][:lay['s'] // 8].reshape(b['M'], H, W)
        assert torch.equal(q, b['q']) and np.array_equal(q.cpu().numpy(), b['fwd']['q'])
        assert b['term'].cpu().numpy().tobytes() == b['fwd']['term'].tobytes()
    blocks = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            blocks[k].append(block_us(fn, reps))
    out = dict(events=n, rounds=rounds, reps=reps, counted=counted)
    for k, v in blocks.items():
        out[k] = dict(us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2),
                      blocks=[round(u, 2) for u in v])
    return out


class Leg:
    def __init__(self, weight):
        torch.manual_seed(1234)
        self.model = Model('cuda', event_representation_depth=BINS).train()
        self.opt = optim.FusedRanger(self.model.predictor.parameters(), lr=1e-3, weight_decay=1e-4)
        self.losses = init_losses((H, W), B, self.model, 'cuda', sequence_length=1)
        self.batches = [synthetic.to_torch(synthetic.make_batch(1234 + 1000 * i, B, H, W, EVENTS), 'cuda')
                        for i in range(2)]
        self.extra = {'avg_timestamp_weight': weight} if weight else {}
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


def step_with_and_without(weight, rounds=7, steps=30, warmup=15):
    legs = {'without': Leg(0.0), 'with': Leg(weight)}
    for leg in legs.values():
        leg.block(warmup)
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, leg in legs.items():
            ms[k].append(round(leg.block(steps), 4))
    off, on = statistics.median(ms['without']), statistics.median(ms['with'])
    return dict(weight=weight, steps_per_block=steps, without_ms=ms['without'], with_ms=ms['with'],
                without_median_ms=off, with_median_ms=on, added_ms=round(on - off, 4),
                added_share=round((on - off) / off, 4))


SHAPES = ((32, 32), (64, 64), (128, 128), (256, 256))      # the network's order: coarsest first
PYRAMID_OPTIONS = (('default', 5, 0), ('polarity', 5, 1))


def block_us_host(fn, reps):
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


def ok(rc):
    assert rc == 0, rc


class Pyramid:
    """The buffers and the two calls of one level table."""

    def __init__(self, d, flows, mask, pol, weights):
        self.lib, F = _lib.lib(), B
        self.M = M = F * bin(mask).count('1') * (1 + pol)
        self.grads = [torch.empty_like(f) for f in flows]
        self.table = L.contrast_level_table((H, W), SHAPES, F, M, weights, [f.data_ptr() for f in flows],
                                            [g.data_ptr() for g in self.grads])
        self.need = self.lib.dvsof_avg_timestamp_pyramid_workspace_bytes(F, mask, pol, H, W, self.table)
        assert self.need == L.avg_timestamp_pyramid_layout(F, M, SHAPES)['bytes']
        self.ws = torch.empty(self.need // 8, dtype=torch.long, device='cuda')
        self.terms, self.value = torch.empty(len(SHAPES), device='cuda'), torch.empty((), device='cuda')
        self.seed = torch.ones((), device='cuda')
        self.head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [d['x'].numel()] + \
            [d['ts'].data_ptr(), d['fs'].data_ptr(), F, H, W, mask, pol]

    def fwd(self):
        ok(self.lib.dvsof_avg_timestamp_pyramid_fwd(*self.head, self.table, self.terms.data_ptr(),
                                                    self.value.data_ptr(), self.ws.data_ptr(), self.need,
                                                    _lib.stream()))

    def bwd(self):
        ok(self.lib.dvsof_avg_timestamp_pyramid_bwd(*self.head, self.table, self.ws.data_ptr(), self.need,
                                                    self.seed.data_ptr(), _lib.stream()))

    def images(self):
        """q, s, base of all levels: the head of the workspace."""
        return self.ws[:3 * self.M * sum(h * w for h, w in SHAPES)]


class FourCalls:
    """dvsof_avg_timestamp_fwd / _bwd once per level on columns shifted beforehand."""

    def __init__(self, d, flows, mask, pol, weights):
        self.lib, F = _lib.lib(), B
        self.M = M = F * bin(mask).count('1') * (1 + pol)
        self.levels = []
        self.seed = torch.ones((), device='cuda')
        inside = (d['x'] >= 0) & (d['x'] < W) & (d['y'] >= 0) & (d['y'] < H)
        for flow, (h, w), weight in zip(flows, SHAPES, weights):
            s_ = L.contrast_level_shift((H, W), (h, w))
            x = torch.where(inside, d['x'] >> s_, torch.full_like(d['x'], -1)).contiguous()
            y = torch.where(inside, d['y'] >> s_, torch.full_like(d['y'], -1)).contiguous()
            need = self.lib.dvsof_avg_timestamp_workspace_bytes(F, mask, pol, h, w)
            lev = dict(x=x, y=y, term=torch.empty((), device='cuda'), need=need, pixels=M * h * w,
                       ws=torch.empty(need // 8, dtype=torch.long, device='cuda'), grad=torch.empty_like(flow),
                       weight=float(weight))
            lev['head'] = [x.data_ptr(), y.data_ptr(), d['t'].data_ptr(), d['p'].data_ptr(), d['s'].data_ptr(),
                           x.numel(), d['ts'].data_ptr(), d['fs'].data_ptr(), flow.data_ptr(), F, h, w, mask, pol]
            self.levels.append(lev)

    def fwd(self):
        for v in self.levels:
            ok(self.lib.dvsof_avg_timestamp_fwd(*v['head'], v['term'].data_ptr(), v['ws'].data_ptr(), v['need'],
                                                _lib.stream()))

    def bwd(self):
        for v in self.levels:
            ok(self.lib.dvsof_avg_timestamp_bwd(*v['head'], v['ws'].data_ptr(), v['need'], self.seed.data_ptr(),
                                                v['weight'], v['grad'].data_ptr(), _lib.stream()))

    def images(self):
        """q of all levels, then s, then base: the order of the pyramid's workspace."""
        return torch.cat([v['ws'][i * v['pixels']:(i + 1) * v['pixels']] for i in range(3) for v in self.levels])


def launches_of(fn):
    """The kernel nodes of a capture of ``fn``, read through the step executor."""
    from dvs_of_training_framework_amd.capture import StepExecutor
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        fn()
    x = StepExecutor(graph, [])
    names = [n[3] for n in x.nodes() if n[3] not in ('(empty)', '?')]
    x.close()
    return len(names)


def pyramid_calls(rounds, reps, seed=0):
    ev = synthetic.make_batch(seed, B, H, W, EVENTS)['events']
    rng = np.random.default_rng(seed)
    c = dict(x=ev['x'], y=ev['y'], t=ev['timestamp'], p=ev['polarity'], s=ev['sample_index'],
             ts=np.tile(np.array([0, synthetic.WINDOW], np.float32), B), fs=np.arange(B, dtype=np.int64))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to('cuda') for k, v in c.items()}
    # sigma 3 pixels at full size, halved with every level
    flows = [torch.from_numpy(rng.normal(0, 3.0 * h / H, (B, 2, h, w)).astype(np.float32)).to('cuda')
             for h, w in SHAPES]
    weights = L.contrast_level_weights(0.5, len(SHAPES))
    out = dict(events=int(d['x'].numel()), rounds=rounds, reps=reps)
    for tag, mask, pol in PYRAMID_OPTIONS:
        one, four = Pyramid(d, flows, mask, pol, weights), FourCalls(d, flows, mask, pol, weights)
        forms = {'pyramid_fwd': one.fwd, 'four_fwd': four.fwd, 'pyramid_bwd': one.bwd, 'four_bwd': four.bwd}
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # the same bits from both forms, before anything is timed
        assert torch.equal(one.images(), four.images())
        assert torch.equal(one.terms, torch.stack([v['term'] for v in four.levels]))
        for g, v in zip(one.grads, four.levels):
            assert torch.equal(g, v['grad']) and bool(g.any())
        launches = {k: launches_of(fn) for k, fn in forms.items()}
        torch.cuda.synchronize()
        blocks = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                blocks[k].append(block_us_host(fn, reps))
        med = {k: statistics.median(u for u, _ in v) for k, v in blocks.items()}
        leg = {k: dict(us=round(med[k], 2), min_us=round(min(u for u, _ in blocks[k]), 2),
                       max_us=round(max(u for u, _ in blocks[k]), 2),
                       host_us=round(statistics.median(h_ for _, h_ in blocks[k]), 2),
                       launches=launches[k], blocks=[round(u, 2) for u, _ in blocks[k]]) for k in forms}
        leg['fwd_ratio_to_four_calls'] = round(med['pyramid_fwd'] / med['four_fwd'], 4)
        leg['bwd_ratio_to_four_calls'] = round(med['pyramid_bwd'] / med['four_bwd'], 4)
        leg['host_us_fwd_plus_bwd'] = dict(
            pyramid=round(leg['pyramid_fwd']['host_us'] + leg['pyramid_bwd']['host_us'], 2),
            four=round(leg['four_fwd']['host_us'] + leg['four_bwd']['host_us'], 2))
        leg['terms'] = [float(v) for v in one.terms]
        leg['workspace_bytes'] = one.need
        out[tag] = leg
    return out


class FramelessLeg(Leg):
    """A frameless batch: the contrast term on the finest flow (a frameless run needs it) and the
    average-timestamp term at the scales asked for."""

    def __init__(self, weight, scales):
        super().__init__(weight)
        self.batches = [dict(b, images=None, shape=(H, W)) for b in self.batches]
        self.extra = {'contrast_weight': 0.25, 'avg_timestamp_weight': weight}
        if scales != 'finest':
            self.extra['avg_timestamp_scales'] = scales


def step_finest_against_all(weight, rounds, steps=30, warmup=15):
    legs = {'finest': FramelessLeg(weight, 'finest'), 'all': FramelessLeg(weight, 'all')}
    for leg in legs.values():
        leg.block(warmup)
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, leg in legs.items():
            ms[k].append(round(leg.block(steps), 4))
    finest, every = statistics.median(ms['finest']), statistics.median(ms['all'])
    return dict(weight=weight, finest_ms=ms['finest'], all_ms=ms['all'], finest_median_ms=finest,
                all_median_ms=every, added_ms=round(every - finest, 4), added_share=round((every - finest) / finest, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--weight', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls-only', action='store_true')
    ap.add_argument('--scales', choices=('finest', 'all'), default='finest',
                    help='all: the legs of the term on every flow scale instead of the one-level ones')
    ap.add_argument('--reps', type=int, default=20, help='calls per block of the --scales all leg')
    args = ap.parse_args()
    if args.scales == 'all':
        out = dict(shape=dict(B=B, H=H, W=W, bins=BINS, events_per_sample=EVENTS, levels=[list(s_) for s_ in SHAPES]),
                   calls=pyramid_calls(args.rounds, args.reps))
        if not args.calls_only:
            out['step'] = step_finest_against_all(args.weight, args.rounds)
        print(json.dumps(out))
        return
    out = dict(shape=dict(B=B, H=H, W=W, bins=BINS, events_per_sample=EVENTS), calls=calls_alone())
    if not args.calls_only:
        out['step'] = step_with_and_without(args.weight, args.rounds)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
