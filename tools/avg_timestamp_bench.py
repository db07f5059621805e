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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--weight', type=float, default=0.5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls-only', action='store_true')
    args = ap.parse_args()
    out = dict(shape=dict(B=B, H=H, W=W, bins=BINS, events_per_sample=EVENTS), calls=calls_alone())
    if not args.calls_only:
        out['step'] = step_with_and_without(args.weight, args.rounds)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
