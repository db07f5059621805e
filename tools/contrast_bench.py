#!/usr/bin/env python3
"""Cost of the contrast-maximisation term (docs/CONTRAST_SPEC.md), one JSON
line (profiles/contrast/README.md).  Batch 8, 256x256, 5 bins, 65 536 events
per sample.

  calls   dvsof_contrast_fwd and dvsof_contrast_bwd alone on random flows
          (sigma 3 pixels): HIP events around blocks of launches, the two
          calls taking turns block by block within one run, the median block
          per call; bytes from the shapes (columns, flow reads, fills, the
          images read back by the statistics and by the backward's corners,
          the fixed-point sums and the gradient) and the 64-bit integer
          atomics counted on the host by the restatement.
  step    the eager training step (Ranger, f32, process_minibatch +
          unit_backward + step) with contrast_weight 0 against --weight, in
          alternating blocks of one run; the median block of each.
  --multi only this: dvsof_contrast_fwd / _bwd, dvsof_contrast_multi_fwd /
          _bwd at mask = start without polarity (the same kernels through
          the general entry point) and at all three references with
          polarity, in alternating blocks of one run
          (profiles/contrast_multi/README.md, profiles/event_images/README.md).
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


def block_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def calls_alone(rounds=7, reps=40, seed=0):
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    batch = synthetic.make_batch(seed, B, H, W, EVENTS)
    ev = batch['events']
    rng = np.random.default_rng(seed)
    c = dict(x=ev['x'], y=ev['y'], t=ev['timestamp'], s=ev['sample_index'],
             ts=np.tile(np.array([0, synthetic.WINDOW], np.float32), B), fs=np.arange(B, dtype=np.int64),
             flow=rng.normal(0, 3, (B, 2, H, W)).astype(np.float32))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.items()}
    n, F, px = d['x'].numel(), B, B * H * W
    q = torch.empty(F, H, W, dtype=torch.long, device=dev)
    count = torch.empty(F, H, W, dtype=torch.int32, device=dev)
    rows = torch.empty(F, 48, dtype=torch.uint8, device=dev)
    term = torch.empty((), device=dev)
    grad = torch.empty(F, 2, H, W, device=dev)
    seed_t = torch.ones((), device=dev)
    need = lib.dvsof_contrast_workspace_bytes(F, H, W)
    ws = torch.empty(need // 8, dtype=torch.long, device=dev)
    cols = [d[k].data_ptr() for k in ('x', 'y', 't', 's')] + [n] + [d[k].data_ptr() for k in ('ts', 'fs', 'flow')]

    def check(rc):
        assert rc == 0, rc
    calls = {
        'fwd': lambda: check(lib.dvsof_contrast_fwd(*cols, F, H, W, q.data_ptr(), count.data_ptr(), rows.data_ptr(),
                                                    term.data_ptr(), ws.data_ptr(), need, stream)),
        'bwd': lambda: check(lib.dvsof_contrast_bwd(*cols, F, H, W, q.data_ptr(), ws.data_ptr(), need,
                                                    seed_t.data_ptr(), 0.25, grad.data_ptr(), stream))}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the device against the restatement once, and the number of atomics from the same arithmetic
    args = (c['x'], c['y'], c['t'], c['s'], c['ts'], c['fs'], c['flow'])
    fwd = L.contrast_fwd_host(*args)
    want, sums = L.contrast_bwd_host(*args, fwd, 1.0, 0.25)
    assert np.array_equal(q.cpu().numpy(), fwd['q']) and term.cpu().numpy().tobytes() == fwd['term'].tobytes()
    assert grad.cpu().numpy().tobytes() == want.tobytes()
    pairs = L._contrast_pairs(*args)
    kept, inside = int(pairs['f'].size), int(pairs['inside'].sum())
    blocks = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            blocks[k].append(block_us(fn, reps))
    # an upper count: every corner of an inside event (corners outside the image and Q = 0 add nothing)
    atomics = {'fwd': kept + 4 * inside, 'bwd': 2 * inside}
    nbytes = {'fwd': n * 28 + kept * 8 + px * (8 + 4 + 16) + px * 12 + kept * 4 + 4 * inside * 8,
              'bwd': n * 28 + kept * 8 + 4 * inside * 8 + 2 * inside * 8 + px * 2 * (8 + 8 + 4)}
    out = dict(events=n, take_part=kept, inside=inside, term=float(fwd['term']))
    for k, v in blocks.items():
        us = statistics.median(v)
        out[k] = dict(us=round(us, 2), min_us=round(min(v), 2), max_us=round(max(v), 2), bytes=nbytes[k],
                      GBps=round(nbytes[k] / us / 1e3, 1), atomics=atomics[k],
                      atomic_GBps=round(atomics[k] * 8 / us / 1e3, 1))
    return out


def calls_multi(rounds=9, reps=40, seed=0):
    """dvsof_contrast_fwd / _bwd (the entry points without options),
    dvsof_contrast_multi_fwd / _bwd at mask = start without polarity (the same
    kernels through the general entry point) and at all three references with
    polarity (six images per frame), the six taking turns block by block
    within one run."""
    dev, lib, stream = 'cuda', _lib.lib(), _lib.stream()
    batch = synthetic.make_batch(seed, B, H, W, EVENTS)
    ev = batch['events']
    rng = np.random.default_rng(seed)
    c = dict(x=ev['x'], y=ev['y'], t=ev['timestamp'], p=ev['polarity'], s=ev['sample_index'],
             ts=np.tile(np.array([0, synthetic.WINDOW], np.float32), B), fs=np.arange(B, dtype=np.int64),
             flow=rng.normal(0, 3, (B, 2, H, W)).astype(np.float32))
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in c.items()}
    n, F = d['x'].numel(), B
    grad = torch.empty(F, 2, H, W, device=dev)
    seed_t = torch.ones((), device=dev)
    tables = [d[k].data_ptr() for k in ('ts', 'fs', 'flow')]

    def check(rc):
        assert rc == 0, rc

    def buffers(M, need):
        return dict(q=torch.empty(M, H, W, dtype=torch.long, device=dev),
                    count=torch.empty(M, H, W, dtype=torch.int32, device=dev),
                    rows=torch.empty(M, 48, dtype=torch.uint8, device=dev), term=torch.empty((), device=dev),
                    ws=torch.empty(need // 8, dtype=torch.long, device=dev), need=need)

    def outs(b):
        return [b[k].data_ptr() for k in ('q', 'count', 'rows', 'term', 'ws')] + [b['need'], stream]

    old = buffers(F, lib.dvsof_contrast_workspace_bytes(F, H, W))
    cols = [d[k].data_ptr() for k in ('x', 'y', 't', 's')] + [n] + tables + [F, H, W]
    calls = {
        'default_fwd': lambda: check(lib.dvsof_contrast_fwd(*cols, *outs(old))),
        'default_bwd': lambda: check(lib.dvsof_contrast_bwd(*cols, old['q'].data_ptr(), old['ws'].data_ptr(),
                                                           old['need'], seed_t.data_ptr(), 0.25, grad.data_ptr(),
                                                           stream))}
    held = {}
    for tag, mask, pol in (('start', 1, 0), ('all_polarity', 7, 1)):
        M = F * bin(mask).count('1') * (1 + pol)
        b = held[tag] = buffers(M, lib.dvsof_contrast_multi_workspace_bytes(F, mask, pol, H, W))
        head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n] + tables + [F, H, W, mask, pol]
        calls[tag + '_fwd'] = lambda head=head, b=b: check(lib.dvsof_contrast_multi_fwd(*head, *outs(b)))
        calls[tag + '_bwd'] = lambda head=head, b=b: check(lib.dvsof_contrast_multi_bwd(
            *head, b['q'].data_ptr(), b['ws'].data_ptr(), b['need'], seed_t.data_ptr(), 0.25, grad.data_ptr(), stream))
    grads = {}
    for k, fn in calls.items():
        for _ in range(3):
            fn()
        grads[k] = grad.clone()
    torch.cuda.synchronize()
    # mask = start without polarity is the term of the entry points without options, bit for bit
    assert torch.equal(old['q'], held['start']['q']) and torch.equal(old['term'], held['start']['term'])
    assert torch.equal(grads['default_bwd'], grads['start_bwd'])
    blocks = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            blocks[k].append(block_us(fn, reps))
    out = dict(events=n, rounds=rounds, reps=reps, terms={k: float(b['term']) for k, b in held.items()})
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
        self.extra = {'contrast_weight': weight} if weight else {}
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


def step_off_against_on(weight, rounds=7, steps=30, warmup=15):
    legs = {'off': Leg(0.0), 'on': Leg(weight)}
    for leg in legs.values():
        leg.block(warmup)
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, leg in legs.items():
            ms[k].append(round(leg.block(steps), 4))
    off, on = statistics.median(ms['off']), statistics.median(ms['on'])
    return dict(weight=weight, off_ms=ms['off'], on_ms=ms['on'], off_median_ms=off, on_median_ms=on,
                added_ms=round(on - off, 4), added_share=round((on - off) / off, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--weight', type=float, default=0.25)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--multi', action='store_true',
                    help='only the leg of the entry points with several references and the polarities '
                         'apart beside those without options (profiles/contrast_multi/README.md)')
    args = ap.parse_args()
    if args.multi:
        print(json.dumps(dict(shape=dict(B=B, H=H, W=W, events_per_sample=EVENTS), multi=calls_multi())))
        return
    print(json.dumps(dict(shape=dict(B=B, H=H, W=W, bins=BINS, events_per_sample=EVENTS),
                          calls=calls_alone(args.rounds), step=step_off_against_on(args.weight, args.rounds))))


if __name__ == '__main__':
    main()
