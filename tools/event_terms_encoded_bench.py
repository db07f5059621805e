#!/usr/bin/env python3
"""The events-only terms on the 9 B/event encoded event columns against the
int64 / float32 wire columns (profiles/event_terms_encoded/README.md).

    python tools/event_terms_encoded_bench.py [--only calls|loop] [--dtypes f32]

GPU only (no device: it fails).  B = 8, 256x256, four flow levels, 65 536 events
per sample, three reference times with the polarities apart.

(a) calls: the device time of each of the eight encoded entry points of
    include/dvsof_event_terms_encoded.h against its wire twin on the decoded
    columns, in alternating blocks of one run (HIP events around a block of
    calls), after the two column forms have been compared bit for bit in every
    output; a difference fails the run.
(b) loop: the train loop fed from host memory through feed.DeviceFeeder with
    the contrast term on every scale, compact against wire batches, every
    kernel enqueued from Python and replayed (capture.CapturedLoop), Ranger, in
    alternating blocks of one run: ms per step from the host clock around a
    block that ends in a device synchronise, and the bytes the feeder moved per
    batch.  (The two forms are not compared bit for bit here: the voxeliser's
    column forms agree to its summation order only.)

The spread of a leg is the range of its block means.  On a commit whose library
lacks the encoded entry points (or whose loss.py lacks wire_event_columns) the
encoded and compact legs are named as lacking and the wire legs are measured
alone, so the same tool gives the parent's numbers.  One JSON line per
measurement."""
import argparse
import itertools
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

B, H, W, BINS, LEVELS = 8, 256, 256, 5, 4
MASK, POL = 7, 1
WEIGHTS = [0.5, 1, 1]
TERMS = {'contrast_weight': 0.25, 'contrast_scales': 'all',
         'contrast_references': ('start', 'middle', 'end'), 'contrast_polarity': True}
PAIRS = ('dvsof_contrast_multi', 'dvsof_contrast_pyramid', 'dvsof_avg_timestamp', 'dvsof_avg_timestamp_pyramid')


def say(**kw):
    print(json.dumps(kw), flush=True)


def host_batches(n):
    """-> ([wire batches], [compact batches]) of the same events, host tensors (pinned)."""
    from dvs_of_training_framework_amd import encoding, synthetic
    wire, compact = [], []
    for i in range(n):
        b = synthetic.to_torch(synthetic.make_batch(1234 + 1000 * i, B, H, W, None))
        enc = encoding.encode_batch(b['events'], b['timestamps'], b['sample_idx'], b['images'], {}, B)
        rest = {k: b[k].pin_memory() for k in ('timestamps', 'sample_idx', 'images')}
        wire.append(dict(rest, events={k: v.pin_memory() for k, v in b['events'].items()}, size=B))
        compact.append(dict(rest, events={k: v.pin_memory() for k, v in encoding.compact_events(enc).items()},
                            size=B))
    return wire, compact


# ------------------------------------------------------------------ (a) the calls
class Calls:
    """The buffers of one pair of entry points and its two column forms."""

    def __init__(self, name, wire, compact, have_encoded):
        from dvs_of_training_framework_amd import _lib, loss as L
        self.lib, self.name, dev = _lib.lib(), name, 'cuda'
        self.pyramid = name.endswith('pyramid')
        contrast = 'contrast' in name
        F = B
        M = F * 3 * 2
        shapes = [(H >> s, W >> s) for s in range(LEVELS)] if self.pyramid else [(H, W)]
        g = torch.Generator().manual_seed(7)
        self.flows = [(torch.randn((F, 2) + s, generator=g) * (2.0 / 2 ** k)).to(dev) for k, s in enumerate(shapes)]
        self.grads = [torch.empty_like(f) for f in self.flows]
        self.ts = torch.tensor([[0.0, 0.04]] * F, dtype=torch.float32, device=dev).reshape(-1)
        self.fs = torch.arange(F, dtype=torch.long, device=dev)
        self.seed = torch.ones((), dtype=torch.float32, device=dev)
        ev = {k: v.to(dev) for k, v in wire['events'].items()}
        cv = {k: v.to(dev) for k, v in compact['events'].items()}
        cv['polarity'] = cv['polarity'].view(torch.uint8)
        self.keep = (ev, cv)
        n = ev['x'].numel()
        self.heads = {'wire': [ev[k].data_ptr() for k in ('x', 'y', 'timestamp', 'polarity', 'sample_index')] + [n]}
        if have_encoded:
            self.heads['encoded'] = [cv[k].data_ptr() for k in ('x', 'y', 'timestamp', 'polarity',
                                                                'sample_event_offsets')] + [B, n]
        self.bytes_per_event = {'wire': 36, 'encoded': 9}
        if self.pyramid:
            self.table = L.contrast_level_table((H, W), shapes, F, M, [0.25 / LEVELS] * LEVELS,
                                                [f.data_ptr() for f in self.flows],
                                                [g_.data_ptr() for g_ in self.grads])
            self.nbytes = getattr(self.lib, name + '_workspace_bytes')(F, MASK, POL, H, W, self.table)
            mid = [self.ts.data_ptr(), self.fs.data_ptr(), F, H, W, MASK, POL, self.table]
        else:
            self.nbytes = getattr(self.lib, name + '_workspace_bytes')(F, MASK, POL, H, W)
            mid = [self.ts.data_ptr(), self.fs.data_ptr(), self.flows[0].data_ptr(), F, H, W, MASK, POL]
        assert self.nbytes > 0
        self.ws = torch.empty(self.nbytes // 8 + 1, dtype=torch.long, device=dev)
        self.terms = torch.zeros(LEVELS + 1, dtype=torch.float32, device=dev)
        if contrast:
            self.rows = torch.empty(len(shapes) * M, 48, dtype=torch.uint8, device=dev)
            if self.pyramid:
                fwd_out = [self.rows.data_ptr(), self.terms.data_ptr(), self.terms[LEVELS:].data_ptr()]
                bwd_mid = []
            else:
                self.q = torch.empty(M, H, W, dtype=torch.long, device=dev)
                self.count = torch.empty(M, H, W, dtype=torch.int32, device=dev)
                fwd_out = [self.q.data_ptr(), self.count.data_ptr(), self.rows.data_ptr(), self.terms.data_ptr()]
                bwd_mid = [self.q.data_ptr()]
        else:
            bwd_mid = []
            fwd_out = [self.terms.data_ptr(), self.terms[LEVELS:].data_ptr()] if self.pyramid else \
                [self.terms.data_ptr()]
        bwd_tail = [self.seed.data_ptr()] if self.pyramid else [self.seed.data_ptr(), 0.25, self.grads[0].data_ptr()]
        self.fwd_args = mid + fwd_out + [self.ws.data_ptr(), self.nbytes]
        self.bwd_args = mid + bwd_mid + [self.ws.data_ptr(), self.nbytes] + bwd_tail

    def call(self, form, which):
        from dvs_of_training_framework_amd import _lib
        suffix = '' if form == 'wire' else '_encoded'
        fn = getattr(self.lib, f'{self.name}_{which}{suffix}')
        rc = fn(*self.heads[form], *(self.fwd_args if which == 'fwd' else self.bwd_args), _lib.stream())
        assert rc == 0, (self.name, form, which, rc)

    def outputs(self, form):
        """Everything a forward and a backward of that form leave behind, as bytes."""
        self.ws.zero_()
        self.call(form, 'fwd')
        torch.cuda.synchronize()
        after = self.ws[:self.nbytes // 8].clone()
        self.call(form, 'bwd')
        torch.cuda.synchronize()
        out = [after, self.ws[:self.nbytes // 8].clone(), self.terms.clone().view(torch.int32)]
        out += [g.clone().view(torch.int32) for g in self.grads]
        for k in ('rows', 'q', 'count'):
            if hasattr(self, k):
                out.append(getattr(self, k).clone())
        return out

    def block(self, form, which, n):
        """-> device ms per call.  A backward needs the forward's images: they are there."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            self.call(form, which)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n


def measure_calls(a, wire, compact, have_encoded):
    for name in PAIRS:
        c = Calls(name, wire, compact, have_encoded)
        forms = list(c.heads)
        if have_encoded:
            # (the whole workspace is compared: it was zeroed before either form ran)
            same = all(torch.equal(u, v) for u, v in zip(c.outputs('wire'), c.outputs('encoded')))
            say(what='bitwise', pair=name, equal=same, workspace_bytes=c.nbytes)
            if not same:
                raise SystemExit(f'{name}: the encoded call does not give the bytes of its wire twin')
        for which in ('fwd', 'bwd'):
            c.call(forms[0], 'fwd')
            for form in forms:
                c.block(form, which, a.warmup)
            blocks = {form: [] for form in forms}
            for _ in range(a.blocks):           # the forms alternate
                for form in forms:
                    blocks[form].append(c.block(form, which, a.block_calls))
            mean = {form: sum(v) / len(v) for form, v in blocks.items()}
            for form, v in blocks.items():
                say(what='call', call=f'{name}_{which}' + ('' if form == 'wire' else '_encoded'), form=form,
                    ms=round(mean[form], 4), block_ms=[round(x, 4) for x in v],
                    spread_ms=round(max(v) - min(v), 4), column_bytes_per_event=c.bytes_per_event[form],
                    events=B * H * W, timed_calls=a.blocks * a.block_calls)
            if have_encoded:
                w = blocks['wire']
                say(what='verdict', call=f'{name}_{which}', encoded_minus_wire_ms=round(mean['encoded'] - mean['wire'], 4),
                    wire_spread_ms=round(max(w) - min(w), 4),
                    encoded_slower_than_the_wire_spread=mean['encoded'] - mean['wire'] > max(w) - min(w))
        del c
        torch.cuda.empty_cache()


# ------------------------------------------------------------------- (b) the loop
class Loop:
    """A model, Ranger and a feeder over host batches, stepped eagerly or as replays."""

    def __init__(self, batches, dtype, replay):
        from dvs_of_training_framework_amd import feed, optim
        from dvs_of_training_framework_amd.capture import CapturedLoop
        from dvs_of_training_framework_amd.loss import init_losses
        from dvs_of_training_framework_amd.net import Model
        torch.manual_seed(1234)
        self.model = Model('cuda', event_representation_depth=BINS, compute_dtype=dtype)
        self.model.train()
        self.opt = optim.FusedRanger(self.model.predictor.parameters(), lr=1e-3, weight_decay=1e-4)
        self.losses = init_losses((H, W), B, self.model, 'cuda', sequence_length=1)
        self.feeder = feed.DeviceFeeder(_Cycle(batches), 'cuda')
        self.it = iter(self.feeder)
        self.loop = CapturedLoop(self.model, self.losses, self.opt, WEIGHTS, 'cuda', 1, None,
                                 loss_options=TERMS) if replay else None

    def step(self):
        batch = next(self.it)
        if self.loop is not None:
            loss = self.loop.run(batch, 0)[0]
            assert self.loop.failed is None, self.loop.failed
            return loss
        from dvs_of_training_framework_amd.loss import unit_backward
        from dvs_of_training_framework_amd.timer import FakeTimer
        from dvs_of_training_framework_amd.training import process_minibatch
        loss, _, _ = process_minibatch(self.model, batch, FakeTimer(), 'cuda', True, self.losses, WEIGHTS, **TERMS)
        unit_backward(loss)
        self.model.strict = False
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        return loss.detach()

    def settle(self, warmup):
        for _ in range(60 if self.loop is not None else 0):
            steps = list(self.loop.bound.values())
            if len(steps) >= 2 and all(s.executor.plan()[1] for s in steps):
                break
            self.step()
        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()

    def block(self, n):
        """-> ms per step, host clock around n steps and the synchronise that ends them."""
        torch.cuda.synchronize()
        moved, t0 = self.feeder.bytes_moved, time.perf_counter()
        for _ in range(n):
            loss = self.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        assert bool(torch.isfinite(loss)), 'the loss is not finite'
        return ms, (self.feeder.bytes_moved - moved) / n

    def close(self):
        if self.loop is not None:
            self.loop.close()


class _Cycle:
    """A loader that never ends: the host batches over and over."""

    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return 1 << 30

    def __iter__(self):
        return itertools.cycle(self.batches)


def measure_loop(a, wire, compact, have_compact, dtype):
    legs = {}
    for form, batches in (('wire', wire), ('compact', compact)):
        if form == 'compact' and not have_compact:
            continue
        for replay in (False, True):
            legs[(form, 'replay' if replay else 'eager')] = Loop(batches, dtype, replay)
    for leg in legs.values():
        leg.settle(a.warmup)
    blocks = {k: [] for k in legs}
    for _ in range(a.blocks):                   # the legs alternate
        for k, leg in legs.items():
            blocks[k].append(leg.block(a.block_steps))
    mean = {}
    for (form, mode), rows in blocks.items():
        ms = [r[0] for r in rows]
        mean[(form, mode)] = sum(ms) / len(ms)
        say(what='loop', dtype=dtype, batches=form, mode=mode, ms_per_step=round(mean[(form, mode)], 4),
            samples_per_s=round(B / mean[(form, mode)] * 1e3, 1), block_ms=[round(v, 4) for v in ms],
            spread_ms=round(max(ms) - min(ms), 4), host_to_device_bytes_per_batch=int(rows[-1][1]),
            timed_steps=a.blocks * a.block_steps)
    if have_compact:
        for mode in ('eager', 'replay'):
            w = [r[0] for r in blocks[('wire', mode)]]
            d = mean[('compact', mode)] - mean[('wire', mode)]
            say(what='verdict', dtype=dtype, mode=mode, compact_minus_wire_ms=round(d, 4),
                wire_spread_ms=round(max(w) - min(w), 4), compact_slower_than_the_wire_spread=d > max(w) - min(w))
    for leg in legs.values():
        leg.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=('calls', 'loop'), default=None)
    ap.add_argument('--dtypes', nargs='+', default=['f32'])
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--block-calls', type=int, default=20)
    ap.add_argument('--block-steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs a GPU'
    from dvs_of_training_framework_amd import _lib, loss as L
    have_encoded = hasattr(_lib.lib(), 'dvsof_contrast_multi_fwd_encoded')
    have_compact = have_encoded and hasattr(L, 'wire_event_columns')
    say(what='shape', B=B, H=H, W=W, bins=BINS, levels=LEVELS, events_per_sample=H * W, mask=MASK, polarity=POL,
        device=torch.cuda.get_device_name(0),
        lacking=([] if have_encoded else ['the eight encoded entry points: the wire calls are measured alone'])
        + ([] if have_compact else ['compact batches with the terms: the wire loops are measured alone']))
    wire, compact = host_batches(4)
    if have_compact:
        dec = L.wire_event_columns(compact[0]['events'])
        assert all(torch.equal(dec[k], wire[0]['events'][k]) for k in dec), 'the compact batch is not the wire batch'
    say(what='feed', wire_bytes_per_event=sum(v.element_size() for k, v in wire[0]['events'].items()
                                              if k != 'element_index'),
        compact_bytes_per_event=sum(v.element_size() for k, v in compact[0]['events'].items()
                                    if k != 'sample_event_offsets'), events=B * H * W)
    if a.only in (None, 'calls'):
        measure_calls(a, wire[0], compact[0], have_encoded)
    if a.only in (None, 'loop'):
        for dtype in a.dtypes:
            measure_loop(a, wire, compact, have_compact, dtype)
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
