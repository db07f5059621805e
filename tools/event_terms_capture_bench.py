#!/usr/bin/env python3
"""The captured step that carries the events-only terms (--capture-event-terms)
against the eager loop at the benchmark shape (profiles/event_terms_capture/
README.md).

    python tools/event_terms_capture_bench.py [--dtypes f32 bf16s] [--configs a b c]

GPU only (no device: it fails).  B = 8, 256x256x5, 65 536 events per sample,
Ranger, two resident batches.  Three configurations:

    a   framed batches + contrast_weight 0.25
    b   frameless batches + the contrast term on every scale, three reference
        times, polarity
    c   b + avg_timestamp_weight 0.5

Per configuration and dtype two legs -- every kernel enqueued from Python | one
C call per step (capture.CapturedTrainStep(bind=True, loss_options=...)) -- each
on its own model and optimizer from one seed.  First the legs' first four steps
are compared bit for bit (losses and, after them, every parameter; the replay
leg's are two eager constructor steps and two replays): a difference fails the
run.  Then, after the executors have settled on a plan and a warm-up of both,
the legs are timed in alternating blocks of one run: ms per step from HIP
events around a block, the host's enqueue time per step (the clock around the
block's calls, before anything waits for the device; beside it the same for
steps issued one at a time to an idle device, where no full queue can hold a
launch back), and the spread of a leg = the range of its block means.  Two more
configurations, f (frameless + contrast_weight 0.25) and w (framed + the options
of b), tell what the batches and what the options add; ask for them by name.
One JSON line per measurement."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

B, H, W, BINS = 8, 256, 256, 5
WEIGHTS = [0.5, 1, 1]
WIDE = {'contrast_weight': 0.25, 'contrast_scales': 'all',
        'contrast_references': ('start', 'middle', 'end'), 'contrast_polarity': True}
CONFIGS = {'a': (False, {'contrast_weight': 0.25}),
           'b': (True, WIDE),
           'c': (True, dict(WIDE, avg_timestamp_weight=0.5)),
           # not among the defaults: apart, what frameless batches and what the options of b add
           'f': (True, {'contrast_weight': 0.25}),
           'w': (False, WIDE)}
DEFAULT = ('a', 'b', 'c')


def say(**kw):
    print(json.dumps(kw), flush=True)


class Leg:
    """A model, Ranger and two resident batches, stepped eagerly or as replays
    of captured steps bound to the batches."""

    def __init__(self, frameless, options, dtype, replay):
        from dvs_of_training_framework_amd import optim, synthetic
        from dvs_of_training_framework_amd.loss import init_losses
        from dvs_of_training_framework_amd.net import Model
        torch.manual_seed(1234)
        self.model = Model('cuda', event_representation_depth=BINS, compute_dtype=dtype)
        self.model.train()
        self.opt = optim.FusedRanger(self.model.predictor.parameters(), lr=1e-3, weight_decay=1e-4)
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda s: 2 ** (-s / 100000))
        self.losses = init_losses((H, W), B, self.model, 'cuda', sequence_length=1)
        self.batches = [synthetic.to_torch(synthetic.make_batch(1234 + 1000 * i, B, H, W, None), 'cuda')
                        for i in range(2)]
        if frameless:
            for batch in self.batches:
                batch['images'], batch['shape'] = None, (H, W)
        self.options, self.replay, self.caps, self.i = dict(options), replay, {}, 0

    def step(self):
        """-> the loss of the step (of a replay: the static output)."""
        k = self.i % 2
        self.i += 1
        if self.replay:
            if k not in self.caps:
                from dvs_of_training_framework_amd.capture import CapturedTrainStep
                self.caps[k] = CapturedTrainStep(self.model, self.losses, self.opt, WEIGHTS, 'cuda',
                                                 self.batches[k], bind=True, loss_options=self.options)
                loss = self.caps[k].first_loss
            else:
                loss = self.caps[k]()[0]
        else:
            from dvs_of_training_framework_amd.loss import unit_backward
            from dvs_of_training_framework_amd.timer import FakeTimer
            from dvs_of_training_framework_amd.training import process_minibatch
            loss, _, _ = process_minibatch(self.model, self.batches[k], FakeTimer(), 'cuda', True,
                                           self.losses, WEIGHTS, **self.options)
            unit_backward(loss)
            self.model.strict = False
            self.opt.step()
            self.opt.zero_grad(set_to_none=True)
            loss = loss.detach()
        self.sched.step()
        return loss

    def first_steps(self, n=4):
        losses = [float(self.step().clone()) for _ in range(n)]
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in self.model.parameters()]

    def settle(self, warmup):
        """Calibration and the executors' plan trials are set-up."""
        for _ in range(60 if self.replay else 0):
            if all(c.executor.plan()[1] for c in self.caps.values()):
                break
            self.step()
        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()

    def block(self, n):
        """-> (device ms per step, host enqueue ms per step)."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        t0 = time.perf_counter()
        for _ in range(n):
            self.step()
        host = time.perf_counter() - t0
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n, host / n * 1e3

    def idle_host_ms(self, n=10):
        """Host time of a step issued to an idle device: the calls alone, no
        queue behind them that could hold a launch back."""
        total = 0.0
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.step()
            total += time.perf_counter() - t0
        torch.cuda.synchronize()
        return total / n * 1e3

    def close(self):
        for c in self.caps.values():
            c.close()


def measure(a, name, dtype):
    frameless, options = CONFIGS[name]
    legs = {'eager': Leg(frameless, options, dtype, False), 'replay': Leg(frameless, options, dtype, True)}
    (l_e, w_e), (l_r, w_r) = legs['eager'].first_steps(), legs['replay'].first_steps()
    same = l_e == l_r and all(torch.equal(u, v) for u, v in zip(w_e, w_r))
    x = legs['replay'].caps[0].executor
    say(what='bitwise', config=name, dtype=dtype, frameless=frameless, options=options, equal=same,
        eager_losses=l_e, replay_losses=l_r, replays=sum(c.replays for c in legs['replay'].caps.values()),
        kernels=x.kernels, lanes=x.lanes, lane_kernels=x.lane_kernels)
    if not same:
        raise SystemExit(f'{name}/{dtype}: the replayed steps are not the eager steps bit for bit')
    del w_e, w_r
    for leg in legs.values():
        leg.settle(a.warmup)
    blocks = {k: [] for k in legs}
    for _ in range(a.blocks):               # the legs alternate
        for k, leg in legs.items():
            blocks[k].append(leg.block(a.block_steps))
    idle = {k: leg.idle_host_ms() for k, leg in legs.items()}
    out = {}
    for k, rows in blocks.items():
        ms, host = [r[0] for r in rows], [r[1] for r in rows]
        out[k] = sum(ms) / len(ms)
        say(what='step', config=name, dtype=dtype, leg=k, ms_per_step=round(out[k], 4),
            host_ms_per_step=round(sum(host) / len(host), 4), idle_host_ms_per_step=round(idle[k], 4),
            samples_per_s=round(B / out[k] * 1e3, 1),
            timed_steps=a.blocks * a.block_steps, block_ms=[round(v, 4) for v in ms],
            block_host_ms=[round(v, 4) for v in host], spread_ms=round(max(ms) - min(ms), 4),
            plan=legs['replay'].caps[0].executor.plan()[0] if k == 'replay' else None)
    e_ms = [r[0] for r in blocks['eager']]
    say(what='verdict', config=name, dtype=dtype, replay_minus_eager_ms=round(out['replay'] - out['eager'], 4),
        eager_spread_ms=round(max(e_ms) - min(e_ms), 4),
        replay_slower_than_the_eager_spread=out['replay'] - out['eager'] > max(e_ms) - min(e_ms))
    for leg in legs.values():
        leg.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtypes', nargs='+', default=['f32', 'bf16s'])
    ap.add_argument('--configs', nargs='+', default=list(DEFAULT), choices=list(CONFIGS))
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--block-steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs a GPU'
    say(what='shape', B=B, H=H, W=W, bins=BINS, events_per_sample=65536, optimizer='ranger',
        device=torch.cuda.get_device_name(0))
    for name in a.configs:
        for dtype in a.dtypes:
            measure(a, name, dtype)
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
