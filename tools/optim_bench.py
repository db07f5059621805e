#!/usr/bin/env python3
"""Ranger (and AdamW as the yardstick) at the benchmark shape: the eager loop
against the step executor's replay, and the update kernels alone.

    python tools/optim_bench.py [--dtypes f32 bf16s] [--legs eager replay] [--fused]
    python tools/optim_bench.py --guard         # the step guard's cost alone

GPU only (no device: it fails).  B = 8, 256x256x5, 65 536 events per sample,
two resident batches.  Per dtype and optimizer the two legs -- every kernel
enqueued from Python | one C call per step -- are timed in alternating blocks
(host clock closed by a device synchronise; blocks x block-steps timed steps
per leg after warm-up), each leg on its own model and optimizer.  The spread
of a leg is the range of its block means.  On a commit whose optimizer lacks
begin_capture / advance / end_capture the replay leg is reported as missing
and only the eager leg is measured.  One JSON line per measurement.

Then the update alone (HIP events around the launch, median of the
repetitions): the RAdam/Ranger update kernel over the predictor's parameters
on a step that does not synchronise the Lookahead slow weights (28 B per
parameter: p, g, m, v read, p, m, v written) and on one that does (36 B), with
the share of 8 TB/s those bytes over that time are; and the gradient
centralisation, one launch per tensor against the multi-tensor launch.

``--guard`` (docs/STEP_GUARD_SPEC.md) measures the step guard instead: f32,
AdamW and Ranger, eager and executor replay, blocks of a guard-off and a
guard-on leg alternating within one run (``set_guard(1e9)``: nothing clips,
nothing skips, so both legs do the same arithmetic; no update inside the
backward in either, which a guard excludes); then the two statistic kernels
alone (HIP events; 4 B per parameter read).  On a commit without ``set_guard``
the guard-off legs alone are measured."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

B, H, W, BINS = 8, 256, 256, 5
HBM_PEAK = 8e12
PROTOCOL = ('begin_capture', 'advance', 'end_capture')


def say(**kw):
    print(json.dumps(kw), flush=True)


class Leg:
    """A model, an optimizer and two resident batches, stepped eagerly or as
    replays of captured steps bound to the batches."""

    def __init__(self, optimizer, dtype, replay, fused, guard=False):
        from dvs_of_training_framework_amd import optim, synthetic
        from dvs_of_training_framework_amd.loss import init_losses
        from dvs_of_training_framework_amd.net import Model
        torch.manual_seed(1234)
        self.model = Model('cuda', event_representation_depth=BINS, compute_dtype=dtype)
        self.model.train()
        params = self.model.predictor.parameters()
        if optimizer == 'ranger':
            self.opt = optim.FusedRanger(params, lr=1e-3, weight_decay=1e-4)
        else:
            self.opt = optim.FusedAdamW(params, lr=1e-3, weight_decay=1e-4, amsgrad=True)
        if fused:
            self.opt.fuse_into_backward(self.model.predictor)
        if guard:
            self.opt.set_guard(1e9, True)       # never binds: the cost of deciding, nothing else
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda s: 2 ** (-s / 100000))
        self.losses = init_losses((H, W), B, self.model, 'cuda', sequence_length=1)
        self.batches = [synthetic.to_torch(synthetic.make_batch(1234 + 1000 * i, B, H, W, None), 'cuda')
                        for i in range(2)]
        self.replay, self.caps, self.i = replay, {}, 0

    def step(self):
        k = self.i % 2
        self.i += 1
        if self.replay:
            if k not in self.caps:
                from dvs_of_training_framework_amd.capture import CapturedTrainStep
                self.caps[k] = CapturedTrainStep(self.model, self.losses, self.opt, [0.5, 1, 1],
                                                 'cuda', self.batches[k], bind=True)
            else:
                self.caps[k]()
        else:
            from dvs_of_training_framework_amd.loss import unit_backward
            from dvs_of_training_framework_amd.timer import FakeTimer
            from dvs_of_training_framework_amd.training import process_minibatch
            loss, _, _ = process_minibatch(self.model, self.batches[k], FakeTimer(), 'cuda', True,
                                           self.losses, [0.5, 1, 1])
            unit_backward(loss)
            self.model.strict = False
            self.opt.step()
            self.opt.zero_grad(set_to_none=True)
        self.sched.step()

    def settle(self, warmup):
        """Captures, calibration and the executors' plan trials are set-up."""
        for _ in range(60 if self.replay else 0):
            if len(self.caps) == 2 and all(c.executor.plan()[1] for c in self.caps.values()):
                break
            self.step()
        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()

    def block(self, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def close(self):
        for c in self.caps.values():
            c.close()


def steps(a, optimizer, dtype):
    from dvs_of_training_framework_amd import optim
    cls = optim.FusedRanger if optimizer == 'ranger' else optim.FusedAdamW
    can_replay = all(hasattr(cls, m) for m in PROTOCOL)
    legs = {}
    if 'eager' in a.legs:
        legs['eager'] = Leg(optimizer, dtype, False, a.fused)
    if can_replay and 'replay' in a.legs:
        legs['replay'] = Leg(optimizer, dtype, True, a.fused)
    elif 'replay' in a.legs:
        say(what='step', optimizer=optimizer, dtype=dtype, leg='replay', ms_per_step=None,
            note=f'not measured: {cls.__name__} has no begin_capture / advance / end_capture '
                 'on this commit')
    for leg in legs.values():
        leg.settle(a.warmup)
    blocks = {name: [] for name in legs}
    for _ in range(a.blocks):           # the legs alternate
        for name, leg in legs.items():
            blocks[name].append(leg.block(a.block_steps))
    for name, ms in blocks.items():
        mean = sum(ms) / len(ms)
        say(what='step', optimizer=optimizer, dtype=dtype, leg=name, fused_into_backward=a.fused,
            ms_per_step=round(mean, 4), samples_per_s=round(B / mean * 1e3, 1),
            timed_steps=a.blocks * a.block_steps, block_ms=[round(v, 4) for v in ms],
            spread_ms=round(max(ms) - min(ms), 4))
    for leg in legs.values():
        leg.close()


def guard_steps(a, optimizer):
    """Guard off against guard on, per launch mode, in alternating blocks."""
    from dvs_of_training_framework_amd import optim
    cls = optim.FusedRanger if optimizer == 'ranger' else optim.FusedAdamW
    has_guard = hasattr(cls, 'set_guard')
    for mode in a.legs:
        replay = mode == 'replay'
        legs = {'guard off': Leg(optimizer, 'f32', replay, False)}
        if has_guard:
            legs['guard on'] = Leg(optimizer, 'f32', replay, False, guard=True)
        else:
            say(what='guard', optimizer=optimizer, mode=mode, leg='guard on', ms_per_step=None,
                note=f'not measured: {cls.__name__} has no set_guard on this commit')
        for leg in legs.values():
            leg.settle(a.warmup)
        blocks = {name: [] for name in legs}
        for _ in range(a.blocks):
            for name, leg in legs.items():
                blocks[name].append(leg.block(a.block_steps))
        for name, ms in blocks.items():
            mean = sum(ms) / len(ms)
            say(what='guard', optimizer=optimizer, mode=mode, leg=name, dtype='f32',
                ms_per_step=round(mean, 4), samples_per_s=round(B / mean * 1e3, 1),
                timed_steps=a.blocks * a.block_steps, block_ms=[round(v, 4) for v in ms],
                spread_ms=round(max(ms) - min(ms), 4))
        if has_guard:
            state = legs['guard on'].opt.guard_state()
            say(what='guard record', optimizer=optimizer, mode=mode,
                **{k: state[k] for k in ('norm', 'scale', 'bad', 'skipped', 'clipped')})
        for leg in legs.values():
            leg.close()


def guard_alone(a):
    """The two statistic kernels (partials, close) over the predictor's
    gradients: HIP events, bytes from the parameter shapes."""
    from dvs_of_training_framework_amd import optim
    from dvs_of_training_framework_amd.net import Model
    if not hasattr(optim.FusedAdamW, 'set_guard'):
        say(what='guard statistic alone', event_ms_median=None,
            note='not measured: no set_guard on this commit')
        return
    torch.manual_seed(1)
    model = Model('cuda', event_representation_depth=BINS)
    plist = list(model.predictor.parameters())
    for p in plist:
        p.grad = torch.randn_like(p) * 1e-3
    opt = optim.FusedAdamW(plist, lr=1e-4, amsgrad=True)
    opt.set_guard(1e9, True)
    opt.step()                                  # state, tables, workspace
    torch.cuda.synchronize()
    work = [(0, opt.param_groups[0], plist)]
    n_params = sum(p.numel() for p in plist)
    med, best = event_ms(lambda: opt._enqueue_guard(work), a.reps)
    say(what='guard statistic alone', launches=2, tensors=len(plist), parameters=n_params,
        work_items=opt._guard_tables[4], bytes=4 * n_params, bytes_per_parameter=4,
        event_ms_median=round(med, 4), event_ms_min=round(best, 4),
        gb_per_s=round(4 * n_params / med / 1e6, 1),
        share_of_8tb_per_s=round(4 * n_params / (med * 1e-3) / HBM_PEAK, 4))


def event_ms(fn, reps):
    """Median HIP-event time of fn() over reps."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2], out[0]


def update_alone(a):
    from dvs_of_training_framework_amd import _lib, optim
    from dvs_of_training_framework_amd.net import Model
    torch.manual_seed(1)
    model = Model('cuda', event_representation_depth=BINS)
    plist = list(model.predictor.parameters())
    for p in plist:
        p.grad = torch.randn_like(p) * 1e-3
    opt = optim.FusedRanger(plist, lr=1e-4)
    opt.step()                                  # state and tables
    torch.cuda.synchronize()
    group = opt.param_groups[0]
    t_ptrs, t_sizes, t_chunks, n = opt._table(0, plist)[:4]
    lib, n_params = _lib.lib(), sum(p.numel() for p in plist)

    def update(step):
        def fn():
            _lib.check(lib.dvsof_radam_step(
                t_ptrs.data_ptr(), t_sizes.data_ptr(), t_chunks.data_ptr(), n, 1e-4, .95, .999,
                1e-5, 0.0, step, 5.0, 1, 1 if step % group['k'] == 0 else 0, group['alpha'],
                _lib.stream()), 'dvsof_radam_step')
        return fn
    for name, step, per in (('no sync', 13, 28), ('sync', 12, 36)):
        med, best = event_ms(update(step), a.reps)
        say(what='update kernel alone', step=name, parameters=n_params, bytes=per * n_params,
            bytes_per_parameter=per, event_ms_median=round(med, 4), event_ms_min=round(best, 4),
            gb_per_s=round(per * n_params / med / 1e6, 1),
            share_of_8tb_per_s=round(per * n_params / (med * 1e-3) / HBM_PEAK, 4))

    wide = [p for p in plist if p.dim() > 1]
    elems = sum(p.numel() for p in wide)

    def per_tensor():
        for p in wide:
            _lib.check(lib.dvsof_grad_centralize(p.grad.data_ptr(), p.shape[0],
                                                 p.numel() // p.shape[0], _lib.stream()), 'gc')
    med, best = event_ms(per_tensor, a.reps)
    say(what='centralisation, one launch per tensor', tensors=len(wide), elements=elems,
        event_ms_median=round(med, 4), event_ms_min=round(best, 4))
    if hasattr(optim, 'centralize_rows'):
        rows, n_rows = optim.centralize_rows([p.grad for p in wide])
        med, best = event_ms(lambda: _lib.check(lib.dvsof_grad_centralize_multi(
            rows.data_ptr(), n_rows, _lib.stream()), 'gc multi'), a.reps)
        say(what='centralisation, multi-tensor launch', tensors=len(wide), rows=n_rows,
            elements=elems, event_ms_median=round(med, 4), event_ms_min=round(best, 4))
    else:
        say(what='centralisation, multi-tensor launch', event_ms_median=None,
            note='not measured: no dvsof_grad_centralize_multi on this commit')


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--dtypes', nargs='+', default=['f32', 'bf16s'])
    p.add_argument('--optimizers', nargs='+', default=['ranger', 'adamw'],
                   choices=('ranger', 'adamw'))
    p.add_argument('--legs', nargs='+', default=['eager', 'replay'], choices=('eager', 'replay'))
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--block-steps', type=int, default=40)
    p.add_argument('--warmup', type=int, default=20)
    p.add_argument('--reps', type=int, default=31, help='repetitions of the update-alone timings')
    p.add_argument('--fused', action='store_true',
                   help='optim.fuse_into_backward in both legs (bench.py does so for f32)')
    p.add_argument('--guard', action='store_true',
                   help='measure the step guard (guard off against guard on, the statistic '
                        'kernels alone) instead of the legs above')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('optim_bench: no GPU; nothing is measured without one')
    say(what='config', device=torch.cuda.get_device_name(0), B=B, H=H, W=W, bins=BINS,
        events_per_sample=H * W, blocks=a.blocks, block_steps=a.block_steps, warmup=a.warmup)
    if a.guard:
        for optimizer in a.optimizers:
            guard_steps(a, optimizer)
        guard_alone(a)
        return
    for dtype in a.dtypes:
        for optimizer in a.optimizers:
            steps(a, optimizer, dtype)
    update_alone(a)


if __name__ == '__main__':
    main()
