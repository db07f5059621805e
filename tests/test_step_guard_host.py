"""CPU checks of the step guard (docs/STEP_GUARD_SPEC.md): the flags and how
they resolve ``--optimizer-in-backward``, the exclusion of ``set_guard`` and
``fuse_into_backward``, the rank-agreement backstop, the torch-optimizer
fallback (training.HostGuard) and the new entry points of the C ABI."""
import math

import pytest
import torch

from dvs_of_training_framework_amd import _lib, optim, parallel, training
from dvs_of_training_framework_amd.timer import FakeTimer

NEW_SYMBOLS = ('dvsof_grad_guard', 'dvsof_grad_guard_record_bytes',
               'dvsof_grad_guard_partial_bytes', 'dvsof_adamw_step_guarded',
               'dvsof_adamw_step_dyn_guarded', 'dvsof_radam_step_guarded',
               'dvsof_radam_step_dyn_guarded')


def parse(tmp_path, *more):
    import train_flownet as tf
    return tf.parse_args(['-m', str(tmp_path / 'm'), '--synthetic', *more])


def test_flags_default_to_off(tmp_path):
    args = parse(tmp_path)
    assert args.clip_grad_norm is None and args.skip_nonfinite_steps is False
    assert args.max_skipped_steps == 32
    assert args.optimizer_in_backward == 'auto'     # nothing to resolve without a guard


@pytest.mark.parametrize('flags', [('--clip-grad-norm', '1.5'), ('--skip-nonfinite-steps',),
                                   ('--clip-grad-norm', '1.5', '--skip-nonfinite-steps')])
def test_auto_resolves_to_off_with_a_guard_and_on_is_an_error(tmp_path, flags, capsys):
    args = parse(tmp_path, *flags)
    assert args.optimizer_in_backward == 'off'
    assert args.clip_grad_norm == (1.5 if '--clip-grad-norm' in flags else None)
    assert args.skip_nonfinite_steps == ('--skip-nonfinite-steps' in flags)
    assert parse(tmp_path, *flags, '--optimizer-in-backward', 'off').optimizer_in_backward == 'off'
    with pytest.raises(SystemExit) as e:
        parse(tmp_path, *flags, '--optimizer-in-backward', 'on')
    assert e.value.code == 2                        # argparse's own error exit
    assert '--optimizer-in-backward on cannot be combined' in capsys.readouterr().err
    # without a guard an explicit `on` stays what it was
    assert parse(tmp_path, '--optimizer-in-backward', 'on').optimizer_in_backward == 'on'


def test_a_clip_value_must_be_positive(tmp_path):
    for bad in ('0', '-1'):
        with pytest.raises(SystemExit):
            parse(tmp_path, '--clip-grad-norm', bad)


class _Predictor:
    bucket_hook = None


@pytest.mark.parametrize('cls', [optim.FusedAdamW, optim.FusedRAdam, optim.FusedRanger])
def test_guard_and_fuse_into_backward_exclude_each_other_in_both_orders(cls):
    def make():
        return cls([torch.zeros(4, requires_grad=True)], lr=1e-3)
    opt = make()
    opt.set_guard(max_norm=1.0)
    with pytest.raises(ValueError, match='set_guard'):
        opt.fuse_into_backward(_Predictor())
    assert not hasattr(opt, 'fused_active')         # the refused request left nothing behind
    opt = make()
    opt.fuse_into_backward(_Predictor())
    with pytest.raises(ValueError, match='fuse_into_backward'):
        opt.set_guard(skip_nonfinite=True)
    assert opt._guard is None
    # removing a guard frees the other way again
    opt = make()
    opt.set_guard(max_norm=2.0, skip_nonfinite=False)
    opt.set_guard(None, False)
    opt.fuse_into_backward(_Predictor())
    with pytest.raises(ValueError):
        make().set_guard(max_norm=0.0)


def test_the_guard_adds_nothing_to_the_state_dict():
    a, b = (optim.FusedRanger([torch.zeros(4, requires_grad=True)], lr=1e-3) for _ in range(2))
    a.set_guard(max_norm=1.0)
    assert a.state_dict() == b.state_dict()


def test_rank_agreement_check():
    rec = dict(skipped=1, clipped=0)
    with pytest.raises(RuntimeError) as e:
        parallel.check_guard_agreement(rec, gather=lambda mine: [(1, 0), (0, 0)])
    assert '(1, 0)' in str(e.value) and '(0, 0)' in str(e.value) and 'rank 1' in str(e.value)
    seen = []

    def gather(mine):
        seen.append(mine)
        return [mine, mine, mine]
    assert parallel.check_guard_agreement(rec, gather=gather) == (1, 0)
    assert seen == [(1, 0)]                         # what a rank contributes is its own counters
    with pytest.raises(RuntimeError):               # the clipped counter is compared too
        parallel.check_guard_agreement(rec, gather=lambda mine: [(1, 0), (1, 0), (1, 3)])


def toy():
    torch.manual_seed(0)
    a = torch.nn.Parameter(torch.randn(3, 5))
    b = torch.nn.Parameter(torch.randn(7))
    return [a, b]


def test_host_guard_clips_like_clip_grad_norm_and_skips_non_finite_steps():
    params = toy()
    twin = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt = torch.optim.AdamW(params, lr=1e-2)
    ref = torch.optim.AdamW(twin, lr=1e-2)
    guard = training.HostGuard(max_norm=0.5, skip_nonfinite=True)
    torch.manual_seed(1)
    for step in range(5):
        grads = [torch.randn_like(p) * 3 for p in params]
        poisoned = step == 2
        for p, q, g in zip(params, twin, grads):
            p.grad, q.grad = g.clone(), g.clone()
        if poisoned:
            params[1].grad[3] = float('inf')
        before = [p.detach().clone() for p in params]
        state_before = {k: {n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.items()}
                        for k, st in opt.state.items()}
        admitted = guard.admit(opt)
        if admitted:
            opt.step()
        rec = guard.state()
        if poisoned:
            assert not admitted and rec['skip'] and rec['bad'] == 1 and math.isnan(rec['norm'])
            assert all(torch.equal(p, q) for p, q in zip(params, before))
            for k, st in opt.state.items():
                for n, v in st.items():
                    assert torch.equal(v, state_before[k][n]) if torch.is_tensor(v) \
                        else v == state_before[k][n]
            assert rec['consecutive'] == 1 and rec['skipped'] == 1
            continue
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
        assert admitted and rec['norm'] == pytest.approx(norm, rel=1e-12)
        assert rec['scale'] == pytest.approx(0.5 / (norm + 1e-6), rel=1e-12) and rec['scale'] < 1
        assert rec['consecutive'] == 0
        torch.nn.utils.clip_grad_norm_(twin, 0.5)
        ref.step()
        for p, q in zip(params, twin):
            assert torch.equal(p, q)
    assert guard.state()['clipped'] == 4 and guard.state()['skipped'] == 1


def test_host_guard_without_clipping_leaves_the_gradients_alone():
    params = toy()
    opt = torch.optim.SGD(params, lr=0.1)
    guard = training.HostGuard(max_norm=None, skip_nonfinite=False)
    for p in params:
        p.grad = torch.full_like(p, 100.0)
    params[0].grad[0, 0] = float('nan')
    assert guard.admit(opt)                 # counted, not skipped: skipping is off
    rec = guard.state()
    assert rec['bad'] == 1 and not rec['skip'] and rec['scale'] == 1.0 and rec['skipped'] == 0
    assert float(params[1].grad[0]) == 100.0


class _Log:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, x):
        self.rows.append((tag, value, x))


class _Scheduler:
    def step(self):
        pass


def _toy_train(guard, poison, steps=6, max_skipped=32, log=None):
    """training.train over a two-tensor toy model with a torch optimizer on
    the CPU; ``poison(step)``: the gradient of that step is non-finite."""
    params = toy()

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = params

        def forward(self, payload, timestamps, sample_idx, size, raw=True, intermediate=True):
            flow = (self.a.sum() + self.b.sum()) * payload
            return [flow.reshape(1, 1, 1, 1)], timestamps, sample_idx, None

    def evaluator(flows, *rest, **kw):
        return ((flows[0].sum(),),) * 3

    def loader():
        for i in range(steps):
            value = float('nan') if poison(i + 1) else 1.0
            yield {'timestamps': torch.zeros(1), 'sample_idx': torch.zeros(1, dtype=torch.long),
                   'images': torch.zeros(1, 1, 2, 2), 'data': torch.tensor(value), 'size': 1}
    model = Model()
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    log = log or _Log()
    training.train(model, 'cpu', loader(), opt, steps, _Scheduler(), log, evaluator,
                   is_raw=False, timers=FakeTimer(), guard=guard,
                   max_skipped_steps=max_skipped)
    return model, log


def test_train_logs_the_guard_and_skips_with_a_torch_optimizer():
    guard = training.HostGuard(max_norm=1.0, skip_nonfinite=True)
    model, log = _toy_train(guard, poison=lambda step: step == 3)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    skipped = [v for t, v, _ in log.rows if t == 'General/skipped steps']
    assert skipped == [0, 0, 1, 1, 1, 1]
    norms = [v for t, v, _ in log.rows if t == 'General/gradient norm']
    assert len(norms) == 6 and math.isnan(norms[2]) and all(math.isfinite(n) for n in norms[3:])
    assert guard.state()['clipped'] == 5            # |grad| = sqrt(22) > 1 on every finite step
    # without a guard the same run poisons the parameters: what the guard is for
    model, log = _toy_train(None, poison=lambda step: step == 3)
    assert not any(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert not any(t.startswith('General/skipped') for t, _, _ in log.rows)


def test_train_aborts_after_max_skipped_steps_in_a_row():
    guard = training.HostGuard(skip_nonfinite=True)
    with pytest.raises(RuntimeError, match=r'step 4: the last 3 optimizer steps were skipped'):
        _toy_train(guard, poison=lambda step: step >= 2, max_skipped=3)
    # interrupted runs of skips do not add up
    guard = training.HostGuard(skip_nonfinite=True)
    _toy_train(guard, poison=lambda step: step in (1, 2, 4, 5), max_skipped=3)
    assert guard.state()['skipped'] == 4 and guard.state()['consecutive'] == 0


def test_new_symbols_are_declared_exported_and_registered():
    declared = _lib.declared_symbols()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib._SIGNATURES and hasattr(lib, name), name
    assert lib.dvsof_grad_guard_record_bytes() == 32
    assert lib.dvsof_grad_guard_partial_bytes() == 16
    # a guarded twin takes its twin's arguments, then the record, then the stream
    for name in ('dvsof_adamw_step', 'dvsof_adamw_step_dyn', 'dvsof_radam_step',
                 'dvsof_radam_step_dyn'):
        res, args = _lib._SIGNATURES[name]
        gres, gargs = _lib._SIGNATURES[name + '_guarded']
        assert gres is res and gargs[:len(args) - 1] == args[:-1] and len(gargs) == len(args) + 1
    # bad arguments are refused on the host, before anything is enqueued
    assert lib.dvsof_grad_guard(None, 5, None, None, 0, None, 0, 1.0, 1, None, None) == -1
    assert lib.dvsof_grad_guard(None, 5, None, None, 3, None, 0, 1.0, 1, 4096, None) == -1
    assert lib.dvsof_grad_guard(4096, 5, 4096, 4096, 3, 4096, 47, 1.0, 1, 4096, None) == -2
    assert lib.dvsof_grad_guard(4096, 5, 4096, 4096, 3, 4096, 48, float('nan'), 1, 4096,
                                None) == -1
    assert lib.dvsof_adamw_step_guarded(4096, 4096, 4096, 1, 1e-3, .9, .999, 1e-8, 0., 1, 0,
                                        None, None) == -1
    assert optim.GUARD_FIELDS == ('scale', 'skip', 'norm', 'bad', 'skipped', 'clipped',
                                  'consecutive')
