"""The step guard on the device (docs/STEP_GUARD_SPEC.md): the statistic
against numpy float64 on the chunk edges, the vector tail, a misaligned
tensor and two parameter groups; the guarded updates of FusedAdamW, FusedRAdam
and FusedRanger never binding (bitwise the unguarded step), clipping (against
the CPU restatements fed the clipped gradients) and skipping (nothing
written, counters advance); the captured step (tests/step_guard_child.py);
train_flownet.main with a NaN pixel in one batch."""
import json
import math
import os
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CHILD = Path(__file__).resolve().parent / 'step_guard_child.py'
DEV = 'cuda'

# the chunk edges of a 1024-element work item, the vector tail, channels_last weights
FLAT = [1, 3, 1023, 1024, 1025, 4099]
CONV = [(32, 5, 3, 3), (64, 130, 3, 3)]
OFFSET_N = 1029         # viewed at +4 bytes from a larger buffer: the misaligned-vector path


def chunk():
    from dvs_of_training_framework_amd import _lib
    return _lib.lib().dvsof_adamw_chunk_elems()


class Params:
    """Two parameter groups: [flat sizes + the +4-byte view + one parameter
    without a gradient] | [channels_last conv weights + a zero-element tensor]."""

    def __init__(self):
        g = torch.Generator().manual_seed(11)
        self.flat = [torch.randn(n, generator=g).to(DEV).requires_grad_(True) for n in FLAT]
        self.buffer = torch.randn(OFFSET_N + 3, generator=g).to(DEV)
        self.offset = self.buffer[1:1 + OFFSET_N].requires_grad_(True)
        assert self.offset.data_ptr() % 16 == 4 and self.offset.is_leaf
        self.no_grad = torch.randn(77, generator=g).to(DEV).requires_grad_(True)
        self.conv = [torch.randn(s, generator=g).to(DEV).contiguous(
            memory_format=torch.channels_last).requires_grad_(True) for s in CONV]
        self.empty = torch.zeros(0, device=DEV, requires_grad=True)
        self.with_grad = self.flat + [self.offset] + self.conv
        self.groups = [{'params': self.flat + [self.offset, self.no_grad]},
                       {'params': self.conv + [self.empty]}]
        self.n = sum(p.numel() for p in self.with_grad)

    def set_grads(self, grads):
        """grads: one CPU float32 tensor per parameter of ``with_grad``."""
        for p, g in zip(self.with_grad, grads):
            if p is self.offset:
                gbuf = torch.zeros(OFFSET_N + 3, device=DEV)
                gbuf[1:1 + OFFSET_N] = g.to(DEV)
                p.grad = gbuf[1:1 + OFFSET_N]
                assert p.grad.data_ptr() % 16 == 4
            elif p.dim() == 4:
                p.grad = g.to(DEV).contiguous(memory_format=torch.channels_last)
            else:
                p.grad = g.to(DEV)
        self.no_grad.grad = None
        self.empty.grad = torch.zeros(0, device=DEV)


def random_grads(seed=3, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * scale for s in
            [(n,) for n in FLAT] + [(OFFSET_N,)] + CONV]


def statistic(grads, max_norm, skip=True):
    """One guarded AdamW step over ``Params`` with these gradients ->
    (record as a dict, its 32 bytes)."""
    from dvs_of_training_framework_amd.optim import FusedAdamW
    ps = Params()
    ps.set_grads(grads)
    opt = FusedAdamW(ps.groups, lr=1e-3)
    opt.set_guard(max_norm, skip)
    opt.step()
    rec = opt.guard_state()
    raw = opt.guard_tensors()[0].cpu().numpy().tobytes()
    assert len(raw) == 32 and struct.unpack('<fIdIIII', raw)[3:] == \
        (rec['bad'], rec['skipped'], rec['clipped'], rec['consecutive'])
    return rec, raw, ps


def ref_norm(grads):
    """numpy float64 norm of the same gradients."""
    return math.sqrt(sum(float((g.numpy().astype(np.float64) ** 2).sum()) for g in grads))


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def ref_scale(max_norm, norm):
    return 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))


def check_statistic(rec, grads, max_norm):
    n = sum(g.numel() for g in grads)
    ref = ref_norm(grads)
    print('norm', rec['norm'], 'ref', ref, 'scale', rec['scale'], 'ref', ref_scale(max_norm, ref))
    assert abs(rec['norm'] - ref) <= n * 2.0 ** -53 * ref       # a float64 sum in any order
    assert ulps(rec['scale'], ref_scale(max_norm, ref)) <= 1
    assert rec['bad'] == 0 and not rec['skip'] and rec['skipped'] == 0
    assert rec['clipped'] == (1 if rec['scale'] < 1 else 0) and rec['consecutive'] == 0


@pytest.mark.parametrize('max_norm', [None, 1.0, 1e9])
def test_statistic_of_random_gradients(max_norm):
    grads = random_grads()
    rec, _, ps = statistic(grads, max_norm)
    assert ps.n == sum(g.numel() for g in grads) == 7175 + OFFSET_N + 1440 + 74880
    check_statistic(rec, grads, max_norm)
    assert (rec['scale'] < 1) == (max_norm == 1.0)


@pytest.mark.parametrize('max_norm', [None, 1.0])
def test_statistic_of_all_zero_gradients(max_norm):
    grads = [torch.zeros_like(g) for g in random_grads()]
    rec, _, _ = statistic(grads, max_norm)
    assert rec['norm'] == 0.0 and rec['scale'] == 1.0 and rec['clipped'] == 0
    assert rec['bad'] == 0 and not rec['skip']


def test_one_huge_element_stays_finite():
    """3e38 squared overflows float32 (and its square root would be Inf): the
    squares are taken in float64."""
    grads = random_grads()
    grads[5][2000] = 3e38
    rec, _, _ = statistic(grads, 1e35)
    check_statistic(rec, grads, 1e35)
    assert math.isfinite(rec['norm']) and rec['norm'] >= 3e38 * (1 - 1e-7)
    assert 0 < rec['scale'] < 1e-3


def test_tiny_elements_do_not_flush_to_zero():
    """1e-30 squared is 0 in float32."""
    grads = [torch.full_like(g, 1e-30) for g in random_grads()]
    rec, _, _ = statistic(grads, 1e-29)
    check_statistic(rec, grads, 1e-29)
    assert rec['norm'] > 1e-28


def places():
    """(tensor index in Params.with_grad, element) of the four places."""
    c = chunk()
    assert c < 4099 and 4099 % 4 == 3
    return {'first': (5, 0), 'last_tail': (5, 4098), 'inside_chunk': (5, c + c // 2 + 1),
            'chunk_first': (5, c)}


@pytest.mark.parametrize('value', [float('nan'), float('inf'), float('-inf')])
@pytest.mark.parametrize('place', ['first', 'last_tail', 'inside_chunk', 'chunk_first'])
def test_one_non_finite_element_is_counted_and_skips(place, value):
    grads = random_grads()
    t, i = places()[place]
    grads[t][i] = value
    rec, _, ps = statistic(grads, 1.0, skip=True)
    assert rec['bad'] == 1 and rec['skip'] and math.isnan(rec['norm'])
    assert rec['skipped'] == 1 and rec['consecutive'] == 1 and rec['clipped'] == 0
    assert rec['scale'] == 1.0
    fresh = Params()        # a skipped step wrote nothing
    for p, q in zip(ps.with_grad, fresh.with_grad):
        assert torch.equal(p, q)


def test_non_finite_elements_everywhere_are_counted_exactly():
    """In every tensor: the first and the last element and, in the
    channels_last weights and the misaligned view, one in the middle; skipping
    off: counted, not skipped."""
    grads = random_grads()
    want = 0
    for k, g in enumerate(grads):
        flat = g.view(-1)
        for i in {0, flat.numel() - 1, flat.numel() // 2}:
            flat[i] = [float('nan'), float('inf'), float('-inf')][(i + k) % 3]
            want += 1
    rec, _, _ = statistic(grads, 1.0, skip=False)
    assert rec['bad'] == want and not rec['skip'] and rec['skipped'] == 0
    assert math.isnan(rec['norm']) and rec['scale'] == 1.0


def test_two_calls_give_the_same_bytes():
    grads = random_grads(seed=8, scale=2.5)
    a = statistic(grads, 1.0)
    b = statistic(grads, 1.0)
    assert a[1] == b[1] and a[0]['clipped'] == 1


# ------------------------------------------------------------------ updates
SHAPES = [(32, 5, 3, 3), (32,), (64, 130, 3, 3), (2, 32, 1, 1), (4099,)]
KINDS = ['adamw', 'radam', 'ranger']
HYPER = dict(lr=2e-3, weight_decay=1e-2)


def fused(kind, params):
    from dvs_of_training_framework_amd.optim import FusedAdamW, FusedRAdam, FusedRanger
    if kind == 'adamw':
        return FusedAdamW(params, amsgrad=True, **HYPER)
    return (FusedRAdam if kind == 'radam' else FusedRanger)(params, **HYPER)


def oracle(kind, params):
    from oracle.ref_optim import RefRAdam, RefRanger
    if kind == 'adamw':
        return torch.optim.AdamW(params, amsgrad=True, **HYPER)
    return (RefRAdam if kind == 'radam' else RefRanger)(params, **HYPER)


def oracle_count_a_skipped_step(kind, ro):
    """The step counter advances on a skipped step; nothing else moves."""
    if kind == 'adamw':
        for st in ro.state.values():
            st['step'] += 1
    else:
        ro.t += 1


def initial():
    torch.manual_seed(5)
    return [torch.randn(s) * 0.1 for s in SHAPES]


def device_params(ps):
    out = []
    for p in ps:
        q = p.clone().to(DEV)
        if q.dim() == 4:
            q = q.contiguous(memory_format=torch.channels_last)
        out.append(q.requires_grad_(True))
    return out


def step_grads(step):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(s, generator=g) * (1 + 0.1 * step) for s in SHAPES]


def put_grads(params, grads):
    for x, g in zip(params, grads):
        gx = g.to(DEV)
        x.grad = gx.contiguous(memory_format=torch.channels_last) if x.dim() == 4 else gx


def state_tensors(opt, params):
    """(empty before the first step: the state is made there)"""
    return [opt.state[p][n] for p in params for n in type(opt).STATE if n in opt.state[p]]


def snapshot(opt, params):
    return [t.detach().clone() for t in list(params) + state_tensors(opt, params)]


def bitwise(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize('kind', KINDS)
def test_a_guard_that_never_binds_changes_no_bit(kind):
    ps = initial()
    a, b = device_params(ps), device_params(ps)
    fa, fb = fused(kind, a), fused(kind, b)
    fb.set_guard(max_norm=1e30, skip_nonfinite=True)
    for step in range(13):
        grads = step_grads(step)
        put_grads(a, grads)
        put_grads(b, grads)
        fa.step()
        fb.step()
        assert bitwise(snapshot(fa, a), snapshot(fb, b)), (kind, step)
        assert [fa.state[p]['step'] for p in a] == [fb.state[p]['step'] for p in b]
    rec = fb.guard_state()
    assert rec['scale'] == 1.0 and rec['clipped'] == rec['skipped'] == rec['bad'] == 0
    assert not bitwise(a, device_params(ps))


MAX_NORM = 100.0    # the smallest step norm of the seeded run is ~sqrt(80515) = 284


@pytest.mark.parametrize('kind', KINDS)
def test_clipping_matches_the_oracle_fed_the_clipped_gradients(kind):
    ps = initial()
    a = device_params(ps)
    b = [p.clone().requires_grad_(True) for p in ps]
    fo, ro = fused(kind, a), oracle(kind, b)
    fo.set_guard(max_norm=MAX_NORM)
    n = sum(p.numel() for p in ps)
    for step in range(13):
        grads = step_grads(step)
        put_grads(a, grads)
        fo.step()
        rec = fo.guard_state()
        ref = ref_norm(grads)       # of the RAW gradients: before Ranger centralises them
        assert ref > MAX_NORM and abs(rec['norm'] - ref) <= n * 2.0 ** -53 * ref
        assert ulps(rec['scale'], MAX_NORM / (ref + 1e-6)) <= 1 and rec['scale'] < 1
        scale = torch.tensor(rec['scale'], dtype=torch.float32)
        for y, g in zip(b, grads):
            y.grad = g * scale
        ro.step()
        for x, y in zip(a, b):
            err = (x.detach().cpu() - y.detach()).abs().max()
            assert err <= 5e-6 * y.abs().max() + 1e-7, (kind, step, float(err))
    assert fo.guard_state()['clipped'] == 13 and fo.guard_state()['skipped'] == 0


@pytest.mark.parametrize('kind', KINDS)
def test_poisoned_steps_write_nothing_and_the_run_goes_on(kind):
    """Steps 4 and 6 (1-based; 6 is a Lookahead step of Ranger) carry one NaN
    in one tensor."""
    ps = initial()
    a = device_params(ps)
    b = [p.clone().requires_grad_(True) for p in ps]
    fo, ro = fused(kind, a), oracle(kind, b)
    fo.set_guard(max_norm=None, skip_nonfinite=True)
    skipped = 0
    for step in range(1, 14):
        grads = step_grads(step)
        poisoned = step in (4, 6)
        if poisoned:
            grads[2].view(-1)[70001] = float('nan')
        put_grads(a, grads)
        before = snapshot(fo, a)
        fo.step()
        after = snapshot(fo, a)
        rec = fo.guard_state()
        assert {fo.state[p]['step'] for p in a} == {step}       # counted whatever the outcome
        if poisoned:
            skipped += 1
            assert bitwise(before, after), (kind, step)
            assert rec['skip'] and rec['bad'] == 1 and rec['consecutive'] == 1
            oracle_count_a_skipped_step(kind, ro)
        else:
            assert not bitwise(before, after)
            assert not rec['skip'] and rec['bad'] == 0 and rec['consecutive'] == 0
            for y, g in zip(b, grads):
                y.grad = g.clone()
            ro.step()
        assert rec['skipped'] == skipped and rec['clipped'] == 0
        for x, y in zip(a, b):
            err = (x.detach().cpu() - y.detach()).abs().max()
            assert err <= 5e-6 * y.abs().max() + 1e-7, (kind, step, float(err))
    assert skipped == 2


def test_the_workspace_is_allocated_once_and_regrown_eagerly():
    from dvs_of_training_framework_amd.optim import FusedAdamW
    ps = Params()
    ps.set_grads(random_grads())
    opt = FusedAdamW(ps.groups, lr=1e-3)
    opt.set_guard(1.0)
    record = opt.guard_tensors()[0]
    opt.step()
    work = opt.guard_tensors()[1]
    for _ in range(3):
        ps.set_grads(random_grads())
        opt.step()
    assert opt.guard_tensors()[0] is record and opt.guard_tensors()[1] is work
    assert record.data_ptr() % 8 == 0 and work.numel() * 8 >= 16 * 89
    opt.set_guard(2.0, False)       # new settings, the same record and counters
    assert opt.guard_tensors()[0] is record and opt.guard_state()['clipped'] == 4


# ------------------------------------------------------------ captured step
def child(scenario, loopback=None):
    env = dict(os.environ)
    env.pop('DVSOF_LOOPBACK', None)
    if loopback:
        env['DVSOF_LOOPBACK'] = loopback
    out = subprocess.run([sys.executable, str(CHILD), scenario], capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize('kind,accum,loopback', [
    ('ranger', 1, None), ('adamw', 2, None), ('adamw', 1, '2:50'), ('ranger', 2, '2:50')])
def test_guarded_replay_equals_its_guarded_eager_twin(kind, accum, loopback):
    """training.train(capture=True) against capture=False under the same
    guard: 6 good steps, a step whose batch holds one NaN pixel, one more good
    step.  Under the loopback communicator (world 2: every bucket comes back
    halved, late) the record's norm is the norm of the EXCHANGED buckets."""
    r = child(f'{kind}:{accum}', loopback)
    assert r['replays'] >= 7 * accum and r['failed'] is None, r
    assert r['roles'] == (['full'] if accum == 1 else ['first', 'last']), r
    assert r['weights_equal'] == [True] * 8 and r['records_equal'] == [True] * 8, r
    assert r['rows_equal'] and r['n_rows'] > 0, r
    for leg in ('eager', 'captured'):
        x = r[leg]
        assert x['skipped'] == [0] * 6 + [1, 1] and x['consecutive'] == [0] * 6 + [1, 0], x
        assert x['moved'] == [True] * 6 + [False, True], x      # the NaN step wrote nothing
        assert x['bad'][6] > 0 and x['bad'][:6] == [0] * 6 and x['bad'][7] == 0, x
        assert x['state_moved'] == [True] * 6 + [False, True], x
        assert x['logged_skipped'] == x['skipped'], x
    assert r['unheld'] == [] and r['audited'] > 0, r
    assert r['guard_kernels'] == [1, 1], r       # partials + close, in the closing role only
    if loopback:
        assert r['comm']['loopback'] and r['comm']['ranks'] == 2, r
        assert r['exchange_violations'] == [] and r['marks'] > 0, r
        if kind == 'adamw':     # (Ranger centralises the buckets in place after the statistic)
            for leg in ('eager', 'captured'):
                for got, want in r[leg]['norm_vs_buckets'][:6]:
                    assert abs(got - want) <= r['n_params'] * 2.0 ** -53 * want, (got, want)


# ---------------------------------------------------------------- end to end
class Log:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, x):
        self.rows.append((tag, value, x))


class PoisonedLoader:
    """The run's own loader; batch 3 carries one NaN pixel -- row 18, column
    27 of its first frame: one the loss reads (the frame pyramid is a cascade
    from an 8 x 8 level that takes rows / columns 0, 9, ..., 63 of a 64 x 64
    frame; the other pixels are never loaded)."""

    def __init__(self, inner):
        self.inner = inner

    def __iter__(self):
        for i, batch in enumerate(self.inner, 1):
            if i == 3:
                images = batch['images'].clone()
                images.view(-1)[18 * 64 + 27] = float('nan')
                batch = dict(batch, images=images)
            yield batch


def run_main(monkeypatch, out, *more):
    import train_flownet as tf
    pkg = Path(tf.__file__).resolve().parent / 'dvs_of_training_framework_amd'
    made, log = [], Log()
    real_loader = tf.make_train_loader

    class Recording(tf.Serializer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    with monkeypatch.context() as m:
        m.setattr(tf, 'Serializer', Recording)
        m.setattr(tf, 'make_logger', lambda args, rank: log)
        m.setattr(tf, 'make_train_loader', lambda *a, **k: PoisonedLoader(real_loader(*a, **k)))
        torch.manual_seed(0)
        tf.main(['-m', str(out), '--flownet_path', str(pkg), '--height', '64', '--width', '64',
                 '-lr', '1e-3', '--event-representation-depth', '3', '--synthetic',
                 '--synthetic-events', '3000', '-bs', '2', '-mbs', '2', '-ne', '6',
                 '-d', 'cuda:0', *more])
    return made[0], log


def tensors_of(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from tensors_of(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from tensors_of(v)


@pytest.mark.parametrize('capture', [False, True])
def test_a_nan_pixel_costs_one_step_with_the_flags(monkeypatch, tmp_path, capture):
    more = ['--capture'] if capture else []
    s, log = run_main(monkeypatch, tmp_path / 'm', '--skip-nonfinite-steps',
                      '--clip-grad-norm', '1.0', *more)
    assert s.refused == []
    file = torch.load(tmp_path / 'm' / 'step_6.pt', weights_only=True)
    ts = list(tensors_of(file))
    assert len(ts) > 10 and all(bool(torch.isfinite(t).all()) for t in ts if t.is_floating_point())
    skipped = [v for t, v, _ in log.rows if t == 'General/skipped steps']
    assert skipped == [0, 0, 1, 1, 1, 1]
    norms = [v for t, v, _ in log.rows if t == 'General/gradient norm']
    assert len(norms) == 6 and math.isnan(norms[2])
    assert all(math.isfinite(v) and v > 0 for v in norms[:2] + norms[3:])
    assert {int(st['step']) for st in file['optimizer']['state'].values()} == {6}


def test_without_the_flags_the_same_run_is_poisoned(monkeypatch, tmp_path):
    s, log = run_main(monkeypatch, tmp_path / 'm')
    assert s.refused and s.refused[-1][0] == 6 and not (tmp_path / 'm' / 'step_6.pt').exists()
    assert not any(t.startswith('General/skipped') for t, _, _ in log.rows)
