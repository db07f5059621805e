"""CPU checks of the optimizer oracles (tests/optim_cases.py; docs/OPTIM_SPEC.md): the
float32 oracle against the published algorithms in float64, its step scalars against the
library's host entry points bit for bit, the premise of the centralisation cases, and that
every case tells the mutants of its branches from the oracle on the GPU test's own inputs."""
import ctypes
import math

import numpy as np
import pytest

from dvs_of_training_framework_amd import _lib, optim  # noqa: F401  (optim registers the entry points)
from tests import optim_cases as oc

F = np.float32


def chunk():
    return _lib.lib().dvsof_adamw_chunk_elems()


def world():
    sp = oc.specs(chunk())
    return sp, oc.initial(sp)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_numpy_float32_keeps_denormals_and_the_slice_reaches_them():
    """The premise of the denormal slice: numpy does not flush, and (1 - beta2) g g of the
    slice IS a float32 denormal."""
    sp, _ = world()
    assert F(1e-30) * F(1e-10) != 0
    g = oc.step_grads(sp, 1)[f'flat{oc.EXTREME}'][oc.TINY]
    term = (oc.ONE - F(0.999)) * g * g
    tiny = np.finfo(F).tiny
    assert (term < tiny).all() and (term > 0).mean() > 0.9, (term.min(), term.max())


def test_the_table_is_the_issue_table():
    c = chunk()
    sp, p0 = world()
    sizes = {s.shape[0] for s in sp if s.layout == 'flat' and s.offset == 0 and s.grad}
    assert sizes >= {1, 2, 3, 4, 5, 1023, 1024, 1025, 1027, c - 1, c, c + 1, 2 * c + 3, 4099, 0}
    assert [s.offset for s in sp if s.offset] == [1, 2, 3]
    assert {s.shape for s in sp if s.layout == 'cl'} == {(32, 5, 3, 3), (64, 130, 3, 3), (2, 32, 1, 1)}
    assert any(s.shape == (16, 40) for s in sp) and any(not s.grad for s in sp)
    assert 8e4 < sum(p.size for p in p0.values()) < 1.2e5
    assert [int(np.prod(s[1:])) for s in oc.GC_SHAPES] == oc.GC_ROW_LENGTHS


@pytest.mark.parametrize('case', oc.CASES, ids=lambda c: c.name)
def test_float32_oracle_against_the_float64_algorithm(case):
    """Per element, the worst error over the 13 steps in units of 2^-24 x the element's
    magnitude budget of the float64 run (oc.UNITS); ordinary elements only."""
    sp, p0 = world()
    o32, o64 = oc.Oracle32(case, sp, p0), oc.Oracle64(case, sp, p0)
    live = [s for s in sp if s.grad and s.shape[0] > 0]
    err = {s.name: dict.fromkeys('pmvx', 0.0) for s in live}
    prev = {s.name: p0[s.name].astype(np.float64) for s in live}
    budget = {s.name: dict(p=np.abs(prev[s.name]), m=0.0, v=0.0) for s in live}
    for t in range(1, oc.STEPS + 1):
        grads = oc.step_grads(sp, t)
        o32.step(grads)
        o64.step(grads)
        for s in live:
            a, b = o32.arrays(s.name), o64.arrays(s.name)
            bud = budget[s.name]
            bud['p'] = bud['p'] + np.abs(b['p'] - prev[s.name])
            bud['m'] = np.maximum(bud['m'], np.abs(b['m']))
            bud['v'] = np.maximum(bud['v'], b['v'])
            prev[s.name] = b['p']
            for q in 'pmvx':
                if b[q] is not None:
                    err[s.name][q] = np.maximum(err[s.name][q], np.abs(a[q].astype(np.float64) - b[q]))
        if case.kind == 'radam' and not case.hyper['degenerated_to_sgd'] and t <= 5:
            # the published rule: no update and no decay while the variance is not tractable
            for s in live:
                assert np.array_equal(bits(o32.p[s.name]), bits(p0[s.name])), (s.name, t)
                assert np.array_equal(o64.arrays(s.name)['p'], p0[s.name].astype(np.float64))
                assert o32.m[s.name].any() and o32.v[s.name].any()
    worst = dict.fromkeys('pmvx', 0.0)
    for s in live:
        mask = oc.ordinary(s)
        for q in 'pmvx':
            e = err[s.name][q]
            if np.isscalar(e):      # the variant has no such buffer
                continue
            b = budget[s.name]['p' if q == 'x' and case.kind == 'ranger' else 'v' if q == 'x' else q]
            assert (e[b == 0] == 0).all(), (s.name, q)
            units = (e / (oc.EPS24 * np.where(b > 0, b, 1.0)))[mask]
            worst[q] = max(worst[q], float(units.max()))
    print(case.name, 'worst units of 2^-24 x budget:', {q: round(u, 3) for q, u in worst.items()})
    for q in 'pmvx':
        assert worst[q] <= oc.UNITS[case.kind][q], (case.name, q, worst[q])


def _adam_row(lr, b1, b2, t):
    out = (ctypes.c_float * 3)()
    _lib.lib().dvsof_adamw_dynamic(lr, b1, b2, t, out)
    return np.array(list(out), dtype=F)


def _radam_row(lr, b1, b2, t, thr, flags, k):
    out = (ctypes.c_float * 4)()
    _lib.lib().dvsof_radam_dynamic(lr, b1, b2, t, thr, flags, k, out)
    return np.array(list(out), dtype=F)


@pytest.mark.parametrize('betas', oc.BETAS)
def test_step_scalars_equal_the_host_entry_points_bit_for_bit(betas):
    """Steps 1-200: {lr, lr / (1 - b1^t), sqrt(1 - b2^t)} of dvsof_adamw_dynamic and {lr, step
    size or -1, rectified, sync} of dvsof_radam_dynamic under RAdam's flags (with and without
    degenerate-to-SGD) and Ranger's (k = 1, 4, 6)."""
    b1, b2 = betas
    seen = set()
    for lr in (oc.LR, 5e-4, 0.0):
        for t in range(1, 201):
            s = oc.adam_scalars(lr, b1, b2, t)
            want = np.array([s['lr'], s['step_size'], s['bc2_sqrt']], dtype=F)
            assert np.array_equal(bits(_adam_row(lr, b1, b2, t)), bits(want)), (lr, t)
            for ge, deg, k in ((True, True, 0), (True, False, 0), (False, True, 1),
                               (False, True, 4), (False, True, 6)):
                s = oc.radam_scalars(lr, b1, b2, t, 5.0, ge, deg, k)
                want = np.array([s['lr'], s['step_size'], s['rectified'], s['sync']], dtype=F)
                got = _radam_row(lr, b1, b2, t, 5.0, (2 if ge else 0) | (1 if deg else 0), k)
                assert np.array_equal(bits(got), bits(want)), (lr, t, ge, deg, k, got, want)
                seen.add((float(want[1]) == -1.0, bool(want[2]), bool(want[3])))
    assert seen == {(True, False, False), (False, False, False), (False, True, False),
                    (False, False, True), (False, True, True)}


def test_no_centralised_row_lies_near_a_rounding_boundary():
    """The premise of comparing a float64 sum in the kernel's order with the exact one: zero
    rows excluded, in the centralisation cases and in every centralised gradient of the
    13 steps of the table."""
    assert sum(oc.unsafe_rows(g) for g in oc.gc_grads('normal')[:-1]) == 0
    sp, _ = world()
    rows = 0
    for t in range(1, oc.STEPS + 1):
        grads = oc.step_grads(sp, t)
        for s in sp:
            if len(s.shape) > 1:
                assert oc.unsafe_rows(grads[s.name]) == 0, (s.name, t)
                rows += s.shape[0]
    assert rows == oc.STEPS * (32 + 64 + 2 + 16)


def test_dyadic_rows_sum_exactly_in_any_order():
    rng = np.random.default_rng(0)
    for g in oc.gc_grads('dyadic')[:-1]:
        for row in g.reshape(g.shape[0], -1).astype(np.float64):
            exact = math.fsum(row.tolist())
            assert float(np.sum(row)) == exact == float(np.cumsum(rng.permutation(row))[-1])


def _differs(case, mut, sp, p0, guarded):
    """Whether the mutant leaves the oracle bitwise in any compared array at any step."""
    a, b = oc.Oracle32(case, sp, p0), oc.Oracle32(case, sp, p0, mutant=mut)
    for t in range(1, oc.STEPS + 1):
        grads = oc.step_grads(sp, t, huge=not guarded)
        scale = oc.ref_scale(grads, oc.MAX_NORM) if guarded else None
        assert scale is None or scale < 1
        a.step(grads, scale)
        b.step(grads, scale)
        for s in sp:
            if not s.grad:
                continue
            x, y = a.arrays(s.name), b.arrays(s.name)
            if any(not np.array_equal(bits(x[q]), bits(y[q])) for q in 'pmvx') or \
                    not np.array_equal(bits(a.g[s.name]), bits(b.g[s.name])):
                return True
    return False


@pytest.mark.parametrize('mut', oc.MUTANTS)
def test_every_case_tells_the_mutant_from_the_oracle(mut):
    sp, p0 = world()
    claimed = 0
    for case in oc.CASES:
        if oc.covers(mut, case):
            claimed += 1
            assert _differs(case, mut, sp, p0, False), (mut, case.name)
    for name in oc.GUARD_CASES:
        if oc.covers(mut, oc.BY_NAME[name], guarded=True):
            claimed += 1
            assert _differs(oc.BY_NAME[name], mut, sp, p0, True), (mut, name, 'guarded')
    assert claimed > 0, mut


@pytest.mark.parametrize('kind', ['dyadic', 'normal'])
@pytest.mark.parametrize('mut', ['gc_f32_mean', 'gc_whole_mean'])
def test_the_centralisation_cases_tell_the_mutants(kind, mut):
    grads = oc.gc_grads(kind)[:-1]
    assert any(not np.array_equal(bits(oc.centralize(g)), bits(oc.centralize(g, mut)))
               for g in grads)
