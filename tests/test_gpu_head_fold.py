"""The small kernels between the conv layers against the references of
tests/head_fold_cases.py: dvsof_flow_head_fwd / dvsof_flow_heads_fwd / dvsof_flow_head_bwd /
dvsof_flow_head_reduce / dvsof_act_bwd (csrc/conv_head.hip), dvsof_flow_fold_weights / _bias /
_grads (csrc/flowfold.hip) and Mish, forward and derivative (act_fwd / act_bwd of
csrc/conv_common.h), through the C ABI.

Every output buffer has 64 guard elements on both sides, is prefilled with NaN (the guards
with a sentinel), and is checked after the call: guards unchanged, no NaN where a value is
due.  Every call runs twice into fresh buffers and the two results are equal bit for bit
(both files claim fixed-order reductions).

'int' data: the result EQUALS the integer reference (every sum is exact in float32 in any
order; tests/test_head_fold_oracle.py checks the range) -- the pin on indexing: a dropped,
duplicated or misplaced pixel, channel, workgroup or border line fails whatever the
tolerance.  Equality is of values: a float32 sum of products that are all -0 is -0 where the
integer reference has 0; everything else about the bits is fixed by the value.  'rnd' data:
per element within the a-priori rounding bound of the kernel's own accumulation order
(head_fold_cases: d_head_*, fold_*_ref).

Paths.  Head widths 16 ... 256 are the five template instances (PPW = 16 ... 1 pixels per
wave).  (1,1,1): one lane group active; (1,1,PPW+1): a ragged wave; (3,5,7): image
boundaries inside a wave; (2,12,20): several trips in the forward; stride_shape(C): the
backward's grid-stride loop (its 512-row workspace is asserted) with a ragged last wave.  The
option matrix of the backward runs in full (2 + 3 x 4 x 2 x 2 launches) at C = 32 and 128.  HEADS_CASES: n = 1 ... 4, the
predictor's own set, a one-workgroup head between larger ones, a NULL bias.  FOLD_CASES: the
three member orders, no skip member, Cx below / across / at whole 64-lane passes, Cout * 9 no
multiple of 16, the second channel pass of the border sums (Cout = 1030), frames of one line,
one column and 2 x 2, the 8-way unrolled border loop on both axes and on W only.

Mish, measured on the MI355X in the units of head_fold_cases.mish_fwd_unit / mish_bwd_unit,
per range [-104,-87) [-87,-20) [-20,0) [0,20) [20,100] (allowed: K32 + 4 = 8.5 forward,
7.5 derivative; the forward also gets, once and outside the units, half a denormal spacing,
2^-150: at x = 1e-45 no float32 is nearer to f):
    forward     1.00  1.26  4.03  1.64  1.00
    derivative  0.99  1.30  3.17  3.10  1.00     (from 20 up to FLT_MAX: 1.00)
(the float32 emulation with correctly rounded operations: 0.00 1.26 4.01 1.57 1.00 and
0.00 1.30 3.03 2.95 1.00; below -87.3 the hardware exp2 gives 0 where the emulation keeps a
denormal.)

NOT covered: the forward head's cap of 65 535 workgroups (about 1 GiB of input to reach).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import head_fold_cases as hc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
GUARD = 64
SENTINEL = -12345.5
EINVAL, ENOSPACE = -1, -2


def conv():
    from dvs_of_training_framework_amd import conv as C
    return C


def L():
    return conv()._lib.lib()


def stream():
    return conv()._lib.stream()


def dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=F32)).to(DEV)


class Out:
    """A guarded float32 (or 16-bit) device buffer: .t is the part a kernel may write."""

    def __init__(self, shape, init=None, bits16=False):
        n = int(np.prod(shape))
        self.n, self.bits16 = n, bits16
        if bits16:
            self.buf = torch.full((n + 2 * GUARD,), 0x5a5a, dtype=torch.int16, device=DEV)
            self.buf[GUARD:GUARD + n] = 0x7fc0          # a bf16 NaN
        else:
            self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
            self.buf[GUARD:GUARD + n] = float('nan')
        self.t = self.buf[GUARD:GUARD + n]
        if init is not None:
            self.t.copy_(torch.tensor(np.ascontiguousarray(init, dtype=F32)).reshape(-1))
        self.shape = tuple(shape)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self, where, written=True):
        """Guards unchanged; no NaN where a value is due (written=False: all still NaN)
        -> the array."""
        b = self.buf.cpu().numpy()
        g = np.concatenate([b[:GUARD], b[GUARD + self.n:]])
        assert (g == (0x5a5a if self.bits16 else F32(SENTINEL))).all(), f'{where}: guard overwritten'
        a = b[GUARD:GUARD + self.n].reshape(self.shape)
        untouched = (a == 0x7fc0) if self.bits16 else np.isnan(a)
        if written:
            assert not untouched.any(), f'{where}: {int(untouched.sum())} of {a.size} elements not written'
        else:
            assert untouched.all(), f'{where}: written to'
        return a


def ptr(t):
    return None if t is None else (t.ptr if isinstance(t, Out) else t.data_ptr())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int16 if a.dtype.itemsize == 2 else np.int32)


def twice(run, where):
    """run() -> {name: array}; two runs into fresh buffers give the same bits -> the first."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), f'{where}: {k} differs between two runs'
    return a


def exact(got, want, where):
    bad = np.flatnonzero(got.astype(np.float64).ravel() != np.asarray(want, np.float64).ravel())
    if bad.size:
        i = int(bad[0])
        pytest.fail(f'{where}: {bad.size} of {got.size} elements differ from the integer reference; '
                    f'first at flat index {i}: got {got.ravel()[i]!r}, want {np.ravel(want)[i]!r}')


def within(got, want, bound, where):
    err = np.abs(got.astype(np.float64) - want)
    bound = np.broadcast_to(bound, err.shape)
    bad = np.flatnonzero((err > bound).ravel() | ~np.isfinite(got).ravel())
    if bad.size:
        i = int(bad[np.argmax((err.ravel() / np.maximum(bound.ravel(), 1e-300))[bad])])
        pytest.fail(f'{where}: {bad.size} of {got.size} elements outside the rounding bound; worst at '
                    f'flat index {i}: got {got.ravel()[i]!r}, want {np.ravel(want)[i]!r}, error '
                    f'{err.ravel()[i]:.3e}, bound {bound.ravel()[i]:.3e}')


def compare(kind, got, want, bound, where):
    if kind == 'int':
        exact(got, want, where)
    else:
        within(got, want, bound, where)


# ---- flow head forward ---------------------------------------------------------------------
def head_fwd_into(x, w, bias, B, H, W, C):
    flow = Out((B, 2, H, W))
    rc = L().dvsof_flow_head_fwd(ptr(x), ptr(w), ptr(bias), flow.ptr, B, H, W, C, stream())
    return rc, flow


@pytest.mark.parametrize('kind', ['int', 'rnd'])
@pytest.mark.parametrize('C', hc.WIDTHS)
def test_head_forward(C, kind):
    for shape in hc.head_shapes(C):
        d = hc.head_inputs(C, shape, kind)
        x, w, b = dev(d['x']), dev(d['w']), dev(d['bias'])
        for with_bias in (True, False):
            where = f'head_fwd C={C} {shape} {kind} bias={with_bias}'

            def run():
                rc, flow = head_fwd_into(x, w, b if with_bias else None, *shape, C)
                assert rc == 0
                return dict(flow=flow.get(where))
            got = twice(run, where)['flow']
            want, bound, _ = hc.head_fwd_ref(d, with_bias)
            compare(kind, got, want, bound, where)


@pytest.mark.parametrize('kind', ['int', 'rnd'])
@pytest.mark.parametrize('name', list(hc.HEADS_CASES))
def test_heads_forward_in_one_launch(name, kind):
    """Every head's flow equals dvsof_flow_head_fwd of that head alone BIT FOR BIT (the same
    body runs: anything else is a workgroup -> head mapping bug) and the reference."""
    case = hc.HEADS_CASES[name]
    B, heads, n = case['B'], case['heads'], len(case['heads'])
    ds = [hc.head_inputs(C, (B, H, W), kind, seed=i + 1) for i, (C, H, W) in enumerate(heads)]
    xs, ws = [dev(d['x']) for d in ds], [dev(d['w']) for d in ds]
    bs = [None if i == case['bias_none'] else dev(d['bias']) for i, d in enumerate(ds)]
    vp, ci = ctypes.c_void_p, ctypes.c_int

    def run():
        flows = [Out((B, 2, H, W)) for _, H, W in heads]
        rc = L().dvsof_flow_heads_fwd(
            n, (vp * n)(*[ptr(t) for t in xs]), (vp * n)(*[ptr(t) for t in ws]),
            (vp * n)(*[ptr(t) for t in bs]), (vp * n)(*[f.ptr for f in flows]), B,
            (ci * n)(*[h[1] for h in heads]), (ci * n)(*[h[2] for h in heads]),
            (ci * n)(*[h[0] for h in heads]), stream())
        assert rc == 0
        return {f'flow{i}': f.get(f'heads_fwd {name} head {i}') for i, f in enumerate(flows)}
    got = twice(run, f'heads_fwd {name} {kind}')
    for i, ((C, H, W), d) in enumerate(zip(heads, ds)):
        where = f'heads_fwd {name} {kind} head {i} (C={C}, {H}x{W})'
        rc, alone = head_fwd_into(xs[i], ws[i], bs[i], B, H, W, C)
        assert rc == 0
        assert np.array_equal(bits(got[f'flow{i}']), bits(alone.get(where))), \
            f'{where}: differs from the head alone'
        want, bound, _ = hc.head_fwd_ref(d, bs[i] is not None)
        compare(kind, got[f'flow{i}'], want, bound, where)


def test_head_forward_refuses_bad_arguments():
    d = hc.head_inputs(32, (1, 2, 3), 'int')
    x, w = dev(d['x']), dev(d['w'])
    flow = Out((1, 2, 2, 3))
    lib, st = L(), stream()
    assert lib.dvsof_flow_head_fwd(x.data_ptr(), w.data_ptr(), None, flow.ptr, 1, 2, 3, 48, st) == EINVAL
    assert lib.dvsof_flow_head_fwd(x.data_ptr(), w.data_ptr(), None, flow.ptr, 1, 0, 3, 32, st) == EINVAL
    assert lib.dvsof_flow_head_fwd(None, w.data_ptr(), None, flow.ptr, 1, 2, 3, 32, st) == EINVAL
    vp, ci = ctypes.c_void_p, ctypes.c_int

    def heads(n, C=32, H=2, xp=x.data_ptr()):
        m = max(n, 1)
        return lib.dvsof_flow_heads_fwd(
            n, (vp * m)(*[xp] * m), (vp * m)(*[w.data_ptr()] * m), None, (vp * m)(*[flow.ptr] * m), 1,
            (ci * m)(*[H] * m), (ci * m)(*[3] * m), (ci * m)(*[C] * m), st)
    assert heads(0) == EINVAL and heads(5) == EINVAL and heads(1, C=48) == EINVAL
    assert heads(1, H=0) == EINVAL and heads(2, xp=None) == EINVAL
    torch.cuda.synchronize()
    flow.get('refused calls', written=False)       # and no launch


# ---- flow head backward --------------------------------------------------------------------
def run_head_bwd(d, opt, where, short_ws=False):
    """One dvsof_flow_head_bwd with the options (gx, gx_in, act, dbias, gx16) -> arrays."""
    C, B, H, W = d['C'], d['B'], d['H'], d['W']
    want_gx, gx_in, act, want_db, want16 = opt
    lib = L()
    nbytes = lib.dvsof_flow_head_bwd_workspace_bytes(B, H, W, C)
    assert nbytes == hc.bwd_rows(B * H * W, C) * (2 * C + 2) * 4
    x, w, gf = dev(d['x']), dev(d['w']), dev(d['gflow'])
    src = dev(d['actsrc']) if act is not None else None
    gx = Out((B, H, W, C), init=d['gx_in'] if gx_in == 'same' else None) if want_gx else None
    gin = gx if gx_in == 'same' else dev(d['gx_in']) if gx_in == 'given' else None
    dw, db = Out((2, C)), Out((2,)) if want_db else None
    g16 = Out((B, H, W, C), bits16=True) if want16 else None
    ws = Out((nbytes // 4,))
    rc = lib.dvsof_flow_head_bwd(ptr(x), ptr(w), ptr(gf), ptr(gin), ptr(src), act or 0, ptr(gx), dw.ptr,
                                 ptr(db), B, H, W, C, ws.ptr, nbytes - (1 if short_ws else 0), ptr(g16),
                                 stream())
    if short_ws:
        assert rc == ENOSPACE
        torch.cuda.synchronize()
        for o in (gx, dw, db, g16, ws):
            if o is not None and not (o is gx and gx_in == 'same'):
                o.get(where + ' (short workspace)', written=False)
        return None
    assert rc == 0, (where, rc)
    ws.get(where + ' workspace')
    out = dict(dw=dw.get(where + ' dw'))
    if db is not None:
        out['db'] = db.get(where + ' dbias')
    if gx is not None:
        out['gx'] = gx.get(where + ' gx')
    if g16 is not None:
        out['gx16'] = g16.get(where + ' gx16')
    return out


def check_head_bwd(d, opt, where):
    want_gx, gx_in, act, want_db, want16 = opt
    kind = d['kind']
    got = twice(lambda: run_head_bwd(d, opt, where), where)
    r = hc.head_bwd_ref(d, gx_in is not None, act)
    compare(kind, got['dw'], r['dw'], r['dw_bound'], where + ' dw')
    if want_db:
        compare(kind, got['db'], r['db'], r['db_bound'], where + ' dbias')
    if want_gx:
        # (Mish is no integer: its factor is compared like the random data)
        compare('rnd' if act == hc.ACT_MISH else kind, got['gx'], r['gx'], r['gx_bound'], where + ' gx')
        if act == hc.ACT_RELU and kind == 'int':
            zero = d['actsrc'] == 0
            assert zero.any() and (got['gx'][zero] == 0).all(), where + ': ReLU derivative at +-0'
    if want16:
        rne = torch.tensor(got['gx']).to(torch.bfloat16).view(torch.int16).numpy()
        assert np.array_equal(got['gx16'], rne), where + ': gx16 is not gx rounded to nearest even'


@pytest.mark.parametrize('kind', ['int', 'rnd'])
@pytest.mark.parametrize('C', hc.WIDTHS)
def test_head_backward(C, kind):
    stride = hc.stride_shape(C)
    rows = L().dvsof_flow_head_bwd_workspace_bytes(*stride, C) // ((2 * C + 2) * 4)
    assert rows == hc.BWD_CAP == 512        # the grid-stride regime, proven
    for shape in hc.head_shapes(C) + [stride]:
        d = hc.head_inputs(C, shape, kind)
        full = C in hc.FULL_MATRIX_WIDTHS and shape == (3, 5, 7)
        for opt in hc.bwd_options(full):
            check_head_bwd(d, opt, f'head_bwd C={C} {shape} {kind} (gx, gx_in, act, dbias, gx16)={opt}')
    d = hc.head_inputs(C, (3, 5, 7), kind)
    run_head_bwd(d, (True, 'given', hc.ACT_RELU, True, True), f'head_bwd C={C}', short_ws=True)


@pytest.mark.parametrize('C', hc.REDUCE_C)
@pytest.mark.parametrize('rows', hc.REDUCE_ROWS)
def test_head_reduce(rows, C):
    """dvsof_flow_head_reduce alone (any C >= 1): double column sums of random partials;
    with and without dbias."""
    part = hc.rng(4, rows, C).standard_normal((rows, 2 * C + 2)).astype(F32)
    p = dev(part)
    want = part.astype(np.float64).sum(0)
    bound = hc.U * np.abs(want) + 2.0 ** -40 * np.abs(part).astype(np.float64).sum(0)
    for with_db in (True, False):
        where = f'head_reduce rows={rows} C={C} dbias={with_db}'

        def run():
            dw, db = Out((2 * C,)), Out((2,))
            assert L().dvsof_flow_head_reduce(p.data_ptr(), rows, C, dw.ptr, db.ptr if with_db else None,
                                              stream()) == 0
            return dict(dw=dw.get(where), db=db.get(where, written=with_db))
        got = twice(run, where)
        within(got['dw'], want[:2 * C], bound[:2 * C], where + ' dw')
        if with_db:
            within(got['db'], want[2 * C:], bound[2 * C:], where + ' dbias')


# ---- activation backward -------------------------------------------------------------------
def run_act_bwd(dy, src, act, in_place, where):
    n = dy.size
    dz = Out((n,), init=dy if in_place else None)
    dyd, srcd = dz if in_place else dev(dy), dev(src)      # alive until the read below
    assert L().dvsof_act_bwd(ptr(dyd), ptr(srcd), act, dz.ptr, n, stream()) == 0, where
    out = dict(dz=dz.get(where))
    del dyd, srcd
    return out


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('n', hc.ACT_BWD_N)
def test_act_bwd(n, in_place):
    """n = 1 ... 5, 1023, 1025: the float4 body and the scalar tail; 2048 * 1024 + 3: the
    grid-stride loop with a ragged tail.  ACT_NONE / ACT_RELU: the bits of the float32 product
    (zeros of both signs in actsrc); ACT_MISH: within K32_BWD + 4 units of dy f'(s)."""
    r = hc.rng(5, n)
    dy, src = r.standard_normal(n).astype(F32), r.standard_normal(n).astype(F32)
    src[::5], src[2::9] = 0.0, -0.0
    for act in (hc.ACT_NONE, hc.ACT_RELU, hc.ACT_MISH):
        where = f'act_bwd n={n} act={act} in_place={in_place}'
        got = twice(lambda: run_act_bwd(dy, src, act, in_place, where), where)['dz']
        if act == hc.ACT_MISH:
            d1 = hc.mish64(src)[1]
            want = dy.astype(np.float64) * d1
            within(got, want, np.abs(dy) * (hc.K32_BWD + hc.GPU_EXTRA) * hc.mish_bwd_unit(src)
                   + hc.U * np.abs(want), where)
        else:
            want = dy * (np.ones(n, F32) if act == hc.ACT_NONE else (src > 0).astype(F32))
            assert np.array_equal(bits(got), bits(want)), where


def test_act_bwd_of_nothing_touches_nothing():
    dz = Out((8,))
    src = dev(np.zeros(8))
    assert L().dvsof_act_bwd(src.data_ptr(), src.data_ptr(), hc.ACT_MISH, dz.ptr, 0, stream()) == 0
    torch.cuda.synchronize()
    dz.get('act_bwd n=0', written=False)


# ---- Mish over the whole range -------------------------------------------------------------
def test_mish_derivative_over_the_whole_range():
    """act_bwd with ACT_MISH and dy = 1 on the sweep: per range within K32_BWD + 4 units of
    f'; from 20 on within ONE unit of 1, up to FLT_MAX (the product takes the clamped
    argument).  What the formula gives at the ends: +inf as 20 does (the select clamps it),
    NaN stays NaN (the select keeps it, where fminf would have made it 20), -inf gives NaN
    (-inf * 0 in the product, as in the forward)."""
    p = np.concatenate([hc.sweep(), hc.BWD_LARGE, np.array([np.inf, -np.inf, np.nan, 20.0], F32)])
    where = 'mish derivative'
    got = twice(lambda: run_act_bwd_nan_ok(p), where)['dz']
    fin = np.isfinite(p)
    x, g = p[fin], got[fin]
    units = np.abs(g.astype(np.float64) - hc.mish64(x)[1]) / hc.mish_bwd_unit(x)
    per_range = hc.units_by_range(x, units)
    print('mish derivative, units per range', hc.RANGES, ':', ' '.join(f'{v:.2f}' for v in per_range),
          '; from 20 on:', float(units[x >= 20].max()))
    assert np.isfinite(g).all()
    assert max(per_range) <= hc.K32_BWD + hc.GPU_EXTRA, per_range
    assert (np.abs(g[x >= 20].astype(np.float64) - 1) <= hc.mish_bwd_unit(x[x >= 20])).all()
    inf, ninf, nan, twenty = got[-4:]
    assert bits(np.array([inf]))[0] == bits(np.array([twenty]))[0] and np.isnan(nan) and np.isnan(ninf)


def run_act_bwd_nan_ok(p):
    n = p.size
    dz = Out((n,))
    one, src = dev(np.ones(n)), dev(p)      # alive until the read below
    assert L().dvsof_act_bwd(one.data_ptr(), src.data_ptr(), hc.ACT_MISH, dz.ptr, n, stream()) == 0
    b = dz.buf.cpu().numpy()
    del one, src
    assert (b[:GUARD] == F32(SENTINEL)).all() and (b[GUARD + n:] == F32(SENTINEL)).all()
    return dict(dz=b[GUARD:GUARD + n])


def test_mish_forward_over_the_whole_range():
    """act_fwd through ONE exact epilogue: a 3x3, stride 1, pad 1 layer 32 -> 32 at
    4 x 8 x 16 whose weight is 1 on the centre tap where co = ci and whose bias is 0, so
    z = x in value (-0 comes back +0: the zero taps sum to +0) and y = act_fwd(x).  The
    finite sweep points, 16 384 per call.  Allowed: K32_FWD + 4 units and, once, half a
    denormal spacing (head_fold_cases.FWD_FLOOR)."""
    C = conv()
    B, H, W, Cc = 4, 8, 16, 32
    per = B * H * W * Cc
    assert per == 16384
    p = hc.sweep()
    p = np.concatenate([p, np.zeros(-p.size % per, F32)])
    w = np.zeros((Cc, 3, 3, Cc), F32)
    w[np.arange(Cc), 1, 1, np.arange(Cc)] = 1
    wd, bd = dev(w), dev(np.zeros(Cc))
    units = np.zeros(p.size)
    for k in range(p.size // per):
        chunk = p[k * per:(k + 1) * per]
        xd = dev(chunk)
        where = f'mish forward call {k}'

        def run():
            desc = C.make_desc([(xd, Cc, C.NHWC)], B, H, W, Cc, 3, 1, 1, False, act=C.ACT_MISH)
            assert L().dvsof_conv2d_scratch_bytes(ctypes.byref(desc)) == 0
            y, z = Out((per,)), Out((per,))
            assert L().dvsof_conv2d_fwd(ctypes.byref(desc), wd.data_ptr(), bd.data_ptr(), None, y.ptr, z.ptr,
                                        stream()) == 0
            return dict(y=y.get(where + ' y'), z=z.get(where + ' z'))
        got = twice(run, where)
        assert np.array_equal(got['z'], chunk), where + ': z is not x'
        assert not np.signbit(got['z'][chunk == 0]).any(), where + ': a zero of z is not +0'
        units[k * per:(k + 1) * per] = hc.mish_fwd_units(got['y'], chunk)
    per_range = hc.units_by_range(p, units)
    print('mish forward, units per range', hc.RANGES, ':', ' '.join(f'{v:.2f}' for v in per_range))
    assert max(per_range) <= hc.K32_FWD + hc.GPU_EXTRA, per_range


# ---- fold kernels --------------------------------------------------------------------------
FOLD_PARAMS = [(n, k) for n in hc.FOLD_CASES for k in ('int', 'rnd')]


@pytest.mark.parametrize('name,kind', FOLD_PARAMS)
def test_fold_weights(name, kind):
    d = hc.fold_inputs(name, kind)
    w, wh = dev(d['w']), dev(d['wh'])
    where = f'fold_weights {name} {kind}'

    def run():
        out = Out((d['Cout'], 9, d['Ctot'] - 2))
        assert L().dvsof_flow_fold_weights(w.data_ptr(), d['Cout'], d['Ctot'], d['cx_off'], d['Cx'],
                                           d['cf_off'], wh.data_ptr(), out.ptr, stream()) == 0
        return dict(weff=out.get(where))
    want, bound, _ = hc.fold_weights_ref(d)
    compare(kind, twice(run, where)['weff'], want, bound, where)


@pytest.mark.parametrize('name,kind', FOLD_PARAMS)
def test_fold_bias(name, kind):
    """bias_eff and all nine border classes of bias_cls, with and without the layer's bias."""
    d = hc.fold_inputs(name, kind)
    w, bh, bias = dev(d['w']), dev(d['bh']), dev(d['bias'])
    for with_bias in (True, False):
        where = f'fold_bias {name} {kind} bias={with_bias}'

        def run():
            eff, cls = Out((d['Cout'],)), Out((9, d['Cout']))
            assert L().dvsof_flow_fold_bias(w.data_ptr(), d['Cout'], d['Ctot'], d['cf_off'], bh.data_ptr(),
                                            bias.data_ptr() if with_bias else None, eff.ptr, cls.ptr,
                                            stream()) == 0
            return dict(eff=eff.get(where), cls=cls.get(where))
        got = twice(run, where)
        eff, eb, cls, cb, _ = hc.fold_bias_ref(d, with_bias)
        compare(kind, got['eff'], eff, eb, where + ' bias_eff')
        compare(kind, got['cls'], cls, cb, where + ' bias_cls')
        assert (got['cls'][0] == 0).all()       # the interior class loses no tap


def fold_grads_call(d, bufs, ws_short=0, **over):
    a = dict(d, **over)
    lib = L()
    nbytes = lib.dvsof_flow_fold_workspace_bytes(d['B'], d['Cout'])
    ws = Out((nbytes // 4 + 1,))
    rc = lib.dvsof_flow_fold_grads(
        bufs['dW'].ptr, bufs['w'].data_ptr(), a['Cout'], a['Ctot'], a['cx_off'], a['Cx'], a['cf_off'],
        bufs['wh'].data_ptr(), bufs['bh'].data_ptr(), bufs['db'].data_ptr(), bufs['g'].data_ptr(),
        a['B'], a['H'], a['W'], bufs['dwh'].ptr, bufs['dbh'].ptr, ws.ptr, nbytes - ws_short, stream())
    return rc, ws


def fold_bufs(d):
    return dict(dW=Out(d['dW'].shape, init=d['dW']), dwh=Out((2, d['Cx']), init=d['dwh0']),
                dbh=Out((2,), init=d['dbh0']), w=dev(d['w']), wh=dev(d['wh']), bh=dev(d['bh']),
                db=dev(d['db']), g=dev(d['g']))


@pytest.mark.parametrize('name,kind', FOLD_PARAMS)
def test_fold_grads(name, kind):
    """The flow columns of dW (prefilled with NaN) from its x columns and the border sums; dWh
    and dbh ACCUMULATED into non-zero starts (start + increment, one float32 add); the x and
    skip columns of dW keep every bit."""
    d = hc.fold_inputs(name, kind)
    cf = d['cf_off']
    where = f'fold_grads {name} {kind}'

    def run():
        bufs = fold_bufs(d)
        rc, ws = fold_grads_call(d, bufs)
        assert rc == 0
        torch.cuda.synchronize()
        b = ws.buf.cpu().numpy()
        assert (b[:GUARD] == F32(SENTINEL)).all() and (b[-GUARD:] == F32(SENTINEL)).all()
        return dict(dW=bufs['dW'].get(where + ' dW'), dwh=bufs['dwh'].get(where + ' dwh'),
                    dbh=bufs['dbh'].get(where + ' dbh'))
    got = twice(run, where)
    keep = np.ones(d['Ctot'], bool)
    keep[cf:cf + 2] = False
    assert np.array_equal(bits(got['dW'][:, :, keep]), bits(d['dW'][:, :, keep])), \
        where + ': an x or skip column of dW changed'
    r = hc.fold_grads_ref(d)
    compare(kind, got['dW'][:, :, cf:cf + 2], r['flow'], r['flow_bound'], where + ' dW flow columns')
    compare(kind, got['dwh'], r['dwh'], r['dwh_bound'], where + ' dwh')
    compare(kind, got['dbh'], r['dbh'], r['dbh_bound'], where + ' dbh')


BAD_OFFSETS = [dict(cx_off=-1), dict(cf_off=-1), dict(cf_off=-2, cx_off=3),
               dict(cx_off=0, cf_off=10),                   # the flow pair inside the x range
               dict(cx_off=4, cf_off=3),                    # its second column is x's first
               dict(cf_off=24), dict(cf_off=0, cx_off=6),   # past Ctot = 25
               dict(Ctot=2, Cx=1, cx_off=0, cf_off=0)]


def test_fold_entries_refuse_bad_arguments():
    """dvsof_flow_fold_grads refuses what dvsof_flow_fold_weights refuses (negative offsets,
    overlapping x / flow ranges, ranges past Ctot, Ctot < 3) with EINVAL before any launch; a
    short workspace is ENOSPACE."""
    d = hc.fold_inputs('xsf_20_5_6x10', 'int')
    assert d['Ctot'] == 25 and d['Cx'] == 20
    bufs = fold_bufs(d)
    weff = Out((d['Cout'], 9, d['Ctot'] - 2))
    for over in BAD_OFFSETS:
        a = dict(d, **over)
        rc, _ = fold_grads_call(d, bufs, **over)
        assert rc == EINVAL, ('fold_grads', over, rc)
        rc = L().dvsof_flow_fold_weights(bufs['w'].data_ptr(), a['Cout'], a['Ctot'], a['cx_off'], a['Cx'],
                                         a['cf_off'], bufs['wh'].data_ptr(), weff.ptr, stream())
        assert rc == EINVAL, ('fold_weights', over, rc)
    rc, _ = fold_grads_call(d, bufs, ws_short=1)
    assert rc == ENOSPACE
    torch.cuda.synchronize()
    weff.get('refused fold_weights', written=False)
    assert np.array_equal(bits(bufs['dW'].buf.cpu().numpy()[GUARD:-GUARD]), bits(d['dW'].ravel()))
    assert np.array_equal(bufs['dwh'].get('refused'), d['dwh0']) and np.array_equal(bufs['dbh'].get('refused'), d['dbh0'])
    rc, _ = fold_grads_call(d, bufs)
    assert rc == 0          # and the good arguments pass
