"""Case tables, float64 references and a-priori error bounds for the small kernels between
the conv layers: the 1x1 flow heads and the elementwise activation backward
(csrc/conv_head.hip), the flow member folded into weight space (csrc/flowfold.hip) and Mish
(act_fwd / act_bwd of csrc/conv_common.h).  tests/test_head_fold_oracle.py ties the
references to float64 autograd and measures the Mish yardstick; tests/test_gpu_head_fold.py
runs the kernels against them.

Two kinds of data.  'int': small integers (|v| <= 3 for activations and gradients, <= 2 for
weights), so that every sum is an integer below 2^24 and exact in float32 IN ANY ORDER -- the
kernel must give the integer reference exactly.  'rnd': standard normal float32, compared per
element against float64 with the rounding bound of the kernel's own accumulation:

    u = 2^-24.  A float32 sum whose longest path from a term to the result passes d
    roundings (a product counts one, every add one) is within gamma(d) * sum |t_i| of the
    exact sum, gamma(d) = d u / (1 - d u).  A float64 accumulator contributes only its final
    cast, u |result| (its own roundings, 2^-53 per add, are covered by a 2^-40 relative term).

Each d below is read off the kernel and derived beside its definition.  No constant here is
fitted to what a kernel returns.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
F32 = np.float32
EXACT = 2 ** 24
ACT_NONE, ACT_RELU, ACT_MISH = 0, 1, 2


def gamma(d):
    return d * U / (1 - d * U)


def rng(*key):
    return np.random.default_rng([7, *[int(k) for k in key]])


def ints(r, shape, m):
    return r.integers(-m, m + 1, size=shape).astype(F32)


def data(r, shape, kind, m=3):
    """'int': integers in [-m, m]; 'rnd': standard normal.  float32."""
    return ints(r, shape, m) if kind == 'int' else r.standard_normal(shape).astype(F32)


# ---- flow head ---------------------------------------------------------------------------
WIDTHS = (16, 32, 64, 128, 256)
BWD_CAP = 512           # head_blocks(): workgroups of the backward = rows of its partials


def ppw(C):
    """Pixels per wave: C/4 lanes share a pixel."""
    return 64 // (C // 4)


def head_shapes(C):
    """(B, H, W): one pixel (one lane group active); a wave and one pixel (ragged tail); 105
    pixels (image boundaries inside a wave: the pixel -> (b, r) split); several iterations
    per wave in the forward."""
    return [(1, 1, 1), (1, 1, ppw(C) + 1), (3, 5, 7), (2, 12, 20)]


def stride_shape(C):
    """The smallest B = 3 shape with B H W > 2048 PPW (the backward's 512 workgroups of
    4 waves each get a second trip of the grid-stride loop) that is no multiple of PPW (a
    ragged last wave) -- at C = 256 PPW is 1 and every count is a multiple."""
    p = ppw(C)
    hw = 2048 * p // 3 + 1
    while p > 1 and (3 * hw) % p == 0:
        hw += 1
    h = max(d for d in range(1, int(math.isqrt(hw)) + 1) if hw % d == 0)
    assert 3 * hw > 2048 * p
    return 3, h, hw // h


def bwd_rows(total, C):
    return min(BWD_CAP, max(1, -(-total // (4 * ppw(C)))))


def bwd_iters(total, C):
    """Trips of head_bwd_kernel's pixel loop for the busiest lane:
    ceil(pixels / (workgroups * 4 waves * PPW))."""
    return -(-total // (bwd_rows(total, C) * 4 * ppw(C)))


def d_head_fwd(C):
    """head_fwd_body: a product (1), three adds inside the lane's float4 (3), log2(C/4)
    shuffle stages, the bias add (1)."""
    return 1 + 3 + int(math.log2(C // 4)) + 1


def d_head_gx(has_addend):
    """head_bwd_kernel: g0 w0 + g1 w1 is a product (1) and an add (1); + gx_in (1)."""
    return 2 + (1 if has_addend else 0)


def d_head_dw(total, C):
    """a0 += g0 * v: a product (1) and one add per trip (iters); log2(PPW) shuffle stages
    over the lanes with the same channels; (red0 + red1) + (red2 + red3) in LDS (2).  The
    reduce over the workgroups is double: u |result| on top."""
    return 1 + bwd_iters(total, C) + int(math.log2(ppw(C))) + 2


def d_head_db(total, C):
    """s0 += g0 per trip (iters), the six stages of wave_sum, the LDS combine (2); then
    double."""
    return bwd_iters(total, C) + 6 + 2


def head_inputs(C, shape, kind, seed=0):
    B, H, W = shape
    r = rng(1, C, B, H, W, kind == 'int', seed)
    d = dict(C=C, B=B, H=H, W=W, kind=kind,
             x=data(r, (B, H, W, C), kind), w=data(r, (2, C), kind, 2), bias=data(r, 2, kind, 2),
             gflow=data(r, (B, 2, H, W), kind), gx_in=data(r, (B, H, W, C), kind),
             actsrc=data(r, (B, H, W, C), kind))
    if kind == 'int':       # exact zeros of both signs where ReLU's derivative is 0
        z = d['actsrc'].reshape(-1)
        z[::7], z[3::11] = 0.0, -0.0
    return d


def head_fwd_ref(d, with_bias):
    """-> (flow [B,2,H,W] float64, bound, largest partial magnitude)."""
    x, w = d['x'].astype(np.float64), d['w'].astype(np.float64)
    b = d['bias'].astype(np.float64) if with_bias else np.zeros(2)
    flow = np.einsum('bhwc,fc->bfhw', x, w) + b[None, :, None, None]
    mag = np.einsum('bhwc,fc->bfhw', np.abs(x), np.abs(w)) + np.abs(b)[None, :, None, None]
    check_exact_range(d, float(mag.max()), 'head forward')
    return flow, gamma(d_head_fwd(d['C'])) * mag, float(mag.max())


def relu_d(s):
    return (s > 0).astype(np.float64)


def head_bwd_ref(d, gx_in, act):
    """act: None (no actsrc) or ACT_*.  -> dict of float64 references and bounds.  gx is
    given as its pre-activation sum `g`, the derivative `da` and their product."""
    C, total = d['C'], d['B'] * d['H'] * d['W']
    x, w, gf = (d[k].astype(np.float64) for k in ('x', 'w', 'gflow'))
    g = np.einsum('bfhw,fc->bhwc', gf, w)
    gmag = np.einsum('bfhw,fc->bhwc', np.abs(gf), np.abs(w))
    if gx_in:
        g, gmag = g + d['gx_in'], gmag + np.abs(d['gx_in'])
    gb = gamma(d_head_gx(gx_in)) * gmag
    s = d['actsrc'].astype(np.float64)
    if act is None or act == ACT_NONE:
        da, dab = np.ones_like(g), 0.0
    elif act == ACT_RELU:
        da, dab = relu_d(s), 0.0
    else:
        da = mish64(s)[1]
        dab = (K32_BWD + GPU_EXTRA) * mish_bwd_unit(s)
    out = dict(g=g, da=da, gx=g * da,
               # |da| gb + |g| dab: the two factors' own errors; the product's rounding
               gx_bound=np.abs(da) * gb + (np.abs(g) + gb) * dab + U * np.abs(g * da) * (act is not None))
    dw = np.einsum('bfhw,bhwc->fc', gf, x)
    dwmag = np.einsum('bfhw,bhwc->fc', np.abs(gf), np.abs(x))
    db, dbmag = gf.sum((0, 2, 3)), np.abs(gf).sum((0, 2, 3))
    out.update(dw=dw, db=db,
               dw_bound=gamma(d_head_dw(total, C)) * dwmag + U * np.abs(dw) + 2.0 ** -40 * dwmag,
               db_bound=gamma(d_head_db(total, C)) * dbmag + U * np.abs(db) + 2.0 ** -40 * dbmag,
               partial=float(max(gmag.max(), dwmag.max(), dbmag.max())))
    check_exact_range(d, out['partial'], 'head backward')
    return out


# the option matrix of dvsof_flow_head_bwd: (gx, gx_in, act, dbias, gx16)
#   gx: given?   gx_in: 'given' | None | 'same' (the buffer of gx)   act: None | ACT_*
def bwd_options(full):
    if not full:
        # the other widths and shapes: everything on; in place, no activation, no dbias
        return [(True, 'given', ACT_RELU, True, True), (True, 'same', None, False, True)]
    # gx None x dbias, then the cross product gx_in x act x dbias x gx16: 2 + 48 launches
    out = [(False, None, None, True, False), (False, None, None, False, False)]
    for gx_in in ('given', None, 'same'):
        for act in (None, ACT_RELU, ACT_MISH, ACT_NONE):
            for dbias in (True, False):
                for gx16 in (True, False):
                    out.append((True, gx_in, act, dbias, gx16))
    return out


FULL_MATRIX_WIDTHS = (32, 128)

# dvsof_flow_heads_fwd: [(C, H, W)] per launch, B; bias_none: the head whose bias is NULL.
# 'predictor': the predictor's own four heads at a small frame.  'one_block_between': the
# middle head is ONE workgroup (16 pixels of 64 channels, 64 per workgroup) between two of
# several.  n = 1 ... 4.
HEADS_CASES = {
    'n1': dict(B=2, heads=[(64, 3, 5)], bias_none=None),
    'n2': dict(B=3, heads=[(16, 9, 11), (256, 1, 3)], bias_none=1),
    'n3_one_block_between': dict(B=1, heads=[(32, 16, 20), (64, 4, 4), (128, 5, 9)], bias_none=0),
    'n4_predictor': dict(B=2, heads=[(256, 2, 3), (128, 4, 6), (64, 8, 12), (32, 16, 24)],
                         bias_none=2),
    'n4_mixed': dict(B=3, heads=[(16, 1, 1), (32, 7, 13), (16, 6, 43), (256, 3, 3)], bias_none=3),
}
HEAD_FWD_ITERS = 4


def fwd_blocks(total, C):
    return max(1, -(-total // (4 * ppw(C) * HEAD_FWD_ITERS)))


REDUCE_ROWS = (1, 63, 64, 65, 200)
REDUCE_C = (16, 100)

ACT_BWD_N = (1, 2, 3, 4, 5, 1023, 1025, 2048 * 1024 + 3)


# ---- Mish ----------------------------------------------------------------------------------
K32_FWD = 4.5           # measured 4.014: test_head_fold_oracle.py::test_k32_constants
K32_BWD = 3.5           # measured 3.033
GPU_EXTRA = 4           # the hardware exp2 and the two reciprocals, ~1 ulp each assumed; one slack
RANGES = ((-104.0, -87.0), (-87.0, -20.0), (-20.0, 0.0), (0.0, 20.0), (20.0, 100.0001))
TWENTY = F32(20)
SPECIAL = np.array([0.0, -0.0, 20.0, np.nextafter(TWENTY, F32(0)), np.nextafter(TWENTY, F32(40)),
                    -87.0, -88.5, -103.0, 88.0, 1e-30, -1e-30, 1e-45], F32)
BWD_LARGE = np.array([1e6, 1e9, 1e10, 1e12, 1e30, np.finfo(F32).max], F32)
TINY = 2.0 ** -126


@functools.lru_cache(maxsize=None)
def sweep():
    """~500 k float32 points: uniform in [-104, 100] and in [-25, 25], standard normal, the
    special points.  Read-only."""
    r = rng(2)
    p = np.concatenate([r.uniform(-104, 100, 200_000), r.uniform(-25, 25, 200_000),
                        r.standard_normal(100_000)]).astype(F32)
    p = np.concatenate([SPECIAL, p])
    p.setflags(write=False)
    return p


def mish64(x):
    """-> (f, f', f'') of Mish in float64 at the float32 points x.  With n = e^x,
    t = n (n + 2): tanh(softplus x) = t / (t + 2), 1 - tanh = 2 / (t + 2) without
    cancellation; q = d tanh(sp) / dx = (1 - tanh^2) sigmoid;
    f = x th, f' = th + x q, f'' = q (2 + x (1 - sg - 2 th sg)).  Past 50 th is 1 to 1e-43."""
    x = np.asarray(x, np.float64)
    xc = np.minimum(x, 50.0)
    n = np.exp(xc)
    t = n * (n + 2)
    th, om = t / (t + 2), 2 / (t + 2)
    sg = 1 / (1 + np.exp(-xc))
    q = om * (1 + th) * sg
    return x * th, th + xc * q, q * (2 + xc * (1 - sg - 2 * th * sg))


def mish_parts(x):
    x = np.asarray(x, np.float64)
    xc = np.minimum(x, 50.0)
    n = np.exp(xc)
    t = n * (n + 2)
    th = t / (t + 2)
    return th, (2 / (t + 2)) * (1 + th) / (1 + np.exp(-xc))


def mish_fwd_unit(x):
    """One unit of the forward: u (|f| + |x f'|) + |x| 2^-126.  x f' allows for the one
    rounding of x log2(e), the floor for exp2 flushing to zero below x ~ -87.3."""
    x = np.asarray(x, np.float64)
    f, d1, _ = mish64(x)
    return U * (np.abs(f) + np.abs(x * d1)) + np.abs(x) * TINY


# Half the spacing of the float32 denormals: no float32 is nearer to a result in general
# (x = 1e-45: f = 8.4e-46, the nearest float32 is 5.6e-46 away, the unit there is 1e-52).
# Allowed ONCE on top of the units, not multiplied by them.
FWD_FLOOR = 2.0 ** -150


def mish_fwd_units(got, x):
    """The forward's error in units, after the representation floor."""
    err = np.abs(np.asarray(got, np.float64) - mish64(x)[0])
    return np.maximum(err - FWD_FLOOR, 0) / np.maximum(mish_fwd_unit(x), 1e-300)


def mish_bwd_unit(x):
    """One unit of the derivative:
    u (|tanh sp| + |x (1 - tanh^2 sp) sigmoid| + |x f''|) + max(1, |x|) 2^-126."""
    x = np.asarray(x, np.float64)
    th, q = mish_parts(x)
    d2 = mish64(x)[2]
    xc = np.minimum(np.abs(x), 50.0)        # (q and f'' are 0 to 1e-40 past 50)
    return U * (np.abs(th) + np.abs(xc * q) + np.abs(xc * d2)) + np.maximum(1, np.abs(x)) * TINY


def _exp2_32(a):
    return np.exp2(a.astype(np.float64)).astype(F32)


def _rcp_32(a):
    return (1.0 / a.astype(np.float64)).astype(F32)


def emu_mish_fwd(x):
    """act_fwd's formula in float32, every operation correctly rounded."""
    x = np.asarray(x, F32)
    with np.errstate(over='ignore', invalid='ignore'):
        n = _exp2_32(np.minimum(x, TWENTY) * F32(1.4426950408889634))
        t = n * (n + F32(2))
        return x * (t * _rcp_32(t + F32(2)))


def emu_mish_bwd(x, fixed=True):
    """act_bwd's formula; fixed=False: with the unclamped s in the product, as it was."""
    x = np.asarray(x, F32)
    with np.errstate(over='ignore', invalid='ignore'):
        n = _exp2_32(np.minimum(x, TWENTY) * F32(1.4426950408889634))
        t = n * (n + F32(2))
        r = _rcp_32(t + F32(2))
        th = t * r
        sg = n * _rcp_32(F32(1) + n)
        s = np.where(x > TWENTY, TWENTY, x) if fixed else x
        return th + s * ((F32(2) * r) * (F32(1) + th)) * sg


def units_by_range(x, err_units):
    """Largest error in units per range of RANGES -> list (nan: no point)."""
    out = []
    for lo, hi in RANGES:
        m = (x >= lo) & (x < hi)
        out.append(float(err_units[m].max()) if m.any() else float('nan'))
    return out


# ---- fold kernels --------------------------------------------------------------------------
# name: (layout, Cx, Cs, Cout, B, H, W) -- layout: member order of the layer's input channels
FOLD_CASES = {
    # x first, ragged lanes (Cx = 20 < 64), Cout * 9 = 45 rows (no multiple of 16)
    'xsf_20_5_6x10': ('xsf', 20, 3, 5, 3, 6, 10),
    # flow first; whole lane pass; one-line frame
    'fsx_64_32_1x9': ('fsx', 64, 5, 32, 1, 1, 9),
    # flow in the middle; a ragged second lane pass (96 = 64 + 32); one-column frame
    'sfx_96_32_9x1': ('sfx', 96, 7, 32, 3, 9, 1),
    # no skip member; everything 1
    'xf_1_1_1x1': ('xsf', 1, 0, 1, 1, 1, 1),
    'fsx_1_5_2x2': ('fsx', 1, 4, 5, 3, 2, 2),
    # border sums: a second channel pass of 6 channels (R = 170, 4 idle threads) after one of 1024
    'xsf_4_1030_2x3': ('xsf', 4, 2, 1030, 1, 2, 3),
    # Cout = 256: R = 4 pixel groups, the 8-way unrolled loop needs len > 28: both axes
    'xsf_20_256_30x37': ('xsf', 20, 3, 256, 3, 30, 37),
    # Cout = 64: R = 16, len > 112: W only
    'sfx_64_64_16x120': ('sfx', 64, 2, 64, 1, 16, 120),
    'xf_96_32_6x10': ('xsf', 96, 0, 32, 1, 6, 10),
}
FOLD_NT = 1024


def fold_offsets(layout, Cx, Cs):
    """-> (cx_off, cf_off, skip offset)."""
    order = {'x': Cx, 's': Cs, 'f': 2}
    off, o = {}, 0
    for m in layout:
        off[m] = o
        o += order[m]
    return off['x'], off['f'], off['s']


def takes_unrolled(Cout, length):
    return length > 7 * (FOLD_NT // min(Cout, FOLD_NT))


def fold_inputs(name, kind):
    layout, Cx, Cs, Cout, B, H, W = FOLD_CASES[name]
    cx, cf, cs = fold_offsets(layout, Cx, Cs)
    ctot = Cx + Cs + 2
    r = rng(3, sorted(FOLD_CASES).index(name), kind == 'int')
    d = dict(name=name, kind=kind, Cx=Cx, Cs=Cs, Cout=Cout, B=B, H=H, W=W, Ctot=ctot,
             cx_off=cx, cf_off=cf, cs_off=cs,
             w=data(r, (Cout, 9, ctot), kind, 2), wh=data(r, (2, Cx), kind, 2),
             bh=data(r, 2, kind, 2), bias=data(r, Cout, kind, 2),
             dW=data(r, (Cout, 9, ctot), kind), g=data(r, (B, H, W, Cout), kind),
             dwh0=data(r, (2, Cx), kind), dbh0=data(r, 2, kind))
    d['dW'][:, :, cf:cf + 2] = np.nan
    d['db'] = d['g'].astype(np.float64).sum((0, 1, 2)).astype(F32)
    return d


def fold_weights_ref(d):
    """Weff[co][t][.] (flowfold.hip header): the flow pair leaves, the x columns take
    sum_f Wflow Wh.  v + (a b + c d): two products, two adds on the longest path: d = 3."""
    w, wh = d['w'].astype(np.float64), d['wh'].astype(np.float64)
    cx, cf, Cx = d['cx_off'], d['cf_off'], d['Cx']
    add = np.einsum('rtf,fc->rtc', w[:, :, cf:cf + 2], wh)
    mag = np.abs(w).copy()
    mag[:, :, cx:cx + Cx] += np.einsum('rtf,fc->rtc', np.abs(w[:, :, cf:cf + 2]), np.abs(wh))
    full = w.copy()
    full[:, :, cx:cx + Cx] += add
    keep = [c for c in range(d['Ctot']) if not cf <= c < cf + 2]
    check_exact_range(d, float(mag.max()), 'fold weights')
    return full[:, :, keep], gamma(3) * mag[:, :, keep], float(mag.max())


def _outside(c, t):
    cy, cxx, ky, kx = c // 3, c % 3, t // 3, t % 3
    return (cy == 1 and ky == 0) or (cy == 2 and ky == 2) or (cxx == 1 and kx == 0) or \
        (cxx == 2 and kx == 2)


def fold_bias_ref(d, with_bias):
    """bias_eff[co] = bias + sum_t Wflow[co][t] . bh; bias_cls[c][co] = - the taps that leave
    the frame for border class c = 3 cy + cx (1: first line, 2: last).  tap: two products
    and an add (2); `all`: nine adds; + bias (1): d = 12.  A class sums its k outside taps:
    d = 2 + k."""
    w, bh = d['w'].astype(np.float64), d['bh'].astype(np.float64)
    cf = d['cf_off']
    tap = w[:, :, cf:cf + 2] @ bh
    tmag = np.abs(w[:, :, cf:cf + 2]) @ np.abs(bh)
    b = d['bias'].astype(np.float64) if with_bias else 0.0
    eff, emag = b + tap.sum(1), np.abs(b) + tmag.sum(1)
    cls, cb = np.zeros((9, d['Cout'])), np.zeros((9, d['Cout']))
    for c in range(9):
        out = [t for t in range(9) if _outside(c, t)]
        cls[c] = -tap[:, out].sum(1)
        cb[c] = gamma(2 + len(out)) * tmag[:, out].sum(1)
    check_exact_range(d, float(emag.max()), 'fold bias')
    return eff, gamma(12) * emag, cls, cb, float(emag.max())


def tap_window(t, H, W):
    """The pixels of g whose tap t = 3 ky + kx reads inside the frame (3x3, pad 1)."""
    ky, kx = t // 3, t % 3
    ys = slice(1, H) if ky == 0 else slice(0, H - 1) if ky == 2 else slice(0, H)
    xs = slice(1, W) if kx == 0 else slice(0, W - 1) if kx == 2 else slice(0, W)
    return ys, xs


def fold_grads_ref(d):
    """dWflow, dWh, dbh of the flowfold.hip header, float64, with the bounds:

    border line sums (flow_border_sums_kernel): a thread adds ceil(len / R) pixels in a chain,
    thread 0..cw-1 then adds the R partials in a chain: d_line = ceil(len / R) + R,
    R = 1024 / (channels of the pass).
    G = db - lines + corners (fold_G): db carries u |db| (it is the float32 of the exact sum);
    then k = 1 (centre row or column), or 3 (corner taps: two lines and the corner) float32
    operations per image on the running value: gamma(k B) (|db| + sum |line| + sum |corner|).
    The centre tap is db itself.
    dWflow = (float)(double sum + bh G): |bh| eG + u |result|.
    dbh += (float)(double sum of Wflow G): sum |Wflow| eG + u |t|, then ONE float32 add.
    dWh += (float)(double sum): u |t|, then one float32 add."""
    Cout, B, H, W, Cx = d['Cout'], d['B'], d['H'], d['W'], d['Cx']
    cx, cf = d['cx_off'], d['cf_off']
    g = d['g'].astype(np.float64)
    ag = np.abs(g)
    w, wh, bh = (d[k].astype(np.float64) for k in ('w', 'wh', 'bh'))
    dWx = d['dW'][:, :, cx:cx + Cx].astype(np.float64)
    db = d['db'].astype(np.float64)
    G, eG, Gmag = np.zeros((Cout, 9)), np.zeros((Cout, 9)), np.zeros((Cout, 9))
    line = {0: ag[:, 0].sum(1), 1: ag[:, H - 1].sum(1), 2: ag[:, :, 0].sum(1), 3: ag[:, :, W - 1].sum(1)}
    d_line = {}
    for ln, length in ((0, W), (1, W), (2, H), (3, H)):
        dl = np.zeros(Cout)
        for c0 in range(0, Cout, FOLD_NT):
            cw = min(Cout - c0, FOLD_NT)
            R = FOLD_NT // cw
            dl[c0:c0 + cw] = -(-length // R) + R
        d_line[ln] = dl
    for t in range(9):
        ys, xs = tap_window(t, H, W)
        G[:, t] = g[:, ys, xs].sum((0, 1, 2))
        ky, kx = t // 3, t % 3
        ly = 0 if ky == 0 else 1 if ky == 2 else None
        lx = 2 if kx == 0 else 3 if kx == 2 else None
        lines = [ln for ln in (ly, lx) if ln is not None]
        mag, err = np.abs(db).copy(), U * np.abs(db)
        for ln in lines:
            mag = mag + line[ln].sum(0)
            err = err + gamma(d_line[ln]) * line[ln].sum(0)
        k = len(lines)
        if k == 2:
            y, x = (0 if ly == 0 else H - 1), (0 if lx == 2 else W - 1)
            mag = mag + ag[:, y, x].sum(0)
            k = 3
        Gmag[:, t] = mag
        eG[:, t] = err + (gamma(k * B) * mag if k else 0.0)
    wf = w[:, :, cf:cf + 2]
    dot = np.einsum('rtc,fc->rtf', dWx, wh)
    dotmag = np.einsum('rtc,fc->rtf', np.abs(dWx), np.abs(wh))
    flow = dot + G[:, :, None] * bh
    flow_b = eG[:, :, None] * np.abs(bh) + U * np.abs(flow) + \
        2.0 ** -40 * (dotmag + np.abs(G)[:, :, None] * np.abs(bh))
    inc_wh = np.einsum('rtf,rtc->fc', wf, dWx)
    whmag = np.einsum('rtf,rtc->fc', np.abs(wf), np.abs(dWx))
    inc_bh = np.einsum('rtf,rt->f', wf, G)
    bhmag = np.einsum('rtf,rt->f', np.abs(wf), np.abs(G))
    dwh = d['dwh0'] + inc_wh
    dbh = d['dbh0'] + inc_bh
    # float32 chains: the sum of magnitudes; double sums: the result that is cast
    partial = float(max(Gmag.max(), np.abs(flow).max(), np.abs(inc_wh).max(), np.abs(inc_bh).max(),
                        np.abs(dwh).max(), np.abs(dbh).max(), dotmag.max()))
    check_exact_range(d, partial, 'fold grads')
    return dict(
        G=G, flow=flow, flow_bound=flow_b, dwh=dwh, dbh=dbh, inc_wh=inc_wh, inc_bh=inc_bh,
        dwh_bound=U * np.abs(inc_wh) + 2.0 ** -40 * whmag + U * np.abs(dwh),
        dbh_bound=np.einsum('rtf,rt->f', np.abs(wf), eG) + U * np.abs(inc_bh) + 2.0 ** -40 * bhmag
        + U * np.abs(dbh), partial=partial)


def assert_exact_range(partial, where):
    assert partial < EXACT, f'{where}: largest partial magnitude {partial} is not below 2^24'


def check_exact_range(d, partial, where):
    """Every reference of an 'int' case asserts it itself: no integer case, here or added
    later, can leave the range in which float32 is exact in any order unnoticed."""
    if d.get('kind') == 'int':
        assert_exact_range(partial, f"{where} {d.get('name', '')} C={d.get('C', d.get('Cout'))}")
