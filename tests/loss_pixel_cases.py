"""Well-conditioned inputs and a vectorised NumPy restatement of ONE scale of
the loss (csrc/loss.hip; oracle/dvsof_oracle.c is the scalar form), for the
per-term, per-pixel pin of tests/test_loss_pixel_oracle.py (CPU) and
tests/test_gpu_loss_pixels.py (GPU).  No GPU, no torch.

Reference.  ``reference_scale(prev, nxt, flow, dtype)`` returns, per term
(0 smoothness, 1 photometric, 2 out-of-border): the value, the gradient field
[N,2,h,w] and a SCALE field of the same shape, the sum of the absolute values
of every contribution added into that pixel.  A pixel's smoothness gradient is
a difference of up to 16 pair derivatives that may cancel: an error is only
meaningful against what was added, not against what was left.  The sampling
grid, ``floor`` and the out-of-border comparison are float32 op for op (as in
the C oracle); everything after runs in ``dtype``.  With float32 the power is
``exp2(-0.55 * log2(s))``, the kernel's own formulation (csrc/common.h), so the
float32 evaluation measures that formulation's rounding amplification.

Inputs are well-conditioned BY CONSTRUCTION and the generator asserts it for
every pixel (no pixel is ever excluded from a comparison):
  * flows come from target sample positions, u = tx - x, v = ty - y with
    tx = integer + frac, frac in [0.12, 0.88]: after the float32 round trip
    through the normalised grid no pixel is within 0.1 px of a ``floor`` kink
    or of the strict +-1 border comparison.  The integer part includes -1 and
    w-1 (one tap column outside), fully outside, and +-1e4 px for a few pixels.
    The fractions come in four classes laid out so that the two pixels of
    every smoothness pair differ in class: no pair's flow difference is below
    0.16 in size, which bounds the smallest pair's share of its sum from below;
  * the previous frame is built from the reference's own float64 warp,
    prev = float32(warped +- (8 + U[0,32])), so the photometric residual is at
    least 8 grey levels everywhere (the Charbonnier second derivative at zero
    residual, ~1.8e3, is what makes random frames uncheckable per pixel).  A
    frame that is the start of several samples lies 8 + U[0,32] above the
    largest or below the smallest of their warps;
  * per (sample, scale) the out-of-border population cycles through no pixel,
    exactly one, about 30 %, every pixel.
"""
import functools
import zlib

import numpy as np

F32 = np.float32
TW, TH, WAVE_ROWS = 64, 16, 4      # loss_main_kernel: tile, rows per wave
FIX_QUANTUM = 2.0 ** -21           # rounding of one workgroup's sum to 2^-20
MAX_SCALES = 8                     # DVSOF_MAX_SCALES
FRAC_LO, FRAC_HI = 0.12, 0.88      # drawn; asserted after float32: [0.1, 0.9]
MARGIN = 0.1
RESIDUAL_FLOOR = 8.0
STATES = ('none', 'one', 'some', 'all')

_ALL = slice(None)
# (first operand, second operand, index of the crop count) of the four pair
# directions ->, v, \, / : d = F[first] - F[second]
_PAIRS = (((_ALL, slice(1, None)), (_ALL, slice(0, -1)), 0),
          ((slice(1, None), _ALL), (slice(0, -1), _ALL), 1),
          ((slice(1, None), slice(1, None)), (slice(0, -1), slice(0, -1)), 2),
          ((slice(0, -1), slice(1, None)), (slice(1, None), slice(0, -1)), 2))


def _power(d, dt):
    """s = d^2 + eps^2 and s^(alpha-1), alpha = 0.45, eps = 1e-3."""
    if dt is np.float64:
        s = d * d + 1e-6
        return s, np.power(s, -0.55)
    # log2 and exp2 correctly rounded to float32 (through float64): the
    # measurement then does not depend on the host's vector math library
    s = d * d + F32(1e-6)
    p = F32(-0.55) * np.log2(s.astype(np.float64)).astype(F32)
    return s, np.exp2(p.astype(np.float64)).astype(F32)


def rho(d, dt):
    s, e = _power(d, dt)
    return np.power(s, 0.45) if dt is np.float64 else s * e


def drho(d, dt):
    _, e = _power(d, dt)
    return dt(0.9) * d * e


def _total(v, dt):
    """Sum of per-sample values [N, ...]: float32 sums stay float32 (per
    sample, then over the samples), as a float32 evaluation would."""
    v = np.ascontiguousarray(v).reshape(v.shape[0], -1)
    return float(v.sum(axis=1, dtype=dt).sum(dtype=dt))


def sampling(flow):
    """The float32 part: normalised grid, unnormalised position, floor and the
    strict out-of-border test (utils/loss.py:150-156, :92-94)."""
    flow = np.asarray(flow, F32)
    N, _, h, w = flow.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(F32)
    half_w, half_h = F32((w - 1) / 2.0), F32((h - 1) / 2.0)
    gx = (xs + flow[:, 0]) / half_w - F32(1)
    gy = (ys + flow[:, 1]) / half_h - F32(1)
    ix, iy = (gx + F32(1)) * half_w, (gy + F32(1)) * half_h
    assert gx.dtype == F32 and ix.dtype == F32
    return dict(gx=gx, gy=gy, ix=ix, iy=iy, fx0=np.floor(ix), fy0=np.floor(iy),
                oob=(gx < -1) | (gx > 1) | (gy < -1) | (gy > 1),
                half_w=half_w, half_h=half_h)


def _warp(nxt, s, dt):
    """grid_sample(bilinear, zeros, align_corners=True) of nxt [N,h,w] at the
    positions of ``s``: taps, weights, value, and which pixels have no tap
    inside the frame."""
    N, h, w = nxt.shape
    x0 = np.clip(s['fx0'], -4, w + 4).astype(np.int64)
    y0 = np.clip(s['fy0'], -4, h + 4).astype(np.int64)
    near = (s['fx0'] == x0) & (s['fy0'] == y0)      # else: every tap is outside
    n = np.arange(N)[:, None, None]
    any_in = np.zeros(near.shape, bool)

    def tap(yy, xx):
        ok = near & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        any_in[...] |= ok
        v = nxt[n, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(ok, v, F32(0)).astype(dt)
    nw, ne = tap(y0, x0), tap(y0, x0 + 1)
    sw, se = tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    ax = s['ix'].astype(dt) - s['fx0'].astype(dt)
    ay = s['iy'].astype(dt) - s['fy0'].astype(dt)
    cx, cy = dt(1) - ax, dt(1) - ay
    warped = nw * cx * cy + ne * ax * cy + sw * cx * ay + se * ax * ay
    return dict(nw=nw, ne=ne, sw=sw, se=se, ax=ax, ay=ay, cx=cx, cy=cy,
                warped=warped, all_out=~any_in)


def reference_scale(prev, nxt, flow, dtype=np.float64):
    """One scale.  prev, nxt [N,h,w] float32 (the start / stop frame of every
    sample), flow [N,2,h,w] float32.  -> dict:
      value [3] float64; grad [3,N,2,h,w] ``dtype``; scale [3,N,2,h,w] float64;
      count [N] out-of-border pixels; all_out [N,h,w] no tap inside the frame;
      residual [N,h,w] |warped - prev|; raw: the un-normalised sums and their
      normalisers (for the fixed-point quantum and the detection check)."""
    dt = np.dtype(dtype).type
    flow = np.asarray(flow, F32)
    prev, nxt = np.asarray(prev, F32), np.asarray(nxt, F32)
    N, _, h, w = flow.shape
    assert h > 1 and w > 1, 'a side of 1 is out of scope'
    s = sampling(flow)
    F = flow.astype(dt)
    grad = np.zeros((3, N, 2, h, w), dt)
    scale = np.zeros((3, N, 2, h, w), np.float64)
    value = np.zeros(3)

    # smoothness, utils/loss.py:76-90: every pair once, +t into the first
    # operand's pixel and -t into the second's
    crop = (N * 2 * h * (w - 1), N * 2 * (h - 1) * w, N * 2 * (h - 1) * (w - 1))
    sm_sum, sm_min, sm_norm = [], [], []
    for a, b, ci in _PAIRS:
        a, b = (Ellipsis,) + a, (Ellipsis,) + b
        d = F[a] - F[b]
        val = rho(d, dt)
        t = drho(d, dt) * dt(1.0 / (4.0 * crop[ci]))
        grad[0][a] += t
        grad[0][b] -= t
        scale[0][a] += np.abs(t)
        scale[0][b] += np.abs(t)
        sm_sum.append(_total(val, dt))
        sm_min.append(float(val.min()))
        sm_norm.append(4.0 * crop[ci])
        value[0] += sm_sum[-1] / sm_norm[-1]

    # photometric, utils/loss.py:58-74
    t = _warp(nxt, s, dt)
    d = t['warped'] - prev.astype(dt)
    gp = drho(d, dt) * dt(1.0 / (N * h * w))
    ew, es = t['ne'] - t['nw'], t['se'] - t['sw']      # along x: north, south
    sn, se_ = t['sw'] - t['nw'], t['se'] - t['ne']     # along y: west, east
    grad[1][:, 0] = gp * (ew * t['cy'] + es * t['ay'])
    grad[1][:, 1] = gp * (sn * t['cx'] + se_ * t['ax'])
    scale[1][:, 0] = np.abs(gp) * (np.abs(ew) * t['cy'] + np.abs(es) * t['ay'])
    scale[1][:, 1] = np.abs(gp) * (np.abs(sn) * t['cx'] + np.abs(se_) * t['ax'])
    ph_sum = _total(rho(d, dt), dt)
    value[1] = ph_sum / (float(N) * h * w)

    # out-of-border, utils/loss.py:96-119 (the mask carries no gradient)
    oob = s['oob']
    count = oob.sum(axis=(1, 2)).astype(np.int64)
    k = np.zeros(N, dt)
    k[count > 0] = dt(1) / (dt(2) * count[count > 0].astype(dt) * dt(N))
    grad[2] = np.where(oob[:, None], k[:, None, None, None] * drho(F, dt), dt(0))
    scale[2] = np.abs(grad[2])
    bval = np.where(oob, rho(F[:, 0], dt) + rho(F[:, 1], dt), dt(0))
    b_sum = np.ascontiguousarray(bval).reshape(N, -1).sum(axis=1, dtype=dt)
    b_norm = 2.0 * count * N
    value[2] = float(sum(float(b) / c for b, c in zip(b_sum, b_norm) if c > 0))
    if dt is F32:       # the terms leave as float32
        value = value.astype(F32).astype(np.float64)
    return dict(value=value, grad=grad, scale=scale, count=count,
                all_out=t['all_out'], residual=np.abs(d).astype(np.float64),
                raw=dict(smooth_sum=sm_sum, smooth_min=sm_min,
                         smooth_norm=sm_norm, photo_norm=float(N) * h * w,
                         border_norm=b_norm.astype(np.float64)))


def tiles(h, w):
    return ((h + TH - 1) // TH) * ((w + TW - 1) // TW)


def term_quantum(ref, N, h, w):
    """What rounding every workgroup's sum to the 2^-20 fixed-point grid can
    move a term by: tiles in the group x 2^-21 on the raw sum, divided by the
    term's normaliser (a group = one sample at one scale; the out-of-border
    count is an integer and exact)."""
    raw, per_sample = ref['raw'], tiles(h, w) * FIX_QUANTUM
    q = np.zeros(3)
    q[0] = sum(N * per_sample / n for n in raw['smooth_norm'])
    q[1] = N * per_sample / raw['photo_norm']
    q[2] = sum(per_sample / c for c in raw['border_norm'] if c > 0)
    return q


def position_class(y, x, h, w):
    """Where a pixel sits in the kernel's decomposition (64x16 tile, 4 rows per
    wave, a lane per column): a seam bug then reads as one."""
    tags = []
    if x % TW == 0:
        tags.append('tile column 0')
    if x % TW == TW - 1:
        tags.append('tile column 63')
    if y % WAVE_ROWS == 0:
        tags.append('wave row 0' + (' (tile row 0)' if y % TH == 0 else ''))
    if y % WAVE_ROWS == WAVE_ROWS - 1:
        tags.append('wave row 3' + (' (tile row 15)' if y % TH == TH - 1 else ''))
    if y == h - 1:
        tags.append('last row')
    if x == w - 1:
        tags.append('last column')
    return ', '.join(tags) or 'interior'


# ---------------------------------------------------------------------------
# cases: the smallest shapes that reach each mechanism
# ---------------------------------------------------------------------------
SEAM_SHAPES = ((16, 64), (15, 63), (17, 65), (33, 130), (2, 2), (2, 70), (70, 2))
_SCALES5 = ((5, 7), (17, 65), (2, 2), (16, 64), (9, 12))
_SCALES8 = _SCALES5 + ((33, 130), (4, 66), (18, 3))
MANY_TILES = (2, 257 * TW)         # 257 tiles per sample: second trip of b += 256


def _identity(N):
    return dict(N=N, D=2 * N, start=list(range(N)), stop=list(range(N, 2 * N)))


# Seam cases sample within 3 px of themselves and have no +-1e4 px pixel, and
# the three tile-sized ones have at most one out-of-border pixel (leaving the
# frame from its middle is a flow of half its width): the smoothness sum stays
# small against its smallest pair (the detection check of the tests).  The
# largest one has too many pairs for that check and keeps the full range.
_SEAM_STATE0 = (0, 0, 0, 3, 1, 2, 3)
CASES = {f'seam_{h}x{w}': dict(_identity(2), shapes=((h, w),), state0=s0,
                               **(dict(reach=3, n_far=0) if h * w < 4000 else {}))
         for s0, (h, w) in zip(_SEAM_STATE0, SEAM_SHAPES)}
CASES.update({
    'scales5': dict(_identity(3), shapes=_SCALES5, state0=0),
    'scales8': dict(_identity(3), shapes=_SCALES8, state0=1),
    'many_tiles': dict(_identity(2), shapes=(MANY_TILES,), state0=0),
    'frames': dict(N=4, D=7, start=[3, 0, 5, 3], stop=[6, 1, 2, 4],
                   shapes=((17, 65),), state0=2),
})
CASES.update({f'samples{n}': dict(_identity(n), shapes=((5, 6), (17, 65)), state0=n)
              for n in (1, 9, 65, 129)})
SEAM_CASES = tuple(f'seam_{h}x{w}' for h, w in SEAM_SHAPES)


def _outside(rng, size, shape):
    """Integer parts with both taps of the axis outside the frame."""
    return np.where(rng.random(shape) < 0.5, rng.integers(-3, -1, shape),
                    rng.integers(size, size + 2, shape))


def make_flow(rng, h, w, state, region=None, reach=None, n_far=2):
    """flow [2,h,w] float32 for one sample.  ``state``: which pixels sample
    outside the border (STATES); ``region`` restricts them to a pixel mask;
    ``reach``: inside pixels sample within that many pixels of themselves
    (None: anywhere in the frame); ``n_far``: at most that many +-1e4 px."""
    ys, xs = np.mgrid[0:h, 0:w]
    if reach is None:
        tx = rng.integers(0, w - 1, (h, w))    # both tap columns inside
        ty = rng.integers(0, h - 1, (h, w))
    else:
        tx = np.clip(xs + rng.integers(-reach, reach + 1, (h, w)), 0, w - 2)
        ty = np.clip(ys + rng.integers(-reach, reach + 1, (h, w)), 0, h - 2)
    if state == 'none':
        out = np.zeros((h, w), bool)
    elif state == 'one':
        out = np.zeros((h, w), bool)
        cand = np.flatnonzero(np.ones((h, w), bool) if region is None else region)
        out.flat[rng.choice(cand)] = True
    elif state == 'some':
        out = rng.random((h, w)) < 0.3
    else:
        out = np.ones((h, w), bool)
    if region is not None:
        out &= region
    # how a pixel leaves: one tap column / row outside on either side, both
    # outside, and (rarely) +-1e4 px
    kind = rng.choice(6, (h, w), p=[.2, .2, .2, .2, .1, .1])
    cand = np.flatnonzero(out)
    if n_far and cand.size > 1:
        pick = rng.choice(cand, min(n_far, cand.size - 1), replace=False)
        kind.flat[pick] = rng.integers(6, 8, pick.size)
    far = np.where(rng.random((h, w)) < 0.5, -10000, 10000)
    for k, (axis, val) in enumerate([
            (0, np.full((h, w), -1)), (0, np.full((h, w), w - 1)),
            (1, np.full((h, w), -1)), (1, np.full((h, w), h - 1)),
            (0, _outside(rng, w, (h, w))), (1, _outside(rng, h, (h, w))),
            (0, xs + far), (1, ys + far)]):
        sel = out & (kind == k)
        if axis == 0:
            tx = np.where(sel, val, tx)
        else:
            ty = np.where(sel, val, ty)
    # kind 6 / 7 pixels also leave along the other axis half of the time
    both = out & (kind >= 6) & (rng.random((h, w)) < 0.5)
    ty = np.where(both & (kind == 6), -1, ty)
    tx = np.where(both & (kind == 7), w - 1, tx)
    # fractions: four classes 0.16, 0.39, 0.61, 0.84 (+- 0.03) laid out so that
    # the two pixels of every smoothness pair (->, v, \, /) differ in class:
    # their flow difference is an integer + a fraction difference of 0.17 ..
    # 0.74 in size, so no pair's |difference| is below 0.16 and the smallest
    # pair's share of its sum is bounded below by construction
    base = np.array([0.16, 0.39, 0.61, 0.84])
    fx = base[(xs + 2 * ys) % 4] + rng.uniform(-0.03, 0.03, (h, w))
    fy = base[(xs + 2 * ys + 1) % 4] + rng.uniform(-0.03, 0.03, (h, w))
    assert FRAC_LO <= min(fx.min(), fy.min()) and max(fx.max(), fy.max()) <= FRAC_HI
    return np.stack([(tx + fx - xs).astype(F32), (ty + fy - ys).astype(F32)])


def _assert_margins(flow):
    """No pixel within MARGIN px of a floor kink or of the +-1 comparison."""
    s = sampling(flow)
    for i, f0, g, half in (('ix', 'fx0', 'gx', 'half_w'), ('iy', 'fy0', 'gy', 'half_h')):
        frac = s[i].astype(np.float64) - s[f0]
        assert frac.min() >= MARGIN and frac.max() <= 1 - MARGIN, (frac.min(), frac.max())
        g64, hf = s[g].astype(np.float64), float(s[half])
        assert (np.abs(g64 - 1) * hf).min() >= MARGIN
        assert (np.abs(g64 + 1) * hf).min() >= MARGIN
    return s


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, N, K, D, shapes, start, stop int32 [N], frames: K arrays
    [D,h,w] float32, flows: K arrays [N,2,h,w] float32, states [K][N]).
    Arrays are shared between the tests and read-only."""
    spec = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    N, D, shapes = spec['N'], spec['D'], spec['shapes']
    start, stop = np.array(spec['start'], np.int32), np.array(spec['stop'], np.int32)
    assert not set(start.tolist()) & set(stop.tolist())
    frames, flows, states = [], [], []
    for k, (h, w) in enumerate(shapes):
        st = [STATES[(spec['state0'] + n + k) % 4] for n in range(N)]
        region = None
        if name == 'many_tiles':    # out-of-border pixels in the first and last tile only
            st = ['some', 'one']
            region = np.zeros((h, w), bool)
            region[:, :TW] = region[:, -TW:] = True
        flow = np.stack([make_flow(rng, h, w, s, region if n == 0 or region is None
                                   else region & (np.arange(w) >= w - TW),
                                   spec.get('reach'), spec.get('n_far', 2))
                         for n, s in enumerate(st)])
        s = _assert_margins(flow)
        fr = (rng.random((D, h, w)) * 255).astype(F32)
        warped = _warp(fr[stop], s, np.float64)['warped']
        for d in sorted(set(start.tolist())):       # shared starts: clear of every user's warp
            users = np.flatnonzero(start == d)
            gap = RESIDUAL_FLOOR + rng.uniform(0, 32, (h, w))
            fr[d] = np.where(rng.random((h, w)) < 0.5, warped[users].max(0) + gap,
                             warped[users].min(0) - gap).astype(F32)
        # the floor holds after the float32 cast of prev as well
        assert np.abs(warped - fr[start]).min() >= RESIDUAL_FLOOR - 1e-4
        cnt = s['oob'].sum(axis=(1, 2))
        for n, state in enumerate(st):
            want = {'none': cnt[n] == 0, 'one': cnt[n] == 1, 'all': cnt[n] == h * w,
                    'some': 0 < cnt[n] < h * w}[state]
            assert want, (name, k, n, state, cnt[n])
        frames.append(fr)
        flows.append(flow)
        states.append(st)
    for a in frames + flows + [start, stop]:
        a.setflags(write=False)
    return dict(name=name, N=N, K=len(shapes), D=D, shapes=shapes, start=start,
                stop=stop, frames=frames, flows=flows, states=states)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.float64):
    """reference_scale of every scale of a case, computed once and shared."""
    c = case(name)
    out = []
    for fr, fl in zip(c['frames'], c['flows']):
        r = reference_scale(fr[c['start']], fr[c['stop']], fl, dtype)
        assert r['residual'].min() >= RESIDUAL_FLOOR - 1e-4
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(r)
    return out


def term_bound(name, k, t32):
    """[3] bound on |term - ref64| at scale k: 4 x T32 relative plus the
    fixed-point quantum."""
    c, r = case(name), reference(name)[k]
    h, w = c['shapes'][k]
    return 4 * np.asarray(t32) * np.abs(r['value']) + term_quantum(r, c['N'], h, w)


def smallest_pair_share(name, k=0):
    """The smallest single smoothness pair's share of the term: its rho over
    its direction's normaliser.  A pair missed by the forward sums moves the
    term by at least this much."""
    raw = reference(name)[k]['raw']
    return min(m / n for m, n in zip(raw['smooth_min'], raw['smooth_norm']))
