"""Shared pieces of the tests of the image of warped events at several
reference times and with the polarities apart (docs/IWE_SPEC.md sections
8-13): the cases of tests/iwe_cases.py with a polarity column, the float64
definition and the per-pixel bound generalised to (rho, channel), and the
argument rules of the new entry point.  Pure numpy; nothing here touches the
package under test."""
import math

import numpy as np

from tests import iwe_cases as ic

F32 = np.float32
MASKS = (1, 2, 4, 5, 7)
RHO = (0.0, 0.5, 1.0)           # bit b of a mask: the reference time RHO[b] of the window
OPTIONS = tuple((mask, pol) for mask in MASKS for pol in (False, True))
CASE_IDS = ic.CASE_IDS
DYADIC_IDS = [c[0] for c in ic.CASES if c[4] == 'dyadic']
PLAIN_DYADIC_IDS = [c[0] for c in ic.CASES if c[4] == 'dyadic' and c[3] in ('plain', 'empty_middle')]


def rhos(mask):
    return [RHO[b] for b in range(3) if mask >> b & 1]


def images_of(F, mask, polarity):
    return F * len(rhos(mask)) * (2 if polarity else 1)


def with_polarity(c, seed=9):
    """The case with a column p of +1 / -1 and, on every eleventh event, 0."""
    rng = np.random.default_rng([seed, c['x'].size])
    p = rng.choice(np.array([-1, 1], np.int64), c['x'].size)
    p[4::11] = 0
    p.setflags(write=False)
    return dict(c, p=p)


_cache = {}


def case(name):
    """The case of that name of iwe_cases with a polarity column; built once, read-only."""
    if name not in _cache:
        _cache[name] = with_polarity(ic.case(name))
    return _cache[name]


def dyadic(name):
    """A case with dyadic times whose finite flow is rounded to multiples of
    1/4: tau and sig are multiples of 2^-8, sig u of 2^-10, the weights'
    products of 2^-20 -- every float32 operation of the splat is exact and
    nothing is truncated.  The special flow values stay what they are."""
    assert name in DYADIC_IDS
    if ('dyadic', name) not in _cache:
        c = case(name)
        with np.errstate(all='ignore'):
            flow = np.where(np.abs(c['flow']) < 1e6, np.round(c['flow'] * 4) / 4, c['flow']).astype(F32)
        flow.setflags(write=False)
        _cache['dyadic', name] = dict(c, flow=flow)
    return _cache['dyadic', name]


def args_of(c):
    """The positional arguments of eval.iwe_splat_multi_host in front of the options."""
    return c['x'], c['y'], c['t'], c['p'], c['begin'], c['ts'], c['flow']


def permuted(c, seed=5):
    """The same events in another order within every frame."""
    rng = np.random.default_rng(seed)
    idx = np.arange(c['x'].size)
    for f in range(len(c['begin']) - 1):
        lo, hi = c['begin'][f], c['begin'][f + 1]
        idx[lo:hi] = lo + rng.permutation(hi - lo)
    return dict(c, **{k: c[k][idx] for k in ('x', 'y', 't', 'p')})


def single_frame(c, f):
    """Frame f alone: the same columns, a table of one frame."""
    return ic.single_frame(c, f)


def frame_of(c):
    """int64 [n]: the frame of every event, -1 for the events of none."""
    F = len(c['begin']) - 1
    e = np.arange(c['x'].size)
    f = np.searchsorted(c['begin'][:F], e, side='right') - 1
    return np.where((e >= c['begin'][0]) & (e < c['begin'][F]), f, -1)


def mirrored(c):
    """The case run backwards, frame by frame: t -> t0 + t1 - t and the flow
    negated.  What was warped to the end of a window is now warped to its
    start.  For cases whose times make that exact (the dyadic ones)."""
    f = frame_of(c)
    k = f >= 0
    t = c['t'].copy()
    total = (c['ts'][0::2].astype(np.float64) + c['ts'][1::2].astype(np.float64))[f[k]]
    t[k] = (total - c['t'][k]).astype(F32)
    assert np.array_equal(t[k].astype(np.float64), total - c['t'][k])      # exact
    return dict(c, t=t, flow=-c['flow'])


def restricted(c, keep):
    """The case with the events of the boolean mask ``keep`` only, the frames' table moved along."""
    f = frame_of(c)
    F = len(c['begin']) - 1
    lead = int((keep & (np.arange(keep.size) < c['begin'][0])).sum())
    per = np.array([int((keep & (f == k)).sum()) for k in range(F)], np.int64)
    begin = lead + np.concatenate([[0], np.cumsum(per)])
    return dict(c, begin=begin.astype(np.int64), **{k: c[k][keep] for k in ('x', 'y', 't', 'p')})


def channel_events(c, polarity, ch):
    """Which events channel ch holds: all without polarity, else by sign(p)."""
    if not polarity:
        return np.ones(c['x'].size, bool)
    return c['p'] > 0 if ch == 0 else c['p'] < 0


def count_image(c, polarity=False, ch=0):
    """uint32 [F,h,w]: the events of channel ch of every frame per pixel, plain numpy."""
    h, w = c['shape']
    F = len(c['begin']) - 1
    f = frame_of(c)
    ok = (f >= 0) & (c['x'] >= 0) & (c['x'] < w) & (c['y'] >= 0) & (c['y'] < h) & channel_events(c, polarity, ch)
    out = np.zeros((F, h, w), np.uint32)
    np.add.at(out, (f[ok], c['y'][ok], c['x'][ok]), 1)
    return out


# ---------------------------------------------------------------------------
# The definition in float64 and the bound of IWE_SPEC section 11
# ---------------------------------------------------------------------------
def _warp64(c, rho, keep):
    """Per frame the events of ``keep`` with coordinates inside the image and
    their warp over sig = tau - rho in float64 from the float32 inputs:
    list of dict(sig, u, v, xw, yw), non-finite positions left out."""
    h, w = c['shape']
    ts, flow = c['ts'].astype(np.float64), c['flow'].astype(np.float64)
    out = []
    for f in range(len(c['begin']) - 1):
        lo, hi = c['begin'][f], c['begin'][f + 1]
        x, y, t = c['x'][lo:hi], c['y'][lo:hi], c['t'][lo:hi].astype(np.float64)
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h) & keep[lo:hi]
        x, y, t = x[ok], y[ok], t[ok]
        t0, d = ts[2 * f], ts[2 * f + 1] - ts[2 * f]
        tau = np.clip((t - t0) / d, 0.0, 1.0) if d > 0 else np.zeros(t.size)
        sig = tau - rho
        u, v = flow[f, 0, y, x], flow[f, 1, y, x]
        with np.errstate(all='ignore'):
            xw, yw = x - sig * u, y - sig * v
        fin = np.isfinite(xw) & np.isfinite(yw)
        out.append(dict(sig=sig[fin], u=u[fin], v=v[fin], xw=xw[fin], yw=yw[fin]))
    return out


def largest_flow(c, rho, keep):
    """U of IWE_SPEC section 11: the largest |u|, |v| under an event whose
    float64 position lies within one pixel of the kept region (the bound is
    asserted to be below one pixel, so these are the events that either
    arithmetic can keep).  An event whose float64 sig is exactly 0 has tau = rho
    in float32 too -- t - t0 <= 0, t - t0 >= d and t - t0 = d / 2 survive the
    rounding of both differences, which is monotone and commutes with halving
    -- and is carried nowhere in either arithmetic, whatever its flow: its flow
    does not enter."""
    h, w = c['shape']
    U = 0.0
    for p in _warp64(c, rho, keep):
        near = (p['xw'] > -2) & (p['xw'] < w + 1) & (p['yw'] > -2) & (p['yw'] < h + 1)
        near &= p['sig'] != 0
        for a in (p['u'][near], p['v'][near]):
            a = np.abs(a[np.isfinite(a)])
            U = max(U, float(a.max(initial=0.0)))
    return U


def coordinate_bound(shape, rho, U):
    """|xw32 - xw64| of an event in reach of the image (IWE_SPEC section 11).
    sig = tau - rho: tau carries three float32 roundings, relative to tau <= 1,
    the subtraction a fourth, relative to |sig| <= 1 -- together below
    2^-24 (3 tau + |sig| / 2), and with tau = sig + rho below
    2^-24 (3.5 |sig| + 3 rho): the first part is relative to the product, on
    |sig u| < S + 1, the second is absolute and enters times |u| <= U.  The
    product is rounded once (2^-24 on S + 1), the difference once below P
    (P 2^-25); 2^-40 for the second order.  Never below section 5's
    (iwe_cases.coordinate_bound), which the maximum only states."""
    S = max(shape)
    P = 2.0 ** math.ceil(math.log2(max(S, 2)))
    delta = 2.0 ** -24 * (4.5 * (S + 1) + 3 * rho * U + P / 2) + 2.0 ** -40
    return max(delta, ic.coordinate_bound(shape))


def contribution_bound(delta):
    """IWE_SPEC section 5's per-contribution bound with the coordinate error delta."""
    return 2 * delta + 5 * 2.0 ** -25 + 2.0 ** -32


def splat64(c, rho=0.0, polarity=False, ch=0):
    """iwe_cases.splat64 for the reference time rho and channel ch -> (image
    float64 [F,h,w], bound float64 [F,h,w]): every kept event adds
    max(0, 1 - |xw - px|) * max(0, 1 - |yw - py|) to pixel (px, py), nothing
    truncated; bound = the contribution bound times the number of events whose
    float64 position lies within 1 + delta of the pixel in both axes."""
    h, w = c['shape']
    keep = channel_events(c, polarity, ch)
    if polarity:
        keep = keep & (c['p'] != 0)
    delta = coordinate_bound(c['shape'], rho, largest_flow(c, rho, keep))
    assert delta < 1.0, delta
    reach = 1.0 + delta
    F = len(c['begin']) - 1
    image, touching = np.zeros((F, h, w)), np.zeros((F, h, w), np.int64)
    for f, p in enumerate(_warp64(c, rho, keep)):
        xw, yw = p['xw'], p['yw']
        near = (xw > -2 - reach) & (xw < w + 1 + reach) & (yw > -2 - reach) & (yw < h + 1 + reach)
        xw, yw = xw[near], yw[near]
        bx, by = np.floor(xw).astype(np.int64), np.floor(yw).astype(np.int64)
        for j in range(-1, 3):
            for i in range(-1, 3):
                px, py = bx + i, by + j
                inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)
                dx, dy = np.abs(xw - px), np.abs(yw - py)
                hit = inside & (dx < reach) & (dy < reach)
                np.add.at(touching[f], (py[hit], px[hit]), 1)
                wgt = np.maximum(0.0, 1.0 - dx) * np.maximum(0.0, 1.0 - dy)
                hit &= wgt > 0
                np.add.at(image[f], (py[hit], px[hit]), wgt[hit])
    return image, contribution_bound(delta) * touching


def definition(c, mask, polarity):
    """-> (image float64 [M,h,w], bound float64 [M,h,w], count uint32 [M,h,w]) in image order."""
    h, w = c['shape']
    F = len(c['begin']) - 1
    R, C = len(rhos(mask)), 2 if polarity else 1
    image, bound = np.zeros((F * R * C, h, w)), np.zeros((F * R * C, h, w))
    count = np.zeros((F * R * C, h, w), np.uint32)
    for r, rho in enumerate(rhos(mask)):
        for ch in range(C):
            m = (np.arange(F) * R + r) * C + ch
            image[m], bound[m] = splat64(c, rho, polarity, ch)
            count[m] = count_image(c, polarity, ch)
    return image, bound, count


def fwl_of(q, count):
    """Flow warp loss per image in float64 from the integer images: var(I) / var(c), NaN where var(c) = 0."""
    M = q.shape[0]
    I = q.reshape(M, -1).astype(np.float64) * 2.0 ** -32
    cn = count.reshape(M, -1).astype(np.float64)
    var_c = (cn * cn).mean(1) - cn.mean(1) ** 2
    with np.errstate(all='ignore'):
        return np.where(var_c == 0, np.nan, ((I * I).mean(1) - I.mean(1) ** 2) / var_c)


# ---------------------------------------------------------------------------
# Argument rules of the entry point (the library is handed in)
# ---------------------------------------------------------------------------
EINVAL = ic.EINVAL


def bad_calls(lib, a, F, h, w, mask=7, polarity=1):
    """(what, zero-argument call): every call must be refused with EINVAL
    before anything is launched.  a: addresses by name (x, y, t, p, begin, ts,
    flow, q, count) and 'n', the number of events; the buffers behind them fit
    F frames of h x w with six images each."""
    def splat(F=F, h=h, w=w, n=None, mask=mask, polarity=polarity, **null):
        p = dict(a, **{k: None for k in null})
        n = a['n'] if n is None else n
        return lambda: lib.dvsof_iwe_splat_multi(p['x'], p['y'], p['t'], p['p'], n, p['begin'], p['ts'], p['flow'],
                                                 F, h, w, mask, polarity, p['q'], p['count'], None)
    sizes = [('F < 0', dict(F=-1)), ('F too large', dict(F=65536)), ('h = 0', dict(h=0)),
             ('w = 0', dict(w=0)), ('h negative', dict(h=-3)), ('h too large', dict(h=32768)),
             ('w too large', dict(w=32768)), ('n_events < 0', dict(n=-1)),
             ('mask 0', dict(mask=0)), ('mask 8', dict(mask=8)), ('mask negative', dict(mask=-1)),
             ('polarity 2', dict(polarity=2)), ('polarity negative', dict(polarity=-1)),
             ('M too large', dict(F=10923)),                # 10923 * 3 * 2 = 65538
             ('M too large without polarity', dict(F=21846, polarity=0)),
             ('M too large at two references', dict(F=16384, mask=5))]
    for what, kw in sizes:
        yield what, splat(**kw)
    for k in ('x', 'y', 't', 'p', 'begin', 'ts', 'flow', 'q', 'count'):
        yield f'null {k}', splat(**{k: 1})


def empty_calls(lib):
    """F = 0 is fine and launches nothing, with no pointer at all."""
    yield lib.dvsof_iwe_splat_multi(None, None, None, None, 0, None, None, None, 0, 4, 4, 7, 1, None, None, None)
