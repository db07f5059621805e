"""Shared pieces of the image-of-warped-events tests (docs/IWE_SPEC.md): the
seeded case builders, an independent float64 splat with the per-pixel bound
the spec derives, and small helpers.  Pure numpy; nothing here touches the
package under test."""
import math

import numpy as np

F32 = np.float32
ONE = float(1 << 32)

# 1x1: everything on one pixel; 5x7, 33x31: odd, no multiple of anything;
# 16x16: warped coordinates reach a power of two; 400x400: 157 blocks of four
# pixels per thread wanted, 128 partial blocks allowed -- more than one block
# per frame, and more pixels than the capped grid covers in one pass
SHAPES = ((1, 1), (5, 7), (16, 16), (33, 31), (400, 400))
PER_FRAME = {(1, 1): 40, (5, 7): 150, (16, 16): 400, (33, 31): 900, (400, 400): 6000}

# (name, shape, F, variant, times)
CASES = tuple(
    [(f'{h}x{w}_F1', (h, w), 1, 'plain', 'dyadic') for h, w in SHAPES] +
    [(f'{h}x{w}_F3_empty_middle', (h, w), 3, 'empty_middle', 'dyadic') for h, w in SHAPES] +
    [('5x7_F3_degenerate', (5, 7), 3, 'degenerate', 'dyadic'),
     ('33x31_F3_degenerate', (33, 31), 3, 'degenerate', 'dyadic'),
     ('16x16_F3_slots_only', (16, 16), 3, 'slots_only', 'dyadic'),
     ('33x31_F3_recorded', (33, 31), 3, 'plain', 'recorded'),
     ('33x31_F1_recorded', (33, 31), 1, 'plain', 'recorded')])
CASE_IDS = [c[0] for c in CASES]

SPECIAL_FLOWS = (np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0)


def _frame_events(rng, shape, n, flow):
    """Events of one frame as (x, y, fraction of the window) and the frame's
    flow [2,h,w], edited in place where an event class needs a certain flow."""
    h, w = shape
    xs, ys, fr = [], [], []

    def add(x, y, f):
        xs.append(np.asarray(x, np.int64).reshape(-1))
        ys.append(np.asarray(y, np.int64).reshape(-1))
        fr.append(np.broadcast_to(np.asarray(f, np.float64), xs[-1].shape).copy())

    # random events, times on a 1/256 grid of the window
    add(rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, 257, n) / 256)
    # tau exactly 0 and exactly 1
    k = max(n // 20, 2)
    add(rng.integers(0, w, k), rng.integers(0, h, k), 0.0)
    add(rng.integers(0, w, k), rng.integers(0, h, k), 1.0)
    # two hundred events on one pixel, spread over the window
    px, py = int(rng.integers(0, w)), int(rng.integers(0, h))
    add(np.full(200, px), np.full(200, py), np.arange(200) / 256)
    # all four borders, flow that pushes corners (half a pixel at tau = 1/2 ...)
    # and whole events (... five pixels) outside, and the same inwards
    # (at tau = 1 a push of 1 lands exactly on -1 and on the side: both dropped)
    push = np.array([1.0, 3.0, 10.0, -1.0, -10.0])
    cols, rows = np.arange(w), np.arange(h)
    flow[0, :, 0], flow[0, :, w - 1] = push[rows % 5], -push[rows % 5]      # xw = x - tau u
    flow[1, 0, :], flow[1, h - 1, :] = push[cols % 5], -push[cols % 5]
    for f in (0.5, 0.25, 1.0):
        add(np.zeros(h), rows, f)
        add(np.full(h, w - 1), rows, f)
        add(cols, np.zeros(w), f)
        add(cols, np.full(w, h - 1), f)
    # flow that lands exactly on integer coordinates: two corners with Q = 0
    iy, ix = int(rng.integers(0, h)), int(rng.integers(0, w))
    flow[:, iy, ix] = (2.0, -4.0)
    add([ix] * 3, [iy] * 3, [0.5, 0.25, 1.0])
    # special flow values under events with tau = 0, inside the window and tau = 1
    # (a window of one pixel has one flow: the signed zero alone, or nothing would be left)
    for s in SPECIAL_FLOWS if h * w > 1 else (-0.0,):
        sy, sx = int(rng.integers(0, h)), int(rng.integers(0, w))
        flow[int(rng.integers(0, 2)), sy, sx] = s
        add([sx] * 3, [sy] * 3, [0.0, 0.375, 1.0])
    # cropped slots inside the frame: both coordinates -1, and one of them
    add([-1] * 5 + [-1, 0], [-1] * 5 + [0, -1], 0.5)
    x, y, f = np.concatenate(xs), np.concatenate(ys), np.concatenate(fr)
    order = rng.permutation(x.size)
    return x[order], y[order], f[order]


def make_case(shape, F, variant='plain', times='dyadic', seed=0):
    """-> dict(x, y int64 [n]; t float32 [n]; begin int64 [F+1]; ts float32
    [2F]; flow float32 [F,2,h,w]; shape).  Every case has begin[0] > 0 (events
    in front that belong to no frame) and padding slots behind begin[F]
    (x = y = -1, t = 0)."""
    h, w = shape
    rng = np.random.default_rng([seed, h, w, F, len(variant), len(times)])
    flow = rng.normal(0, 3, (F, 2, h, w))
    n = PER_FRAME[tuple(shape)]
    if times == 'dyadic':       # every frame: t0 = 0, d = 0.5
        starts, stops = np.zeros(F), np.full(F, 0.5)
        origin = 0.0
    else:                       # seconds since 1970, 45 Hz, narrowed as SEQUENCE_SPEC narrows them
        starts = 1.5e9 + 0.3127 + np.arange(F) / 45.0
        stops = starts + 1 / 45.0
        origin = starts.min()
    if variant == 'degenerate':
        stops[1] = starts[1] = 0.25         # d = 0
        starts[2], stops[2] = 0.5, 0.0      # d < 0
    xs, ys, tt, begin = [], [], [], []
    # events of no frame in front: valid coordinates, must not be counted
    lead = 17
    xs.append(rng.integers(0, w, lead))
    ys.append(rng.integers(0, h, lead))
    tt.append(np.full(lead, starts[0]))
    at = lead
    for f in range(F):
        begin.append(at)
        if variant == 'empty_middle' and f == 1:
            continue
        x, y, frac = _frame_events(rng, shape, n, flow[f])
        if variant == 'slots_only' and f == 1:
            x[:], y[:] = -1, -1
        span = stops[f] - starts[f]
        t = starts[f] + frac * (span if span > 0 else 0.5)
        xs.append(x)
        ys.append(y)
        tt.append(t)
        at += x.size
    begin.append(at)
    pad = 29
    xs.append(np.full(pad, -1))
    ys.append(np.full(pad, -1))
    tt.append(np.full(pad, origin))
    t64 = np.concatenate(tt)
    stamps = np.stack([starts, stops], 1).reshape(-1)
    return dict(x=np.concatenate(xs).astype(np.int64), y=np.concatenate(ys).astype(np.int64),
                t=(t64 - origin).astype(F32), begin=np.array(begin, np.int64),
                ts=(stamps - origin).astype(F32), flow=flow.astype(F32), shape=(h, w))


_cache = {}


def case(name):
    """The case of that name, built once; callers must not modify it."""
    if name not in _cache:
        _, shape, F, variant, times = CASES[CASE_IDS.index(name)]
        c = make_case(shape, F, variant, times)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = c
    return _cache[name]


def count_image(c):
    """uint32 [F,h,w]: the events of every frame per pixel, plain numpy."""
    h, w = c['shape']
    F = len(c['begin']) - 1
    out = np.zeros((F, h, w), np.uint32)
    for f in range(F):
        x, y = (c[k][c['begin'][f]:c['begin'][f + 1]] for k in ('x', 'y'))
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        np.add.at(out[f], (y[ok], x[ok]), 1)
    return out


def permuted(c, seed=5):
    """The same events in another order within every frame."""
    rng = np.random.default_rng(seed)
    idx = np.arange(c['x'].size)
    for f in range(len(c['begin']) - 1):
        lo, hi = c['begin'][f], c['begin'][f + 1]
        idx[lo:hi] = lo + rng.permutation(hi - lo)
    return dict(c, x=c['x'][idx], y=c['y'][idx], t=c['t'][idx])


def single_frame(c, f):
    """Frame f alone: the same columns, a table of one frame."""
    return dict(c, begin=c['begin'][f:f + 2], ts=c['ts'][2 * f:2 * f + 2], flow=c['flow'][f:f + 1])


# ---------------------------------------------------------------------------
# The definition in float64 and the bound of IWE_SPEC section 5
# ---------------------------------------------------------------------------
def coordinate_bound(shape):
    """|xw32 - xw64| of a kept event (IWE_SPEC section 5): tau carries three
    float32 roundings and the product a fourth, each 2^-24 relative, on
    |tau u| < S + 1; the difference is rounded once at a magnitude below P,
    the power of two that bounds the larger side; 2^-40 for the second order."""
    S = max(shape)
    P = 2.0 ** math.ceil(math.log2(max(S, 2)))
    return 2.0 ** -24 * (4 * (S + 1) + P / 2) + 2.0 ** -40


def contribution_bound(shape):
    """One event's contribution to one pixel, float32 restatement against the
    float64 definition: both coordinates (the tent is 1-Lipschitz in each and
    at most 1 in the other), fx and 1 - fx in both axes (2^-25 each), the
    product (2^-25), the truncation (2^-32)."""
    return 2 * coordinate_bound(shape) + 4 * 2.0 ** -25 + 2.0 ** -25 + 2.0 ** -32


def splat64(c):
    """-> (image float64 [F,h,w], touching int64 [F,h,w]): every kept event
    adds max(0, 1 - |xw - px|) * max(0, 1 - |yw - py|) to pixel (px, py), with
    tau, xw, yw in float64 from the float32 inputs and nothing truncated;
    ``touching`` counts per pixel the events whose float64 position lies
    within 1 + coordinate_bound of it in both axes: every event that can
    contribute in either arithmetic."""
    h, w = c['shape']
    F = len(c['begin']) - 1
    image = np.zeros((F, h, w))
    touching = np.zeros((F, h, w), np.int64)
    reach = 1.0 + coordinate_bound(c['shape'])
    ts, flow = c['ts'].astype(np.float64), c['flow'].astype(np.float64)
    for f in range(F):
        lo, hi = c['begin'][f], c['begin'][f + 1]
        x, y, t = c['x'][lo:hi], c['y'][lo:hi], c['t'][lo:hi].astype(np.float64)
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        x, y, t = x[ok], y[ok], t[ok]
        t0, d = ts[2 * f], ts[2 * f + 1] - ts[2 * f]
        tau = np.clip((t - t0) / d, 0.0, 1.0) if d > 0 else np.zeros(t.size)
        with np.errstate(all='ignore'):
            xw = x - tau * flow[f, 0, y, x]
            yw = y - tau * flow[f, 1, y, x]
        fin = np.isfinite(xw) & np.isfinite(yw)
        xw, yw = xw[fin], yw[fin]
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
    return image, touching


# ---------------------------------------------------------------------------
# Argument rules of the three entry points (the library is handed in)
# ---------------------------------------------------------------------------
EINVAL, ENOSPACE = -1, -2


def bad_calls(lib, a, F, h, w):
    """(what, zero-argument call, expected code): every call must be refused
    before anything is launched.  a: addresses by name (x, y, t, begin, ts,
    flow, q, count, result, ws, canvas) and 'n', the number of events; the
    buffers behind them fit F frames of h x w."""
    need = lib.dvsof_iwe_stats_workspace_bytes(F, h, w)

    def splat(F=F, h=h, w=w, n=None, **null):
        p = dict(a, **{k: None for k in null})
        n = a['n'] if n is None else n
        return lambda: lib.dvsof_iwe_splat(p['x'], p['y'], p['t'], n, p['begin'], p['ts'],
                                           p['flow'], F, h, w, p['q'], None)

    def stats(F=F, h=h, w=w, nbytes=need, **null):
        p = dict(a, **{k: None for k in null})
        return lambda: lib.dvsof_iwe_stats(p['q'], p['count'], F, h, w, p['result'], p['ws'],
                                           nbytes, None)

    def render(F=F, h=h, w=w, **null):
        p = dict(a, **{k: None for k in null})
        return lambda: lib.dvsof_iwe_render(p['q'], p['count'], p['result'], F, h, w,
                                            p['canvas'], None)
    sizes = [('F < 0', dict(F=-1)), ('F too large', dict(F=65536)), ('h = 0', dict(h=0)),
             ('w = 0', dict(w=0)), ('h negative', dict(h=-3)), ('h too large', dict(h=32768)),
             ('w too large', dict(w=32768))]
    for name, make in (('splat', splat), ('stats', stats), ('render', render)):
        for what, kw in sizes:
            yield f'{name}: {what}', make(**kw), EINVAL
    yield 'splat: n_events < 0', splat(n=-1), EINVAL
    for k in ('x', 'y', 't', 'begin', 'ts', 'flow', 'q'):
        yield f'splat: null {k}', splat(**{k: 1}), EINVAL
    for k in ('q', 'count', 'result'):
        yield f'stats: null {k}', stats(**{k: 1}), EINVAL
    yield 'stats: no workspace', stats(ws=1), ENOSPACE
    yield 'stats: workspace too small', stats(nbytes=need - 1), ENOSPACE
    yield 'stats: workspace of zero bytes', stats(nbytes=0), ENOSPACE
    for k in ('q', 'count', 'result', 'canvas'):
        yield f'render: null {k}', render(**{k: 1}), EINVAL


def empty_calls(lib):
    """F = 0 is fine and launches nothing, with no pointer at all."""
    yield lib.dvsof_iwe_splat(None, None, None, 0, None, None, None, 0, 4, 4, None, None)
    yield lib.dvsof_iwe_stats(None, None, 0, 4, 4, None, None, 0, None)
    yield lib.dvsof_iwe_render(None, None, None, 0, 4, 4, None, None)
