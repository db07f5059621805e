"""Shared pieces of the contrast-maximisation tests (docs/CONTRAST_SPEC.md):
the seeded case builders, an independent float64 oracle in torch (index_add
splat, gradient by autograd) with the bounds the spec derives, and the
argument rules of the two entry points.  Nothing here touches the package
under test."""
import numpy as np
import torch

from tests import iwe_cases as ic

F32 = np.float32
KINK = 2.0 ** -10       # the random cases keep every warped coordinate this far from an integer
KEYS = ('x', 'y', 't', 's', 'ts', 'fs', 'flow')


def _windows(F):
    """Frames 2k and 2k+1 belong to sample k and share the time 0.5: a sample
    carries the events of both (as with --prefix-length / --suffix-length),
    and an event at exactly 0.5 takes part in both.  A single frame has the
    window [0.25, 0.75] inside the events' [0, 1]."""
    if F == 1:
        return np.array([0.25, 0.75], F32), np.zeros(1, np.int64)
    ts = np.array([(0.0, 0.5) if f % 2 == 0 else (0.5, 1.0) for f in range(F)], F32).reshape(-1)
    return ts, np.arange(F, dtype=np.int64) // 2


def _finish(c):
    for k in KEYS:
        c[k].setflags(write=False)
    return c


def pairs64(c):
    """Per frame the events that take part and their warp in float64 from the
    float32 inputs: list of dict(e, x, y, tau, xw, yw, inside)."""
    h, w = c['shape']
    ts, flow = c['ts'].astype(np.float64), c['flow'].astype(np.float64)
    out = []
    for f in range(len(c['fs'])):
        keep = (c['s'] == c['fs'][f]) & (c['x'] >= 0) & (c['x'] < w) & (c['y'] >= 0) & (c['y'] < h) \
            & (c['ts'][2 * f] <= c['t']) & (c['t'] <= c['ts'][2 * f + 1])
        e = np.flatnonzero(keep)
        x, y, t = c['x'][e], c['y'][e], c['t'][e].astype(np.float64)
        t0, d = ts[2 * f], ts[2 * f + 1] - ts[2 * f]
        tau = np.clip((t - t0) / d, 0.0, 1.0) if d > 0 else np.zeros(e.size)
        with np.errstate(all='ignore'):
            xw, yw = x - tau * flow[f, 0, y, x], y - tau * flow[f, 1, y, x]
            inside = (xw > -1) & (xw < w) & (yw > -1) & (yw < h)
        out.append(dict(e=e, x=x, y=y, tau=tau, xw=xw, yw=yw, inside=inside))
    return out


def make_case(shape, F, per_frame, kind='random', seed=0):
    """-> dict(x, y, s int64 [n]; t float32 [n]; ts float32 [2F]; fs int64 [F];
    flow float32 [F,2,h,w]; shape).  Beside the events of the frames: -1 slots,
    events of samples no frame belongs to, and (F = 1) events outside the
    window.  kind 'random': times and flows at random, resampled until every
    event that takes part has its float64 xw, yw at least KINK from an integer;
    'dyadic': tau, u, v on a 2^-4 grid, an eighth of the flow on integers."""
    h, w = shape
    rng = np.random.default_rng([seed, h, w, F, per_frame, len(kind)])
    ts, fs = _windows(F)
    n_samples = int(fs.max()) + 1
    n = per_frame * F
    x, y = rng.integers(0, w, n), rng.integers(0, h, n)
    s = rng.integers(0, n_samples, n)
    flow = rng.normal(0, 2.0, (F, 2, h, w))
    if kind == 'dyadic':
        flow = np.round(flow * 16) / 16
        whole = rng.random(flow.shape) < 0.125
        flow[whole] = np.round(flow[whole])
        t = rng.integers(0, 33, n) / 32.0           # tau = k/16 in either window, and in [0.25, 0.75]
    else:
        t = rng.random(n)
    # slots and strangers
    x[::17], y[::17] = -1, -1
    s[5::23] = n_samples + 3
    s[7::29] = -1
    c = dict(x=x.astype(np.int64), y=y.astype(np.int64), s=s.astype(np.int64), t=t.astype(F32), ts=ts,
             fs=fs, flow=flow.astype(F32), shape=(h, w))
    while kind == 'random':
        bad = np.zeros(n, bool)
        for p in pairs64(c):
            for a in (p['xw'], p['yw']):
                bad[p['e'][np.abs(a - np.round(a)) < KINK]] = True
        if not bad.any():
            break
        c['t'][bad] = rng.random(int(bad.sum())).astype(F32)
    return _finish(c)


# name -> (shape, F, events per frame, kind)
ORACLE_CASES = {
    'random_5x7_F1': ((5, 7), 1, 300, 'random'),
    'random_16x16_F3': ((16, 16), 3, 600, 'random'),
    'random_33x31_F4': ((33, 31), 4, 1500, 'random'),
    'dyadic_5x7_F1': ((5, 7), 1, 300, 'dyadic'),
    'dyadic_16x16_F3': ((16, 16), 3, 600, 'dyadic'),
    'dyadic_33x31_F4': ((33, 31), 4, 1500, 'dyadic'),
}
RANDOM_IDS = [k for k in ORACLE_CASES if k.startswith('random')]
DYADIC_IDS = [k for k in ORACLE_CASES if k.startswith('dyadic')]
_cache = {}


def case(name):
    """The case of that name, built once; its arrays are read-only."""
    if name not in _cache:
        _cache[name] = make_case(*ORACLE_CASES[name])
    return _cache[name]


def permuted(c, seed=5):
    """The same events in another order."""
    idx = np.random.default_rng(seed).permutation(c['x'].size)
    return dict(c, x=c['x'][idx], y=c['y'][idx], t=c['t'][idx], s=c['s'][idx])


def single_frame(c, f):
    """Frame f alone: the same columns, tables of one frame."""
    return dict(c, ts=c['ts'][2 * f:2 * f + 2], fs=c['fs'][f:f + 1], flow=c['flow'][f:f + 1])


def args_of(c):
    """The positional arguments of loss.contrast_fwd_host / contrast_bwd_host."""
    return c['x'], c['y'], c['t'], c['s'], c['ts'], c['fs'], c['flow']


# ---------------------------------------------------------------------------
# The definition: torch float64 on the CPU, the gradient by autograd
# ---------------------------------------------------------------------------
def _var(a, N):
    return (a * a).sum() / N - (a.sum() / N) ** 2


def oracle64(c):
    """-> dict(term float, grad float64 [F,2,h,w] = d term / d flow, image
    float64 [F,h,w], count float64 [F,h,w]).  Weights from the float64
    coordinate, nothing truncated, the floor convention of the kernels."""
    h, w = c['shape']
    F, N = len(c['fs']), h * w
    flow = torch.tensor(c['flow'].astype(np.float64), requires_grad=True)
    term = torch.zeros((), dtype=torch.float64)
    images, counts = [], []
    for f, p in enumerate(pairs64(c)):
        x, y = torch.from_numpy(p['x']), torch.from_numpy(p['y'])
        tau = torch.from_numpy(p['tau'])
        count = torch.zeros(N, dtype=torch.float64).index_add(0, y * w + x, torch.ones(len(x), dtype=torch.float64))
        k = torch.from_numpy(p['inside'])
        x, y, tau = x[k], y[k], tau[k]
        xw = x - tau * flow[f, 0, y, x]
        yw = y - tau * flow[f, 1, y, x]
        bx, by = torch.floor(xw).detach(), torch.floor(yw).detach()
        fx, fy = xw - bx, yw - by
        image = torch.zeros(N, dtype=torch.float64)
        for j, wy in enumerate((1 - fy, fy)):
            for i, wx in enumerate((1 - fx, fx)):
                px, py = (bx + i).long(), (by + j).long()
                ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
                image = image.index_add(0, (py * w + px)[ok], (wy * wx)[ok])
        var_c = _var(count, N)
        if var_c > 0:
            term = term + (1 - _var(image, N) / var_c)
        images.append(image.detach().numpy().reshape(h, w))
        counts.append(count.numpy().reshape(h, w))
    term = term / F
    if term.requires_grad:
        term.backward()
    grad = flow.grad.numpy() if flow.grad is not None else np.zeros(flow.shape)
    return dict(term=float(term.detach()), grad=grad, image=np.stack(images), count=np.stack(counts))


def bounds(c, o, seed=1.0, weight=1.0):
    """CONTRAST_SPEC section 7 for a case without kinks -> (bound of |term32 -
    term64|, bound of |grad32 - seed weight grad64| per element [F,2,h,w]).
    Computed from the case and the oracle's float64 quantities only."""
    h, w = c['shape']
    F, N = len(c['fs']), float(h * w)
    delta, eps = ic.coordinate_bound(c['shape']), ic.contribution_bound(c['shape'])
    assert delta < KINK         # both arithmetics take the same floor and the same inside test
    d_tau, d_w = 2.0 ** -22, delta + 2.0 ** -24
    b_term, b_grad = 0.0, np.zeros((F, 2, h, w))
    for f, p in enumerate(pairs64(c)):
        k = p['inside']
        x, y, tau, xw, yw = (p[n][k] for n in ('x', 'y', 'tau', 'xw', 'yw'))
        bx, by = np.floor(xw).astype(np.int64), np.floor(yw).astype(np.int64)
        fx, fy = xw - bx, yw - by
        I, cnt = o['image'][f], o['count'][f]
        # every event touches its four corners, in both arithmetics
        touching = np.zeros((h, w))
        corner = {}
        for j in range(2):
            for i in range(2):
                px, py = bx + i, by + j
                ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
                np.add.at(touching, (py[ok], px[ok]), 1)
                corner[j, i] = (ok, np.where(ok, py, 0), np.where(ok, px, 0))
        b = eps * touching                                  # |I32 - I64| per pixel
        mean, b_mean = I.sum() / N, b.sum() / N
        var_i = (I * I).sum() / N - mean ** 2
        var_c = (cnt * cnt).sum() / N - (cnt.sum() / N) ** 2
        if not var_c > 0:
            continue
        d_var = (2 * I * b + b * b).sum() / N + 2 * mean * b_mean + b_mean ** 2 \
            + (N + 4) * 2.0 ** -52 * ((I * I).sum() / N + mean ** 2)
        b_term += d_var / var_c + 2.0 ** -50 * abs(var_i / var_c)
        coef = 2.0 / (N * var_c)
        G = -coef * (I - mean)
        d_G = coef * (b + b_mean) + 2.0 ** -49 * coef * (I + mean)
        gmax = coef * max(I.max() - mean, mean) + coef * (b.max() + b_mean)
        trunc = 2.0 ** -39 * gmax                           # one unit, 2^(e-40) with 2^(e-1) <= gmax
        for ch, (wa, pairs_) in enumerate((((1 - fy, fy), (((0, 1), (0, 0)), ((1, 1), (1, 0)))),
                                           ((1 - fx, fx), (((1, 0), (0, 0)), ((1, 1), (0, 1)))))):
            exact, upper = np.zeros(x.size), np.zeros(x.size)
            for wgt, (hi, lo) in zip(wa, pairs_):
                (okh, yh, xh), (okl, yl, xl) = corner[hi], corner[lo]
                D = np.where(okh, G[yh, xh], 0.0) - np.where(okl, G[yl, xl], 0.0)
                d_D = np.where(okh, d_G[yh, xh], 0.0) + np.where(okl, d_G[yl, xl], 0.0)
                exact += wgt * np.abs(D)
                upper += (wgt + d_w) * (np.abs(D) + d_D)
            per_event = (tau + d_tau) * upper - tau * exact + 2.0 ** -49 * tau * exact + trunc
            np.add.at(b_grad[f, ch], (y, x), per_event)
    sw = abs(seed * weight)
    want = sw * np.abs(o['grad'])
    b_grad = sw * b_grad / F
    b_grad = b_grad + 2.0 ** -22 * (want + b_grad) + 2.0 ** -149
    return b_term / F + 2.0 ** -24 * abs(o['term']) + 2.0 ** -149, b_grad


# ---------------------------------------------------------------------------
# A pattern that translates with a known constant flow
# ---------------------------------------------------------------------------
def translating_pattern(shape=(24, 24), flow=(3.0, -2.0), points=40, per_point=24, seed=11):
    """Events of ``points`` scene points that move by ``flow`` pixels over the
    window [0, 1]: the point that is at (px, py) at time 0 fires at the pixel
    round((px, py) + t flow) at ``per_point`` times.  Warped back with the true
    flow the events of a point land within half a pixel of where it started."""
    h, w = shape
    rng = np.random.default_rng(seed)
    px = rng.uniform(4, w - 5, points)
    py = rng.uniform(4, h - 5, points)
    t = np.tile((np.arange(per_point) + 0.5) / per_point, points)
    x = np.round(np.repeat(px, per_point) + t * flow[0]).astype(np.int64)
    y = np.round(np.repeat(py, per_point) + t * flow[1]).astype(np.int64)
    ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    x, y, t = x[ok], y[ok], t[ok]
    return dict(x=x, y=y, t=t.astype(F32), s=np.zeros(x.size, np.int64), ts=np.array([0, 1], F32),
                fs=np.zeros(1, np.int64), shape=(h, w))


def constant_flow(shape, uv):
    flow = np.empty((1, 2) + tuple(shape), F32)
    flow[0, 0], flow[0, 1] = uv
    return flow


# ---------------------------------------------------------------------------
# Cases of the device tests: every path of the kernels, special values included
# ---------------------------------------------------------------------------
def device_case(shape, F, n_events, seed=0):
    """A case of exactly ``n_events`` events for the device-against-restatement
    test: random events and flows, and among them (as far as n_events reaches)
    -1 slots, samples outside the batch, times just outside and exactly on both
    window ends, the special flows of tests/iwe_cases.py under events, events
    and corners pushed over every border, flows that land on integers."""
    h, w = shape
    rng = np.random.default_rng([seed, h, w, F, n_events])
    ts, fs = _windows(F)
    n_samples = int(fs.max()) + 1
    n = n_events
    x, y = rng.integers(0, w, n), rng.integers(0, h, n)
    s = rng.integers(0, n_samples, n)
    t = rng.random(n).astype(F32)
    flow = rng.normal(0, 2.0, (F, 2, h, w)).astype(F32)
    ends = np.unique(ts)
    edge = np.concatenate([ends, np.nextafter(ends, F32(-9)), np.nextafter(ends, F32(9))]).astype(F32)
    k = np.arange(n)
    t[k % 7 == 3] = edge[(k[k % 7 == 3] // 7) % edge.size]
    x[k % 19 == 5], y[k % 19 == 5] = -1, -1
    x[k % 41 == 6] = w
    y[k % 43 == 8] = -1
    s[k % 23 == 9] = n_samples + 2
    s[k % 29 == 11] = -1
    if h * w > 1:
        for i, v in enumerate(ic.SPECIAL_FLOWS):
            flow[i % F, i % 2, (3 * i) % h, (5 * i + 1) % w] = v
        flow[:, 0, :, 0], flow[:, 0, :, w - 1] = 3.0, -3.0          # over the left and right border
        flow[:, 1, 0, :], flow[:, 1, h - 1, :] = 1.5, -1.5          # corners over the top and bottom
        flow[:, :, h // 2, w // 2] = (2.0, -4.0)                    # integer landings at tau = 1/2, 1
    return _finish(dict(x=x.astype(np.int64), y=y.astype(np.int64), s=s.astype(np.int64), t=t, ts=ts, fs=fs,
                        flow=flow, shape=(h, w)))


def one_pixel_case(n_events=4097):
    """All events on one pixel of a 5x7 frame, spread over the window."""
    c = device_case((5, 7), 1, n_events, seed=3)
    x, y, s = np.full(n_events, 3, np.int64), np.full(n_events, 2, np.int64), np.zeros(n_events, np.int64)
    t = (0.25 + 0.5 * np.arange(n_events) / n_events).astype(F32)
    flow = c['flow'].copy()
    flow[0, :, 2, 3] = (1.25, -0.75)
    return _finish(dict(c, x=x, y=y, s=s, t=t, flow=flow))


def degenerate_case():
    """d == 0 (events at exactly that time take part with tau = 0), d < 0 (no
    event can take part) and a frame whose sample has no events."""
    c = device_case((5, 7), 3, 257, seed=4)
    ts = np.array([0.5, 0.5, 0.75, 0.25, 0.0, 1.0], F32)
    fs = np.array([0, 0, 7], np.int64)
    t = c['t'].copy()
    t[::3] = 0.5
    return _finish(dict(c, ts=ts, fs=fs, t=t, s=np.zeros_like(c['s'])))


def many_frames_case():
    """More frames than the closing wave has lanes: 130 frames of 2x3, eight
    events each on average; a lane of the wave takes frames k, k + 64, k + 128."""
    return device_case((2, 3), 130, 1040)


DEVICE_SHAPES = ((1, 1), (2, 3), (5, 7), (16, 16), (33, 31))
DEVICE_COUNTS = (0, 1, 255, 256, 257, 4097)


def device_cases():
    """name -> case: F in {1, 3} x the shapes at 257 events, every event count
    at 5x7 and 33x31, two frames large enough for several partial blocks in the
    statistics, the two special cases, and 130 frames."""
    out = {}
    for F in (1, 3):
        for shape in DEVICE_SHAPES:
            out[f'{shape[0]}x{shape[1]}_F{F}_n257'] = device_case(shape, F, 257)
        for n in DEVICE_COUNTS:
            for shape in ((5, 7), (33, 31)):
                out[f'{shape[0]}x{shape[1]}_F{F}_n{n}'] = device_case(shape, F, n)
    # the statistics' closing wave with several partials: 1600 pixels are two blocks; 160 000 are
    # the 128 blocks allowed, two partials per closing lane and five rounds per thread
    out['40x40_F3_n4097'] = device_case((40, 40), 3, 4097)
    out['400x400_F1_n4097'] = device_case((400, 400), 1, 4097)
    out['one_pixel_4097'] = one_pixel_case()
    out['degenerate_windows'] = degenerate_case()
    out['2x3_F130_n1040'] = many_frames_case()
    return out


# ---------------------------------------------------------------------------
# Argument rules of the entry points (the library is handed in)
# ---------------------------------------------------------------------------
EINVAL, ENOSPACE = -1, -2


def bad_calls(lib, a, F, h, w):
    """(what, zero-argument call, expected code): every call must be refused
    before anything is launched.  a: addresses by name (x, y, t, s, ts, fs,
    flow, q, count, result, term, ws, seed, grad) and 'n', the number of
    events; the buffers behind them fit F frames of h x w."""
    need = lib.dvsof_contrast_workspace_bytes(F, h, w)

    def fwd(F=F, h=h, w=w, n=None, nbytes=need, **null):
        p = dict(a, **{k: None for k in null})
        n = a['n'] if n is None else n
        return lambda: lib.dvsof_contrast_fwd(p['x'], p['y'], p['t'], p['s'], n, p['ts'], p['fs'], p['flow'],
                                              F, h, w, p['q'], p['count'], p['result'], p['term'], p['ws'],
                                              nbytes, None)

    def bwd(F=F, h=h, w=w, n=None, nbytes=need, **null):
        p = dict(a, **{k: None for k in null})
        n = a['n'] if n is None else n
        return lambda: lib.dvsof_contrast_bwd(p['x'], p['y'], p['t'], p['s'], n, p['ts'], p['fs'], p['flow'],
                                              F, h, w, p['q'], p['ws'], nbytes, p['seed'], 1.0, p['grad'], None)
    sizes = [('F < 0', dict(F=-1)), ('F too large', dict(F=65536)), ('h = 0', dict(h=0)),
             ('w = 0', dict(w=0)), ('h negative', dict(h=-3)), ('h too large', dict(h=32768)),
             ('w too large', dict(w=32768)), ('n_events < 0', dict(n=-1))]
    for name, make in (('fwd', fwd), ('bwd', bwd)):
        for what, kw in sizes:
            yield f'{name}: {what}', make(**kw), EINVAL
        yield f'{name}: no workspace', make(ws=1), ENOSPACE
        yield f'{name}: workspace too small', make(nbytes=need - 1), ENOSPACE
        yield f'{name}: workspace of zero bytes', make(nbytes=0), ENOSPACE
    for k in ('x', 'y', 't', 's', 'ts', 'fs', 'flow', 'q', 'count', 'result', 'term'):
        yield f'fwd: null {k}', fwd(**{k: 1}), EINVAL
    for k in ('x', 'y', 't', 's', 'ts', 'fs', 'flow', 'q', 'seed', 'grad'):
        yield f'bwd: null {k}', bwd(**{k: 1}), EINVAL


def empty_calls(lib):
    """F = 0 is fine and launches nothing, with no pointer at all."""
    yield lib.dvsof_contrast_fwd(None, None, None, None, 0, None, None, None, 0, 4, 4, None, None, None, None,
                                 None, 0, None)
    yield lib.dvsof_contrast_bwd(None, None, None, None, 0, None, None, None, 0, 4, 4, None, None, 0, None, 1.0,
                                 None, None)
