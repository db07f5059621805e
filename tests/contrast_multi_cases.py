"""Shared pieces of the tests of the contrast term with several reference
times and the polarities apart (docs/CONTRAST_SPEC.md sections 11-15): the
cases of tests/contrast_cases.py with a polarity column, the float64
definition, the warp and the bounds generalised to a reference time, and the
argument rules of the new entry points.  Nothing here touches the package
under test."""
import math

import numpy as np
import torch

from tests import contrast_cases as cc

F32 = np.float32
KINK = cc.KINK
MASKS = (1, 2, 4, 5, 7)
RHO = (0.0, 0.5, 1.0)           # bit b of a mask: the reference time RHO[b] of the window
KEYS = cc.KEYS + ('p',)


def rhos(mask):
    return [RHO[b] for b in range(3) if mask >> b & 1]


def with_polarity(c, seed=9):
    """The case with a column p of +1 / -1 and, on every eleventh event, 0."""
    rng = np.random.default_rng([seed, c['x'].size])
    p = rng.choice(np.array([-1, 1], np.int64), c['x'].size)
    p[4::11] = 0
    p.setflags(write=False)
    return dict(c, p=p)


def args_of(c):
    """The positional arguments of loss.contrast_multi_fwd_host / _bwd_host."""
    return c['x'], c['y'], c['t'], c['p'], c['s'], c['ts'], c['fs'], c['flow']


def permuted(c, seed=5):
    idx = np.random.default_rng(seed).permutation(c['x'].size)
    return dict(c, **{k: c[k][idx] for k in ('x', 'y', 't', 's', 'p')})


def restricted(c, keep):
    """The case with the events of the boolean mask ``keep`` only."""
    return dict(c, **{k: c[k][keep] for k in ('x', 'y', 't', 's', 'p')})


def channel_events(c, polarity, ch):
    """Which events channel ch holds: all without polarity, else by sign(p)."""
    if not polarity:
        return np.ones(c['x'].size, bool)
    return c['p'] > 0 if ch == 0 else c['p'] < 0


def pairs64(c, rho=0.0, keep=None):
    """contrast_cases.pairs64 for the reference time rho: per frame the events
    that take part (of the boolean mask ``keep``, if given) and their warp over
    sig = tau - rho in float64 from the float32 inputs: list of dict(e, x, y,
    tau, sig, xw, yw, inside)."""
    h, w = c['shape']
    ts, flow = c['ts'].astype(np.float64), c['flow'].astype(np.float64)
    out = []
    for f in range(len(c['fs'])):
        take = (c['s'] == c['fs'][f]) & (c['x'] >= 0) & (c['x'] < w) & (c['y'] >= 0) & (c['y'] < h) \
            & (c['ts'][2 * f] <= c['t']) & (c['t'] <= c['ts'][2 * f + 1])
        if keep is not None:
            take &= keep
        e = np.flatnonzero(take)
        x, y, t = c['x'][e], c['y'][e], c['t'][e].astype(np.float64)
        t0, d = ts[2 * f], ts[2 * f + 1] - ts[2 * f]
        tau = np.clip((t - t0) / d, 0.0, 1.0) if d > 0 else np.zeros(e.size)
        sig = tau - rho
        with np.errstate(all='ignore'):
            xw, yw = x - sig * flow[f, 0, y, x], y - sig * flow[f, 1, y, x]
            inside = (xw > -1) & (xw < w) & (yw > -1) & (yw < h)
        out.append(dict(e=e, x=x, y=y, tau=tau, sig=sig, xw=xw, yw=yw, inside=inside))
    return out


def make_case(name, max_rounds=64):
    """The random case of that name of contrast_cases.ORACLE_CASES, its times
    resampled until every event that takes part has its float64 xw, yw of
    EVERY reference at least KINK from an integer, with a polarity column.
    -> (case, rounds it took)."""
    base = cc.case(name)
    c = dict(base, t=base['t'].copy())
    rng = np.random.default_rng([21, len(name), c['x'].size])
    for rounds in range(max_rounds):
        bad = np.zeros(c['x'].size, bool)
        for rho in RHO:
            for p in pairs64(c, rho):
                for a in (p['xw'], p['yw']):
                    bad[p['e'][np.abs(a - np.round(a)) < KINK]] = True
        if not bad.any():
            c['t'].setflags(write=False)
            return with_polarity(c), rounds
        c['t'][bad] = rng.random(int(bad.sum())).astype(F32)
    raise AssertionError(f'{name}: still {int(bad.sum())} events on a kink after {max_rounds} rounds')


_cache = {}


def case(name):
    """Random names: ``make_case``; dyadic names: the case of contrast_cases
    with a polarity column.  Built once, read-only."""
    if name not in _cache:
        _cache[name] = make_case(name)[0] if name in cc.RANDOM_IDS else with_polarity(cc.case(name))
    return _cache[name]


def mirrored(c):
    """A one-frame case run backwards: t -> t0 + t1 - t and the flow negated.
    What was warped to the end of the window is now warped to its start."""
    assert len(c['fs']) == 1
    t = (c['ts'][0] + c['ts'][1] - c['t']).astype(F32)
    assert np.array_equal(t.astype(np.float64), c['ts'].astype(np.float64).sum() - c['t'])   # exact
    return dict(c, t=t, flow=-c['flow'])


# ---------------------------------------------------------------------------
# The definition: torch float64 on the CPU, the gradient by autograd
# ---------------------------------------------------------------------------
def oracle64(c, mask=1, polarity=False):
    """-> dict(term float, grad float64 [F,2,h,w] = d term / d flow, image
    float64 [M,h,w], count float64 [M,h,w], image_term [M]); m = (f R + r) C + c.
    Weights from the float64 coordinate, nothing truncated, the floor
    convention of the kernels."""
    h, w = c['shape']
    F, N = len(c['fs']), h * w
    R, C = len(rhos(mask)), 2 if polarity else 1
    M = F * R * C
    flow = torch.tensor(c['flow'].astype(np.float64), requires_grad=True)
    term = torch.zeros((), dtype=torch.float64)
    images, counts, image_terms = [None] * M, [None] * M, np.zeros(M)
    for r, rho in enumerate(rhos(mask)):
        for ch in range(C):
            for f, p in enumerate(pairs64(c, rho, channel_events(c, polarity, ch))):
                m = (f * R + r) * C + ch
                x, y = torch.from_numpy(p['x']), torch.from_numpy(p['y'])
                sig = torch.from_numpy(p['sig'])
                count = torch.zeros(N, dtype=torch.float64).index_add(0, y * w + x,
                                                                      torch.ones(len(x), dtype=torch.float64))
                k = torch.from_numpy(p['inside'])
                x, y, sig = x[k], y[k], sig[k]
                xw = x - sig * flow[f, 0, y, x]
                yw = y - sig * flow[f, 1, y, x]
                bx, by = torch.floor(xw).detach(), torch.floor(yw).detach()
                fx, fy = xw - bx, yw - by
                image = torch.zeros(N, dtype=torch.float64)
                for j, wy in enumerate((1 - fy, fy)):
                    for i, wx in enumerate((1 - fx, fx)):
                        px, py = (bx + i).long(), (by + j).long()
                        ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
                        image = image.index_add(0, (py * w + px)[ok], (wy * wx)[ok])
                var_c = cc._var(count, N)
                if var_c > 0:
                    one = 1 - cc._var(image, N) / var_c
                    image_terms[m] = float(one.detach())
                    term = term + one
                images[m] = image.detach().numpy().reshape(h, w)
                counts[m] = count.numpy().reshape(h, w)
    term = term / M
    if term.requires_grad:
        term.backward()
    grad = flow.grad.numpy() if flow.grad is not None else np.zeros(flow.shape)
    return dict(term=float(term.detach()), grad=grad, image=np.stack(images), count=np.stack(counts),
                image_term=image_terms, mask=mask, polarity=polarity)


def coordinate_bound(c):
    """|xw32 - xw64| of an event that stays in reach of the image, for any
    reference (CONTRAST_SPEC section 15).  sig = tau - rho carries the three
    roundings of tau (3 * 2^-24 absolute on a value of at most 1) and one of
    its own (2^-25, |sig| <= 1): below 4 * 2^-24 absolute, but after the
    subtraction no longer relative, so its share of the product is bounded by
    U = max |flow| and not by the product's size; the product is rounded once
    (2^-24 on |sig u| < S + 1) and the difference once below P (P 2^-25);
    2^-40 for the second order.  Not below iwe_cases.coordinate_bound."""
    S = max(c['shape'])
    P = 2.0 ** math.ceil(math.log2(max(S, 2)))
    U = float(np.abs(c['flow'][np.isfinite(c['flow'])]).max())
    return 2.0 ** -24 * (4 * max(U, S + 1) + P / 2) + 2.0 ** -40


def bounds(c, o, seed=1.0, weight=1.0):
    """contrast_cases.bounds for the oracle o = oracle64(c, mask, polarity) ->
    (bound of |term32 - term64|, bound of |grad32 - seed weight grad64| per
    element [F,2,h,w]).  Computed from the case and the oracle's float64
    quantities only."""
    h, w = c['shape']
    mask, polarity = o['mask'], o['polarity']
    R, C = len(rhos(mask)), 2 if polarity else 1
    F, N = len(c['fs']), float(h * w)
    M = F * R * C
    delta = coordinate_bound(c)
    eps = 2 * delta + 5 * 2.0 ** -25 + 2.0 ** -32         # IWE_SPEC section 5 with this delta
    assert delta < KINK         # both arithmetics take the same floor and the same inside test
    d_sig, d_w = 2.0 ** -22, delta + 2.0 ** -24
    unit_loss = 2.0 ** -39 if R == 1 else 2.0 ** -37      # one unit against the frame's gmax
    b_term, b_grad = 0.0, np.zeros((F, 2, h, w))
    per_image = {}
    for r, rho in enumerate(rhos(mask)):
        for ch in range(C):
            for f, p in enumerate(pairs64(c, rho, channel_events(c, polarity, ch))):
                per_image[(f * R + r) * C + ch] = (f, p)
    # the frames' gmax first: the unit of a frame comes from the largest over its images
    prepared, frame_gmax = {}, np.zeros(F)
    for m, (f, p) in per_image.items():
        k = p['inside']
        x, y, sig, xw, yw = (p[n][k] for n in ('x', 'y', 'sig', 'xw', 'yw'))
        bx, by = np.floor(xw).astype(np.int64), np.floor(yw).astype(np.int64)
        I, cnt = o['image'][m], o['count'][m]
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
        frame_gmax[f] = max(frame_gmax[f], coef * max(I.max() - mean, mean) + coef * (b.max() + b_mean))
        prepared[m] = (f, x, y, np.abs(sig), xw - bx, yw - by, corner, G, d_G)
    for m, (f, x, y, asig, fx, fy, corner, G, d_G) in prepared.items():
        trunc = unit_loss * frame_gmax[f]
        for comp, (wa, pairs_) in enumerate((((1 - fy, fy), (((0, 1), (0, 0)), ((1, 1), (1, 0)))),
                                             ((1 - fx, fx), (((1, 0), (0, 0)), ((1, 1), (0, 1)))))):
            exact, upper = np.zeros(x.size), np.zeros(x.size)
            for wgt, (hi, lo) in zip(wa, pairs_):
                (okh, yh, xh), (okl, yl, xl) = corner[hi], corner[lo]
                D = np.where(okh, G[yh, xh], 0.0) - np.where(okl, G[yl, xl], 0.0)
                d_D = np.where(okh, d_G[yh, xh], 0.0) + np.where(okl, d_G[yl, xl], 0.0)
                exact += wgt * np.abs(D)
                upper += (wgt + d_w) * (np.abs(D) + d_D)
            per_event = (asig + d_sig) * upper - asig * exact + 2.0 ** -49 * asig * exact + trunc
            np.add.at(b_grad[f, comp], (y, x), per_event)
    sw = abs(seed * weight)
    want = sw * np.abs(o['grad'])
    b_grad = sw * b_grad / M
    b_grad = b_grad + 2.0 ** -22 * (want + b_grad) + 2.0 ** -149
    return b_term / M + 2.0 ** -24 * abs(o['term']) + 2.0 ** -149, b_grad


# ---------------------------------------------------------------------------
# The sink flow of the collapse measurement (CONTRAST_SPEC section 10)
# ---------------------------------------------------------------------------
def sink_case(shape=(24, 24), n=4000, seed=3):
    """Uniform events over the window [0, 1] and the flow u = x - w/2,
    v = y - h/2, which carries every event onto the centre at tau = 1."""
    h, w = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    flow = np.stack([xx - w / 2, yy - h / 2])[None].astype(F32)
    c = dict(x=rng.integers(0, w, n), y=rng.integers(0, h, n), t=rng.random(n).astype(F32),
             s=np.zeros(n, np.int64), ts=np.array([0, 1], F32), fs=np.zeros(1, np.int64), flow=flow, shape=shape)
    return with_polarity(c)


# ---------------------------------------------------------------------------
# Cases of the device tests
# ---------------------------------------------------------------------------
DEVICE_SHAPES = ((1, 1), (2, 3), (5, 7), (33, 31))
DEVICE_COUNTS = (0, 1, 255, 256, 257, 4097)
OPTIONS = tuple((mask, pol) for mask in MASKS for pol in (False, True))


def device_matrix():
    """name -> (case, mask, polarity): the shapes x F in {1, 3} at 257 events
    for every mask and both polarity settings; every event count at 5x7 and
    33x31, the one-pixel and degenerate-window cases and 40x40 F=3 (M = 18,
    two partial blocks per image) at mask 7 with polarity; 130 frames, more
    than the closing wave has lanes, with one image a frame and with six."""
    out = {}
    for F in (1, 3):
        for shape in DEVICE_SHAPES:
            c = with_polarity(cc.device_case(shape, F, 257))
            for mask, pol in OPTIONS:
                out[f'{shape[0]}x{shape[1]}_F{F}_n257_m{mask}_p{int(pol)}'] = (c, mask, pol)
    for n in DEVICE_COUNTS:
        for shape in ((5, 7), (33, 31)):
            out[f'{shape[0]}x{shape[1]}_F3_n{n}_m7_p1'] = (with_polarity(cc.device_case(shape, 3, n)), 7, True)
    out['one_pixel_4097_m7_p1'] = (with_polarity(cc.one_pixel_case()), 7, True)
    out['degenerate_windows_m7_p1'] = (with_polarity(cc.degenerate_case()), 7, True)
    out['40x40_F3_n4097_m7_p1'] = (with_polarity(cc.device_case((40, 40), 3, 4097)), 7, True)
    many = with_polarity(cc.many_frames_case())
    out['2x3_F130_n1040_m1_p0'] = (many, 1, False)
    out['2x3_F130_n1040_m7_p1'] = (many, 7, True)
    return out


# ---------------------------------------------------------------------------
# Argument rules of the entry points (the library is handed in)
# ---------------------------------------------------------------------------
EINVAL, ENOSPACE = cc.EINVAL, cc.ENOSPACE


def bad_calls(lib, a, F, h, w, mask=7, polarity=1):
    """(what, zero-argument call, expected code): every call must be refused
    before anything is launched.  a: addresses by name (x, y, t, p, s, ts, fs,
    flow, q, count, result, term, ws, seed, grad) and 'n', the number of
    events; the buffers behind them fit F frames of h x w with six images each."""
    need = lib.dvsof_contrast_multi_workspace_bytes(F, mask, polarity, h, w)

    def fwd(F=F, h=h, w=w, n=None, nbytes=need, mask=mask, polarity=polarity, **null):
        p = dict(a, **{k: None for k in null})
        n = a['n'] if n is None else n
        return lambda: lib.dvsof_contrast_multi_fwd(p['x'], p['y'], p['t'], p['p'], p['s'], n, p['ts'], p['fs'],
                                                    p['flow'], F, h, w, mask, polarity, p['q'], p['count'],
                                                    p['result'], p['term'], p['ws'], nbytes, None)

    def bwd(F=F, h=h, w=w, n=None, nbytes=need, mask=mask, polarity=polarity, **null):
        p = dict(a, **{k: None for k in null})
        n = a['n'] if n is None else n
        return lambda: lib.dvsof_contrast_multi_bwd(p['x'], p['y'], p['t'], p['p'], p['s'], n, p['ts'], p['fs'],
                                                    p['flow'], F, h, w, mask, polarity, p['q'], p['ws'], nbytes,
                                                    p['seed'], 1.0, p['grad'], None)
    sizes = [('F < 0', dict(F=-1)), ('F too large', dict(F=65536)), ('h = 0', dict(h=0)),
             ('w = 0', dict(w=0)), ('h negative', dict(h=-3)), ('h too large', dict(h=32768)),
             ('w too large', dict(w=32768)), ('n_events < 0', dict(n=-1)),
             ('mask 0', dict(mask=0)), ('mask 8', dict(mask=8)), ('mask negative', dict(mask=-1)),
             ('polarity 2', dict(polarity=2)), ('polarity negative', dict(polarity=-1)),
             ('M too large', dict(F=10923)),                # 10923 * 3 * 2 = 65538
             ('M too large without polarity', dict(F=21846, polarity=0)),
             ('M too large at two references', dict(F=16384, mask=5))]
    for name, make in (('fwd', fwd), ('bwd', bwd)):
        for what, kw in sizes:
            yield f'{name}: {what}', make(**kw), EINVAL
        yield f'{name}: no workspace', make(ws=1), ENOSPACE
        yield f'{name}: workspace too small', make(nbytes=need - 1), ENOSPACE
        yield f'{name}: workspace of zero bytes', make(nbytes=0), ENOSPACE
    for k in ('x', 'y', 't', 'p', 's', 'ts', 'fs', 'flow', 'q', 'count', 'result', 'term'):
        yield f'fwd: null {k}', fwd(**{k: 1}), EINVAL
    for k in ('x', 'y', 't', 'p', 's', 'ts', 'fs', 'flow', 'q', 'seed', 'grad'):
        yield f'bwd: null {k}', bwd(**{k: 1}), EINVAL


def empty_calls(lib):
    """F = 0 is fine and launches nothing, with no pointer at all."""
    yield lib.dvsof_contrast_multi_fwd(None, None, None, None, None, 0, None, None, None, 0, 4, 4, 7, 1, None, None,
                                       None, None, None, 0, None)
    yield lib.dvsof_contrast_multi_bwd(None, None, None, None, None, 0, None, None, None, 0, 4, 4, 7, 1, None, None,
                                       0, None, 1.0, None, None)
