"""Shared pieces of the tests of the average-timestamp term
(docs/AVG_TIMESTAMP_SPEC.md): the cases of tests/contrast_multi_cases.py, the
float64 definition in torch with its gradient by autograd, the bounds the spec
derives (section 8), and the argument rules of the entry points.  Nothing here
touches the package under test."""
import numpy as np
import torch

from tests import contrast_cases as cc, contrast_multi_cases as mc

F32 = np.float32
EPS = 2.0 ** -10                # T = A / (I + EPS), the decision of section 3
MASKS = mc.MASKS
KEYS = mc.KEYS
ORACLE_IDS = list(cc.ORACLE_CASES)
MIN_WEIGHT = 2.0 ** -20         # every positive float64 corner weight of every case lies above it

case = mc.case
args_of = mc.args_of
permuted = mc.permuted
rhos = mc.rhos
sink_case = mc.sink_case
device_matrix = mc.device_matrix
coordinate_bound = mc.coordinate_bound


def images_of(c, mask, polarity):
    """(m, f, pairs) for every image m = (f R + r) C + ch: contrast_multi_cases.pairs64
    of its reference and channel."""
    R, C = len(rhos(mask)), 2 if polarity else 1
    for r, rho in enumerate(rhos(mask)):
        for ch in range(C):
            for f, p in enumerate(mc.pairs64(c, rho, mc.channel_events(c, polarity, ch))):
                yield (f * R + r) * C + ch, f, p


def corner_weights64(c, mask, polarity):
    """Every float64 corner weight of the events that stay in reach of their image."""
    out = []
    for _, _, p in images_of(c, mask, polarity):
        k = p['inside']
        fx, fy = p['xw'][k] - np.floor(p['xw'][k]), p['yw'][k] - np.floor(p['yw'][k])
        out += [wy * wx for wy in (1 - fy, fy) for wx in (1 - fx, fx)]
    return np.concatenate(out) if out else np.zeros(0)


def moving_points_case(flow=(3.0, -2.0)):
    """contrast_cases.translating_pattern with a polarity column; -> (case at zero flow, case at
    the true flow)."""
    c = cc.translating_pattern(flow=flow)
    zero = mc.with_polarity(dict(c, flow=cc.constant_flow(c['shape'], (0.0, 0.0))))
    return zero, dict(zero, flow=cc.constant_flow(c['shape'], flow))


def all_leave_case():
    """One 5x7 frame whose events are all carried far outside it at either end of the window
    (|sig| >= 1/4 at both, the flow 64 pixels), and a second frame whose sample has no events."""
    n = 40
    rng = np.random.default_rng(17)
    flow = np.zeros((2, 2, 5, 7), F32)
    flow[0, 0] = 64.0
    c = dict(x=rng.integers(0, 7, n), y=rng.integers(0, 5, n), t=(0.25 + 0.5 * rng.random(n)).astype(F32),
             s=np.zeros(n, np.int64), ts=np.array([0, 1, 0, 1], F32), fs=np.array([0, 5], np.int64), flow=flow,
             shape=(5, 7))
    return mc.with_polarity(c)


# ---------------------------------------------------------------------------
# The definition: torch float64 on the CPU, the gradient by autograd
# ---------------------------------------------------------------------------
def oracle64(c, mask=5, polarity=False):
    """-> dict(term float, grad float64 [F,2,h,w] = d term / d flow, and per image I, A (the
    images of weights and of weight times distance), count, base [M,h,w], S, S0, n, n0, value
    [M]).  Weights from the float64 coordinate, nothing truncated, the floor convention of the
    kernels; n is the number of pixels with I > 0, a constant of the derivative."""
    h, w = c['shape']
    F, N = len(c['fs']), h * w
    R, C = len(rhos(mask)), 2 if polarity else 1
    M = F * R * C
    flow = torch.tensor(c['flow'].astype(np.float64), requires_grad=True)
    term = torch.zeros((), dtype=torch.float64)
    keep = {k: np.zeros((M, h, w)) for k in ('I', 'A', 'count', 'base')}
    stat = {k: np.zeros(M) for k in ('S', 'S0', 'n', 'n0', 'value')}
    for m, f, p in images_of(c, mask, polarity):
        x, y = torch.from_numpy(p['x']), torch.from_numpy(p['y'])
        sig = torch.from_numpy(p['sig'])
        a = sig.abs()
        own = y * w + x
        count = torch.zeros(N, dtype=torch.float64).index_add(0, own, torch.ones(len(x), dtype=torch.float64))
        base = torch.zeros(N, dtype=torch.float64).index_add(0, own, a)
        k = torch.from_numpy(p['inside'])
        x, y, sig, a = x[k], y[k], sig[k], a[k]
        xw = x - sig * flow[f, 0, y, x]
        yw = y - sig * flow[f, 1, y, x]
        bx, by = torch.floor(xw).detach(), torch.floor(yw).detach()
        fx, fy = xw - bx, yw - by
        I, A = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
        for j, wy in enumerate((1 - fy, fy)):
            for i, wx in enumerate((1 - fx, fx)):
                px, py = (bx + i).long(), (by + j).long()
                ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
                I = I.index_add(0, (py * w + px)[ok], (wy * wx)[ok])
                A = A.index_add(0, (py * w + px)[ok], (wy * wx * a)[ok])
        T, T0 = A / (I + EPS), base / (count + EPS)
        S, S0 = (T * T).sum(), (T0 * T0).sum()
        n, n0 = int((I.detach() > 0).sum()), int((count > 0).sum())
        if float(S0) > 0:
            value = (S / n) / (S0 / n0) if n > 0 else torch.ones((), dtype=torch.float64)
            term = term + value
            stat['value'][m] = float(value.detach())
        for name, v in (('I', I), ('A', A), ('count', count), ('base', base)):
            keep[name][m] = v.detach().numpy().reshape(h, w)
        stat['S'][m], stat['S0'][m], stat['n'][m], stat['n0'][m] = float(S.detach()), float(S0), n, n0
    term = term / M
    if term.requires_grad:
        term.backward()
    grad = flow.grad.numpy() if flow.grad is not None else np.zeros(flow.shape)
    return dict(keep, **stat, term=float(term.detach()), grad=grad, mask=mask, polarity=polarity)


def bounds(c, o, seed=1.0, weight=1.0):
    """AVG_TIMESTAMP_SPEC section 8 for the oracle o = oracle64(c, mask, polarity) -> (bound of
    |term32 - term64|, bound of |grad32 - seed weight grad64| per element [F,2,h,w]).  Computed
    from the case and the oracle's float64 quantities only.  Per pixel, with D = 1 / (I + EPS):
      |I32 - I64| <= b_I = e_w touching                 (e_w: IWE_SPEC section 5 with this delta)
      |A32 - A64| <= b_A = (e_w + 2^-25 + 2^-32) touching + d_sig I
                         (w32 a32 - w a = (w32 - w) a32 + w (a32 - a); one rounding, one truncation)
      |T32 - T64| <= b_T = (b_A + T b_I) / (I + EPS - b_I): it scales with D(p)
    and from there S, S0, k and G = 2 k T D (a - T) term by term."""
    h, w = c['shape']
    mask, polarity = o['mask'], o['polarity']
    R, C = len(rhos(mask)), 2 if polarity else 1
    F, N = len(c['fs']), float(h * w)
    M = F * R * C
    delta = coordinate_bound(c)
    e_w = 2 * delta + 5 * 2.0 ** -25 + 2.0 ** -32
    assert delta < mc.KINK      # both arithmetics take the same floor and the same inside test
    d_sig, d_w = 2.0 ** -22, delta + 2.0 ** -24
    unit_loss = 2.0 ** -39 if R == 1 else 2.0 ** -37      # one unit against the frame's gmax
    b_term, b_grad = 0.0, np.zeros((F, 2, h, w))
    prepared, frame_gmax = {}, np.zeros(F)
    for m, f, p in images_of(c, mask, polarity):
        I, A, cnt, base = (o[k][m] for k in ('I', 'A', 'count', 'base'))
        S, S0, n, n0 = (o[k][m] for k in ('S', 'S0', 'n', 'n0'))
        if not S0 > 0:
            assert cnt.sum() == 0, 'an image whose events all sit on the reference: not a case of these bounds'
            continue
        if n == 0:
            continue            # 1 in both arithmetics, no gradient in either
        k = p['inside']
        x, y, sig, xw, yw = (p[name][k] for name in ('x', 'y', 'sig', 'xw', 'yw'))
        bx, by = np.floor(xw).astype(np.int64), np.floor(yw).astype(np.int64)
        touching = np.zeros((h, w))
        corner = {}
        for j in range(2):
            for i in range(2):
                px, py = bx + i, by + j
                ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
                np.add.at(touching, (py[ok], px[ok]), 1)
                corner[j, i] = (ok, np.where(ok, py, 0), np.where(ok, px, 0))
        b_I = e_w * touching
        b_A = (e_w + 2.0 ** -25 + 2.0 ** -32) * touching + d_sig * I
        den = I + EPS
        assert (den > 2 * b_I).all()
        T, D, D_up = A / den, 1 / den, 1 / (den - b_I)
        b_T = D_up * (b_A + T * b_I) + 2.0 ** -50 * T
        b_D = b_I * D * D_up + 2.0 ** -52 * D
        b_S = (2 * T * b_T + b_T * b_T).sum() + (N + 4) * 2.0 ** -52 * (S + (2 * T * b_T + b_T * b_T).sum())
        # the baseline: a32 against a64, truncated once, count of them on a pixel
        T0 = base / (cnt + EPS)
        b_T0 = cnt * (d_sig + 2.0 ** -32) / (cnt + EPS) + 2.0 ** -50 * T0
        b_S0 = (2 * T0 * b_T0 + b_T0 * b_T0).sum() + (N + 4) * 2.0 ** -52 * (S0 + (2 * T0 * b_T0 + b_T0 * b_T0).sum())
        assert S0 > 2 * b_S0
        ratio = n0 / n
        value = ratio * S / S0
        b_term += ratio * (b_S / (S0 - b_S0) + S * b_S0 / (S0 * (S0 - b_S0))) + 2.0 ** -49 * value
        kk = n0 / (n * S0)
        b_k = kk * b_S0 / (S0 - b_S0) + 2.0 ** -50 * kk
        H = 2 * kk * T * D                                  # G = H (a - T)
        b_H = 2 * ((kk + b_k) * (T + b_T) * (D + b_D) - kk * T * D) + 2.0 ** -49 * H
        frame_gmax[f] = max(frame_gmax[f], (H + b_H).max() * (1 + 2.0 ** -49))
        prepared[m] = (f, x, y, sig, xw - bx, yw - by, corner, T, H, b_T, b_H)
    for m, (f, x, y, sig, fx, fy, corner, T, H, b_T, b_H) in prepared.items():
        a, asig = np.abs(sig), np.abs(sig)
        trunc = unit_loss * frame_gmax[f]
        G, d_G = {}, {}
        for key, (ok, yy, xx) in corner.items():
            dist = a - T[yy, xx]
            G[key] = np.where(ok, H[yy, xx] * dist, 0.0)
            slack = d_sig + b_T[yy, xx]
            d_G[key] = np.where(ok, b_H[yy, xx] * (np.abs(dist) + slack) + H[yy, xx] * slack
                                + 2.0 ** -49 * np.abs(H[yy, xx] * dist), 0.0)
        for comp, (wa, pairs_) in enumerate((((1 - fy, fy), (((0, 1), (0, 0)), ((1, 1), (1, 0)))),
                                             ((1 - fx, fx), (((1, 0), (0, 0)), ((1, 1), (0, 1)))))):
            exact, upper = np.zeros(x.size), np.zeros(x.size)
            for wgt, (hi, lo) in zip(wa, pairs_):
                Dlt = G[hi] - G[lo]
                exact += wgt * np.abs(Dlt)
                upper += (wgt + d_w) * (np.abs(Dlt) + d_G[hi] + d_G[lo])
            per_event = (asig + d_sig) * upper - asig * exact + 2.0 ** -49 * asig * exact + trunc
            np.add.at(b_grad[f, comp], (y, x), per_event)
    sw = abs(seed * weight)
    want = sw * np.abs(o['grad'])
    b_grad = sw * b_grad / M
    b_grad = b_grad + 2.0 ** -22 * (want + b_grad) + 2.0 ** -149
    return b_term / M + 2.0 ** -24 * abs(o['term']) + 2.0 ** -149, b_grad


# ---------------------------------------------------------------------------
# Argument rules of the entry points (the library is handed in)
# ---------------------------------------------------------------------------
EINVAL, ENOSPACE = cc.EINVAL, cc.ENOSPACE


def bad_calls(lib, a, F, h, w, mask=7, polarity=1):
    """(what, zero-argument call, expected code): every call must be refused before anything is
    launched.  a: addresses by name (x, y, t, p, s, ts, fs, flow, term, ws, seed, grad) and 'n',
    the number of events; the buffers behind them fit F frames of h x w with six images each."""
    need = lib.dvsof_avg_timestamp_workspace_bytes(F, mask, polarity, h, w)

    def fwd(F=F, h=h, w=w, n=None, nbytes=need, mask=mask, polarity=polarity, **null):
        p = dict(a, **{k: None for k in null})
        n = a['n'] if n is None else n
        return lambda: lib.dvsof_avg_timestamp_fwd(p['x'], p['y'], p['t'], p['p'], p['s'], n, p['ts'], p['fs'],
                                                   p['flow'], F, h, w, mask, polarity, p['term'], p['ws'], nbytes,
                                                   None)

    def bwd(F=F, h=h, w=w, n=None, nbytes=need, mask=mask, polarity=polarity, **null):
        p = dict(a, **{k: None for k in null})
        n = a['n'] if n is None else n
        return lambda: lib.dvsof_avg_timestamp_bwd(p['x'], p['y'], p['t'], p['p'], p['s'], n, p['ts'], p['fs'],
                                                   p['flow'], F, h, w, mask, polarity, p['ws'], nbytes, p['seed'],
                                                   1.0, p['grad'], None)
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
    for k in ('x', 'y', 't', 'p', 's', 'ts', 'fs', 'flow', 'term'):
        yield f'fwd: null {k}', fwd(**{k: 1}), EINVAL
    for k in ('x', 'y', 't', 'p', 's', 'ts', 'fs', 'flow', 'seed', 'grad'):
        yield f'bwd: null {k}', bwd(**{k: 1}), EINVAL


def empty_calls(lib):
    """F = 0 is fine and launches nothing, with no pointer at all."""
    yield lib.dvsof_avg_timestamp_fwd(None, None, None, None, None, 0, None, None, None, 0, 4, 4, 7, 1, None, None,
                                      0, None)
    yield lib.dvsof_avg_timestamp_bwd(None, None, None, None, None, 0, None, None, None, 0, 4, 4, 7, 1, None, 0,
                                      None, 1.0, None, None)


# every positive float64 corner weight of every oracle case, at every reference and in either
# channel, lies above MIN_WEIGHT: float32 keeps it positive (delta < KINK, so either factor stays
# above 2^-11 and Q >= 1), and the restatement and the definition count the same pixels in n
for _name in ORACLE_IDS:
    _w = corner_weights64(case(_name), 7, False)
    assert _w.size and _w[_w > 0].min() > MIN_WEIGHT, (_name, _w[_w > 0].min())
