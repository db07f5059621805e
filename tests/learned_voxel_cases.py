"""Learnable event representation: numpy restatement of
docs/LEARNED_VOXEL_SPEC.md and the seeded inputs shared by
tests/test_learned_voxel_oracle.py (CPU) and tests/test_gpu_learned_voxel.py.

Everything up to the weight ``w`` is float32, one rounding per operation (the
device arithmetic: the HIP library is built with -ffp-contract=off); the
forward accumulates the float32 products in float64 and rounds once, the
backward is float64 from ``g`` on.
"""
from collections import namedtuple

import numpy as np

from tests import voxel_cases as vc

F32 = np.float32

Forward = namedtuple('Forward', 'grid acc k absw')
Backward = namedtuple('Backward', 'gtheta absterms')
Case = namedtuple('Case', 'ev t0 t1 B C H W R S theta')


def num_knots(R, S):
    return 2 * R * S + 1


def theta_init(R, S):
    d = np.arange(num_knots(R, S), dtype=np.float64) / S - R
    return np.maximum(0.0, 1.0 - np.abs(d)).astype(F32)


def _kept(ev, t0, t1, B, C, H, W):
    """Drop rule and tn of docs/VOXEL_SPEC.md (as tests/voxel_cases.py:voxel_exact).
    -> live (kept and polarity != 0), tn f32, sample, y, x, sign."""
    x, y, p, s = (np.asarray(ev[k], np.int64) for k in ('x', 'y', 'polarity', 'sample_index'))
    t = np.asarray(ev['timestamp'], F32)
    t0, t1 = np.asarray(t0, F32), np.asarray(t1, F32)
    ok = (s >= 0) & (s < B) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    sb, xs, ys = np.where(ok, s, 0), np.where(ok, x, 0), np.where(ok, y, 0)
    lo, hi = t0[sb], t1[sb]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ok &= (t >= lo) & (t <= hi)             # a NaN timestamp is dropped
        dt = hi - lo
        pos = ok & (dt > 0)
        q = np.where(pos, t - lo, F32(0)) / np.where(pos, dt, F32(1))
        tn = np.where(pos, q * F32(C - 1), F32(0))
    assert tn.dtype == F32 and np.isfinite(tn).all()
    sg = np.sign(p)
    return ok & (sg != 0), tn, sb, ys, xs, sg


def _pairs(ev, t0, t1, B, C, H, W, R, S):
    """Every kept (event, bin): -> lin (voxel), j, g (f32), sign."""
    live, tn, sb, ys, xs, sg = _kept(ev, t0, t1, B, C, H, W)
    lin, jj, gg, ss = [], [], [], []
    for c in range(C):
        u = ((tn - F32(c)) + F32(R)) * F32(S)
        assert u.dtype == F32
        kept = live & (u >= 0) & (u < F32(2 * R * S))
        j = np.floor(u[kept]).astype(np.int64)
        g = u[kept] - j.astype(F32)
        assert g.dtype == F32 and ((g >= 0) & (g < 1)).all()
        lin.append((((sb * C + c) * H + ys) * W + xs)[kept])
        jj.append(j)
        gg.append(g)
        ss.append(sg[kept])
    return tuple(np.concatenate(v) for v in (lin, jj, gg, ss))


def learned_forward(ev, t0, t1, theta, R, S, B, C, H, W):
    """-> Forward(grid f32 [B,C,H,W], acc = the float64 sums (flat), k addends per
    voxel, absw = sum |w| per voxel)."""
    theta = np.asarray(theta, F32)
    assert theta.shape == (num_knots(R, S),)
    lin, j, g, s = _pairs(ev, t0, t1, B, C, H, W, R, S)
    w = theta[j] * (F32(1) - g) + theta[j + 1] * g
    assert w.dtype == F32
    total = B * C * H * W
    acc, absw = np.zeros(total), np.zeros(total)
    np.add.at(acc, lin, s * w.astype(np.float64))
    np.add.at(absw, lin, np.abs(w.astype(np.float64)))
    k = np.bincount(lin, minlength=total)
    return Forward(acc.astype(F32).reshape(B, C, H, W), acc, k, absw)


def forward_bound(fw, got):
    """Per-voxel bound for a float32 sum in any order against ``fw.acc``
    (LEARNED_VOXEL_SPEC, Forward): k * 2^-24 * sum|w| + ulp/2."""
    half_ulp = np.spacing(np.abs(np.asarray(got, F32)).ravel()).astype(np.float64) / 2
    return fw.k * 2.0 ** -24 * fw.absw + half_ulp


def forward64(ev, t0, t1, theta64, R, S, B, C, H, W):
    """The forward with float64 weights (u, j, g as specified): linear in theta."""
    lin, j, g, s = _pairs(ev, t0, t1, B, C, H, W, R, S)
    g = g.astype(np.float64)
    theta64 = np.asarray(theta64, np.float64)
    out = np.zeros(B * C * H * W)
    np.add.at(out, lin, s * (theta64[j] * (1 - g) + theta64[j + 1] * g))
    return out.reshape(B, C, H, W)


def learned_backward(ev, t0, t1, gV, R, S, B, C, H, W):
    """float64 gradient of theta and, per knot, the sum of |terms|."""
    lin, j, g, s = _pairs(ev, t0, t1, B, C, H, W, R, S)
    g = g.astype(np.float64)
    sg = s * np.asarray(gV, np.float64).ravel()[lin]
    K = num_knots(R, S)
    gth, absterms = np.zeros(K), np.zeros(K)
    np.add.at(gth, j, sg * (1 - g))
    np.add.at(gth, j + 1, sg * g)
    np.add.at(absterms, j, np.abs(sg * (1 - g)))
    np.add.at(absterms, j + 1, np.abs(sg * g))
    return Backward(gth, absterms)


BWD_THREADS, BWD_EPT, BWD_MAX_BLOCKS = 128, 8, 512


def bwd_blocks(n):
    return min(max(-(-n // (BWD_THREADS * BWD_EPT)), 1), BWD_MAX_BLOCKS)


def chain(n, S):
    """m of LEARNED_VOXEL_SPEC: the longest chain of float32 roundings of a term."""
    per_thread = -(-n // (bwd_blocks(n) * BWD_THREADS)) if n else 0
    return (2 if S == 1 else 1) * per_thread + 11


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def _theta(seed, R, S, kind):
    if kind == 'init':
        return theta_init(R, S)
    return np.random.default_rng(seed).uniform(-1.5, 1.5, num_knots(R, S)).astype(F32)


def _edges(ev, t0, t1, B, sample_past_end):
    """Events exactly at t0 and t1, a NaN timestamp, x = y = -1 padding slots
    and (wire columns only) polarity 0 and a sample index equal to B."""
    s, t = ev['sample_index'], ev['timestamp']
    for b in range(B):
        i = np.flatnonzero(s == b)
        if i.size < 40:
            continue
        t[i[0::29]] = t0[b]
        t[i[1::29]] = t1[b]
        t[i[2::29]] = np.nan
        ev['x'][i[3::29]] = -1
        ev['y'][i[3::29]] = -1
    if sample_past_end:
        ev['polarity'][4::29] = 0
        ev['sample_index'][-7:] = B         # still sorted
    return ev


CASES = {}


def _case(name, seed, B, C, H, W, R, S, kind, counts, wire_only=False, flat_window=None):
    def build():
        ev, t0, t1 = vc.spread(seed, B, H, W, counts)
        if flat_window is not None:         # t0 == t1: only t == t0 is kept (bin 0)
            t1[flat_window] = t0[flat_window]
            i = np.flatnonzero(ev['sample_index'] == flat_window)
            ev['timestamp'][i[::2]] = t0[flat_window]
        ev = _edges(ev, t0, t1, B, wire_only)
        return Case(ev, t0, t1, B, C, H, W, R, S, _theta(seed, R, S, kind))
    CASES[name] = build


#      name            seed B  C  H   W   R  S  theta     events per sample
_case('edges_r2s8', 201, 2, 5, 16, 48, 2, 8, 'random', 1000, wire_only=True)
_case('flat_r1s1', 202, 3, 3, 32, 32, 1, 1, 'random', [700, 0, 700], flat_window=2)
_case('r2s1', 203, 2, 3, 32, 32, 2, 1, 'random', 1000)
_case('r1s8_init', 204, 3, 5, 16, 48, 1, 8, 'init', [600, 800, 600], flat_window=0)
_case('r2s8_init', 205, 2, 5, 32, 32, 2, 8, 'init', 1000)
_case('empty', 206, 2, 3, 16, 48, 2, 8, 'random', 0)

WIRE_ONLY = ('edges_r2s8',)     # polarity 0 / sample == B: not expressible in the encoded columns


def dyadic_case(seed=210, B=2, C=5, H=32, W=32, per=1000):
    """Initial theta, S = 8, timestamps with tn a multiple of 2^-8: the grid is
    bit-identical to the fixed voxel grid."""
    ev, t0, t1 = vc.spread(seed, B, H, W, per, dyadic=True)
    return Case(ev, t0, t1, B, C, H, W, 2, 8, theta_init(2, 8))
