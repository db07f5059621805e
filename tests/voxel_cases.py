"""Voxeliser test matrix: the fixed-point oracle, the launch plan and the inputs
(numpy only, no GPU) shared by tests/test_voxel_exact.py (CPU self-tests) and
tests/test_gpu_voxel_exact.py.

``voxel_exact`` restates docs/VOXEL_SPEC.md the way the TILED path accumulates:
every step up to the fraction ``f`` in float32 (the device arithmetic: the HIP
library is built with -ffp-contract=off -fno-fast-math), then integers,
``F = trunc(f * 2^32)``, 64-bit sums of ``s * (2^32 - F)`` and ``s * F``, one
rounding to float32 at the end.  The tiled kernels must reproduce its grid BIT
FOR BIT on any input; the thread-per-event kernel (float atomics) must do so on
DYADIC input, where every weight is a multiple of 2^-8 and every partial sum is
exact in float32 whatever the order (``Exact.order_free``), and stay within
``v1_bound`` per voxel otherwise.

``plan`` restates v2_plan / v2_launch of csrc/voxel.hip; the CPU test compares
what it implies with dvsof_voxelize_control_bytes / _workspace_bytes for every
case, and every case names the kernel it means to reach, so a moved threshold
cannot silently move a case to the other kernel.
"""
from collections import namedtuple

import numpy as np

F32 = np.float32
TWO32 = 1 << 32
WINDOW = 0.04
KEYS = ('x', 'y', 'timestamp', 'polarity', 'sample_index')

Exact = namedtuple('Exact', 'grid bin0 lin0 acc k absacc quantum order_free')
Plan = namedtuple('Plan', 'tiled kernel ept lp lx TX TY ntile cap control workspace tile_lds')
Case = namedtuple('Case', 'ev t0 t1 B C H W kernel ept dyadic')


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
def voxel_exact(ev, t0, t1, B, C, H, W):
    """-> Exact(grid f32 [B,C,H,W], bin0 i32 [n], lin0 i64 [n], acc i64 (2^-32 fixed
    point, flat), k addends per voxel, absacc = sum |w| per voxel (fixed point),
    quantum = the largest power of two dividing every weight, order_free = any
    float32 summation order of these weights is exact)."""
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
    assert q.dtype == F32 and tn.dtype == F32
    assert np.isfinite(tn).all(), 'not a window: t0 = -inf or t = t1 = +inf makes tn NaN'
    c0 = np.minimum(np.floor(tn).astype(np.int64), C - 1)
    f = tn - c0.astype(F32)
    assert f.dtype == F32 and ((f >= 0) & (f < 1)).all()
    Fx = np.trunc(f.astype(np.float64) * TWO32).astype(np.int64)
    lin = ((sb * C + c0) * H + ys) * W + xs
    bin0 = np.where(ok, c0, -1).astype(np.int32)
    lin0 = np.where(ok, lin, -1).astype(np.int64)
    sg = np.sign(p)
    live = ok & (sg != 0)
    up = live & (c0 + 1 < C)
    total = B * C * H * W
    acc, absacc = np.zeros(total, np.int64), np.zeros(total, np.int64)
    idx = np.concatenate([lin[live], lin[up] + H * W])
    w = np.concatenate([TWO32 - Fx[live], Fx[up]])
    np.add.at(acc, idx, np.concatenate([sg[live], sg[up]]) * w)
    np.add.at(absacc, idx, w)
    k = np.bincount(idx, minlength=total)
    # the last step (int64 -> float64 -> float32) is exact up to the one rounding
    assert k.max(initial=0) < 1 << 21 and absacc.max(initial=0) < 1 << 53
    grid = (acc.astype(np.float64) * 2.0 ** -32).astype(F32).reshape(B, C, H, W)
    bits = int(np.bitwise_or.reduce(w)) if w.size else TWO32
    quantum = bits & -bits if bits else TWO32
    order_free = int(absacc.max(initial=0)) < quantum << 24
    return Exact(grid, bin0, lin0, acc, k, absacc, quantum, order_free)


def v1_bound(ex, got):
    """Per-voxel bound for the thread-per-event kernel against ``acc * 2^-32``:
    k float32 additions, each rounding a partial sum of at most S = sum |w|
    (k * 2^-24 * S); the float32 rounding of 1 - f and the truncation of F
    (k * (2^-25 + 2^-32)); half an ulp of the result for the oracle's own
    final rounding.  Derived, not measured."""
    k = ex.k.astype(np.float64)
    S = ex.absacc.astype(np.float64) * 2.0 ** -32
    half_ulp = np.spacing(np.abs(np.asarray(got, F32)).ravel()).astype(np.float64) / 2
    return k * 2.0 ** -24 * S + k * (2.0 ** -25 + 2.0 ** -32) + half_ulp


def oracle_bound(ex, want):
    """Per-voxel bound between ``voxel_exact`` and orc.voxelize (double sums of
    the float32 products): 2^-32 truncation of F and 2^-25 rounding of 1 - f per
    addend, one ulp for the two final roundings."""
    k = ex.k.astype(np.float64)
    return k * (2.0 ** -32 + 2.0 ** -25) + np.spacing(np.abs(np.asarray(want, F32)).ravel())


# ---------------------------------------------------------------------------
# the launch plan (v2_plan, v2_launch, dvsof_voxelize_*_bytes)
# ---------------------------------------------------------------------------
V2_MAX_TILES = 8192
V1_BELOW = 4096
EPT8_FROM = 1 << 21
EPT16_FROM = 3 << 20
V1_GRID = 2048 * 256        # threads of the largest thread-per-event launch


def plan(n, B, C, H, W):
    lp = 9 if C * 1024 * 8 > 52 * 1024 else 10
    lx, best_pad = 6, 1 << 30
    for c in range(6, lp + 1):
        wd = 1 << c
        padded = (W + wd - 1) // wd * wd
        if padded * 8 <= W * 9:
            lx, best_pad = c, 0
        elif best_pad and padded - W < best_pad:
            lx, best_pad = c, padded - W
    TX = (W + (1 << lx) - 1) >> lx
    TY = (H + (1 << (lp - lx)) - 1) >> (lp - lx)
    nt = B * TX * TY
    cap = (2 * (n // nt) + 256 + 63) // 64 * 64
    tile_lds = (C << lp) * 8
    tiled = (n >= V1_BELOW and nt <= V2_MAX_TILES and tile_lds <= 150 * 1024 and C <= 1023
             and cap <= 1 << 24)
    control = ((nt + 3) * 4 + 255) // 256 * 256 if tiled else 0
    workspace = control + nt * cap * 8 + n * 16 + 256 if tiled else n * 32 + 64
    ept = (16 if n >= EPT16_FROM else 8 if n >= EPT8_FROM else 4) if tiled else 0
    return Plan(tiled, 'tiled' if tiled else 'v1', ept, lp, lx, TX, TY, nt, cap, control,
                workspace, tile_lds)


def tile_ids(ev, ex, pl):
    """Tile of every event that reaches a bucket (kept, polarity != 0)."""
    live = (ex.bin0 >= 0) & (np.asarray(ev['polarity']) != 0)
    x, y, s = (np.asarray(ev[k])[live] for k in ('x', 'y', 'sample_index'))
    return (s * pl.TY + (y >> (pl.lp - pl.lx))) * pl.TX + (x >> pl.lx)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def windows(rng, B, kind):
    if kind == 'zero':
        return np.zeros(B, F32), np.full(B, WINDOW, F32)
    if kind == 'dyadic':        # t0 = i / 16 (never 0), t1 - t0 = 2^-3
        t0 = (rng.integers(1, 65, B) / 16).astype(F32)
        return t0, t0 + F32(0.125)
    t0 = rng.uniform(0.0, 4.0, B).astype(F32)               # per sample, up to ~4 s
    return t0, (t0 + rng.uniform(0.01, 0.2, B).astype(F32)).astype(F32)


def stamps(rng, t0, t1, s, dyadic, g=8):
    """float32 timestamps inside the window of each event's sample; dyadic:
    t0 + j * 2^-(3+g), j in [0, 2^g] -- every float32 step up to f is exact."""
    lo, hi = t0[s], t1[s]
    if dyadic:
        t = lo + (rng.integers(0, (1 << g) + 1, s.size) * 2.0 ** -(3 + g)).astype(F32)
        assert t.dtype == F32
        return t
    t = (lo + rng.random(s.size, dtype=F32) * (hi - lo)).astype(F32)
    return np.clip(t, lo, hi)


def spread(seed, B, H, W, per_sample, window='per_sample', dyadic=False):
    """Well-spread events grouped by sample; per_sample: int or one count per sample."""
    rng = np.random.default_rng(seed)
    counts = [per_sample] * B if np.isscalar(per_sample) else list(per_sample)
    assert len(counts) == B
    t0, t1 = windows(rng, B, 'dyadic' if dyadic else window)
    s = np.repeat(np.arange(B, dtype=np.int64), counts)
    n = s.size
    ev = {'x': rng.integers(0, W, n, dtype=np.int64), 'y': rng.integers(0, H, n, dtype=np.int64),
          'timestamp': stamps(rng, t0, t1, s, dyadic),
          'polarity': rng.integers(0, 2, n, dtype=np.int64) * 2 - 1, 'sample_index': s}
    return ev, t0, t1


def crowd(ev, pl, B, H, W, fills, seed=0):
    """Move events so that tile ``tile`` holds EXACTLY ``fills[tile]`` of them and
    every other event lies outside the crowded tiles (same sample, other pixel)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    pix_tile = ((yy >> (pl.lp - pl.lx)) * pl.TX + (xx >> pl.lx)).ravel()
    s = ev['sample_index']
    todo = np.ones(s.size, bool)
    for tile, cnt in fills.items():
        b, local = divmod(tile, pl.TX * pl.TY)
        inside = np.flatnonzero(pix_tile == local)
        take = np.flatnonzero(todo & (s == b))[:cnt]
        assert take.size == cnt and inside.size
        pix = inside[rng.integers(0, inside.size, cnt)]
        ev['y'][take], ev['x'][take] = pix // W, pix % W
        todo[take] = False
    for b in range(B):
        crowded = [t % (pl.TX * pl.TY) for t in fills if t // (pl.TX * pl.TY) == b]
        rest = np.flatnonzero(todo & (s == b))
        free = np.flatnonzero(~np.isin(pix_tile, crowded))
        pix = free[rng.integers(0, free.size, rest.size)]
        ev['y'][rest], ev['x'][rest] = pix // W, pix % W
    return ev


def shuffled(ev, seed=0):
    perm = np.random.default_rng(seed).permutation(ev['x'].size)
    return {k: v[perm] for k, v in ev.items()}


def compactable(ev, B):
    """Can the encoded (9 B/event) entry carry these events?"""
    s = ev['sample_index']
    return bool(s.size and (np.diff(s) >= 0).all() and s.min() >= 0 and s.max() < B
                and (np.abs(ev['polarity']) == 1).all()
                and all(-(1 << 15) <= ev[k].min() and ev[k].max() < 1 << 15 for k in 'xy'))


def compact(ev, B):
    """Encoded columns + sample_event_offsets (empty samples repeat an offset)."""
    assert compactable(ev, B)
    off = np.searchsorted(ev['sample_index'], np.arange(B + 1)).astype(np.int64)
    return {'x': ev['x'].astype(np.int16), 'y': ev['y'].astype(np.int16),
            'timestamp': ev['timestamp'].astype(F32), 'polarity': ev['polarity'] > 0,
            'sample_event_offsets': off}


def window_edges(ev, t0, t1, dyadic):
    """Overwrite slices of a 4-sample input with the window's edges.  Sample 2:
    t0 == t1 (events on it land in bin 0 with f = 0), sample 3: t1 < t0 (all
    dropped).  Samples 0 and 1 keep their windows."""
    s, t = ev['sample_index'], ev['timestamp']
    t0, t1 = t0.copy(), t1.copy()
    t1[2] = t0[2]
    t0[3], t1[3] = t1[3], t0[3]
    on2 = np.flatnonzero(s == 2)
    t[on2[::2]] = t0[2]                                    # on the degenerate window
    t[on2[1::4]] = np.nextafter(t0[2], F32(np.inf))        # one ulp off it: dropped
    for b in (0, 1):
        i = np.flatnonzero(s == b)
        lo, hi = t0[b], t1[b]
        t[i[0::23]] = lo                                           # first bin, f = 0
        t[i[1::23]] = hi                                           # tn = C - 1: clamped
        t[i[2::23]] = np.nextafter(lo, F32(-np.inf))               # one ulp outside
        t[i[3::23]] = np.nextafter(hi, F32(np.inf))
        t[i[4::23]] = np.nan                                       # dropped (VOXEL_SPEC)
        t[i[5::23]] = np.inf
        t[i[6::23]] = -np.inf
        if not dyadic:      # (their weights are not multiples of 2^-8)
            t[i[7::23]] = np.nextafter(lo, F32(np.inf))            # tiny f: F truncates
            t[i[8::23]] = np.nextafter(hi, F32(-np.inf))           # f just below 1
    return ev, t0, t1


def drops(ev, B):
    """Coordinates / samples outside the frame, the batch and int32; polarity -3..3."""
    rng = np.random.default_rng(5)
    n = ev['x'].size
    ev['polarity'] = rng.integers(-3, 4, n).astype(np.int64)
    ev['x'][0::31] = -1
    ev['y'][1::31] = -5
    ev['x'][2::31] = (1 << 32) + 3
    ev['y'][3::31] = -(1 << 32)
    ev['sample_index'][4::31] = -1
    ev['sample_index'][5::31] = B
    ev['sample_index'][6::31] = 1 << 32
    return ev


CASES = {}


def case(name, kernel, ept=0, dyadic=False):
    def reg(fn):
        def build():
            ev, t0, t1, B, C, H, W = fn()
            return Case(ev, t0, t1, B, C, H, W, kernel, ept, dyadic)
        CASES[name] = build
        return fn
    return reg


def both(name, kernel, ept, fn):
    """Register ``fn(dyadic)`` with random float and with dyadic timestamps."""
    case(name, kernel, ept)(lambda: fn(False))
    case(name + '_dyadic', kernel, ept, True)(lambda: fn(True))


def _basic(seed, B, C, H, W, per, **kw):
    def fn(dyadic):
        return spread(seed, B, H, W, per, dyadic=dyadic, **kw) + (B, C, H, W)
    return fn


# kernel variant -------------------------------------------------------------
both('v1_small', 'v1', 0, _basic(1, 2, 5, 37, 53, 1000))
both('ept4', 'tiled', 4, _basic(2, 4, 5, 128, 160, 10000))
case('ept8', 'tiled', 8)(lambda: _basic(3, 2, 5, 256, 256, 1_100_000)(False))
case('ept16', 'tiled', 16)(lambda: _basic(4, 4, 12, 512, 512, 800_000)(False))
both('v1_grid_stride', 'v1', 0, _basic(5, 1, 38, 32, 48, 600_000))
# tile: 1024 pixels up to C = 6, 512 above; 64 KiB of LDS at C = 16, the raised
# limit from C = 17 to the deepest tiled C = 37, thread-per-event above
for _C in (1, 5, 6, 7, 12, 16, 17, 37):
    both(f'depth{_C}', 'tiled', 4, _basic(10 + _C, 2, _C, 70, 90, 6000))
both('depth38_fallback', 'v1', 0, _basic(48, 2, 38, 70, 90, 6000))
# frame: tiles wider than the frame, ragged right / bottom tiles, scalar stores
for _H, _W in ((70, 16), (300, 1), (1, 640), (260, 346), (64, 640)):
    both(f'frame{_H}x{_W}', 'tiled', 4, _basic(_H + _W, 2, 5, _H, _W, 6000))
# tile count: just under, exactly at and above the bucket pass's histogram
case('tiles8160', 'tiled', 4)(lambda: _basic(60, 32, 1, 510, 512, 2048)(False))
case('tiles8192', 'tiled', 4)(lambda: _basic(61, 32, 1, 512, 512, 2048)(False))
case('tiles8448_fallback', 'v1')(lambda: _basic(62, 33, 1, 512, 512, 2048)(False))


# window ---------------------------------------------------------------------
def _edges(per):
    def fn(dyadic):
        ev, t0, t1 = spread(70, 4, 64, 96, per, dyadic=dyadic)
        return window_edges(ev, t0, t1, dyadic) + (4, 9, 64, 96)
    return fn


both('window_edges', 'tiled', 4, _edges(5000))
both('window_edges_v1', 'v1', 0, _edges(800))


def _open_window(per):
    def fn():
        ev, t0, t1 = spread(71, 2, 64, 96, per)
        t1[0] = np.inf                      # dt = inf: every event from t0 on, tn = 0
        return ev, t0, t1, 2, 9, 64, 96
    return fn


case('window_open_end', 'tiled', 4)(_open_window(5000))
case('window_open_end_v1', 'v1')(_open_window(800))

# bucket fill: B = 2, 64 x 96, 8192 events -> 16 tiles of 64 x 16, cap = 1280
FILL_SHAPE = (2, 5, 64, 96)
FILL_N = 4096
FILL_CAP = 1280
FILL_TILE = 13                              # sample 1, a right-hand tile


def _fill(fills):
    def fn(dyadic):
        B, C, H, W = FILL_SHAPE
        ev, t0, t1 = spread(80, B, H, W, FILL_N, dyadic=dyadic)
        pl = plan(B * FILL_N, B, C, H, W)
        return crowd(ev, pl, B, H, W, fills), t0, t1, B, C, H, W
    return fn


for _n in (1023, 1024, 1025, FILL_CAP - 1, FILL_CAP, FILL_CAP + 1):
    both(f'fill{_n}', 'tiled', 4, _fill({FILL_TILE: _n}))
# three buckets of two samples overflow in one call next to well-spread tiles
MULTI_FILLS = {2: FILL_CAP + 300, 7: FILL_CAP + 1, FILL_TILE: 2 * FILL_CAP}
both('fill_three_overflows', 'tiled', 4, _fill(MULTI_FILLS))


def _one_pixel(dyadic):
    B, C, H, W = FILL_SHAPE
    ev, t0, t1 = spread(81, B, H, W, FILL_N, dyadic=dyadic)
    ev['x'][:], ev['y'][:], ev['sample_index'][:] = 77, 41, 1
    return ev, t0, t1, B, C, H, W


both('one_pixel', 'tiled', 4, _one_pixel)


# dropped ----------------------------------------------------------------------
def _drops(per):
    def fn(dyadic):
        ev, t0, t1 = spread(90, 3, 70, 90, per, dyadic=dyadic)
        return drops(ev, 3), t0, t1, 3, 5, 70, 90
    return fn


both('drops', 'tiled', 4, _drops(4000))
both('drops_v1', 'v1', 0, _drops(1000))


def _all_dropped():
    ev, t0, t1 = spread(91, 2, 70, 90, 3000)
    ev['x'][:] = -1
    return ev, t0, t1, 2, 5, 70, 90


def _all_zero():
    ev, t0, t1 = spread(92, 2, 70, 90, 3000)
    ev['polarity'][:] = 0
    return ev, t0, t1, 2, 5, 70, 90


case('all_dropped', 'tiled', 4)(_all_dropped)
case('all_polarity_zero', 'tiled', 4)(_all_zero)


# order --------------------------------------------------------------------------
def _shuffled(dyadic):
    ev, t0, t1 = spread(95, 6, 128, 160, 5000, dyadic=dyadic)
    return shuffled(ev), t0, t1, 6, 7, 128, 160


both('shuffled_across_samples', 'tiled', 4, _shuffled)
both('one_sample_empty', 'tiled', 4, _basic(96, 3, 5, 70, 90, [5000, 0, 5000]))


# encoded entry: empty samples first / middle / last, negative int16 coordinates
def _gaps(counts):
    def fn(dyadic):
        ev, t0, t1 = spread(97, 6, 70, 90, counts, dyadic=dyadic)
        ev['x'][0::41] = -3
        ev['y'][1::41] = -32768
        return ev, t0, t1, 6, 5, 70, 90
    return fn


both('encoded_gaps', 'tiled', 4, _gaps([0, 4000, 0, 0, 4000, 0]))
both('encoded_gaps_v1', 'v1', 0, _gaps([0, 700, 0, 0, 900, 0]))

ENCODED_FAMILY = [n for n in CASES if n.startswith('encoded_')]
