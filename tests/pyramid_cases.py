"""The frame pyramid (csrc/loss.hip: resize_bilinear_ac_kernel, loss_pyramid_kernel,
pyramid_plan, pyramid_launch) restated in numpy, operation by operation, with the case
tables of tests/test_pyramid_oracle.py (CPU) and tests/test_gpu_pyramid.py (GPU).
docs/PYRAMID_SPEC.md is the text.  No GPU, no torch.

``resize_host`` / ``pyramid_host`` are the values: float32 operation by float32 operation,
the dtype asserted after every step, so the device's bytes can be compared with theirs.
``plan_host`` / ``regions_host`` restate which kernel runs and what one tile of it stages and
stores: no entry point reports that, so these two show that a case reaches a mechanism.
"""
import functools
import zlib

import numpy as np

F32 = np.float32
TH, TW = 16, 64            # the small tile of the finest level; the big one is twice that
PYR_MAXR = 1536            # floats per staged region (one of two LDS buffers)
MAX_SCALES = 8             # DVSOF_MAX_SCALES
BIG_FROM = 2048            # small workgroups from which big tiles are tried
MAX_FRAMES = 65535         # gridDim.z of the per-level kernel
EINVAL = -1                # DVSOF_EINVAL, include/dvsof.h
# a coarse pixel is stored by the first tile whose region holds it: strictly past the
# previous tile's region end in both directions
STORE_RULE = 'y > pey[k] && x > pex[k]'


def _f32(a):
    assert a.dtype == F32, a.dtype
    return a


# ---------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------
def step(nin, nout):
    """Input step per output pixel: float32 quotient of two exact float32 integers."""
    return _f32(F32(nin - 1) / F32(nout - 1)) if nout > 1 else F32(0)


def axis_host(nin, nout):
    """-> i0, i1 (int64 tap indices), l, h (float32 weights of i1, i0) of every output index."""
    s = step(nin, nout)
    o = _f32(np.arange(nout).astype(F32))
    f = _f32(s * o)
    i0 = np.minimum(f.astype(np.int32), nin - 1).astype(np.int64)   # f >= 0: truncation is floor
    i1 = i0 + (i0 < nin - 1)
    lo = _f32(f - _f32(i0.astype(F32)))
    hi = _f32(F32(1) - lo)
    return i0, i1, lo, hi


def resize_host(src, hout, wout):
    """src [n,hin,win] float32 -> [n,hout,wout] float32, the operations of the spec in its order."""
    src = _f32(np.asarray(src))
    n, hin, win = src.shape
    y0, y1, ly, hy = axis_host(hin, hout)
    x0, x1, lx, hx = axis_host(win, wout)
    ly, hy = ly[None, :, None], hy[None, :, None]
    lx, hx = lx[None, None, :], hx[None, None, :]
    a, b = src[:, y0][:, :, x0], src[:, y0][:, :, x1]
    c, d = src[:, y1][:, :, x0], src[:, y1][:, :, x1]
    with np.errstate(all='ignore'):     # 0 * inf, inf - inf, subnormal products: IEEE results
        top = _f32(_f32(hx * a) + _f32(lx * b))
        bot = _f32(_f32(hx * c) + _f32(lx * d))
        v = _f32(_f32(hy * top) + _f32(ly * bot))
    assert v.shape == (n, hout, wout)
    return np.ascontiguousarray(v)     # indexing with arrays leaves other strides


def pyramid_host(images, shapes):
    """The cascade: level k resamples level k-1, level 0 the images [D,H,W]."""
    out, cur = [], _f32(np.asarray(images))
    for h, w in shapes:
        cur = resize_host(cur, h, w)
        out.append(cur)
    return out


# ---------------------------------------------------------------------------
# plan and regions
# ---------------------------------------------------------------------------
def fits_host(shapes, th, tw):
    """pyramid_plan's bound of the staged regions of a th x tw tile (double arithmetic on
    the float32 steps; the finest level itself is not staged)."""
    rh, rw = float(th), float(tw)
    for k in range(len(shapes) - 1, 0, -1):
        rh = rh * float(step(shapes[k - 1][0], shapes[k][0])) + 3
        rw = rw * float(step(shapes[k - 1][1], shapes[k][1])) + 3
        rh, rw = min(rh, shapes[k - 1][0]), min(rw, shapes[k - 1][1])
        if rh * rw > PYR_MAXR:
            return False
    return True


def small_tiles(D, shapes):
    h, w = shapes[-1]
    return D * (-(-w // TW)) * (-(-h // TH))


def plan_host(D, H, W, shapes):
    """-> ('fused', big) or 'per_level' (D = 0 takes the per-level branch and launches
    nothing).  Arguments that the entry points refuse are not a plan: assert."""
    K = len(shapes)
    assert D >= 0 and H >= 1 and W >= 1 and 1 <= K <= MAX_SCALES
    assert all(h >= 1 and w >= 1 for h, w in shapes)
    if D == 0:
        return 'per_level'
    if any(shapes[k][0] < shapes[k - 1][0] or shapes[k][1] < shapes[k - 1][1] for k in range(1, K)):
        return 'per_level'
    if not fits_host(shapes, TH, TW):
        return 'per_level'
    big = small_tiles(D, shapes) >= BIG_FROM and fits_host(shapes, 2 * TH, 2 * TW)
    th, tw = (2 * TH, 2 * TW) if big else (TH, TW)
    if D * (-(-shapes[-1][1] // tw)) * (-(-shapes[-1][0] // th)) > 0x3fffffff:
        return 'per_level'
    return 'fused', bool(big)


def tile_grid(shapes, big):
    th, tw = (2 * TH, 2 * TW) if big else (TH, TW)
    return -(-shapes[-1][0] // th), -(-shapes[-1][1] // tw)


def _lo(s, o):
    return int(_f32(s * F32(o)))


def _hi(s, o, nin):
    i0 = min(_lo(s, o), nin - 1)
    return i0 + (i0 < nin - 1)


def regions_host(H, W, shapes, big, ty, tx, aligned=True):
    """What tile (ty, tx) of the fused kernel does, per level k: the region
    [ry0, ry1] x [rx0, rx1] it computes (and, for k < K-1, stages), the previous tile's
    region end (pey, pex; -1: none), the window it stores (sy0.., inclusive; empty when
    sy0 > ry1 or sx0 > rx1) and, for the finest level, whether the 16-byte stores run."""
    K = len(shapes)
    th, tw = (2 * TH, 2 * TW) if big else (TH, TW)
    r = [None] * K
    h, w = shapes[-1]
    r[-1] = dict(ry0=ty * th, ry1=min(ty * th + th - 1, h - 1), rx0=tx * tw,
                 rx1=min(tx * tw + tw - 1, w - 1), pey=ty * th - 1, pex=tx * tw - 1)
    for k in range(K - 2, -1, -1):
        n, (hin, win) = r[k + 1], shapes[k]
        sh, sw = step(hin, shapes[k + 1][0]), step(win, shapes[k + 1][1])
        r[k] = dict(ry0=_lo(sh, n['ry0']), ry1=_hi(sh, n['ry1'], hin),
                    rx0=_lo(sw, n['rx0']), rx1=_hi(sw, n['rx1'], win),
                    pey=-1 if n['pey'] < 0 else _hi(sh, n['pey'], hin),
                    pex=-1 if n['pex'] < 0 else _hi(sw, n['pex'], win))
    for k, q in enumerate(r):
        q['rh'], q['rw'] = q['ry1'] - q['ry0'] + 1, q['rx1'] - q['rx0'] + 1
        q['staged'] = k < K - 1
        q['vector'] = bool(k == K - 1 and q['rw'] % 4 == 0 and shapes[k][1] % 4 == 0 and aligned)
        if q['vector']:     # every pixel of the region is this tile's
            q['sy0'], q['sx0'] = q['ry0'], q['rx0']
        else:
            q['sy0'], q['sx0'] = max(q['ry0'], q['pey'] + 1), max(q['rx0'], q['pex'] + 1)
    return r


def chain_properties(H, W, shapes, big, aligned=True):
    """Walk every tile of a fused plan.  -> dict(counts: per level an int array [h,w] of how
    many tiles store each pixel; taps_ok: every tap of every region row and column lies in
    the previous level's region; largest: the largest staged region in floats; overlap: a
    tile whose coarse region starts at or before the previous tile's end; vector / scalar:
    tiles of the finest level on either store path)."""
    K = len(shapes)
    counts = [np.zeros(s, np.int64) for s in shapes]
    out = dict(counts=counts, taps_ok=True, largest=0, overlap=False, vector=0, scalar=0)
    ny, nx = tile_grid(shapes, big)
    for ty in range(ny):
        for tx in range(nx):
            r = regions_host(H, W, shapes, big, ty, tx, aligned)
            for k, q in enumerate(r):
                counts[k][q['sy0']:q['ry1'] + 1, q['sx0']:q['rx1'] + 1] += 1
                if q['staged']:
                    out['largest'] = max(out['largest'], q['rh'] * q['rw'])
                    if (q['pey'] >= q['ry0'] and ty) or (q['pex'] >= q['rx0'] and tx):
                        out['overlap'] = True
                if k:
                    p = r[k - 1]
                    y0, y1, _, _ = axis_host(shapes[k - 1][0], shapes[k][0])
                    x0, x1, _, _ = axis_host(shapes[k - 1][1], shapes[k][1])
                    ys, xs = slice(q['ry0'], q['ry1'] + 1), slice(q['rx0'], q['rx1'] + 1)
                    out['taps_ok'] &= bool(y0[ys].min() >= p['ry0'] and y1[ys].max() <= p['ry1'] and
                                           x0[xs].min() >= p['rx0'] and x1[xs].max() <= p['rx1'])
            out['vector' if r[-1]['vector'] else 'scalar'] += 1
    return out


# ---------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


SUBNORMALS = (F32(1e-45), F32(-3e-42), F32(1.1e-38))


def frames_host(kind, D, H, W):
    """'random': uniform 0..255; 'integer': integers 0..255; 'special': random, and in every
    frame one +inf in row 0, one NaN in column 0 below it (a tap of weight 0 then decides:
    0 * inf is NaN -- also for a kernel that reads one row past a frame, into the next one's
    row 0), one -0.0 and three subnormals elsewhere."""
    rng = _rng(kind, D, H, W)
    if kind == 'integer':
        return rng.integers(0, 256, (D, H, W)).astype(F32)
    a = (rng.random((D, H, W)) * 255).astype(F32)
    if kind == 'special':
        assert H >= 2 and W >= 2 and (H - 1) * (W - 1) >= 4
        for d in range(D):
            a[d, 0, rng.integers(0, W)] = F32('inf')
            a[d, rng.integers(1, H), 0] = F32('nan')
            pix = rng.choice((H - 1) * (W - 1), 4, replace=False)
            for p, v in zip(pix, (F32(-0.0),) + SUBNORMALS):
                a[d, 1 + p // (W - 1), 1 + p % (W - 1)] = v
    else:
        assert kind == 'random', kind
    return a


# ---------------------------------------------------------------------------
# cases: the smallest shapes that reach each mechanism
# ---------------------------------------------------------------------------
# dvsof_resize_bilinear_ac: (hin, win) -> (hout, wout), each with n in RESIZE_N
RESIZE_N = (1, 3)
RESIZE_CASES = (
    ((1, 1), (1, 1)), ((1, 1), (5, 7)), ((5, 7), (1, 1)), ((7, 9), (1, 70)), ((7, 9), (70, 1)),
    ((4, 64), (4, 64)),                                       # identity: the source's bytes
    ((3, 63), (3, 63)), ((3, 63), (4, 64)), ((3, 63), (5, 65)),   # block seams of the 64 x 4 grid
    ((9, 33), (17, 65)), ((17, 65), (9, 33)), ((260, 346), (33, 44)), ((2, 2), (33, 130)),
)


def _c(src, shapes, D=3, data='random', offset=0):
    return dict(src=src, shapes=tuple(shapes), D=D, data=data, offset=offset)


_FINE = {f'fine_{h}x{w}': _c((40, 50), ((8, 32), (h, w)))
         for h in (15, 16, 17) for w in (63, 64, 65)}
_K8 = ((9, 57), (10, 58), (11, 60), (12, 61), (14, 62), (15, 64), (16, 65), (18, 66))

# dvsof_loss_pyramid.  offset: floats by which the finest level's pointer is moved off its
# 16-byte alignment
PYRAMID_CASES = {
    'copy': _c((20, 40), ((20, 40),)),
    'to_1x1': _c((20, 40), ((1, 1),)),
    'all_1x1': _c((20, 40), ((1, 1), (1, 1), (1, 1))),
    'rows_1xW': _c((20, 40), ((1, 5), (1, 64), (1, 65))),
    'cols_Hx1': _c((20, 40), ((3, 1), (16, 1), (17, 1))),
    **_FINE,
    'growth': _c((40, 50), ((5, 7), (9, 12), (16, 64), (17, 65), (33, 130))),
    'far_up': _c((40, 50), ((2, 2), (33, 132))),
    'equal': _c((96, 80), ((12, 10), (12, 10), (48, 40))),
    'k8': _c((40, 50), _K8),
    # equal wide levels: a small tile stages 17 x 65 = 1 105 floats, more than two thirds of PYR_MAXR
    'wide_region': _c((40, 50), ((20, 70), (20, 70))),
    'small_511': _c((20, 40), ((9, 33), (17, 65)), D=511),
    'big_512': _c((20, 40), ((9, 33), (17, 65)), D=512),
    'big_ragged': _c((40, 50), ((17, 65), (33, 129)), D=228),
    # at D = 256 these two chains have 1 024 small tiles, below the threshold, and run on small
    # tiles; their D = 512 twins reach the big tiles and the refused fits(32, 128)
    'd256_aligned': _c((40, 50), ((16, 64), (32, 128)), D=256),
    'big_aligned': _c((40, 50), ((16, 64), (32, 128)), D=512),
    'd256_nofit': _c((40, 50), ((23, 90), (32, 128)), D=256),
    'nofit_2048': _c((40, 50), ((23, 90), (32, 128)), D=512),
    'unaligned': _c((40, 50), ((2, 2), (33, 132)), offset=1),
    'unaligned_big': _c((40, 50), ((16, 64), (32, 128)), D=512, offset=1),
    'shrink': _c((40, 50), ((32, 32), (16, 16))),
    'shrink_one_dim': _c((40, 50), ((16, 64), (17, 63))),
    'dyadic': _c((33, 65), ((17, 33), (33, 65), (33, 65)), data='integer'),
    'special_small': _c((10, 14), ((12, 20), (20, 70), (33, 132)), data='special'),
    'special_big': _c((8, 30), ((9, 33), (17, 65)), D=512, data='special'),
    'special_per_level': _c((12, 12), ((32, 32), (16, 16)), data='special'),
}

# dvsof_loss_fused_pyramid: the frames it leaves, and the loss through them
FUSED_SHAPES = ((5, 7), (9, 12), (17, 65), (33, 130))
FUSED_SRC = (40, 50)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, src, shapes, D, data, offset, images [D,H,W], levels: the restatement's
    K arrays, plan).  Computed once, shared, read-only."""
    c = dict(PYRAMID_CASES[name], name=name)
    H, W = c['src']
    c['images'] = frames_host(c['data'], c['D'], H, W)
    c['levels'] = pyramid_host(c['images'], c['shapes'])
    c['plan'] = plan_host(c['D'], H, W, c['shapes'])
    for a in [c['images']] + c['levels']:
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def resize_case(i, n):
    (hin, win), (hout, wout) = RESIZE_CASES[i]
    src = frames_host('random', n, hin, win)
    dst = resize_host(src, hout, wout)
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst


def same_bits(a, b):
    """NaNs by position, everything else by bits (so +0 and -0 differ)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != F32 or b.dtype != F32:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and
                np.array_equal(np.where(na, F32(0), a).view(np.uint32),
                               np.where(nb, F32(0), b).view(np.uint32)))


def first_difference(a, b):
    """A line for an assertion message: where two arrays first differ under same_bits."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return f'shapes {a.shape} {b.shape}'
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
    if not bad.any():
        return 'equal'
    i = tuple(int(v) for v in np.argwhere(bad)[0])
    return f'{int(bad.sum())} of {bad.size} differ, first at {i}: {a[i]!r} vs {b[i]!r}'
