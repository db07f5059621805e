"""Cases and the independent restatement of docs/AUGMENT_SPEC.md (flip, LUT
rotation, crop; csrc/augment.hip).  No GPU and no torch at import.

The restatement is the spec written as plain per-pixel loops on Python floats
and ints: Python's float is IEEE float64, ``a * b`` and ``a + b`` are one
correctly rounded operation each and never contracted, ``round`` rounds ties to
even.  It shares no code with oracle/cpu_oracle.py, so the two can be held
against each other (tests/test_augment_oracle.py) before the kernels are held
against this one (tests/test_gpu_augment_exact.py).

``VARIANTS`` names deliberately wrong readings of the spec.  The oracle test
proves that the case table tells each of them from the spec, i.e. that a
kernel with that mistake could not pass the GPU test.
"""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

# ---------------------------------------------------------------------------
# The case table (AUGMENT_SPEC section 8): the smallest set at which the kernels can
# still go wrong.  Odd x even frames have rounding ties at 90 degrees; 9x9,
# 7x9 and 17x31 have pixels where a fused product changes the result at +-45.
# ---------------------------------------------------------------------------
FRAMES = [(1, 1), (1, 7), (7, 1), (5, 8), (8, 5), (9, 9), (7, 9), (16, 16), (17, 31), (33, 20)]
ANGLES = [0, 90, -90, 180, 270, 360, 45, -45, 30, 0.001, -29.9, 12.5, 37.5, -20.25, 3.0]
FLIPS = [False, True]
LARGE_FRAME = (260, 346)                        # the geometry of tests/test_gpu_augment.py
LARGE_ANGLES = [0, 90, -90, 180, 37.5, -20.25, 3.0, 12.5, -29.9]


def boxes(H, W):
    """name -> (y0, x0, h, w): the whole frame, one pixel, the four corners
    (one shape, so that they fit one batch) and an interior box.  On frames too
    thin for one, the interior box keeps the whole of that axis."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    iy, ih = (1, H - 2) if H >= 3 else (0, H)
    ix, iw = (1, W - 2) if W >= 3 else (0, W)
    return {'full': (0, 0, H, W), 'one': (H // 2, W // 2, 1, 1),
            'top_left': (0, 0, ch, cw), 'top_right': (0, W - cw, ch, cw),
            'bottom_left': (H - ch, 0, ch, cw), 'bottom_right': (H - ch, W - cw, ch, cw),
            'interior': (iy, ix, ih, iw)}


def box_groups(H, W):
    """The boxes of a frame grouped by their (h, w): a batch has one crop shape."""
    groups = {}
    for name, b in boxes(H, W).items():
        groups.setdefault(b[2:], []).append((name, b))
    return list(groups.values())


def samples(H, W, group):
    """Every (angle, flip, box) of one box group as the samples of one batch:
    -> list of dicts with 'angle', 'flip', 'box', 'name'."""
    return [dict(angle=a, flip=f, box=b, name=f'{H}x{W}/{a}/{"flip" if f else "noflip"}/{n}')
            for a in ANGLES for f in FLIPS for n, b in group]


def cos_sin(angle):
    """(cos, sin) of an angle in degrees as the host computes them
    (augment.augment_batch): numpy float64 of angle * pi / 180."""
    rad = np.float64(angle) * np.pi / 180
    return float(np.cos(rad)), float(np.sin(rad))


def u8_frame(d, H, W):
    """uint8 test frame d: over 256 or more pixels it holds all 256 values, and
    no two neighbours are equal (101 is odd, so p -> 101 p + 7 d is a bijection mod 256)."""
    return [[(101 * (r * W + col) + 7 * d) % 256 for col in range(W)] for r in range(H)]


# float32 bit patterns a copy must keep: +-0, denormals, +-Inf, quiet and
# signalling NaNs with payloads, the extremes.  Held as int32.
F32_SPECIAL = [0x00000000, -0x80000000, 0x00000001, 0x007FFFFF, -0x7FFFFFFF, 0x7F800000,
               -0x00800000, 0x7FC00000, 0x7FC12345, -0x00345678, 0x7F800001, 0x7FA5A5A5,
               -0x005A5A5B, 0x7F7FFFFF, -0x00800001, 0x00800000, 0x3F800000, -0x40800000]


def f32_bits_frame(d, H, W):
    """float32 test frame d as int32 bit patterns: the special values in turn,
    between them ordinary numbers that differ from pixel to pixel."""
    out = []
    for r in range(H):
        row = []
        for col in range(W):
            p = r * W + col + 5 * d
            row.append(F32_SPECIAL[(p // 2) % len(F32_SPECIAL)] if p % 2 == 0
                       else 0x3F800000 + 4099 * p)
        out.append(row)
    return out


def edge_events(H, W, B):
    """(x, y, sample) triples that must all be dropped (AUGMENT_SPEC section 5): each
    coordinate and the sample index outside its range, among them int64 values
    whose low 32 bits are a valid coordinate."""
    bad = [-1, W, H, 2 ** 31, 2 ** 32, 2 ** 32 + 1, -2 ** 32]
    ev = []
    for v in bad:
        if not 0 <= v < W:
            ev.append((v, 0, 0))
        if not 0 <= v < H:
            ev.append((0, v, 0))
    ev += [(0, 0, s) for s in (-1, B, 2 ** 32)]
    return ev


# ---------------------------------------------------------------------------
# The restatement
# ---------------------------------------------------------------------------
VARIANTS = ('half_away', 'fma_first', 'fma_second', 'lut_largest', 'rotate_before_flip',
            'flip_rotated_column', 'truncate_int32')
# half_away            rint replaced by round-half-away-from-zero
# fma_first            (fma(c, x, (-s)*y)) + W/2, and fma(s, x, c*y) + H/2
# fma_second           (fma(-s, y, c*x)) + W/2, and fma(c, y, s*x) + H/2
# lut_largest          the largest rotated index wins a source pixel in the LUT
# rotate_before_flip   rotation, then flip, then crop -- frames and events alike
# flip_rotated_column  frames only: the flip mirrors the rotated pixel's column
#                      instead of the source pixel's; events follow the spec
# truncate_int32       events: x, y and sample cut to their low 32 bits (as
#                      a signed int) before the range check


def _fma(a, b, c):
    """fma(a, b, c) in float64, exactly: the rational a*b + c rounded once
    (int / int division is correctly rounded, ties to even)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _sum2(a, p, b, q, variant):
    """a*p + b*q under the spec (two products, one sum) or a contraction."""
    if variant == 'fma_first':
        return _fma(a, p, b * q)
    if variant == 'fma_second':
        return _fma(b, q, a * p)
    return a * p + b * q


def _rint(v, variant):
    r = round(v)                        # ties to even, an exact int
    if variant == 'half_away' and abs(v - math.trunc(v)) == 0.5:
        r = math.trunc(v) + (1 if v > 0 else -1)    # (the difference is exact below 2^52)
    return r


def unrounded(c, s, H, W, oy, ox, variant=None):
    """-> (fx, fy): AUGMENT_SPEC section 2 before the rounding."""
    x, y = ox - W / 2, oy - H / 2
    return _sum2(c, x, -s, y, variant) + W / 2, _sum2(s, x, c, y, variant) + H / 2


def source_pixel(c, s, H, W, oy, ox, variant=None):
    """-> (sy, sx) the source pixel of rotated pixel (oy, ox), or None."""
    fx, fy = unrounded(c, s, H, W, oy, ox, variant)
    sx, sy = _rint(fx, variant), _rint(fy, variant)
    return (sy, sx) if 0 <= sx < W and 0 <= sy < H else None


@lru_cache(maxsize=None)
def sources(c, s, H, W, variant=None):
    """-> tuple over the rotated index o = oy*W + ox of source_pixel."""
    v = variant if variant in ('half_away', 'fma_first', 'fma_second') else None
    return tuple(source_pixel(c, s, H, W, oy, ox, v) for oy in range(H) for ox in range(W))


@lru_cache(maxsize=None)
def lut(c, s, H, W, variant=None):
    """-> tuple over the source index of the rotated index that an event there
    moves to; H*W where no rotated pixel reads it (AUGMENT_SPEC section 4)."""
    empty = H * W
    table = [empty] * (H * W)
    for o, src in enumerate(sources(c, s, H, W, variant)):
        if src is None:
            continue
        k = src[0] * W + src[1]
        if table[k] == empty or variant == 'lut_largest':
            table[k] = o
    return tuple(table)


def readers(c, s, H, W):
    """-> list over the source index of how many rotated pixels read it."""
    n = [0] * (H * W)
    for src in sources(c, s, H, W):
        if src is not None:
            n[src[0] * W + src[1]] += 1
    return n


def frames(src, frame_sample, flip, cs, box, h, w, variant=None):
    """src: D frames as nested lists [H][W] of numbers (or of bit patterns:
    a pixel is copied or 0); frame_sample[d], flip[b], cs[b] = (c, s),
    box[b] = (y0, x0, ., .).  -> D nested lists [h][w] (AUGMENT_SPEC section 3)."""
    out = []
    for d, img in enumerate(src):
        H, W = len(img), len(img[0])
        b = frame_sample[d]
        table = sources(cs[b][0], cs[b][1], H, W, variant)
        y0, x0 = box[b][0], box[b][1]
        res = []
        for y in range(h):
            row = []
            for x in range(w):
                oy, ox = y + y0, x + x0
                v = 0
                if 0 <= oy < H and 0 <= ox < W:
                    if flip[b] and variant in ('rotate_before_flip', 'flip_rotated_column'):
                        ox = W - 1 - ox
                    p = table[oy * W + ox]
                    if p is not None:
                        sy, sx = p
                        if flip[b] and variant not in ('rotate_before_flip', 'flip_rotated_column'):
                            sx = W - 1 - sx
                        v = img[sy][sx]
                row.append(v)
            res.append(row)
        out.append(res)
    return out


def _low32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def events(xs, ys, ss, flip, cs, box, B, H, W, variant=None, use_lut=True):
    """-> (new x, new y) lists; a dropped event has -1 in both (AUGMENT_SPEC section 5).
    use_lut False is the lut == NULL path: the rotation is the identity."""
    nx, ny = [], []
    for x, y, b in zip(xs, ys, ss):
        if variant == 'truncate_int32':
            x, y, b = _low32(x), _low32(y), _low32(b)
        px = py = -1
        if 0 <= b < B and 0 <= x < W and 0 <= y < H:
            y0, x0, bh, bw = box[b]
            if flip[b] and variant != 'rotate_before_flip':
                x = W - 1 - x
            o = lut(cs[b][0], cs[b][1], H, W, variant)[y * W + x] if use_lut else y * W + x
            if o < H * W:
                oy, ox = divmod(o, W)
                if flip[b] and variant == 'rotate_before_flip':
                    ox = W - 1 - ox
                if x0 <= ox < x0 + bw and y0 <= oy < y0 + bh:
                    px, py = ox - x0, oy - y0
        nx.append(px)
        ny.append(py)
    return nx, ny


def pixel_events(B, H, W):
    """One event on every pixel of every sample: -> x, y, sample lists."""
    xs, ys, ss = [], [], []
    for b in range(B):
        for y in range(H):
            for x in range(W):
                xs.append(x)
                ys.append(y)
                ss.append(b)
    return xs, ys, ss


# ---------------------------------------------------------------------------
# The reference's form of section 2: a 2x2 matrix times the 2xN coordinates (np.dot).
# Which products a BLAS fuses is its own business (AUGMENT_SPEC section 7).
# ---------------------------------------------------------------------------
def matrix_product_sources(angle, H, W):
    """-> (x1, y1 int64[H*W], fx, fy float64[H*W] unrounded) of the np.dot form."""
    x, y = np.meshgrid(range(W), range(H))
    x, y = x.ravel().astype(float) - W / 2, y.ravel().astype(float) - H / 2
    c, s = cos_sin(angle)
    m = np.array([[c, -s], [s, c]]).dot(np.vstack((x[None], y[None])))
    fx, fy = m[0] + W / 2, m[1] + H / 2
    return np.rint(fx).astype(np.int64), np.rint(fy).astype(np.int64), fx, fy


def ulps_from_half(v):
    """Distance of v from the nearest k + 0.5 in units of v's ulp."""
    half = math.floor(v) + 0.5
    return abs(v - half) / math.ulp(max(abs(v), abs(half)))
