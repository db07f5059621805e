"""Shared pieces of the rendering tests (docs/RENDER_SPEC.md): a float32
restatement of flow2img (utils/visualization.py:5-18, cv2 by our reading of
OpenCV) written operation by operation, the float64 hue with its decided /
undecided rule, the exact HSV -> BGR table, the seeded cases and the mosaic
literal.  Pure numpy; nothing here touches the package under test."""
import functools

import numpy as np

F = np.float32
SHAPES = [(1, 1), (3, 5), (7, 5), (16, 16), (33, 67), (130, 173)]
BATCHES = [1, 3]
SCALES = [0.01, 3.0, 1e4]           # image i of a case is drawn at SCALES[i % 3]
PYRAMID = [(6, 10), (12, 20), (24, 40), (48, 80)]      # coarse -> fine
HUE_MARGIN = 1e-3       # |a - integer| below this: the hue is undecided (section 4 of the spec)
UNDECIDED_CAP = 0.01    # share of a case


# ---------------------------------------------------------------------------
# float32, one rounding per operation
# ---------------------------------------------------------------------------
def magnitude32(fx, fy):
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    with np.errstate(all='ignore'):
        xx = np.multiply(fx, fx, dtype=F)
        yy = np.multiply(fy, fy, dtype=F)
        return np.sqrt(np.add(xx, yy, dtype=F), dtype=F)


def stats32(fx, fy):
    """-> (lo, hi, nonfinite) over the pixels whose two components are finite;
    (+inf, -inf, n) when there is none."""
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    finite = np.isfinite(fx) & np.isfinite(fy)
    mag = magnitude32(fx, fy)[finite]
    bad = int((~finite).sum())
    if mag.size == 0:
        return F(np.inf), F(-np.inf), bad
    return F(mag.min()), F(mag.max()), bad


def value32(fx, fy, max_magnitude=0.0):
    """The V plane (uint8), 0 where a component is not finite."""
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    finite = np.isfinite(fx) & np.isfinite(fy)
    mag = magnitude32(fx, fy)
    lo, hi, _ = stats32(fx, fy)
    m = F(max_magnitude)
    if m > 0:
        lo, hi, mag = F(0), m, np.fmin(mag, m)
    with np.errstate(all='ignore'):
        span = np.subtract(hi, lo, dtype=F)
        scale = np.divide(F(255), span, dtype=F) if span > 0 else F(0)
        x = np.multiply(np.subtract(mag, lo, dtype=F), scale, dtype=F)
        v = np.trunc(np.fmin(x, F(255)))
    out = np.zeros(fx.shape, np.uint8)
    out[finite] = v[finite].astype(np.uint8)
    return out


def hue32(fx, fy):
    """numpy's own float32 arctan2 path (not what the device is held to)."""
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    with np.errstate(all='ignore'):
        a = np.multiply(np.add(np.arctan2(fy, fx, dtype=F), F(np.pi), dtype=F),
                        F(180.0 / np.pi / 2.0), dtype=F)
    finite = np.isfinite(fx) & np.isfinite(fy)
    return np.where(finite, np.trunc(a), 0).astype(np.int64)


@functools.lru_cache(maxsize=None)
def bgr_table():
    """uint8 [181,256,3]: BGR of (hue, V) at S = 255 by OpenCV's float formula,
    float32 scalars, channel = rint(x * 255) with ties to even."""
    order = [(1, 3, 0), (1, 0, 2), (3, 0, 1), (0, 2, 1), (0, 1, 3), (2, 1, 0)]
    out = np.zeros((181, 256, 3), np.uint8)
    for h in range(181):
        f = F(h % 30) / F(30)
        for V in range(256):
            v = F(V) / F(255)
            tab = (v, F(0), F(v * F(F(1) - f)), F(v * f))
            out[h, V] = [int(np.rint(F(tab[k] * F(255)))) for k in order[(h // 30) % 6]]
    return out


def flow2img32(fx, fy, max_magnitude=0.0):
    """The float32 restatement of the whole function."""
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    image = bgr_table()[hue32(fx, fy), value32(fx, fy, max_magnitude)]
    image[~(np.isfinite(fx) & np.isfinite(fy))] = 0
    return image


# ---------------------------------------------------------------------------
# the float64 hue and the decided / undecided rule
# ---------------------------------------------------------------------------
def hue64(fx, fy):
    fx, fy = np.asarray(fx, F).astype(np.float64), np.asarray(fy, F).astype(np.float64)
    with np.errstate(all='ignore'):
        return (np.arctan2(fy, fx) + np.pi) * (180.0 / np.pi / 2.0)


def judge(got, fx, fy, max_magnitude=0.0):
    """got uint8 [H,W,3] against the oracle -> (wrong bool [H,W], undecided
    bool [H,W]).  A decided pixel must equal the oracle's BGR; an undecided
    one (its float64 hue within HUE_MARGIN of an integer, V > 0) the BGR of
    one of the two hues that meet at that integer."""
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    finite = np.isfinite(fx) & np.isfinite(fy)
    V = value32(fx, fy, max_magnitude)
    a = np.where(finite, hue64(fx, fy), 0.5)
    k = np.rint(a)
    undecided = (np.abs(a - k) <= HUE_MARGIN) & finite & (V > 0)
    table = bgr_table()
    clip = lambda h: np.clip(h, 0, 180).astype(np.int64)       # noqa: E731
    same = lambda h: (got == table[clip(h), V]).all(-1)        # noqa: E731
    ok = np.where(undecided, same(k - 1) | same(k), same(np.floor(a)))
    ok = np.where(finite, ok, (got == 0).all(-1))
    return ~ok, undecided


def value_of(image):
    """The V plane back out of a BGR image: one channel is always rint(v * 255) = V."""
    return np.asarray(image).max(-1)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def flows(n, shape, seed=11):
    """float32 [n,2,h,w]; image i at SCALES[i % 3], so a scale leaking from
    one image to the next moves V by orders of magnitude."""
    rng = np.random.default_rng(seed)
    out = rng.standard_normal((n, 2) + tuple(shape)).astype(F)
    for i in range(n):
        out[i] *= F(SCALES[i % len(SCALES)])
    return out


def wheel(maximum=7.0):
    """float32 [2,180,256]: row k at angle -pi + (k + 0.5) * 2 degrees (hue k,
    half a unit from both integers), column j at magnitude j / 255 * maximum."""
    theta = -np.pi + (np.arange(180) + 0.5) * np.deg2rad(2.0)
    mag = np.arange(256) / 255.0 * maximum
    return np.stack([np.outer(np.cos(theta), mag), np.outer(np.sin(theta), mag)]).astype(F)


def pyramid(n=2, seed=5):
    """The levels [n,2,h,w] of PYRAMID, coarse -> fine."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((n, 2) + s) * (k + 1)).astype(F) for k, s in enumerate(PYRAMID)]


def pyramid_literal(images):
    """images: the four rendered levels [h,w,3] of ONE sample, coarse -> fine
    (PYRAMID) -> the 72x80 mosaic, by slicing."""
    out = np.zeros((48 + 24, 80, 3), np.uint8)
    out[0:48, 0:80] = images[3]
    out[48:72, 0:40] = images[2]
    out[48:60, 40:60] = images[1]
    out[48:54, 60:70] = images[0]
    return out
