"""Shared pieces of the evaluation tests (docs/EVAL_SPEC.md): the stand-in for
``cv2.remap(..., INTER_NEAREST)`` the golden tool hands to the reference, a
float64 restatement of the reference's two evaluation functions
(utils/eval.py), restated helpers of utils/data.py, and the seeded case
builders of tools/make_goldens_eval.py.  Pure numpy; nothing here touches the
package under test."""
import types

import numpy as np

INTER_NEAREST = 0
CAR_ROWS = 190


# ---------------------------------------------------------------------------
# cv2 stand-in: nearest-neighbour remap, our reading of OpenCV (float maps ->
# saturate_cast<short>(cvRound): ties to even, int16 saturation; constant
# border 0).  Not pinned by the reference: cv2 is not installed.
# ---------------------------------------------------------------------------
def nearest_index(c):
    """float coordinates -> (int64 index, in-int16-range-and-finite)."""
    r = np.rint(np.asarray(c, dtype=np.float64))
    ok = np.isfinite(r)
    r = np.clip(np.where(ok, r, -32768.0), -32768.0, 32767.0)
    return r.astype(np.int64), ok


def remap(src, map_x, map_y, interpolation, *args, **kwargs):
    assert interpolation == INTER_NEAREST and not args and not kwargs
    H, W = src.shape
    ix, okx = nearest_index(map_x)
    iy, oky = nearest_index(map_y)
    inside = okx & oky & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    out = np.zeros(map_x.shape, src.dtype)
    out[inside] = src[iy[inside], ix[inside]]
    return out


def cv2_standin():
    m = types.ModuleType('cv2')
    m.INTER_NEAREST = INTER_NEAREST
    m.remap = remap
    return m


# ---------------------------------------------------------------------------
# utils/data.py helpers, restated
# ---------------------------------------------------------------------------
class EventCrop:
    """events [n,4] -> those inside box = (y0, x0, h, w), shifted."""

    def __init__(self, box):
        self.box = box

    def __call__(self, events):
        y0, x0, h, w = self.box
        x, y = events[:, 0], events[:, 1]
        keep = (x >= x0) & (x < x0 + w) & (y >= y0) & (y < y0 + h)
        events = events[keep]
        events[:, 0] -= x0
        events[:, 1] -= y0
        return events


class ImageCrop:
    """[H,W,C] -> [h,w,C] window of box = (y0, x0, h, w)."""

    def __init__(self, box):
        self.box = box

    def __call__(self, img):
        y0, x0, h, w = self.box
        return img[y0:y0 + h, x0:x0 + w]


class Opaque:
    """The same callable without a ``.box``: evaluate cannot fold it."""

    def __init__(self, fun):
        self._fun = fun

    def __call__(self, a):
        return self._fun(a)


def get_count_image(events, imsize):
    """Events per pixel, uint64 [H,W]; coordinates outside the image raise."""
    cols = np.asarray(events[0]).astype(np.int64)
    rows = np.asarray(events[1]).astype(np.int64)
    if cols.size and (cols.min() < 0 or cols.max() >= imsize[1] or
                      rows.min() < 0 or rows.max() >= imsize[0]):
        raise ValueError('event outside the image')
    image = np.zeros(tuple(imsize), np.uint64)
    np.add.at(image, (rows, cols), 1)
    return image


def frame_generator(events, frames):
    """(columns of the events with start < t <= stop, start, stop) per frame."""
    t = np.asarray(events[2])
    for start, stop in np.asarray(frames).reshape(-1, 2):
        lo = int(np.searchsorted(t, start, side='right'))
        hi = int(np.searchsorted(t, stop, side='right'))
        yield [column[lo:hi] for column in events], start, stop


# ---------------------------------------------------------------------------
# float64 restatement of utils/eval.py
# ---------------------------------------------------------------------------
def plan64(ts, start, stop):
    """-> (direct?, [map index], [scale]) of utils/eval.py:118-172."""
    ts = np.asarray(ts, np.float64)
    k = int(np.searchsorted(ts, start, side='right')) - 1
    gt_dt, dt = ts[k + 1] - ts[k], np.float64(stop) - np.float64(start)
    if gt_dt > dt:
        return True, [k, k], [float(dt), float(gt_dt)]
    maps, scales = [k], [float((ts[k + 1] - start) / gt_dt)]
    k += 1
    while ts[k + 1] < stop:
        maps.append(k)
        scales.append(1.0)
        k += 1
    maps.append(k)
    scales.append(float((stop - ts[k]) / (ts[k + 1] - ts[k])))
    return False, maps, scales


def propagate64(x_maps, y_maps, ts, start, stop):
    """Ground-truth flow over [start, stop] on the full frame, every step
    computed in float64 and rounded to float32 once.  Propagated frames come
    back as float32, direct-scale frames as float64 (the reference's types)."""
    direct, maps, scales = plan64(ts, start, stop)
    if direct:
        k = maps[0]
        return (x_maps[k].astype(np.float64) * scales[0] / scales[1],
                y_maps[k].astype(np.float64) * scales[0] / scales[1])
    H, W = x_maps[0].shape
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32),
                         np.arange(H, dtype=np.float32))
    x, y = xs.copy(), ys.copy()
    keep_x = np.ones((H, W), bool)
    keep_y = np.ones((H, W), bool)
    with np.errstate(invalid='ignore', over='ignore'):
        for k, s in zip(maps, scales):
            fx = remap(x_maps[k], x, y, INTER_NEAREST).astype(np.float64)
            fy = remap(y_maps[k], x, y, INTER_NEAREST).astype(np.float64)
            keep_x &= fx != 0
            keep_y &= fy != 0
            x = (x.astype(np.float64) + fx * s).astype(np.float32)
            y = (y.astype(np.float64) + fy * s).astype(np.float32)
        u = np.where(keep_x, x - xs, np.float32(0))
        v = np.where(keep_y, y - ys, np.float32(0))
    return u, v


def error_mask(gt, count, is_car, is_dense):
    """Pixels flow_error_dense counts (gt as float32, the kernel's input)."""
    h, w = gt.shape[:2]
    g = gt.astype(np.float32)
    rows = np.arange(h)[:, None] < (min(CAR_ROWS, h) if is_car else h)
    with np.errstate(invalid='ignore', over='ignore'):
        norm = np.sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1])
    valid = ~np.isinf(g[..., 0]) & ~np.isinf(g[..., 1]) & (norm > 0)
    events = np.ones((h, w), bool) if is_dense else np.squeeze(count) > 0
    return rows & valid & events


def endpoint_error64(gt, pred):
    d = gt.astype(np.float32).astype(np.float64) - pred.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)


def flow_error64(gt, pred, count, is_car=False, is_dense=False):
    """-> (AEE, percent_AEE, n_points) with EE and its mean in float64."""
    m = error_mask(gt, count, is_car, is_dense)
    ee = endpoint_error64(gt, pred)[m]
    n = int(ee.size)
    aee = float(ee.sum() / n) if n else float('nan')
    return aee, float((ee < 3.0).sum()) / float(n + 1e-5), n


# ---------------------------------------------------------------------------
# comparison: finite entries bitwise equal, non-finite ones of the same class
# ---------------------------------------------------------------------------
def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    fin = np.isfinite(want)
    if not np.array_equal(fin, np.isfinite(got)):
        return False
    if not np.array_equal(got[fin].view(np.uint8), want[fin].view(np.uint8)):
        return False
    g, w = got[~fin], want[~fin]
    return bool(np.array_equal(np.isnan(g), np.isnan(w)) and
                np.array_equal(np.signbit(g) & ~np.isnan(g),
                               np.signbit(w) & ~np.isnan(w)))


# ---------------------------------------------------------------------------
# seeded cases (tools/make_goldens_eval.py writes them next to what the
# reference makes of them; the tests read the golden file)
# ---------------------------------------------------------------------------
SHAPES = ((12, 20), (37, 70))
CAR_SHAPE = (260, 346)
WINDOWS = {(12, 20): (3, 5, 9, 15), (37, 70): (5, 11, 32, 59)}   # odd corner, to the bottom right edge
K_MAPS = 6
# dyadic timestamps: every scale factor is exact
GT_TS = 10.0 + 0.25 * np.arange(K_MAPS + 1)
PROP_FRAMES = (
    ('direct', 10.3125, 10.375),            # inside one gap
    ('start_on_ts', 10.25, 10.625),         # first step at scale 1
    ('end_on_ts', 11.125, 11.5),            # last step at scale 1
    ('one_gap', 10.3125, 10.5625),          # dt == gt_dt: propagates, crosses one timestamp
    ('three_gaps', 10.125, 10.9375),        # two middle steps at scale 1
)


def prop_key(shape, dtype):
    return f'prop_{shape[0]}x{shape[1]}_{np.dtype(dtype).name}'


def make_maps(shape, dtype, seed):
    """K_MAPS displacement maps per axis: smooth-ish flows of a few pixels,
    ~10 % exact zeros, one inf, outward flows along every edge (pixels leave
    the image on each side) and patches of exactly 0.5 / 1.5 (both halves of
    round-half-to-even, on odd and even coordinates, after a scale-1 step)."""
    H, W = shape
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3, 3, (K_MAPS, H, W))
    y = rng.uniform(-3, 3, (K_MAPS, H, W))
    x[:, :, :2] = -5.25
    x[:, :, -2:] = 5.25
    y[:, :2, :] = -5.25
    y[:, -2:, :] = 5.25
    x[:, 2:6, 2:8], y[:, 2:6, 2:8] = 0.5, 1.5
    x[:, 6:10, 8:14], y[:, 6:10, 8:14] = 1.5, 0.5
    x[rng.random(x.shape) < 0.1] = 0.0
    y[rng.random(y.shape) < 0.1] = 0.0
    x[1, H // 2, W // 2] = np.inf
    y[3, H // 2 - 1, W // 2 + 1] = -np.inf
    return x.astype(dtype), y.astype(dtype)


def make_error_case(shape, seed, empty=False):
    """gt, pred [h,w,2] float32 and count [h,w] uint64: about half the pixels
    without events, gt with inf and zero vectors, predictions moved so that
    no float64 EE lies within 1e-3 of the 3 px threshold.  Values sit on a
    1/64 (gt) and 1/256 (pred) grid so that the fixture compresses."""
    h, w = shape
    rng = np.random.default_rng(seed)
    gt = np.round(rng.normal(0, 4, (h, w, 2)) * 64) / 64
    gt[rng.random((h, w)) < 0.05] = 0.0
    gt[rng.random((h, w)) < 0.02, 0] = np.inf
    gt[rng.random((h, w)) < 0.02, 1] = -np.inf
    gt = gt.astype(np.float32)
    pred = np.where(np.isfinite(gt), gt, 0) + rng.normal(0, 1.6, (h, w, 2))
    pred = (np.round(pred * 256) / 256).astype(np.float32)
    for _ in range(100):
        ee = endpoint_error64(gt, pred)
        near = np.isfinite(ee) & (np.abs(ee - 3.0) < 2e-3)
        if not near.any():
            break
        pred[near, 0] += np.float32(1 / 64)
    count = rng.integers(0, 4, (h, w)) * (rng.random((h, w)) < 0.5)
    if empty:
        count[:] = 0
    return gt, pred, count.astype(np.uint64)


ERROR_VARIANTS = (('plain', False, False), ('car', True, False),
                  ('dense', False, True), ('car_dense', True, True))
ERROR_CASES = (('12x20', (12, 20), 11, False), ('37x70', (37, 70), 12, False),
               ('260x346', CAR_SHAPE, 13, False), ('empty', (37, 70), 14, True))

EVAL_SHAPE = (37, 70)
EVAL_BOX = (2, 3, 32, 64)       # central 32 x 64: ((37-32)//2, (70-64)//2)
EVAL_FRAMES = ((10.03125, 10.28125), (10.28125, 10.34375), (10.34375, 10.625),
               (10.625, 10.9375), (10.9375, 11.0), (11.0, 11.1875),
               (11.1875, 11.46875))


def make_eval_case(seed=21, per_frame=700):
    """A 7-frame sequence on 37 x 70 maps (float64, like MVSEC) with a central
    32 x 64 crop: events [x, y, t, p] as float64 columns sorted by t, and the
    flows [7,32,64,2] a fake network answers with."""
    rng = np.random.default_rng(seed)
    H, W = EVAL_SHAPE
    xm, ym = make_maps(EVAL_SHAPE, np.float64, seed)
    n = per_frame * len(EVAL_FRAMES)
    t = np.sort(rng.uniform(EVAL_FRAMES[0][0] - 0.01, EVAL_FRAMES[-1][1] + 0.01, n))
    events = [rng.integers(0, W, n).astype(np.float64),
              rng.integers(0, H, n).astype(np.float64), t,
              rng.choice([-1.0, 1.0], n)]
    flows = (np.round(rng.normal(0, 2.5, (len(EVAL_FRAMES),) + EVAL_BOX[2:] + (2,))
                      * 256) / 256).astype(np.float32)
    crop = ImageCrop(EVAL_BOX)
    for i, (a, b) in enumerate(EVAL_FRAMES):    # keep every EE away from 3 px
        gt = crop(np.dstack(propagate64(xm, ym, GT_TS, a, b)))
        for _ in range(100):
            ee = endpoint_error64(gt, flows[i])
            near = np.isfinite(ee) & (np.abs(ee - 3.0) < 2e-3)
            if not near.any():
                break
            flows[i][near, 0] += np.float32(1 / 64)
    return dict(x_maps=xm, y_maps=ym, ts=GT_TS.copy(), events=np.stack(events),
                frames=np.array(EVAL_FRAMES), flows=flows)


class FakeFlow:
    """An ``of`` with the reference contract that answers with prescribed
    flows, looked up by the window's start time: numpy [B,H,W,2]."""

    def __init__(self, frames, flows):
        self._index = {float(f[0]): i for i, f in enumerate(frames)}
        self._flows = flows
        self.batches = []

    def __call__(self, events, start, stop):
        assert len(events) == len(start) == len(stop)
        self.batches.append(len(start))
        return np.stack([self._flows[self._index[float(s)]] for s in start])
