"""Shared pieces of the evaluation-panel tests (docs/EVAL_PANELS_SPEC.md): the
seeded cases, the strided destination and the byte mask of its pictures.
Pure numpy; nothing here touches the package under test."""
import numpy as np

from . import render_cases as rc

F32 = np.float32
JUNK = 0xCD
# (1,1); w = 5: the four panels start at byte offsets 0, 3, 2, 1 mod 4; (130,33): three chunks;
# (70,2100): chunk rows decided by the 64-chunk cap
SHAPES = [(1, 1), (3, 5), (7, 5), (33, 67), (130, 33), (70, 2100)]
BATCHES = [1, 3]
# per shape a seed for which the float64 hue oracle alone leaves at most UNDECIDED_CAP of the
# flow-panel pixels of the three-frame case undecided (test_eval_panels_oracle checks it)
SEEDS = {(1, 1): 1, (3, 5): 1, (7, 5): 1, (33, 67): 1, (130, 33): 1, (70, 2100): 1}


def case(n, shape, seed=None):
    """-> dict(pred [n,2,h,w], gt_u, gt_v [n,h,w] float32, count2 int32
    [n,2,h,w] (uint32 counts), frames uint8 [n,h,w]).  The prediction is the
    ground truth plus an error around the 3 px threshold; ~5 % zero ground
    truth, ~3 % +inf / -inf components each, one NaN prediction pixel per
    frame (images of more than four pixels), about half the pixels without an
    event, a few saturated counts."""
    h, w = shape
    rng = np.random.default_rng(SEEDS[tuple(shape)] if seed is None else seed)
    gt = (rng.standard_normal((n, 2, h, w)) * 3).astype(F32)
    pred = (gt + rng.normal(0, 2.2, gt.shape)).astype(F32)
    if h * w > 4:
        gt[:, :, rng.random((h, w)) < 0.05] = 0.0
        gt[:, 0][rng.random((n, h, w)) < 0.03] = np.inf
        gt[:, 1][rng.random((n, h, w)) < 0.03] = -np.inf
        for i in range(n):
            pred[i, i % 2, (3 * i + 1) % h, (5 * i + 2) % w] = np.nan
    count2 = rng.integers(0, 3, (n, 2, h, w)) * (rng.random((n, 1, h, w)) < 0.5)
    count2[rng.random(count2.shape) < 0.02] = 300
    frames = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
    return dict(pred=pred, gt_u=np.ascontiguousarray(gt[:, 0]), gt_v=np.ascontiguousarray(gt[:, 1]),
                count2=count2.astype(np.int32), frames=frames)


def undecided_share(c, stats_of):
    """Share of the flow-panel pixels of a case whose hue the float64 oracle
    leaves undecided at the scale the panels are drawn with.  stats_of(f) ->
    max_magnitude of frame f."""
    total = undecided = 0
    for f in range(len(c['pred'])):
        m = stats_of(f)
        for fx, fy in ((c['pred'][f, 0], c['pred'][f, 1]), (c['gt_u'][f], c['gt_v'][f])):
            blank = np.zeros(fx.shape + (3,), np.uint8)
            undecided += int(rc.judge(blank, fx, fy, m)[1].sum())
            total += fx.size
    return undecided / total


def strides(shape, n, pad=0, gap=0):
    """-> (frame_stride, row_stride, total bytes) of n pictures of h x 4w
    pixels with ``pad`` spare bytes per row, ``gap`` between pictures and 64
    after the last."""
    h, w = shape
    row = 12 * w + pad
    frame = h * row + gap
    return frame, row, (n - 1) * frame + h * row + 64


def picture_bytes(shape, n, frame_stride, row_stride, total):
    """bool [total]: the bytes that belong to a picture."""
    h, w = shape
    mask = np.zeros(total, bool)
    for f in range(n):
        for r in range(h):
            at = f * frame_stride + r * row_stride
            mask[at:at + 12 * w] = True
    return mask
