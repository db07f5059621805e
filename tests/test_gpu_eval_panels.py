"""Evaluation panels and the polarity count on the device (csrc/eval_panels.hip,
csrc/eval.hip) against visualization.eval_panels_numpy and numpy; arithmetic
in docs/EVAL_PANELS_SPEC.md.  Events panel, error panel and statistics are
bitwise; the flow panels are byte-identical to the flow renderer and held to
the float64 hue oracle of tests/render_cases.py."""
import functools

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import eval as dev_eval, visualization as vis
from tests import eval_panel_cases as pc
from tests import render_cases as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def reference(n, shape, **kw):
    """The case and what the numpy restatement makes of it (computed once)."""
    c = pc.case(n, shape)
    image, stats = vis.eval_panels_numpy(c['pred'], c['gt_u'], c['gt_v'], c['count2'], c['frames'],
                                         return_stats=True, **dict(kw))
    return c, image, stats


def destination(n, shape, pad, gap):
    frame, row, total = pc.strides(shape, n, pad, gap)
    flat = torch.full((total,), pc.JUNK, dtype=torch.uint8, device=DEV)
    view = torch.as_strided(flat, (n, shape[0], 4 * shape[1], 3), (frame, row, 3, 1))
    return flat, view, pc.picture_bytes(shape, n, frame, row, total)


def check_flow_panels(got, c, stats, w):
    """Byte-identical to the flow renderer at the frame's scale, and held to the oracle."""
    undecided = 0
    for f in range(len(got)):
        m = float(vis.panel_scale(stats[f]))
        planes = [c['pred'][f], np.stack([c['gt_u'][f], c['gt_v'][f]])]
        drawn = vis.render_flows(dev(np.stack(planes)), max_magnitude=m).cpu().numpy()
        for k, flow in enumerate(planes):
            panel = got[f, :, (k + 1) * w:(k + 2) * w]
            assert np.array_equal(panel, drawn[k]), (f, k)
            assert np.array_equal(rc.value_of(panel), rc.value32(flow[0], flow[1], m))
            wrong, und = rc.judge(panel, flow[0], flow[1], m)
            assert not wrong.any(), (f, k, np.argwhere(wrong)[:5])
            undecided += int(und.sum())
    return undecided


@pytest.mark.parametrize('pad, gap', [(0, 0), (5, 37)], ids=['tight', 'padded'])
@pytest.mark.parametrize('n', pc.BATCHES)
@pytest.mark.parametrize('shape', pc.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_panels_against_the_restatement(shape, n, pad, gap):
    c, want, want_stats = reference(n, shape)
    h, w = shape
    flat, view, mine = destination(n, shape, pad, gap)
    image, stats = vis.eval_panels(dev(c['pred']), dev(c['gt_u']), dev(c['gt_v']), dev(c['count2']),
                                   dev(c['frames']), out=view, return_stats=True)
    assert image is view
    got, stats, flat = image.cpu().numpy(), vis.read_panel_stats(stats), flat.cpu().numpy()
    assert (flat[~mine] == pc.JUNK).all()                   # row padding, the gap, what follows
    assert stats.tobytes() == want_stats.tobytes()
    assert np.array_equal(got[:, :, :w], want[:, :, :w])                    # events
    assert np.array_equal(got[:, :, 3 * w:], want[:, :, 3 * w:])            # endpoint error
    undecided = check_flow_panels(got, c, stats, w)
    print(f'undecided {undecided} of {n * 2 * h * w}')
    assert undecided <= rc.UNDECIDED_CAP * n * 2 * h * w
    if h * w > 1000:        # the case holds what it claims
        assert (stats['pred_nonfinite'] == 1).all() and (stats['n_below'] > 0).all()
        assert (stats['n_below'] < stats['n_counted']).all()


@pytest.mark.parametrize('kw', [dict(max_row=20), dict(count2=None), dict(frames=None),
                                dict(count2=None, frames=None, max_row=0),
                                dict(flow_scale=2.5, err_max=1.5, gain=3)],
                         ids=['max_row', 'dense', 'no_frames', 'bare', 'scales'])
def test_optional_inputs_and_scales(kw):
    c = pc.case(3, (33, 67))
    a = dict(c, max_row=None, flow_scale=0.0, err_max=6.0, gain=85)
    a.update(kw)
    want, want_stats = vis.eval_panels_numpy(a['pred'], a['gt_u'], a['gt_v'], a['count2'], a['frames'],
                                             a['max_row'], a['flow_scale'], a['err_max'], a['gain'],
                                             return_stats=True)
    image, stats = vis.eval_panels(dev(a['pred']), dev(a['gt_u']), dev(a['gt_v']), dev(a['count2']),
                                   dev(a['frames']), a['max_row'], a['flow_scale'], a['err_max'],
                                   a['gain'], return_stats=True)
    got, stats = image.cpu().numpy(), vis.read_panel_stats(stats)
    assert stats.tobytes() == want_stats.tobytes()
    assert np.array_equal(got[:, :, :67], want[:, :, :67])
    assert np.array_equal(got[:, :, 201:], want[:, :, 201:])
    for f in range(3):      # the given scale, or the frame's own
        m = float(vis.panel_scale(stats[f], a['flow_scale']))
        drawn = vis.render_flows(dev(np.stack([c['pred'][f], np.stack([c['gt_u'][f], c['gt_v'][f]])])),
                                 max_magnitude=m).cpu().numpy()
        assert np.array_equal(got[f, :, 67:134], drawn[0]) and np.array_equal(got[f, :, 134:201], drawn[1])
    # the metric's own counts on the same tensors
    count = None if a['count2'] is None else dev(a['count2'].sum(1).astype(np.int32))
    res = dev_eval.read_results(dev_eval.flow_error(dev(a['gt_u']), dev(a['gt_v']), dev(a['pred']),
                                                    count, a['max_row']))
    assert stats['n_counted'].tolist() == res['n_points'].tolist()
    assert stats['n_below'].tolist() == res['n_below'].tolist()
    assert (res['n_points'] > 0).all() or a['max_row'] == 0


def test_no_usable_ground_truth_maximum_takes_the_predictions():
    c = pc.case(2, (7, 5))
    gu = np.zeros_like(c['gt_u'])
    gu[1] = np.inf
    image, stats = vis.eval_panels(dev(c['pred']), dev(gu), dev(np.zeros_like(gu)), return_stats=True)
    got, stats = image.cpu().numpy(), vis.read_panel_stats(stats)
    want, want_stats = vis.eval_panels_numpy(c['pred'], gu, np.zeros_like(gu), return_stats=True)
    assert stats.tobytes() == want_stats.tobytes() and stats['n_counted'].tolist() == [0, 0]
    assert [float(vis.panel_scale(s)) for s in stats] == stats['pred_hi'].tolist()
    assert (got[:, :, 15:] == 64).all() and not got[:, :, :5].any() and not got[:, :, 10:15].any()
    check_flow_panels(got, dict(c, gt_u=gu, gt_v=np.zeros_like(gu)), stats, 5)


def test_same_bytes_again_and_alone():
    c, _, _ = reference(3, (130, 33))
    d = [dev(c[k]) for k in ('pred', 'gt_u', 'gt_v', 'count2', 'frames')]
    first, stats = vis.eval_panels(*d, return_stats=True)
    again, stats2 = vis.eval_panels(*d, return_stats=True)
    assert torch.equal(first, again) and torch.equal(stats, stats2)
    for i in range(3):
        alone, s = vis.eval_panels(*(t[i:i + 1] for t in d), return_stats=True)
        assert torch.equal(alone[0], first[i]) and torch.equal(s[0], stats[i])


# ------------------------------------------------------------ polarity count
def events(rng, n, shape, pad=0):
    H, W = shape
    x, y = rng.integers(0, W, n), rng.integers(0, H, n)
    p = rng.choice([-1, 0, 1], n)
    if pad:         # padding slots among the events: x = y = -1, whatever the polarity
        slots = rng.choice(n, pad, replace=False)
        x[slots] = y[slots] = -1
    return x.astype(np.int64), y.astype(np.int64), p.astype(np.int64)


def count2_numpy(x, y, p, begin, shape, box):
    y0, x0, h, w = box
    out = np.zeros((len(begin) - 1, 2, h, w), np.int64)
    for f, (a, b) in enumerate(zip(begin[:-1], begin[1:])):
        xs, ys, ps = x[a:b] - x0, y[a:b] - y0, p[a:b]
        keep = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
        np.add.at(out[f], (np.where(ps[keep] > 0, 0, 1), ys[keep], xs[keep]), 1)
    return out


@pytest.mark.parametrize('shape, box, begin, pad', [
    ((37, 70), None, [0, 1000, 1000, 2500, 4000], 0),               # an empty frame
    ((37, 70), (5, 11, 32, 59), [0, 700, 1900, 4000], 0),           # a box at an odd corner
    ((33, 67), None, [0, 1500, 3000], 500),                         # padding slots inside the frames
    ((33, 67), (1, 2, 7, 5), [100, 2000, 3900], 0),                 # events before and after the frames
    ((130, 173), None, [0, 600000], 0),                             # more events than one grid pass
], ids=['empty_frame', 'odd_box', 'padding', 'inner_range', 'large'])
def test_polarity_count_is_exact(shape, box, begin, pad):
    rng = np.random.default_rng(7)
    n = max(begin[-1], 4000)
    x, y, p = events(rng, n, shape, pad)
    h, w = shape if box is None else box[2:]
    got = dev_eval.count_image_polarity_batched(dev(x), dev(y), dev(p), begin, (h, w), box)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(begin) - 1, 2, h, w)
    want = count2_numpy(x, y, p, begin, shape, box or (0, 0, h, w))
    assert np.array_equal(got.cpu().numpy(), want)
    assert want[:, 0].sum() > 0 and want[:, 1].sum() > want[:, 0].sum()     # p = 0 counts as OFF
    both = dev_eval.count_image_batched(dev(x), dev(y), begin, (h, w), box)
    assert torch.equal(got.sum(1).to(torch.int32), both)
    # the call zeroes its output: a second call gives the same
    assert torch.equal(dev_eval.count_image_polarity_batched(dev(x), dev(y), dev(p), begin, (h, w), box), got)


def test_polarity_count_without_events():
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    got = dev_eval.count_image_polarity_batched(none, none, none, [0, 0, 0], (5, 7))
    assert tuple(got.shape) == (2, 2, 5, 7) and not bool(got.any())
    x, y, p = (dev(a) for a in events(np.random.default_rng(1), 100, (5, 7)))
    assert not bool(dev_eval.count_image_polarity_batched(x, y, p, [40, 40], (5, 7)).any())
    assert tuple(dev_eval.count_image_polarity_batched(x, y, p, [0], (5, 7)).shape) == (0, 2, 5, 7)
