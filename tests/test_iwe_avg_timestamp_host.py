"""The numpy restatement of the average-timestamp images of the validation
metric and the ratio derived from them (eval.iwe_avg_timestamp_host,
iwe_avg_timestamp_rows_host, derive_rsat; docs/IWE_SPEC.md sections 14-21),
without a GPU.  Everything is compared exactly: q and count against
eval.iwe_splat_multi_host, all four images and the rows against
loss.avg_timestamp_fwd_host where the two frame rules pick the same events
(which tests/test_avg_timestamp_oracle.py holds to the float64 definition), and
the properties that make the ratio a metric: 1 at zero flow, no dependence on
the order of the events or on the batch, below 1 for the true flow of moving
points."""
import numpy as np
import pytest

from dvs_of_training_framework_amd import eval as dev_eval, loss as L
from tests import avg_timestamp_cases as ac, iwe_avg_timestamp_cases as rc

_want = {}


def want(name, mask, polarity):
    """The restatement's answer, computed once: (q, s, base, count)."""
    key = (name, mask, polarity)
    if key not in _want:
        _want[key] = dev_eval.iwe_avg_timestamp_host(*rc.args_of(rc.case(name)), mask, polarity)
    return _want[key]


def same_images(got, expected):
    return all(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, expected))


@pytest.mark.parametrize('name', rc.CASE_IDS)
def test_q_and_count_are_those_of_the_image_of_warped_events(name):
    c = rc.case(name)
    F, (h, w) = len(c['begin']) - 1, c['shape']
    for mask, polarity in rc.OPTIONS:
        q, s, base, count = want(name, mask, polarity)
        M = rc.images_of(F, mask, polarity)
        assert q.dtype == s.dtype == base.dtype == np.int64 and count.dtype == np.uint32
        assert q.shape == s.shape == base.shape == count.shape == (M, h, w)
        q2, count2 = dev_eval.iwe_splat_multi_host(*rc.args_of(c), mask, polarity)
        assert np.array_equal(q, q2) and np.array_equal(count, count2), (mask, polarity)
        # weight times a distance of at most 1; the distances of count events
        assert (0 <= s).all() and (s <= q).all() and (0 <= base).all() and (base <= count.astype(np.int64) << 32).all()


def test_the_images_are_views_of_one_region_laid_out_as_the_header_says():
    q, s, base, count = want('5x7_F3_degenerate', 5, True)
    P = q.size
    region = q.base
    while region.base is not None:
        region = region.base
    assert region.dtype == np.uint8 and region.size == dev_eval.iwe_avg_timestamp_image_bytes(12, 5, 7) == 28 * P
    start = region.ctypes.data
    assert [a.ctypes.data - start for a in (q, s, base, count)] == [0, 8 * P, 16 * P, 24 * P]
    assert dev_eval.iwe_avg_timestamp_image_bytes(1, 1, 1) == 32        # 28 bytes, padded
    assert dev_eval.iwe_avg_timestamp_image_bytes(3, 3, 3) == 760


@pytest.mark.parametrize('name', rc.ONE_PER_SAMPLE_IDS)
def test_with_one_frame_per_sample_the_images_and_rows_are_the_training_terms(name):
    c = rc.case(name)
    for mask, polarity in rc.OPTIONS:
        images = want(name, mask, polarity)
        term = L.avg_timestamp_fwd_host(*rc.one_frame_per_sample(c), mask, polarity)
        for k, a in zip(rc.IMAGES, images):
            assert a.dtype == term[k].dtype and np.array_equal(a, term[k]), (k, mask, polarity)
        rows = dev_eval.iwe_avg_timestamp_rows_host(*images)
        assert rows.dtype == L.AVG_TIMESTAMP_ROW_DTYPE and rows.tobytes() == term['rows'].tobytes()
        # the term counts an image without a baseline as 0, the metric leaves it out (NaN)
        rsat = dev_eval.derive_rsat(rows)
        live = rows['S0'] > 0
        assert np.array_equal(np.isnan(rsat), ~live) and np.array_equal(rsat[live], term['image_value'][live])
        total = np.float64(0)
        for v in np.where(live, rsat, 0.0):         # in image order
            total = total + v
        assert np.float32(total / np.float64(len(rsat))).tobytes() == term['term'].tobytes(), (mask, polarity)


@pytest.mark.parametrize('name', rc.CASE_IDS)
def test_zero_flow_gives_exactly_one(name):
    c = rc.case(name)
    still = dict(c, flow=np.zeros_like(c['flow']))
    for mask, polarity in ((7, True), (1, False), (4, False)):
        q, s, base, count = dev_eval.iwe_avg_timestamp_host(*rc.args_of(still), mask, polarity)
        assert np.array_equal(q, count.astype(np.int64) << 32) and np.array_equal(s, base)
        rows = dev_eval.iwe_avg_timestamp_rows_host(q, s, base, count)
        rsat = dev_eval.derive_rsat(rows)
        live = rows['S0'] > 0
        assert live.any() and (rsat[live] == 1.0).all() and np.isnan(rsat[~live]).all(), (mask, polarity)


@pytest.mark.parametrize('name', rc.CASE_IDS)
def test_the_order_of_the_events_and_the_batch_do_not_matter(name):
    c = rc.case(name)
    F = len(c['begin']) - 1
    for mask, polarity in ((7, True), (5, False)):
        expected = want(name, mask, polarity)
        assert same_images(dev_eval.iwe_avg_timestamp_host(*rc.args_of(rc.permuted(c)), mask, polarity), expected)
        per = rc.images_of(1, mask, polarity)
        rows = dev_eval.iwe_avg_timestamp_rows_host(*expected)
        for f in range(F if F > 1 else 0):
            alone = dev_eval.iwe_avg_timestamp_host(*rc.args_of(rc.single_frame(c, f)), mask, polarity)
            assert same_images(alone, [a[f * per:(f + 1) * per] for a in expected]), (f, mask, polarity)
            assert dev_eval.iwe_avg_timestamp_rows_host(*alone).tobytes() == rows[f * per:(f + 1) * per].tobytes()


def test_the_three_branches_of_the_ratio():
    rows = np.zeros(6, L.AVG_TIMESTAMP_ROW_DTYPE)
    rows['S'] = [0.0, 3.0, 0.0, 0.5, 7.0, 2.0]
    rows['S0'] = [0.0, 0.0, 2.0, 2.0, 1.75, -1.0]
    rows['n'] = [0, 4, 0, 2, 7, 3]
    rows['n0'] = [0, 4, 5, 8, 3, 3]
    rsat = dev_eval.derive_rsat(rows)
    assert rsat.dtype == np.float64 and rsat.shape == (6,)
    # no events; all of them on the reference (a baseline of 0, whatever landed); S0 <= 0 in any form
    assert np.isnan(rsat[[0, 1, 5]]).all()
    # every event left the image: never rewarded
    assert rsat[2] == 1.0
    # (S / n) / (S0 / n0), in this order
    assert rsat[3] == (0.5 / 2) / (2.0 / 8) == 1.0 and rsat[4] == (7.0 / 7) / (1.75 / 3)
    # the rows as the device hands them over: uint8 [M,32]
    raw = rows.view(np.uint8).reshape(6, 32)
    assert np.array_equal(np.isnan(dev_eval.derive_rsat(raw)), np.isnan(rsat))
    assert np.array_equal(dev_eval.derive_rsat(raw)[2:5], rsat[2:5])
    assert dev_eval.read_avg_timestamp_rows(raw).tobytes() == rows.tobytes()
    assert dev_eval.derive_rsat(np.zeros(0, L.AVG_TIMESTAMP_ROW_DTYPE)).shape == (0,)


def as_frames(c):
    """A case of tests/contrast_cases.py (one sample, one window) as the metric takes it."""
    n = c['x'].size
    return c['x'], c['y'], c['t'], c['p'], np.array([0, n], np.int64), c['ts'], c['flow']


def rsat_of(c, mask=5, polarity=False):
    images = dev_eval.iwe_avg_timestamp_host(*as_frames(c), mask, polarity)
    return dev_eval.derive_rsat(dev_eval.iwe_avg_timestamp_rows_host(*images))


def test_the_true_flow_of_moving_points_lies_below_one_and_below_the_reversed_flows():
    zero, true = ac.moving_points_case()
    wrong = dict(zero, flow=-true['flow'])
    for mask, polarity in ((5, False), (1, False), (7, True)):
        at_zero, at_true, at_wrong = (rsat_of(c, mask, polarity) for c in (zero, true, wrong))
        print('moving points', mask, polarity, 'true flow:', at_true, 'reversed:', at_wrong)
        assert (at_zero == 1.0).all()
        assert (at_true < 1.0).all() and (at_true >= 0.0).all() and (at_true < at_wrong).all(), (mask, polarity)


def test_events_that_all_leave_give_one_and_no_events_give_nan():
    c = ac.all_leave_case()
    n = c['x'].size
    begin = np.array([0, n, n], np.int64)       # the second frame holds no events
    images = dev_eval.iwe_avg_timestamp_host(c['x'], c['y'], c['t'], c['p'], begin, c['ts'], c['flow'], 5, False)
    rows = dev_eval.iwe_avg_timestamp_rows_host(*images)
    assert images[3][:2].any() and not images[0][:2].any() and not images[3][2:].any()
    rsat = dev_eval.derive_rsat(rows)
    assert list(rsat[:2]) == [1.0, 1.0] and np.isnan(rsat[2:]).all()


def test_the_render_is_grey_on_the_fixed_scale():
    q, s, base, count = want('5x7_F3_degenerate', 7, True)
    canvas = dev_eval.iwe_avg_timestamp_render_host(q, s, base, count)
    M, h, w = q.shape
    assert canvas.dtype == np.uint8 and canvas.shape == (M, h, 2 * w, 3)
    assert (canvas[..., 0] == canvas[..., 1]).all() and (canvas[..., 0] == canvas[..., 2]).all()
    T, _, T0 = L.avg_timestamp_pixels_host(q, s, base, count.astype(np.int64))
    assert (T < 1).all() and (T0 < 1).all()
    f32 = np.float32
    left = np.minimum((T0.astype(f32) * f32(255) + f32(0.5)).astype(np.int64), 255)
    right = np.minimum((T.astype(f32) * f32(255) + f32(0.5)).astype(np.int64), 255)
    assert np.array_equal(canvas[:, :, :w, 0], left) and np.array_equal(canvas[:, :, w:, 0], right)
    assert not canvas[:, :, :w][count == 0].any() and canvas.max() > 100
    # host input goes to the restatement
    assert np.array_equal(dev_eval.iwe_avg_timestamp_render(q, s, base, count), canvas)


def test_host_input_runs_the_restatement():
    c = rc.case('16x16_F3_slots_only')
    events = {'x': c['x'], 'y': c['y'], 'timestamp': c['t'], 'polarity': c['p']}
    images, rows = dev_eval.iwe_avg_timestamp(events, c['begin'], c['ts'], c['flow'], ('start', 'end'), True)
    assert same_images(images, want('16x16_F3_slots_only', 5, True))
    assert rows.dtype == np.uint8 and rows.shape == (len(images[0]), 32)
    assert rows.tobytes() == dev_eval.iwe_avg_timestamp_rows_host(*images).tobytes()
    with pytest.raises(ValueError, match='polarity column'):
        dev_eval.iwe_avg_timestamp({k: events[k] for k in ('x', 'y', 'timestamp')}, c['begin'], c['ts'], c['flow'],
                                   1, True)


def test_no_frames_and_no_events():
    empty = np.zeros(0, np.int64)
    q, s, base, count = dev_eval.iwe_avg_timestamp_host(empty, empty, np.zeros(0, np.float32), empty,
                                                        np.zeros(1, np.int64), np.zeros(0, np.float32),
                                                        np.zeros((0, 2, 4, 5), np.float32), 7, True)
    assert q.shape == s.shape == base.shape == count.shape == (0, 4, 5)
    assert dev_eval.iwe_avg_timestamp_rows_host(q, s, base, count).shape == (0,)
    images = dev_eval.iwe_avg_timestamp_host(empty, empty, np.zeros(0, np.float32), empty, np.zeros(3, np.int64),
                                             np.array([0, 1, 0, 1], np.float32), np.ones((2, 2, 4, 5), np.float32),
                                             5, False)
    assert all(a.shape == (4, 4, 5) and not a.any() for a in images)
    rows = dev_eval.iwe_avg_timestamp_rows_host(*images)
    assert not rows.view(np.uint8).any() and np.isnan(dev_eval.derive_rsat(rows)).all()
