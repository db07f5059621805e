"""CPU side of the image of warped events (docs/IWE_SPEC.md): the package's
numpy float32 restatement through the public functions, on hand-made cases
with exact answers, against an independent float64 splat within the bound the
spec derives, the statistics against plain integer sums and math.fsum, the
render restatement, the argument rules of the C ABI (nothing is launched) and
the host logic of the hook and its flags."""
import math

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import eval as dev_eval, hooks

from . import iwe_cases as ic


def splat(c):
    """The public function on host arrays: the restatement."""
    return dev_eval.iwe_splat({'x': c['x'], 'y': c['y'], 'timestamp': c['t']}, c['begin'], c['ts'],
                              c['flow'])


def rows_of(q, count):
    rows = dev_eval.iwe_stats(q, count)
    assert rows.dtype == np.uint8 and rows.shape == (len(q), 48)
    return dev_eval.read_iwe_results(rows)


# ------------------------------------------------------------- exact cases
@pytest.mark.parametrize('name', ic.CASE_IDS)
def test_zero_flow_gives_the_count_image_and_a_loss_of_exactly_one(name):
    c = ic.case(name)
    c = dict(c, flow=np.zeros_like(c['flow']))
    q, count = splat(c), ic.count_image(c)
    assert q.dtype == np.int64 and q.shape == count.shape
    assert np.array_equal(q, count.astype(np.int64) << 32)
    res = rows_of(q, count)
    fwl, kept = dev_eval.derive_fwl(res, q.shape[1] * q.shape[2])
    for f in range(len(q)):
        if count[f].max() == count[f].min():        # no variance: no events, or one pixel
            assert np.isnan(fwl[f])
        else:
            assert fwl[f] == 1.0
        if count[f].any():
            assert kept[f] == 1.0
        else:
            assert np.isnan(kept[f])


def bar(u, width=32):
    """Four rows, events at x = 10 + k, t = k / 8, k = 1 .. 8, a window of
    length 1, constant flow (u, 0)."""
    k = np.arange(1, 9)
    x = np.tile(10 + k, 4)
    y = np.repeat(np.arange(4), 8)
    t = np.tile(k / 8, 4).astype(np.float32)
    flow = np.zeros((1, 2, 4, width), np.float32)
    flow[0, 0] = u
    c = dict(x=x, y=y, t=t, begin=np.array([0, 32]), ts=np.array([0, 1], np.float32), flow=flow,
             shape=(4, width))
    q, count = splat(c), ic.count_image(c)
    res = rows_of(q, count)
    fwl, kept = dev_eval.derive_fwl(res, 4 * width)
    assert kept[0] == 1.0 and int(res['count_sum'][0]) == 32 and int(res['count_sq'][0]) == 32
    return q[0], res[0], float(fwl[0])


def test_moving_bar():
    N = 4 * 32
    var_cnt = 32 / N - (32 / N) ** 2            # 32 pixels of 1
    # u = 8: every event lands on column 10, 8 per row
    q, res, fwl = bar(8.0)
    want = np.zeros((4, 32), np.int64)
    want[:, 10] = 8 << 32
    assert np.array_equal(q, want)
    assert (res['sum_sq'], res['sum_q'], res['max_q']) == (4 * 64.0, 32 << 32, 8 << 32)
    assert fwl == (4 * 64 / N - (32 / N) ** 2) / var_cnt and fwl > 10
    # ... on a window of 24 columns the same by hand: 11.5
    _, _, fwl24 = bar(8.0, 24)
    assert fwl24 == (4 * 64 / 96 - (32 / 96) ** 2) / (32 / 96 - (32 / 96) ** 2)
    assert fwl24 == pytest.approx(11.5, rel=1e-15)
    # u = -8: x = 10 + 2 k, the same histogram, shifted
    q, res, fwl = bar(-8.0)
    want[:] = 0
    want[:, 12:27:2] = 1 << 32
    assert np.array_equal(q, want) and fwl == 1.0
    # u = -4: x = 10 + 1.5 k, half-integers for odd k: per row 4 pixels of 1 and 8 of 1/2
    q, res, fwl = bar(-4.0)
    want[:] = 0
    for k in range(1, 9):
        if k % 2:
            want[:, 10 + (3 * k - 1) // 2] = want[:, 10 + (3 * k + 1) // 2] = 1 << 31
        else:
            want[:, 10 + 3 * k // 2] = 1 << 32
    assert np.array_equal(q, want)
    assert res['sum_sq'] == 4 * (4 + 8 * 0.25)
    assert fwl == (24 / N - (32 / N) ** 2) / var_cnt and fwl < 1


def test_an_event_is_dropped_or_clipped_as_the_spec_says():
    """One event at (2, 1) of a 3 x 4 window, tau = 1."""
    def one(u, v, x=2, y=1, t=1.0, ts=(0, 1)):
        flow = np.zeros((1, 2, 3, 4), np.float32)
        flow[0, :, y, x] = (u, v)
        return splat(dict(x=np.array([x]), y=np.array([y]), t=np.array([t], np.float32),
                          begin=np.array([0, 1]), ts=np.array(ts, np.float32), flow=flow))[0]
    full, half, quarter = 1 << 32, 1 << 31, 1 << 30
    assert one(0, 0).tolist() == [[0, 0, 0, 0], [0, 0, full, 0], [0, 0, 0, 0]]
    assert one(-0.0, -0.0).tolist() == one(0, 0).tolist()
    assert one(0.5, 0.5).tolist() == [[0, quarter, quarter, 0], [0, quarter, quarter, 0], [0, 0, 0, 0]]
    assert one(2.5, 0).tolist() == [[0, 0, 0, 0], [half, 0, 0, 0], [0, 0, 0, 0]]      # a corner outside
    assert one(-1.5, -1.5).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, quarter]]
    assert one(1, 1).tolist() == [[0, full, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]          # corners with Q = 0
    for u, v in ((3, 0), (-2, 0), (0, 2), (0, -2), (np.nan, 0), (0, np.nan), (np.inf, 0), (-np.inf, 0),
                 (1e30, 0), (0, -1e30)):
        assert not one(u, v).any(), (u, v)                      # -1, w, h exactly, and beyond
    # tau: clamped to [0, 1]; 0 for a window of no or negative length; 0 * inf is dropped
    assert one(1, 0, t=0.5).tolist() == [[0, 0, 0, 0], [0, half, half, 0], [0, 0, 0, 0]]
    assert one(1, 0, t=7.0).tolist() == one(1, 0).tolist()
    assert one(1, 0, t=-3.0).tolist() == one(0, 0).tolist()
    assert one(1, 0, ts=(1, 1)).tolist() == one(0, 0).tolist()
    assert one(1, 0, ts=(1, 0)).tolist() == one(0, 0).tolist()
    assert one(1e30, 0, t=0.0).tolist() == one(0, 0).tolist()
    assert not one(np.inf, 0, t=0.0).any()
    # a weight below 2^-32 truncates to nothing: fx = 2^-20, fy = 2^-20
    tiny = one(-2.0 ** -20, -2.0 ** -20, x=1, y=1)
    assert tiny[2, 2] == 0 and tiny[1, 2] == tiny[2, 1] == (1 << 12) - 1 and tiny.sum() < full


# ------------------------------------------------- the definition in float64
@pytest.mark.parametrize('name', ic.CASE_IDS)
def test_restatement_against_the_float64_definition(name):
    c = ic.case(name)
    q = splat(c)
    image, touching = ic.splat64(c)
    bound = touching * ic.contribution_bound(c['shape'])
    err = np.abs(q.astype(np.float64) * 2.0 ** -32 - image)
    print(name, 'largest error', err.max(), 'of bound', (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), np.argwhere(err > bound)[:5]
    assert (q >= 0).all()
    # the cases are what they claim to be
    F = len(c['begin']) - 1
    count = ic.count_image(c)
    assert c['begin'][0] > 0 and c['begin'][-1] < c['x'].size and (c['x'][c['begin'][-1]:] == -1).all()
    assert count.max() >= min(200, ic.PER_FRAME[c['shape']])
    if 'empty_middle' in name:
        assert c['begin'][1] == c['begin'][2] and not q[1].any()
    if 'slots_only' in name:
        assert c['begin'][1] < c['begin'][2] and not q[1].any() and not count[1].any()
    if 'degenerate' in name:        # tau = 0: every event stays where it is, unless 0 * flow is a NaN
        finite = np.isfinite(c['flow']).all(1)
        assert np.array_equal(q[1:], (count[1:].astype(np.int64) << 32) * finite[1:])
        assert not finite[1:].all()
    assert all(q[f].any() for f in range(F) if count[f].any())
    assert q.sum() < (count.astype(np.int64).sum() << 32) or 'degenerate' in name      # mass left the image


def test_cases_hold_every_special_flow_under_an_event():
    c = ic.case('33x31_F1')
    lo, hi = c['begin'][0], c['begin'][1]
    x, y = c['x'][lo:hi], c['y'][lo:hi]
    ok = x >= 0
    under = c['flow'][0][:, y[ok], x[ok]]
    assert np.isnan(under).any() and (under == np.inf).any() and (under == -np.inf).any()
    assert (under == np.float32(1e30)).any() and (under == np.float32(-1e30)).any()
    assert ((under == 0) & np.signbit(under)).any()
    t = c['t'][lo:hi]
    assert (t == 0).any() and (t == 0.5).any() and (~ok).any()


# ------------------------------------------------------------- statistics
@pytest.mark.parametrize('name', ic.CASE_IDS)
def test_statistics(name):
    c = ic.case(name)
    q, count = splat(c), ic.count_image(c)
    res = rows_of(q, count)
    n = q.shape[1] * q.shape[2]
    for f in range(len(q)):
        qs, cs = [int(v) for v in q[f].ravel()], [int(v) for v in count[f].ravel()]
        assert int(res['sum_q'][f]) == sum(qs) and int(res['max_q'][f]) == max(qs)
        assert int(res['count_sum'][f]) == sum(cs) and int(res['count_max'][f]) == max(cs)
        assert int(res['count_sq'][f]) == sum(v * v for v in cs)
        want = math.fsum((v * 2.0 ** -32) ** 2 for v in qs)
        assert abs(res['sum_sq'][f] - want) <= n * 2.0 ** -53 * want
    # the count image may come as int32 bits (eval.count_image_batched) or as a tensor
    again = dev_eval.read_iwe_results(dev_eval.iwe_stats(torch.from_numpy(q),
                                                         torch.from_numpy(count.view(np.int32))))
    assert again.tobytes() == res.tobytes()


def test_derive_fwl():
    res = np.zeros(3, dev_eval.IWE_RESULT_DTYPE)
    res['sum_sq'], res['sum_q'] = [12.0, 0.0, 5.0], [6 << 32, 0, 3 << 32]
    res['count_sq'], res['count_sum'] = [10, 0, 4], [6, 0, 4]       # counts 2 2 1 1; none; 1 1 1 1
    fwl, kept = dev_eval.derive_fwl(res, 4)
    assert fwl[0] == (12 / 4 - 1.5 ** 2) / (10 / 4 - 1.5 ** 2) == 3.0
    assert np.isnan(fwl[1]) and np.isnan(kept[1]) and np.isnan(fwl[2])      # 4 pixels of 1: no variance
    assert kept.tolist()[::2] == [1.0, 0.75]


# ----------------------------------------------------------------- render
@pytest.mark.parametrize('name', ['5x7_F3_empty_middle', '33x31_F3_recorded', '16x16_F3_slots_only'])
def test_render_restatement(name):
    c = ic.case(name)
    q, count = splat(c), ic.count_image(c)
    rows = dev_eval.iwe_stats(q, count)
    canvas = dev_eval.iwe_render(q, count, rows)
    F, h, w = q.shape
    assert canvas.dtype == np.uint8 and canvas.shape == (F, h, 2 * w, 3)
    assert (canvas[..., 0] == canvas[..., 1]).all() and (canvas[..., 0] == canvas[..., 2]).all()
    grey = canvas[..., 0]
    for f in range(F):
        left, right = grey[f, :, :w], grey[f, :, w:]
        if not count[f].any():                      # an all-zero frame is black
            assert not left.any() and not right.any()
            continue
        assert left.ravel()[count[f].argmax()] == 255 and right.ravel()[q[f].argmax()] == 255
        assert np.array_equal(left == 0, count[f] * 510 < count[f].max())
        # by hand, in float32: one division, one product, one sum, truncation
        m = np.float32(float(q[f].max()) * 2.0 ** -32)
        value = (q[f].astype(np.float64) * 2.0 ** -32).astype(np.float32)
        want = np.minimum((value / m * np.float32(255) + np.float32(0.5)).astype(np.int64), 255)
        assert np.array_equal(right, want)
    # every byte is written: a canvas that starts as 0xAA or as 0x55 ends the same
    res = dev_eval.read_iwe_results(rows)
    assert np.array_equal(dev_eval.iwe_render_host(q, count, res), canvas)


# --------------------------------------------------------- argument rules
def test_argument_rules_are_checked_on_the_host():
    """No GPU is needed to be refused: nothing is launched."""
    lib = dev_eval._lib.lib()
    F, h, w, n = 2, 5, 7, 11
    t = dict(x=torch.zeros(n, dtype=torch.long), y=torch.zeros(n, dtype=torch.long), t=torch.zeros(n),
             begin=torch.tensor([0, 5, 11]), ts=torch.zeros(2 * F), flow=torch.zeros(F, 2, h, w),
             q=torch.full((F, h, w), 7, dtype=torch.long), count=torch.zeros(F, h, w, dtype=torch.int32),
             result=torch.full((F, 48), 7, dtype=torch.uint8),
             ws=torch.zeros(lib.dvsof_iwe_stats_workspace_bytes(F, h, w), dtype=torch.uint8),
             canvas=torch.full((F, h, 2 * w, 3), 7, dtype=torch.uint8))
    a = {k: v.data_ptr() for k, v in t.items()}
    a['n'] = n
    seen = 0
    for what, call, expect in ic.bad_calls(lib, a, F, h, w):
        assert call() == expect, what
        seen += 1
    assert seen >= 35
    for k in ('q', 'result', 'canvas'):
        assert bool((t[k] == 7).all()), k
    assert all(rc == 0 for rc in ic.empty_calls(lib))
    assert lib.dvsof_iwe_stats_workspace_bytes(F, h, w) == 48 * F
    assert lib.dvsof_iwe_stats_workspace_bytes(3, 400, 400) == 48 * 3 * 128     # the block count is capped
    assert lib.dvsof_iwe_stats_workspace_bytes(1, 33, 31) == 48
    assert lib.dvsof_iwe_stats_workspace_bytes(1, 33, 32) == 48 * 2
    for bad in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 32768)):
        assert lib.dvsof_iwe_stats_workspace_bytes(*bad) == 0


# ------------------------------------------------------------- host logic
def test_sharpness_frames_against_a_literal():
    ts = [1.0, 1.5, 2.0, 2.5, 3.0, 3.5]
    assert hooks.sharpness_frames(ts, 3.25) == [(1.0, 1.5), (1.5, 2.0), (2.0, 2.5), (2.5, 3.0)]
    assert hooks.sharpness_frames(ts, 3.25, 2) == [(1.0, 2.0), (1.5, 2.5), (2.0, 3.0)]
    assert hooks.sharpness_frames(ts, 9.0) == [(1.0, 1.5), (1.5, 2.0), (2.0, 2.5), (2.5, 3.0), (3.0, 3.5)]
    assert hooks.sharpness_frames(ts, 9.0, 5) == [(1.0, 3.5)]
    assert hooks.sharpness_frames(ts, 9.0, 6) == [] and hooks.sharpness_frames(ts, 0.5) == []
    with pytest.raises(ValueError, match='at least one image'):
        hooks.sharpness_frames(ts, 9.0, 0)


def test_flags_parse_and_period_zero_builds_nothing(tmp_path):
    import train_flownet as tf
    args = tf.parse_args(['-m', str(tmp_path / 'm')])
    assert (args.sharpness_period, args.sharpness_frame_step, args.sharpness_pictures) == (0, 1, 4)
    args = tf.parse_args(['-m', str(tmp_path / 'm'), '--sharpness-period', '50',
                          '--sharpness-frame-step', '4', '--sharpness-pictures', '2'])
    assert (args.sharpness_period, args.sharpness_frame_step, args.sharpness_pictures) == (50, 4, 2)
    hooks_, periodic = {}, {}
    tf.add_sharpness(tf.parse_args(['-m', str(tmp_path / 'm')]), hooks_, periodic, None, 'cpu', None, 0)
    assert hooks_ == {} and periodic == {} and not (tmp_path / 'm' / 'sharpness').exists()


def test_a_period_without_a_sequence_exits_and_names_the_flag(tmp_path):
    import train_flownet as tf
    args = tf.parse_args(['-m', str(tmp_path / 'm'), '--sharpness-period', '5'])
    with pytest.raises(SystemExit) as e:
        tf.add_sharpness(args, {}, {}, None, 'cpu', None, 0)
    assert '--sharpness-period' in str(e.value) and '--validation-sequence' in str(e.value)
    assert '--validation-ground-truth' not in str(e.value)


def test_other_ranks_build_a_hook_that_needs_nothing(tmp_path):
    import train_flownet as tf
    args = tf.parse_args(['-m', str(tmp_path / 'm'), '--sharpness-period', '5',
                          '--validation-sequence', str(tmp_path / 'none')])
    hooks_, periodic = {}, {}
    tf.add_sharpness(args, hooks_, periodic, None, 'cpu', None, 1)
    assert set(hooks_) == set(periodic) == {'sharpness'}
    assert hooks_['sharpness'](5, 50) is None and not (tmp_path / 'm' / 'sharpness').exists()


def test_the_two_hooks_share_one_sequence(tmp_path, monkeypatch):
    import train_flownet as tf
    from dvs_of_training_framework_amd import sequence

    class Recorded:
        shape, image_ts, t = (8, 8), np.arange(4.0), np.array([2.5])

        def __len__(self):
            return 1
    loads = []
    monkeypatch.setattr(sequence.FrameSequence, 'from_directory',
                        classmethod(lambda cls, path, device: loads.append(path) or Recorded()))
    args = tf.parse_args(['-m', str(tmp_path / 'm'), '--sharpness-period', '5', '--height', '4',
                          '--width', '4', '--validation-sequence', 'seq'])
    hooks_ = {'evaluation': type('E', (), {'sequence': Recorded()})()}
    tf.add_sharpness(args, hooks_, {}, None, 'cpu', None, 0)
    assert hooks_['sharpness'].sequence is hooks_['evaluation'].sequence and loads == []
    assert hooks_['sharpness'].frames == [(0.0, 1.0), (1.0, 2.0)] and hooks_['sharpness'].box == (2, 2, 4, 4)
    alone = {}
    tf.add_sharpness(args, alone, {}, None, 'cpu', None, 0)
    assert len(loads) == 1 and isinstance(alone['sharpness'].sequence, Recorded)
