"""CPU checks of the evaluation path (docs/EVAL_SPEC.md): the float64
restatement of tests/eval_cases.py reproduces what the reference's
utils/eval.py computed for every golden case (tools/make_goldens_eval.py), the
host-side planner reproduces the reference's step lists, and the restated
helpers of testing.py behave as the reference's."""
import numpy as np
import pytest

from dvs_of_training_framework_amd import eval as dev_eval
from dvs_of_training_framework_amd import testing
from tests import eval_cases as ec
from tests.conftest import load_golden


@pytest.fixture(scope='module')
def golden():
    return load_golden('eval_reference')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape', ec.SHAPES)
def test_restatement_reproduces_the_reference_propagation(golden, shape, dtype):
    key = ec.prop_key(shape, dtype)
    xm, ym = golden[f'{key}_x'], golden[f'{key}_y']
    assert xm.dtype == dtype and xm.shape == (ec.K_MAPS,) + shape
    for f, (start, stop) in enumerate(golden['prop_frames']):
        u, v = ec.propagate64(xm, ym, golden['prop_ts'], start, stop)
        for got, name in ((u, 'u'), (v, 'v')):
            want = golden[f'{key}_{name}{f}']
            assert ec.same_bits(got.astype(want.dtype), want), (key, name, f)


def test_golden_propagation_cases_cover_what_they_claim(golden):
    """Masks, infinities, pixels leaving on every side and both halves of
    round-half-to-even are really in the cases."""
    key = ec.prop_key((12, 20), np.float32)
    xm, ym = golden[f'{key}_x'], golden[f'{key}_y']
    assert 0.05 < (xm == 0).mean() < 0.2 and np.isinf(xm).sum() == 1
    modes = [int(golden[f'plan_mode{f}']) for f in range(len(ec.PROP_FRAMES))]
    assert modes == [1, 0, 0, 0, 0]
    assert not np.isfinite(golden[f'{key}_u0']).all()       # inf, direct scale
    assert not (np.isfinite(golden[f'{key}_u4']).all()      # inf reached by propagation
                and np.isfinite(golden[f'{key}_v4']).all())
    # after the scale-1 first step of frame 1 the 0.5 / 1.5 patches sit on
    # half-integer coordinates, on odd and on even columns and rows
    H, W = 12, 20
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    x1 = np.where(np.isfinite(xm[1]), xs + xm[1], 0)
    half = x1 - np.floor(x1) == 0.5
    assert (np.floor(x1[half]) % 2 == 0).any() and (np.floor(x1[half]) % 2 == 1).any()
    y1 = np.where(np.isfinite(ym[1]), ys + ym[1], 0)
    half = y1 - np.floor(y1) == 0.5
    assert (np.floor(y1[half]) % 2 == 0).any() and (np.floor(y1[half]) % 2 == 1).any()
    # pixels leave on every side
    assert (x1 < -0.5).any() and (x1 > W - 0.5).any()
    assert (y1 < -0.5).any() and (y1 > H - 0.5).any()


@pytest.mark.parametrize('case', [c[0] for c in ec.ERROR_CASES])
@pytest.mark.parametrize('variant', ec.ERROR_VARIANTS, ids=lambda v: v[0])
def test_restatement_reproduces_the_reference_error(golden, case, variant):
    vname, is_car, is_dense = variant
    gt, pred = golden[f'err_{case}_gt'], golden[f'err_{case}_pred']
    count = golden[f'err_{case}_count']
    aee, pct, n = ec.flow_error64(gt, pred, count, is_car, is_dense)
    want = golden[f'err_{case}_{vname}']
    assert n == int(want[2])
    if n == 0:
        assert np.isnan(aee) and np.isnan(want[0]) and pct == 0.0 == want[1]
    else:
        assert abs(aee - want[0]) <= 5e-6 * abs(want[0])
        assert pct == want[1]       # exact counts, the same float64 quotient


def test_restatement_reproduces_the_reference_evaluate(golden):
    crop = ec.ImageCrop(ec.EVAL_BOX)
    ev_crop = ec.EventCrop(ec.EVAL_BOX)
    frames = golden['eval_frames']
    rows = []
    for i, (e, a, b) in enumerate(ec.frame_generator(list(golden['eval_events']), frames)):
        e = ev_crop(np.array(e).T).T
        gt = crop(np.dstack(ec.propagate64(golden['eval_x_maps'], golden['eval_y_maps'],
                                           golden['eval_ts'], a, b)))
        rows.append(ec.flow_error64(gt, golden['eval_flows'][i],
                                    ec.get_count_image(e, gt.shape[:2])))
    rows, want = np.array(rows), golden['eval_frame_results']
    assert np.array_equal(rows[:, 2], want[:, 2]) and (want[:, 2] > 0).all()
    np.testing.assert_allclose(rows[:, 0], want[:, 0], rtol=5e-6, atol=0)
    np.testing.assert_allclose(rows[:, 1], want[:, 1], rtol=0, atol=1e-9)
    np.testing.assert_allclose(rows[:, :2].mean(0), golden['eval_mean'], rtol=5e-6)


@pytest.mark.parametrize('f', range(len(ec.PROP_FRAMES)), ids=[p[0] for p in ec.PROP_FRAMES])
def test_planner_reproduces_the_reference_step_lists(golden, f):
    """direct mode, start on a timestamp, end on one, spans of 1 and 3 gaps:
    map indices and scale factors exactly as the reference's run used them."""
    start, stop = golden['prop_frames'][f]
    mode, maps, scales = dev_eval.plan_gt_steps(golden['prop_ts'], start, stop)
    assert mode == int(golden[f'plan_mode{f}'])
    assert maps == golden[f'plan_maps{f}'].tolist()
    assert scales == golden[f'plan_scales{f}'].tolist()


def test_planner_edges_against_literals():
    ts = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    plan = dev_eval.plan_gt_steps
    assert plan(ts, 1.25, 1.5) == (1, [1, 1], [0.25, 1.0])
    # a start ON a timestamp belongs to the gap it opens (side='right')
    assert plan(ts, 1.0, 2.5) == (0, [1, 2], [1.0, 0.5])
    # an end ON a timestamp closes with a full last step (strict <), not a zero one
    assert plan(ts, 0.5, 3.0) == (0, [0, 1, 2], [0.5, 1.0, 1.0])
    # dt == gt_dt is NOT the direct branch (strict >)
    assert plan(ts, 0.5, 1.5) == (0, [0, 1], [0.5, 0.5])
    with pytest.raises(ValueError):
        plan(ts, -1.0, 0.5)
    with pytest.raises(IndexError):
        plan(ts, 3.5, 5.5)


def test_step_table_layout():
    plans = [(1, [4, 4], [0.25, 1.0]), (0, [4, 5, 6], [0.5, 1.0, 0.75])]
    begin, maps, scales, mode = dev_eval.step_table(plans, map_offset=4)
    assert begin.tolist() == [0, 2, 5] and begin.dtype == np.int32
    assert maps.tolist() == [0, 0, 0, 1, 2] and maps.dtype == np.int32
    assert scales.tolist() == [0.25, 1.0, 0.5, 1.0, 0.75] and scales.dtype == np.float64
    assert mode.tolist() == [1, 0] and mode.dtype == np.int32


def test_derived_values():
    res = np.zeros(3, dev_eval.RESULT_DTYPE)
    res['sum_ee'], res['n_points'], res['n_below'] = [6.0, 0.0, 1.0], [4, 0, 3], [2, 0, 3]
    aee, pct = dev_eval.derive(res)
    assert aee[0] == 1.5 and np.isnan(aee[1]) and aee[2] == 1.0 / 3
    assert pct.tolist() == [2 / (4 + 1e-5), 0.0, 3 / (3 + 1e-5)]


def test_frame_generator_against_literals():
    t = np.array([0.0, 1.0, 1.0, 2.0, 3.0, 5.0])
    events = [np.arange(6), np.arange(6) + 10, t, np.ones(6)]
    got = list(testing.frame_generator(events, [(1.0, 3.0), (0.5, 0.75), (3.0, 9.0)]))
    # side='right' on both ends: events AT start are out, events AT stop are in
    assert [g[0][0].tolist() for g in got] == [[3, 4], [], [5]]
    assert [g[0][1].tolist() for g in got] == [[13, 14], [], [15]]
    assert [(g[1], g[2]) for g in got] == [(1.0, 3.0), (0.5, 0.75), (3.0, 9.0)]


def test_ravel_config_against_literals():
    cfg = dict(start=[0, 5], stop=None, step=1, test_shape=[256, 256],
               crop_type='central', is_car=[False, True])
    got = list(testing.ravel_config(cfg))
    assert [(c.start, c.is_car) for c in got] == [(0, False), (0, True), (5, False), (5, True)]
    assert all(c.test_shape == [256, 256] and c.stop is None and c.step == 1
               and c.crop_type == 'central' for c in got)
    cfg['test_shape'] = [[256, 256], [128, 128]]
    assert [c.test_shape for c in testing.ravel_config(cfg)][:4:2] == [[256, 256], [128, 128]]


def test_read_config(tmp_path):
    p = tmp_path / 'c.yml'
    p.write_text('start: 1\nis_car: [true, false]\n')
    assert testing.read_config(p) == {'start': 1, 'is_car': [True, False]}


def test_read_config_lets_a_yaml_error_through(tmp_path):
    import yaml
    p = tmp_path / 'bad.yml'
    p.write_text('start: [1, 2\n')
    with pytest.raises(yaml.YAMLError):
        testing.read_config(p)


def test_evaluate_refuses_an_empty_frame_list():
    gt = dict(timestamps=np.arange(3.0), x_flow_dist=np.zeros((3, 4, 4)),
              y_flow_dist=np.zeros((3, 4, 4)))
    events = [np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0)]
    with pytest.raises(ValueError, match='at least one frame'):
        testing.evaluate(lambda e, a, b: None, events, [], gt)


def test_box_folding_against_literals():
    fold = testing.fold_box
    assert fold(ec.EventCrop([2, 3, 32, 64]), (37, 70)) == (2, 3, 32, 64)
    assert fold(ec.ImageCrop((0, 0, 37, 70)), (37, 70)) == (0, 0, 37, 70)
    assert fold(ec.ImageCrop(np.array([5, 6, 32, 64])), (37, 70)) == (5, 6, 32, 64)
    assert fold(None, (37, 70)) is None
    assert fold(ec.Opaque(ec.ImageCrop([2, 3, 32, 64])), (37, 70)) is None
    assert fold(lambda a: a, (37, 70)) is None
    # a box that leaves the frame is not folded: numpy slicing would clip it,
    # the host path keeps that behaviour
    assert fold(ec.ImageCrop([6, 3, 32, 64]), (37, 70)) is None
    assert fold(ec.ImageCrop([2, -1, 32, 64]), (37, 70)) is None
    assert fold(ec.ImageCrop([2.5, 3, 32, 64]), (37, 70)) is None


def test_eval_modules_have_no_cpu_fallback():
    import torch
    z = torch.zeros
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        dev_eval.flow_error(z(1, 4, 4), z(1, 4, 4), z(1, 2, 4, 4))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        dev_eval.propagate(z(2, 4, 4), z(2, 4, 4), [(0, [0, 1], [0.5, 0.5])])
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        dev_eval.count_image_batched(z(3, dtype=torch.long), z(3, dtype=torch.long),
                                     [0, 3], (4, 4))
