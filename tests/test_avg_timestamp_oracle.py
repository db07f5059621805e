"""CPU: the numpy restatement of docs/AVG_TIMESTAMP_SPEC.md
(loss.avg_timestamp_fwd_host / avg_timestamp_bwd_host), which the kernels are
pinned to byte for byte, against the float64 definition of
tests/avg_timestamp_cases.py within the bounds derived there; and the
properties the spec states: exactly 1 at zero flow, below 1 at the true flow,
0 without events, 1 without a gradient when every event leaves, no order."""
import numpy as np
import pytest

from dvs_of_training_framework_amd import loss as L
from tests import avg_timestamp_cases as ac

_oracles = {}


def oracle(name, mask, pol):
    key = (name, mask, pol)
    if key not in _oracles:
        _oracles[key] = ac.oracle64(ac.case(name), mask, pol)
    return _oracles[key]


@pytest.mark.parametrize('pol', (False, True))
@pytest.mark.parametrize('mask', ac.MASKS)
@pytest.mark.parametrize('name', ac.ORACLE_IDS)
def test_restatement_holds_the_definition_within_the_bounds(name, mask, pol):
    c = ac.case(name)
    o = oracle(name, mask, pol)
    fwd = L.avg_timestamp_fwd_host(*ac.args_of(c), mask, pol)
    grad, _ = L.avg_timestamp_bwd_host(*ac.args_of(c), fwd, seed=-1.5, weight=0.25)
    b_term, b_grad = ac.bounds(c, o, seed=-1.5, weight=0.25)
    assert np.array_equal(fwd['rec']['n'], o['n']) and np.array_equal(fwd['rec']['n0'], o['n0'])
    assert np.array_equal(fwd['count'], o['count'])
    err = abs(float(fwd['term']) - o['term'])
    print(f'{name} mask {mask} pol {pol}: term {o["term"]:.6f} error {err:.3e} bound {b_term:.3e}')
    assert err <= b_term
    diff = np.abs(grad.astype(np.float64) - (-1.5 * 0.25) * o['grad'])
    worst = np.unravel_index(np.argmax(diff / b_grad), diff.shape)
    print(f'  gradient: largest {0.375 * np.abs(o["grad"]).max():.3e}, error nearest its bound {diff[worst]:.3e} '
          f'of {b_grad[worst]:.3e}, largest bound {b_grad.max():.3e}')
    assert (diff <= b_grad).all()
    assert np.abs(o['grad']).max() > 0 and 0 < o['term']


@pytest.mark.parametrize('pol', (False, True))
@pytest.mark.parametrize('mask', ac.MASKS)
def test_zero_flow_gives_exactly_one(mask, pol):
    c = ac.case('random_16x16_F3')
    c = dict(c, flow=np.zeros_like(c['flow']))
    fwd = L.avg_timestamp_fwd_host(*ac.args_of(c), mask, pol)
    assert fwd['count'].reshape(len(fwd['rec']), -1).sum(1).all(), 'every image has events'
    assert (fwd['image_value'] == 1.0).all()
    assert fwd['term'].dtype == np.float32 and fwd['term'] == np.float32(1.0)
    assert np.array_equal(fwd['s'], fwd['base'])
    assert np.array_equal(fwd['q'], fwd['count'].astype(np.int64) << 32)


def test_the_true_flow_of_moving_points_lies_below_one():
    zero, true = ac.moving_points_case()
    at_zero = L.avg_timestamp_fwd_host(*ac.args_of(zero))
    at_true = L.avg_timestamp_fwd_host(*ac.args_of(true))
    assert at_zero['term'] == np.float32(1.0)
    print('moving points, true flow:', at_true['term'])
    assert at_true['term'] < np.float32(1.0), at_true['term']
    wrong = dict(zero, flow=-true['flow'])
    assert L.avg_timestamp_fwd_host(*ac.args_of(wrong))['term'] > at_true['term']


def test_no_events_give_zero_and_events_that_all_leave_give_one_without_a_gradient():
    c = ac.all_leave_case()
    fwd = L.avg_timestamp_fwd_host(*ac.args_of(c), 5, False)
    assert fwd['count'][:2].any() and not fwd['q'][:2].any() and not fwd['count'][2:].any()
    assert list(fwd['image_value']) == [1.0, 1.0, 0.0, 0.0] and not fwd['rec']['k2'].any()
    assert fwd['term'] == np.float32(0.5)
    grad, sums = L.avg_timestamp_bwd_host(*ac.args_of(c), fwd)
    assert not grad.any() and not sums.any()
    o = ac.oracle64(c, 5, False)
    assert o['term'] == 0.5 and not o['grad'].any()


@pytest.mark.parametrize('name', ('random_33x31_F4', 'dyadic_16x16_F3'))
def test_a_permutation_of_the_events_gives_the_same_bytes(name):
    c = ac.case(name)
    a = L.avg_timestamp_fwd_host(*ac.args_of(c), 7, True)
    b = L.avg_timestamp_fwd_host(*ac.args_of(ac.permuted(c)), 7, True)
    for k in ('q', 's', 'base', 'count', 'rows', 'rec', 'unit', 'term'):
        assert a[k].tobytes() == b[k].tobytes(), k
    ga, sa = L.avg_timestamp_bwd_host(*ac.args_of(c), a)
    gb, sb = L.avg_timestamp_bwd_host(*ac.args_of(ac.permuted(c)), b)
    assert ga.tobytes() == gb.tobytes() and np.array_equal(sa, sb) and ga.any()


@pytest.mark.parametrize('mask,pol', ((5, False), (7, True), (2, False)))
def test_q_and_count_are_those_of_the_contrast_term(mask, pol):
    c = ac.case('random_33x31_F4')
    ours = L.avg_timestamp_fwd_host(*ac.args_of(c), mask, pol)
    theirs = L.contrast_multi_fwd_host(*ac.args_of(c), mask, pol)
    assert np.array_equal(ours['q'], theirs['q']) and np.array_equal(ours['count'], theirs['count'])
    assert theirs['q'].any() and (ours['s'] <= ours['q']).all() and ours['s'].any()


def test_the_collapsing_flow_of_the_spec():
    """A report, not a threshold: the value on the sink flow that docs/AVG_TIMESTAMP_SPEC.md
    section 9 quotes, from the float64 definition; the restatement agrees to float32."""
    c = ac.sink_case()
    for mask, name in ((1, 'start'), (2, 'middle'), (4, 'end'), (5, 'start,end')):
        o = ac.oracle64(c, mask, False)
        got = L.avg_timestamp_fwd_host(*ac.args_of(c), mask, False)['term']
        print(f'sink flow, {name}: {o["term"]:.4f}')
        assert abs(float(got) - o['term']) <= 1e-4 * o['term']
