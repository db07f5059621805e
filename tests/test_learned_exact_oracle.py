"""The integer restatement of the order-independent learned forward
(tests/learned_exact_cases.py) against the two restatements it must agree with
(CPU, numpy only): the fixed-point voxel oracle and the float64 learned forward."""
from argparse import ArgumentParser

import numpy as np
import pytest

from tests import learned_exact_cases as le
from tests import learned_voxel_cases as lc
from tests import voxel_cases as vc

RS = ((2, 8), (3, 16), (1, 1))
FAMILIES = ('v1_small', 'ept4', 'depth7', 'frame70x16', 'fill_three_overflows', 'one_pixel',
            'window_edges', 'window_open_end', 'drops', 'all_polarity_zero', 'encoded_gaps')


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_dyadic_input_gives_the_fixed_grid_and_the_float64_grid_bitwise():
    c = lc.dyadic_case()
    ex = le.learned_exact(c.ev, c.t0, c.t1, c.theta, c.R, c.S, c.B, c.C, c.H, c.W)
    fixed = vc.voxel_exact(c.ev, c.t0, c.t1, c.B, c.C, c.H, c.W)
    fw = lc.learned_forward(c.ev, c.t0, c.t1, c.theta, c.R, c.S, c.B, c.C, c.H, c.W)
    assert np.array_equal(bits(ex.grid), bits(fixed.grid))
    assert np.array_equal(bits(ex.grid), bits(fw.grid))
    assert np.array_equal(ex.acc, fixed.acc)        # the same integers, not only the same floats
    assert int(np.count_nonzero(ex.grid)) > 1000 and int(ex.k.max()) >= 2


@pytest.mark.parametrize('name', FAMILIES)
def test_truncation_bound_against_the_float64_sum(name):
    """|A * 2^-32 - acc64| <= k * 2^-32 per voxel (truncation per addend; the
    float64 sum's own rounding, k * 2^-53 * sum|w|, is far below one quantum)."""
    c = vc.CASES[name]()
    for i, (R, S) in enumerate(RS):
        theta = le.random_theta(i, R, S)
        ex = le.learned_exact(c.ev, c.t0, c.t1, theta, R, S, c.B, c.C, c.H, c.W)
        fw = lc.learned_forward(c.ev, c.t0, c.t1, theta, R, S, c.B, c.C, c.H, c.W)
        assert np.array_equal(ex.k, fw.k)
        err = np.abs(ex.acc.astype(np.float64) * 2.0 ** -32 - fw.acc)
        slack = fw.k * 2.0 ** -52 * fw.absw
        assert (err <= fw.k * 2.0 ** -32 + slack).all(), (name, R, S, float(err.max()))
        # ... and the grid inside the bound the GPU test uses, and inside the float-atomics one
        gerr = np.abs(ex.grid.ravel().astype(np.float64) - fw.acc)
        assert (gerr <= le.exact_bound(fw, ex.grid)).all()
        assert (gerr <= lc.forward_bound(fw, ex.grid) + fw.k * 2.0 ** -32).all()
        assert float(fw.absw.max(initial=0.0)) < 2.0 ** 31


def test_negated_polarities_negate_every_sum_exactly():
    c = vc.CASES['drops']()
    theta = le.random_theta(7, 2, 8)
    neg = dict(c.ev, polarity=-c.ev['polarity'])
    a = le.learned_exact(c.ev, c.t0, c.t1, theta, 2, 8, c.B, c.C, c.H, c.W)
    b = le.learned_exact(neg, c.t0, c.t1, theta, 2, 8, c.B, c.C, c.H, c.W)
    assert np.array_equal(a.acc, -b.acc) and np.array_equal(a.absq, b.absq)
    assert np.array_equal(a.grid, -b.grid)
    assert int(np.count_nonzero(a.acc)) > 1000


def test_order_of_the_events_changes_nothing():
    c = vc.CASES['one_pixel']()
    theta = le.random_theta(8, 3, 16)
    a = le.learned_exact(c.ev, c.t0, c.t1, theta, 3, 16, c.B, c.C, c.H, c.W)
    b = le.learned_exact(vc.shuffled(c.ev), c.t0, c.t1, theta, 3, 16, c.B, c.C, c.H, c.W)
    assert np.array_equal(a.acc, b.acc) and int(a.k.max()) > 2000


def test_the_colliding_batch_collides():
    for pad in (None, 4096):
        b = le.colliding_batch(3, pad_to=pad)
        assert b['events']['x'].size == (pad or 3000)
        assert le.collision_share(b) > 0.5
    assert le.collision_share(le.colliding_batch(3)) == le.collision_share(le.colliding_batch(3, pad_to=4096))


def _args(*extra):
    from dvs_of_training_framework_amd import options
    parser = options.add_train_arguments(ArgumentParser())
    return options.validate_train_args(parser.parse_args(
        ['-m', 'unused', '--flownet_path', 'dvs_of_training_framework_amd', '-bs', '2',
         '-mbs', '2'] + list(extra)))


def test_the_switch_reaches_the_model_kwargs_and_needs_the_learnable_layer():
    import inspect
    import train_flownet as tf
    from dvs_of_training_framework_amd import net, options
    kw = options.options2model_kwargs(_args('--learnable-representation',
                                            '--representation-deterministic'))
    assert kw['representation_deterministic'] is True and 'representation_resident' not in kw
    kw = options.options2model_kwargs(_args('--learnable-representation'))
    assert 'representation_deterministic' not in kw
    assert _args().representation_deterministic is False
    with pytest.raises(SystemExit, match='--learnable-representation'):
        _args('--representation-deterministic')
    # ... and the launcher's own check, for arguments that did not come through validate_train_args
    bad = _args('--learnable-representation', '--representation-deterministic')
    bad.learnable_representation = False
    with pytest.raises(SystemExit, match='--representation-deterministic'):
        tf.check_representation_args(bad, 1)
    p = inspect.signature(net.Model.__init__).parameters
    assert p['representation_deterministic'].default is False
    assert inspect.signature(net.LearnedVoxelGrid.__init__).parameters['deterministic'].default is False
    with pytest.raises(AssertionError, match='learnable_representation'):
        net.Model('cpu', event_representation_depth=5, representation_deterministic=True)
    layer = net.Model('cpu', event_representation_depth=5, learnable_representation=True,
                      representation_deterministic=True).quantization_layer
    assert layer.deterministic is True and not layer.capture_ready
