"""CPU checks of the learnable event representation: the numpy restatement of
docs/LEARNED_VOXEL_SPEC.md against the fixed voxel grid's oracle and against
central differences, and the training front end's wiring (flags, parameter
groups, the representation group's learning rate)."""
from argparse import ArgumentParser

import numpy as np
import pytest
import torch
from torch import nn

import train_flownet as tf
from dvs_of_training_framework_amd import options
from tests import learned_voxel_cases as lc
from tests import voxel_cases as vc

# the fixed voxeliser's own cases, without the multi-million-event ones
SMALL = sorted(n for n in vc.CASES
               if not any(t in n for t in ('ept8', 'ept16', 'grid_stride', 'tiles8')))


@pytest.mark.parametrize('name', SMALL)
def test_initial_theta_is_the_fixed_voxel_grid(name):
    """Dyadic timestamps: bit for bit.  Float timestamps: (tn - c) and (+ R) round
    a value below 8 once each (2 * 2^-22 in bin units; * S is exact), the
    interpolant's slope is at most 1 per bin, its three operations round values
    <= 1 (3 * 2^-24), the oracle's fixed point truncates 2^-32: below 2^-20 per
    addend, plus one ulp for the two final roundings."""
    c = vc.CASES[name]()
    ex = vc.voxel_exact(c.ev, c.t0, c.t1, c.B, c.C, c.H, c.W)
    fw = lc.learned_forward(c.ev, c.t0, c.t1, lc.theta_init(2, 8), 2, 8, c.B, c.C, c.H, c.W)
    if c.dyadic:
        assert np.array_equal(fw.grid, ex.grid)
        return
    bound = ex.k * 2.0 ** -20 + np.spacing(np.abs(ex.grid).ravel())
    assert (np.abs(fw.grid.astype(np.float64) - ex.grid).ravel() <= bound).all()


def test_initial_theta_other_tables():
    """R = 1 and S = 1, 2, 16 are the triangle kernel too (dyadic: exact)."""
    c = vc.CASES['v1_small_dyadic']()
    ex = vc.voxel_exact(c.ev, c.t0, c.t1, c.B, c.C, c.H, c.W)
    for R, S in ((1, 1), (1, 8), (2, 1), (3, 2), (3, 16)):
        fw = lc.learned_forward(c.ev, c.t0, c.t1, lc.theta_init(R, S), R, S, c.B, c.C, c.H, c.W)
        assert np.array_equal(fw.grid, ex.grid), (R, S)


@pytest.mark.parametrize('name', sorted(lc.CASES))
def test_backward_is_the_derivative_of_the_forward(name):
    """The forward is linear in theta: central differences of the float64 forward
    are exact to rounding."""
    c = lc.CASES[name]()
    rng = np.random.default_rng(1)
    gV = rng.standard_normal((c.B, c.C, c.H, c.W))
    bw = lc.learned_backward(c.ev, c.t0, c.t1, gV, c.R, c.S, c.B, c.C, c.H, c.W)
    theta, h = c.theta.astype(np.float64), 1.0
    fd = np.zeros_like(bw.gtheta)
    for j in range(theta.size):
        e = np.zeros_like(theta)
        e[j] = h
        args = (c.R, c.S, c.B, c.C, c.H, c.W)
        d = lc.forward64(c.ev, c.t0, c.t1, theta + e, *args) - \
            lc.forward64(c.ev, c.t0, c.t1, theta - e, *args)
        fd[j] = (gV * d).sum() / (2 * h)
    np.testing.assert_allclose(fd, bw.gtheta, rtol=1e-9, atol=0)
    if c.ev['x'].size == 0:
        assert not bw.gtheta.any()
    else:
        assert np.count_nonzero(bw.gtheta) > 2


def test_cases_cover_what_they_name():
    c = lc.CASES['edges_r2s8']()
    ev = c.ev
    assert (ev['polarity'] == 0).any() and (ev['sample_index'] == c.B).any()
    assert np.isnan(ev['timestamp']).any() and ((ev['x'] == -1) & (ev['y'] == -1)).any()
    s = ev['sample_index']
    assert (ev['timestamp'][s == 0] == c.t0[0]).any() and (ev['timestamp'][s == 0] == c.t1[0]).any()
    c = lc.CASES['flat_r1s1']()
    assert c.t0[2] == c.t1[2] and not (c.ev['sample_index'] == 1).any()
    assert lc.CASES['empty']().ev['x'].size == 0
    assert lc.chain(2000, 8) == 8 + 11 and lc.chain(2000, 1) == 16 + 11 and lc.chain(0, 8) == 11
    assert lc.bwd_blocks(1 << 19) == 512 and lc.chain(1 << 20, 8) == 16 + 11


# ---------------------------------------------------------------- front end
def _args(*extra):
    parser = options.add_train_arguments(ArgumentParser())
    return options.validate_train_args(parser.parse_args(
        ['-m', 'unused', '--optimizer', 'ADAM', '-ne', '100', '--half_life', '50',
         '--representation-start', '0.5'] + list(extra)))


class _StandIn(nn.Module):
    """A CPU model with the attributes the train tools split on."""

    def __init__(self, learnable, knots=33):
        super().__init__()
        self.quantization_layer = nn.Module()
        if learnable:
            self.quantization_layer.kernel = nn.Parameter(torch.zeros(knots))
        self.predictor = nn.Linear(3, 2)


def test_flag_reaches_the_model_kwargs():
    kw = options.options2model_kwargs(_args('--learnable-representation',
                                            '--representation-radius', '3',
                                            '--representation-knots', '4'))
    assert kw['learnable_representation'] is True
    assert (kw['representation_radius'], kw['representation_knots']) == (3, 4)
    kw = options.options2model_kwargs(_args('--learnable-representation'))
    assert (kw['representation_radius'], kw['representation_knots']) == (2, 8)


def test_without_the_flag_nothing_changes():
    kw = options.options2model_kwargs(_args())
    assert sorted(kw) == ['activation', 'dynamic_sample_length', 'event_representation_depth',
                          'max_sequence_length', 'prefix_length', 'suffix_length']
    optimizer, _ = tf.construct_train_tools(_args(), _StandIn(False))
    assert len(optimizer.param_groups) == 1 and len(optimizer.param_groups[0]['params']) == 2


def test_representation_group_starts_at_rs():
    args = _args('--learnable-representation')
    model = _StandIn(True)
    optimizer, scheduler = tf.construct_train_tools(args, model)
    assert len(optimizer.param_groups) == 2
    rep, pred = optimizer.param_groups
    assert rep['params'][0] is model.quantization_layer.kernel
    assert rep['weight_decay'] == args.wdw
    pred_scheduler, _ = tf.make_schedulers(args)
    start = args.training_steps * args.rs
    for step in range(100):
        assert pred['lr'] == pytest.approx(args.lr * pred_scheduler(step), rel=1e-12)
        if step <= start:
            assert rep['lr'] == 0
        else:
            assert rep['lr'] == pred['lr'] > 0
        optimizer.step()
        scheduler.step()


def test_model_signature_and_capture_refusal():
    import inspect
    from dvs_of_training_framework_amd import net, training
    p = inspect.signature(net.Model.__init__).parameters
    assert p['learnable_representation'].default is False
    assert (p['representation_radius'].default, p['representation_knots'].default) == (2, 8)
    layer = net.LearnedVoxelGrid(5)
    assert [n for n, _ in layer.named_parameters()] == ['kernel']
    assert np.array_equal(layer.kernel.detach().numpy(), lc.theta_init(2, 8))
    assert np.array_equal(net.LearnedVoxelGrid(3, 3, 5).kernel.detach().numpy(), lc.theta_init(3, 5))

    class Proto:
        begin_capture = advance = end_capture = None
    assert training.capture_refusal(Proto(), True, _StandIn(False)) is None
    assert 'representation' in training.capture_refusal(Proto(), True, _StandIn(True))
