"""Learnable event representation on the GPU (docs/LEARNED_VOXEL_SPEC.md):
forward and table gradient against the numpy restatement
(tests/learned_voxel_cases.py), the first layer's data gradient against float64
autograd, and the wiring through predictor, optimizers and train()."""
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

from tests import learned_voxel_cases as lc
from tests import voxel_cases as vc

pytestmark = pytest.mark.gpu

CONV_RTOL = 1e-4        # the per-layer conv tolerance of tests/test_gpu_conv.py


def _dev(ev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in ev.items()}


def _windows(c):
    return torch.from_numpy(c.t0).cuda(), torch.from_numpy(c.t1).cuda()


def _compactable(name, c):
    return name not in lc.WIRE_ONLY and vc.compactable(c.ev, c.B)


def _forward(c, ev, theta=None):
    from dvs_of_training_framework_amd import learned_voxel as lv
    t0, t1 = _windows(c)
    th = torch.from_numpy(c.theta if theta is None else theta).cuda()
    return lv.voxelize(ev, t0, t1, th, c.R, c.S, c.B, c.C, c.H, c.W)


@pytest.fixture(scope='module')
def restated():
    """Case, forward restatement, one grid gradient and its backward restatement:
    computed once per case, shared and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            c = lc.CASES[name]()
            fw = lc.learned_forward(c.ev, c.t0, c.t1, c.theta, c.R, c.S, c.B, c.C, c.H, c.W)
            gV = np.random.default_rng(11).standard_normal((c.B, c.C, c.H, c.W)).astype(np.float32)
            bw = lc.learned_backward(c.ev, c.t0, c.t1, gV, c.R, c.S, c.B, c.C, c.H, c.W)
            cache[name] = (c, fw, gV, bw)
        return cache[name]
    return get


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize('name', sorted(lc.CASES))
def test_forward_against_the_restatement(name, restated):
    """Per voxel within k * 2^-24 * sum|w| + ulp/2 (float32 sum of k addends in
    any order against the float64 sum rounded once; the weights themselves are
    bit-exact: tests/test_gpu_voxel_exact.py's derivation with |w| <= max|theta|).
    Wire and compact columns, each against the restatement; two sums within the
    bound of the same value are within twice the bound of each other."""
    c, fw, _, _ = restated(name)
    got = _forward(c, _dev(c.ev)).cpu().numpy()
    bound = lc.forward_bound(fw, got)
    err = np.abs(got.astype(np.float64).ravel() - fw.acc)
    print(name, 'wire: max err', err.max(initial=0), 'max bound', bound.max(initial=0))
    assert (err <= bound).all()
    assert not got.ravel()[fw.k == 0].any()            # untouched voxels: exactly 0
    if c.ev['x'].size:
        assert np.count_nonzero(got) > 100
    if not _compactable(name, c):
        assert name in lc.WIRE_ONLY or c.ev['x'].size == 0
        return
    enc = _forward(c, _dev(vc.compact(c.ev, c.B))).cpu().numpy()
    err = np.abs(enc.astype(np.float64).ravel() - fw.acc)
    assert (err <= lc.forward_bound(fw, enc)).all()
    assert (np.abs(enc.astype(np.float64) - got).ravel() <= bound + lc.forward_bound(fw, enc)).all()


def test_initial_theta_dyadic_is_the_fixed_voxel_grid_bitwise():
    from dvs_of_training_framework_amd import voxel
    c = lc.dyadic_case()
    ev, (t0, t1) = _dev(c.ev), _windows(c)
    want = voxel.voxelize(ev, t0, t1, c.B, c.C, c.H, c.W)
    assert torch.equal(_forward(c, ev), want)
    assert torch.equal(_forward(c, _dev(vc.compact(c.ev, c.B))), want)
    assert int(want.count_nonzero()) > 1000


def _batch(B, H, W, n=1500, seed=7, dyadic=False):
    from dvs_of_training_framework_amd import synthetic
    b = synthetic.make_batch(seed, B, H, W, n)
    if dyadic:      # window [0, 2^-5], timestamps j * 2^-13 (sorted per sample): tn = j / 64 at C = 5
        rng = np.random.default_rng(seed)
        j = np.sort(rng.integers(0, 257, (B, n)), axis=1).ravel()
        b['events']['timestamp'] = j.astype(np.float32) * np.float32(2.0 ** -13)
        b['timestamps'] = np.tile(np.array([0, 2.0 ** -5], np.float32), B)
    return synthetic.to_torch(b, 'cuda')


def test_untrained_learnable_model_predicts_what_the_default_model_predicts():
    from dvs_of_training_framework_amd.net import Model
    torch.manual_seed(3)
    B, H, W, C = 2, 32, 32, 5
    plain = Model('cuda', event_representation_depth=C)
    learn = Model('cuda', event_representation_depth=C, learnable_representation=True)
    assert [k for k in learn.state_dict() if not k.startswith('predictor.')] == \
        ['quantization_layer.kernel']
    assert list(plain.state_dict()) == [k for k in learn.state_dict() if k.startswith('predictor.')]
    learn.predictor.load_state_dict(plain.predictor.state_dict())
    b = _batch(B, H, W, dyadic=True)
    with torch.no_grad():
        # (the grids are compared first: the premise of the comparison of the flows)
        g0 = plain.quantize(b['events'], b['timestamps'], b['sample_idx'], (H, W))
        g1 = learn.quantize(b['events'], b['timestamps'], b['sample_idx'], (H, W))
        f0 = plain(b['events'], b['timestamps'], b['sample_idx'], (H, W))[0]
        f1 = learn(b['events'], b['timestamps'], b['sample_idx'], (H, W))[0]
    assert torch.equal(g0, g1) and int(g0.count_nonzero()) > 1000
    for u, v in zip(f0, f1):
        assert torch.equal(u, v)


# ----------------------------------------------------------------- backward
@pytest.mark.parametrize('name', sorted(lc.CASES))
def test_table_gradient_against_the_restatement(name, restated):
    """kernel.grad through the autograd function: per knot within
    m * 2^-24 * sum|terms_j| of the float64 restatement (m: the spec's longest
    chain), untouched knots exactly 0, two runs bitwise equal, compact columns
    the same bits as wire columns (the same terms in the same order)."""
    from dvs_of_training_framework_amd.net import LearnedVoxelGrid
    from dvs_of_training_framework_amd import learned_voxel as lv
    c, _, gV, bw = restated(name)
    layer = LearnedVoxelGrid(c.C, c.R, c.S).cuda()
    with torch.no_grad():
        layer.kernel.copy_(torch.from_numpy(c.theta))
    ev, (t0, t1) = _dev(c.ev), _windows(c)
    g = torch.from_numpy(gV).cuda()

    def run(events):
        layer.kernel.grad = None
        layer(events, t0, t1, c.B, c.H, c.W).backward(g)
        return layer.kernel.grad.clone()
    got = run(ev)
    n = c.ev['x'].size
    m = lc.chain(n, c.S)
    assert m == lv.reduction_chain(n, c.S)
    bound = m * 2.0 ** -24 * bw.absterms
    err = np.abs(got.cpu().numpy().astype(np.float64) - bw.gtheta)
    print(name, 'm', m, 'max err', err.max(), 'max bound', bound.max())
    assert (err <= bound).all()
    assert not got.cpu().numpy()[bw.absterms == 0].any()
    if n == 0:
        assert not got.any()
    else:
        assert int(got.count_nonzero()) > 2
    assert torch.equal(run(ev), got)
    if _compactable(name, c):
        assert torch.equal(run(_dev(vc.compact(c.ev, c.B))), got)


def test_knots_no_event_reaches_have_an_exactly_zero_gradient():
    """Every event at t0: tn = 0, bin c sees offset -c, so only the knots at
    offsets 0, -1 and -2 are touched (and their upper neighbours with g = 0)."""
    from dvs_of_training_framework_amd import learned_voxel as lv
    c = lc.CASES['r2s8_init']()
    ev = {k: v.copy() for k, v in c.ev.items()}
    ev['timestamp'] = c.t0[ev['sample_index']]
    gV = np.random.default_rng(5).standard_normal((c.B, c.C, c.H, c.W)).astype(np.float32)
    bw = lc.learned_backward(ev, c.t0, c.t1, gV, c.R, c.S, c.B, c.C, c.H, c.W)
    touched = np.flatnonzero(bw.absterms)
    assert set(touched) <= {0, 8, 16} and touched.size == 3
    t0, t1 = _windows(c)
    got = lv.voxelize_bwd(_dev(ev), t0, t1, c.R, c.S, torch.from_numpy(gV).cuda()).cpu().numpy()
    assert not got[bw.absterms == 0].any() and got[touched].all()
    bound = lc.chain(ev['x'].size, c.S) * 2.0 ** -24 * bw.absterms
    assert (np.abs(got.astype(np.float64) - bw.gtheta) <= bound).all()


def test_no_grad_runs_the_forward_only():
    from dvs_of_training_framework_amd.net import LearnedVoxelGrid
    c = lc.CASES['r2s1']()
    layer = LearnedVoxelGrid(c.C, c.R, c.S).cuda()
    ev, (t0, t1) = _dev(c.ev), _windows(c)
    with torch.no_grad():
        out = layer(ev, t0, t1, c.B, c.H, c.W)
    assert not out.requires_grad and out.grad_fn is None
    assert layer(ev, t0, t1, c.B, c.H, c.W).requires_grad


# ------------------------------------------------- first layer data gradient
def _first_dgrad_reference(gz, w):
    """float64 autograd through conv2d on the CPU."""
    B, Ho, Wo, _ = gz.shape
    x = torch.zeros(B, w.shape[1], 2 * Ho, 2 * Wo, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(x, w.detach().cpu().double().contiguous(), stride=2, padding=1)
    y.backward(gz.detach().cpu().double().permute(0, 3, 1, 2))
    return x.grad


def _close(got, want, rtol=CONV_RTOL):
    err = (got.detach().cpu().double() - want).abs().max().item()
    ref = want.abs().max().item()
    print('max err', err, 'of', ref)
    assert ref > 0 and err <= rtol * ref, (err, ref)


@pytest.mark.parametrize('H,W', [(16, 32), (48, 16)])
@pytest.mark.parametrize('C', [3, 5, 9, 16])
def test_first_dgrad_against_float64_autograd(C, H, W):
    from dvs_of_training_framework_amd import conv
    g = torch.Generator().manual_seed(100 * C + H)
    B = 2
    gz = torch.randn(B, H // 2, W // 2, 64, generator=g).cuda()
    w = torch.randn(64, C, 3, 3, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    got = conv.first_dgrad(gz, w, B, C, H, W)
    _close(got, _first_dgrad_reference(gz, w))
    assert torch.equal(conv.first_dgrad(gz, w, B, C, H, W), got)


# -------------------------------------------------------------------- wiring
def _args(*extra):
    from dvs_of_training_framework_amd import options
    parser = options.add_train_arguments(ArgumentParser())
    return options.validate_train_args(parser.parse_args(
        ['-m', 'unused', '--flownet_path', 'dvs_of_training_framework_amd', '--height', '32',
         '--width', '32', '--event-representation-depth', '5', '-bs', '2', '-mbs', '2',
         '--learnable-representation'] + list(extra)))


@pytest.mark.parametrize('mish', [False, True])
def test_one_eager_step_routes_the_gradient_to_the_table(mish, monkeypatch):
    """grid.grad is the data gradient of enc.0 applied to the tensor its weight
    gradient consumes (checked against float64 autograd through conv2d, so the
    convention -- act' already applied -- is checked with it: the parameter
    gradient of enc.0 must come out of the same tensor); kernel.grad is the
    backward kernel applied to grid.grad, bitwise."""
    from dvs_of_training_framework_amd import conv, learned_voxel as lv, predictor
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.model import init_model
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    torch.manual_seed(9)
    B, H, W = 2, 32, 32
    model = init_model(_args(*(['--mish'] if mish else [])), torch.device('cuda'))
    assert type(model.quantization_layer).__name__ == 'LearnedVoxelGrid'
    model.train()
    seen = {}
    real = conv.first_dgrad

    def spy(gz, weight, *shape):
        seen['gz'] = gz.clone()
        return real(gz, weight, *shape)
    monkeypatch.setattr(predictor.C, 'first_dgrad', spy)

    def keep(module, inputs, output):
        if output.requires_grad:
            output.retain_grad()
            seen['grid'], seen['inputs'] = output, inputs
    model.quantization_layer.register_forward_hook(keep)
    ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
    loss, _, _ = process_minibatch(model, _batch(B, H, W), FakeTimer(), 'cuda', True, ev, [0.5, 1, 1])
    loss.backward()
    grid, w = seen['grid'], model.predictor.enc[0].conv.weight
    assert grid.grad is not None and float(grid.grad.abs().max()) > 0
    _close(grid.grad, _first_dgrad_reference(seen['gz'], w))
    # the same tensor gives enc.0's weight gradient: d/d(pre-activation), for ReLU and Mish
    x = grid.detach().cpu().double()
    wd = w.detach().cpu().double().contiguous().requires_grad_(True)
    torch.nn.functional.conv2d(x, wd, stride=2, padding=1).backward(
        seen['gz'].cpu().double().permute(0, 3, 1, 2))
    _close(w.grad, wd.grad)
    events, t0, t1 = seen['inputs'][:3]
    kernel = model.quantization_layer.kernel
    assert torch.equal(kernel.grad, lv.voxelize_bwd(events, t0, t1, 2, 8, grid.grad))
    assert int(kernel.grad.count_nonzero()) > 8


@pytest.mark.parametrize('fuse', [False, True])
@pytest.mark.parametrize('opt_name', ['ADAM', 'RANGER'])
def test_table_is_frozen_until_rs_and_then_follows_the_optimizer(opt_name, fuse):
    """Four steps, the boundary after the second (training_steps * rs = 1, the
    factor is 0 while step <= 1): knots bit-identical to their initial values
    before it; afterwards FusedAdamW follows torch.optim.AdamW and FusedRanger
    the restated Ranger (oracle/ref_optim.py) fed with the same gradients, at
    the tolerances tests/test_gpu_model.py uses for them -- with and without
    the predictor's update fused into the backward (the knots are in no
    predictor bucket: step() updates them on the step boundary)."""
    import train_flownet as tf
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.model import init_model
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    from oracle.ref_optim import RefRanger
    torch.manual_seed(4)
    B, H, W = 2, 32, 32
    args = _args('--optimizer', opt_name, '-ne', '4', '--representation-start', '0.25',
                 '-lr', '1e-2', '--half_life', '8')
    model = init_model(args, torch.device('cuda'))
    model.train()
    optimizer, scheduler = tf.construct_train_tools(args, model)
    assert type(optimizer).__name__ == ('FusedAdamW' if opt_name == 'ADAM' else 'FusedRanger')
    assert len(optimizer.param_groups) == 2
    if fuse:
        optimizer.fuse_into_backward(model.predictor)
    kernel = model.quantization_layer.kernel
    assert optimizer.param_groups[0]['params'][0] is kernel
    initial = kernel.detach().clone()
    ref = initial.cpu().clone().requires_grad_(True)
    if opt_name == 'ADAM':
        ref_opt = torch.optim.AdamW([ref], lr=args.lr, weight_decay=args.wdw, amsgrad=True)
    else:
        ref_opt = RefRanger([ref], lr=args.lr, weight_decay=args.wdw)
    ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
    enc0 = model.predictor.enc[0].conv.weight
    for step in range(4):
        before = enc0.detach().clone()
        loss, _, _ = process_minibatch(model, _batch(B, H, W, seed=20 + step), FakeTimer(), 'cuda',
                                       True, ev, [0.5, 1, 1])
        loss.backward()
        model.strict = False
        lr = optimizer.param_groups[0]['lr']
        assert (lr == 0) == (step <= 1)
        ref.grad = kernel.grad.detach().cpu().clone()
        if opt_name == 'ADAM':
            ref_opt.param_groups[0]['lr'] = lr
        else:
            ref_opt.lr = lr
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        scheduler.step()
        ref_opt.step()
        assert not torch.equal(before, enc0)        # the predictor trains from step 0
        if step <= 1:
            assert torch.equal(kernel.detach(), initial)
            continue
        got, want = kernel.detach().cpu(), ref.detach()
        err = (got - want).abs().max()
        if opt_name == 'ADAM':
            assert err <= 2e-6 * want.abs().max(), (step, float(err))
        else:
            assert err <= 5e-6 * want.abs().max() + 1e-7, (step, float(err))
        # the knots moved, as far as the reference's did (how far depends on the optimizer:
        # Ranger's first steps are un-rectified momentum steps, lr * m / (1 - beta1^t))
        moved = float((got - initial.cpu()).abs().max())
        ref_moved = float((want - initial.cpu()).abs().max())
        print(opt_name, fuse, 'step', step, 'moved', moved, 'reference moved', ref_moved, 'err', float(err))
        assert ref_moved > 0 and moved > 0
        assert abs(moved - ref_moved) <= (2e-6 if opt_name == 'ADAM' else 5e-6) * float(want.abs().max()) + 1e-7


def test_capture_is_refused_and_the_loop_trains_eagerly(capsys):
    import train_flownet as tf
    from dvs_of_training_framework_amd import synthetic, training
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.model import init_model
    from dvs_of_training_framework_amd.timer import FakeTimer
    torch.manual_seed(6)
    B, H, W = 2, 32, 32
    args = _args('--optimizer', 'ADAM', '-ne', '2', '--representation-start', '0')
    model = init_model(args, torch.device('cuda'))
    optimizer, scheduler = tf.construct_train_tools(args, model)
    ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
    kernel = model.quantization_layer.kernel
    initial = kernel.detach().clone()
    loader = (synthetic.to_torch(synthetic.make_batch(30 + i, B, H, W, 1500)) for i in range(3))
    capsys.readouterr()
    training.train(model, 'cuda', loader, optimizer, num_steps=2, scheduler=scheduler,
                   logger=None, evaluator=ev, timers=FakeTimer(), capture=True,
                   max_events_per_batch=10 ** 6)
    lines = [ln for ln in capsys.readouterr().err.splitlines() if ln.startswith('capture:')]
    assert len(lines) == 1 and 'event representation has parameters' in lines[0]
    # step 0 has factor 0 (step > 0 starts the representation), step 1 moves the knots
    assert not torch.equal(kernel.detach(), initial)
    assert bool(torch.isfinite(kernel).all())
