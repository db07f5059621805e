"""The contrast-maximisation term without a GPU (docs/CONTRAST_SPEC.md): the
numpy restatement loss.contrast_fwd_host / contrast_bwd_host, which the
kernels are pinned to byte for byte (tests/test_gpu_contrast.py), against an
independent torch float64 definition whose gradient autograd takes, within
the bounds the spec derives; the exact identities; the sign of the gradient
on a translating pattern; and the host plumbing of --contrast-weight."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import loss as L, options, training
from tests import contrast_cases as cc

_done = {}


def run(name):
    """(case, restatement forward, gradient, fixed-point sums, oracle), once per case."""
    if name not in _done:
        c = cc.case(name)
        fwd = L.contrast_fwd_host(*cc.args_of(c))
        grad, sums = L.contrast_bwd_host(*cc.args_of(c), fwd)
        _done[name] = (c, fwd, grad, sums, cc.oracle64(c))
    return _done[name]


# ------------------------------------------------- against the definition
@pytest.mark.parametrize('name', cc.RANDOM_IDS)
def test_restatement_within_the_derived_bounds_of_the_float64_definition(name):
    c, fwd, grad, _, o = run(name)
    assert fwd['count'].sum() > 100 and np.array_equal(fwd['count'], o['count'].astype(np.uint32))
    b_term, b_grad = cc.bounds(c, o)
    err_term, err_grad = abs(float(fwd['term']) - o['term']), np.abs(grad.astype(np.float64) - o['grad'])
    print(name, 'term', float(fwd['term']), 'error', err_term, 'bound', b_term, '| grad max',
          np.abs(o['grad']).max(), 'worst error', err_grad.max(), 'worst error / bound', (err_grad / b_grad).max())
    assert grad.dtype == np.float32 and fwd['term'].dtype == np.float32
    assert err_term <= b_term
    assert (err_grad <= b_grad).all()               # every element, none left out
    # the bounds say something: far below the quantities they bound
    assert b_term < 1e-2 * abs(o['term']) and np.median(b_grad[o['grad'] != 0] / np.abs(o['grad'][o['grad'] != 0])) < 1e-2


def test_weight_and_seed_scale_the_gradient_within_the_bound():
    c, fwd, _, _, o = run('random_16x16_F3')
    grad, _ = L.contrast_bwd_host(*cc.args_of(c), fwd, seed=-1.5, weight=0.25)
    _, b_grad = cc.bounds(c, o, seed=-1.5, weight=0.25)
    assert (np.abs(grad.astype(np.float64) - (-1.5 * 0.25) * o['grad']) <= b_grad).all()


@pytest.mark.parametrize('name', cc.DYADIC_IDS)
def test_dyadic_cases_are_exact(name):
    """tau, u, v on a 2^-4 grid, integer landings included: the float32 warp
    and weights are exact and q is the float64 image times 2^32."""
    c, fwd, _, _, o = run(name)
    scaled = o['image'] * 2.0 ** 32
    assert np.array_equal(scaled, np.round(scaled)) and scaled.max() > 2.0 ** 32
    assert np.array_equal(fwd['q'], scaled.astype(np.int64))
    assert np.array_equal(fwd['count'], o['count'].astype(np.uint32))


# ------------------------------------------------------- exact identities
def test_zero_flow_gives_exactly_zero():
    for name in ('random_5x7_F1', 'random_33x31_F4'):
        c = cc.case(name)
        c = dict(c, flow=np.zeros_like(c['flow']))
        fwd = L.contrast_fwd_host(*cc.args_of(c))
        assert fwd['count'].sum() > 100 and np.array_equal(fwd['q'], fwd['count'].astype(np.int64) << 32)
        assert fwd['term'].tobytes() == np.float32(0).tobytes()
        assert all(v == 0.0 for v in fwd['frame_term'])


def test_frames_without_contrast_contribute_nothing():
    """No events, and the same count on every pixel: var(c) = 0, the frame's
    share of the term is 0 and its gradient is zeros, whatever the flow."""
    base = cc.case('random_5x7_F1')
    h, w = base['shape']
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[:h, :w]
    uniform = dict(x=np.tile(xx.ravel(), 3), y=np.tile(yy.ravel(), 3), s=np.ones(3 * h * w, np.int64),
                   t=rng.uniform(0.3, 0.7, 3 * h * w).astype(np.float32))
    cols = {k: np.concatenate([base[k], uniform[k]]) for k in ('x', 'y', 's', 't')}
    # frame 0: the base case; frame 1: three events on every pixel; frame 2: a sample without events
    c = dict(cols, ts=np.tile(base['ts'], 3), fs=np.array([0, 1, 2], np.int64),
             flow=np.concatenate([base['flow'], rng.normal(0, 2, (2, 2, h, w)).astype(np.float32)]), shape=(h, w))
    fwd = L.contrast_fwd_host(*cc.args_of(c))
    grad, sums = L.contrast_bwd_host(*cc.args_of(c), fwd)
    assert (fwd['count'][1] == 3).all() and not fwd['count'][2].any() and fwd['q'][1].any()
    assert fwd['frame_term'][0] != 0 and fwd['frame_term'][1] == 0.0 and fwd['frame_term'][2] == 0.0
    assert fwd['coef'][1] == 0.0 and fwd['coef'][2] == 0.0
    assert grad[0].any() and not grad[1:].any() and not sums[1:].any()
    alone = L.contrast_fwd_host(*cc.args_of(base))
    assert float(fwd['term']) == pytest.approx(float(alone['term']) / 3, rel=1e-6)


@pytest.mark.parametrize('name', ['random_16x16_F3', 'dyadic_33x31_F4'])
def test_the_order_of_the_events_changes_no_byte(name):
    c, fwd, grad, sums, _ = run(name)
    p = cc.permuted(c)
    fwd_p = L.contrast_fwd_host(*cc.args_of(p))
    grad_p, sums_p = L.contrast_bwd_host(*cc.args_of(p), fwd_p)
    assert np.array_equal(fwd_p['q'], fwd['q']) and np.array_equal(fwd_p['count'], fwd['count'])
    assert fwd_p['result'].tobytes() == fwd['result'].tobytes()
    assert fwd_p['term'].tobytes() == fwd['term'].tobytes()
    assert np.array_equal(sums_p, sums) and grad_p.tobytes() == grad.tobytes()


@pytest.mark.parametrize('name', ['random_16x16_F3', 'random_33x31_F4'])
def test_a_frame_alone_equals_the_frame_in_its_batch(name):
    """q, the statistics and the fixed-point sums of a frame do not depend on
    the batch: the unit is per frame and 1/F is applied after the sums."""
    c, fwd, _, sums, _ = run(name)
    for f in range(len(c['fs'])):
        one = cc.single_frame(c, f)
        fwd1 = L.contrast_fwd_host(*cc.args_of(one))
        _, sums1 = L.contrast_bwd_host(*cc.args_of(one), fwd1)
        assert np.array_equal(fwd1['q'][0], fwd['q'][f]) and np.array_equal(fwd1['count'][0], fwd['count'][f])
        assert fwd1['result'][0].tobytes() == fwd['result'][f].tobytes()
        assert fwd1['unit'][0] == fwd['unit'][f] and fwd1['coef'][0] == fwd['coef'][f]
        assert np.array_equal(sums1[0], sums[f]) and sums[f].any()


def test_sum_sq_in_the_kernels_order_is_a_sum_of_the_same_terms():
    """More than one block and more than one round per thread (400 x 400)."""
    import math
    from dvs_of_training_framework_amd import eval as ev
    rng = np.random.default_rng(1)
    for shape in ((1, 1, 1), (2, 33, 31), (1, 400, 400)):
        q = rng.integers(0, 5 << 32, shape)
        got = ev.iwe_sum_sq_kernel_order(q)
        for f in range(shape[0]):
            exact = math.fsum((int(v) * 2.0 ** -32) ** 2 for v in q[f].ravel())
            assert abs(got[f] - exact) <= q[f].size * 2.0 ** -53 * exact


# ------------------------------------------------------------ sign and use
def test_gradient_steps_on_a_translating_pattern_sharpen_it():
    """Events of a pattern that moves by (3, -2) pixels over the window; a
    constant flow of two parameters, started at half the true one, follows the
    restatement's gradient for twenty steps of 0.25 (a step moves the flow by
    a few hundredths of a pixel: first-order descent).  The term falls at
    every step and the flow ends nearer the true one."""
    true = np.array([3.0, -2.0])
    p = cc.translating_pattern(flow=tuple(true))
    uv = (true / 2).astype(np.float32)
    terms = []
    for step in range(21):
        c = dict(p, flow=cc.constant_flow(p['shape'], uv))
        fwd = L.contrast_fwd_host(*cc.args_of(c))
        terms.append(float(fwd['term']))
        if step == 20:
            break
        grad, _ = L.contrast_bwd_host(*cc.args_of(c), fwd)
        uv = (uv - np.float32(0.25) * grad[0].sum((1, 2))).astype(np.float32)
    print('terms', terms, 'flow', uv)
    assert all(b < a for a, b in zip(terms, terms[1:]))
    assert terms[-1] < 0 < terms[0]
    assert np.linalg.norm(uv - true) < np.linalg.norm(true / 2)


# ------------------------------------------------------------ host plumbing
def _parser():
    from argparse import ArgumentParser
    return options.add_preprocessed_dataset_arguments(options.add_train_arguments(ArgumentParser()))


def test_contrast_weight_parses_and_refuses_what_it_cannot_do():
    a = options.validate_train_args(_parser().parse_args(['-m', '/tmp/m']))
    assert a.contrast_weight == 0.0
    a = options.validate_train_args(_parser().parse_args(['-m', '/tmp/m', '--contrast-weight', '0.25']))
    assert a.contrast_weight == 0.25 and a.is_raw
    # at the default the other flags are what they were
    options.validate_train_args(_parser().parse_args(['-m', '/tmp/m', '--ev_images']))
    options.validate_train_args(_parser().parse_args(['-m', '/tmp/m', '--compact-events']))
    for extra, what in ((['--ev_images'], 'ev_images'), (['--compact-events'], 'compact-events')):
        with pytest.raises(SystemExit, match=what):
            options.validate_train_args(_parser().parse_args(['-m', '/tmp/m', '--contrast-weight', '0.5'] + extra))
    with pytest.raises(SystemExit, match='negative'):
        options.validate_train_args(_parser().parse_args(['-m', '/tmp/m', '--contrast-weight', '-0.5']))


class _Optimizer:
    def begin_capture(self): pass
    def advance(self): pass
    def end_capture(self): pass


def test_capture_refusal_names_the_flag():
    assert training.capture_refusal(_Optimizer(), True) is None
    assert training.capture_refusal(_Optimizer(), True, None, 0.0) is None
    why = training.capture_refusal(_Optimizer(), True, None, 0.25)
    assert '--contrast-weight' in why and '0.25' in why


class _Untouchable:
    """Events that must not be looked at."""

    def __getattribute__(self, name):
        raise AssertionError(f'events.{name} was read')

    def __getitem__(self, key):
        raise AssertionError(f'events[{key!r}] was read')

    def __iter__(self):
        raise AssertionError('events were iterated')


class _Evaluator:
    def __init__(self):
        self.contrast_calls = []

    def __call__(self, flows, *rest, **kw):
        return tuple(tuple(torch.tensor(float(10 * t + k)) for k in range(len(flows))) for t in range(3))

    def contrast(self, flows, flow_ts, flow_sample_idx, events, weight=None):
        self.contrast_calls.append((events, weight))
        return torch.tensor(-0.5 * weight), torch.tensor(-0.5)


def test_combined_loss_leaves_the_events_alone_at_weight_zero():
    flows = (torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 4, 4))
    ev = _Evaluator()
    plain, terms0 = training.combined_loss(ev, flows, None, None, None, None, None, None)
    loss, terms = training.combined_loss(ev, flows, None, None, None, None, None, None, contrast_weight=0.0,
                                         events=_Untouchable())
    assert float(loss) == float(plain) and not ev.contrast_calls
    assert type(terms) is type(terms0) and not hasattr(terms, 'contrast')
    events = {'x': None}
    loss, terms = training.combined_loss(ev, flows, None, None, None, None, None, None, contrast_weight=0.25,
                                         events=events)
    assert ev.contrast_calls == [(events, 0.25)]
    assert float(loss) == float(plain) - 0.125 and float(terms.contrast) == -0.5
    # the [3,K] structure and its reader are what they were
    assert [[float(v) for v in row] for row in terms] == [[float(v) for v in row] for row in terms0]
    back = training.TermReadback(terms)
    assert [list(r) for r in back] == [[0.0, 1.0], [10.0, 11.0], [20.0, 21.0]] and back.contrast() == -0.5
    assert training.TermReadback(terms0).contrast() is None
    with pytest.raises(ValueError, match='raw events'):
        training.combined_loss(ev, flows, None, None, None, None, None, None, contrast_weight=0.25)
    with pytest.raises(ValueError, match='negative'):
        training.combined_loss(ev, flows, None, None, None, None, None, None, contrast_weight=-1.0, events=events)


class _LoopEvaluator:
    """CPU stand-in with the Losses call signature and a contrast term of -0.5."""

    def __call__(self, flows, flow_ts, fsi, images, ts, si):
        return (tuple(f.mean() for f in flows), tuple(2 * f.mean() for f in flows),
                tuple(0 * f.mean() for f in flows))

    def contrast(self, flows, flow_ts, flow_sample_idx, events, weight=None):
        assert events['x'].numel() == events['sample_index'].numel() > 0
        term = -0.5 * flows[-1].mean()
        return term * weight, term.detach()


class _Logger:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, v, x):
        self.rows.append((tag, float(v), x))


def _loader(n):
    from dvs_of_training_framework_amd import synthetic
    return [synthetic.to_torch(synthetic.make_batch(i, 2, 16, 16, 10)) for i in range(n)]


def test_train_and_validate_log_the_term_only_when_it_is_on():
    """The fake network's flows are its one parameter `scale` (1.0), so the
    three terms are 1, 2, 0 on every scale, the loss without the term is 2.5
    and the term is -0.5."""
    import sys
    from pathlib import Path
    from dvs_of_training_framework_amd.timer import FakeTimer
    sys.path.insert(0, str(Path(__file__).parent))
    from fake_flownet.net import Model as Fake
    sys.path.pop(0)
    for weight, loss in ((0.0, 2.5), (0.25, 2.5 - 0.125)):
        log = _Logger()
        training.validate(Fake('cpu'), 'cpu', _loader(2), 7, log, _LoopEvaluator(), contrast_weight=weight)
        vals = {t: v for t, v, _ in log.rows}
        assert vals['General/Validation loss'] == pytest.approx(loss)
        assert vals['Validation/photometric loss/2x2'] == pytest.approx(2.0)
        assert ('Validation/contrast' in vals) == (weight > 0)
        model = Fake('cpu')
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
        log = _Logger()
        training.train(model, 'cpu', _loader(4), opt, num_steps=1, scheduler=sch, logger=log,
                       evaluator=_LoopEvaluator(), accumulation_steps=2, timers=FakeTimer(),
                       max_events_per_batch=10 ** 6, contrast_weight=weight)
        vals = {t: v for t, v, _ in log.rows}
        assert vals['General/Train loss'] == pytest.approx(loss)
        assert vals['Train/smoothness loss/16x16'] == pytest.approx(1.0)
        assert ('Train/contrast' in vals) == (weight > 0)
        if weight:
            assert vals['Train/contrast'] == pytest.approx(-0.5)
        # d loss / d scale = 2.5 - 0.5 * weight per micro-batch
        assert float(model.scale) == pytest.approx(1 - 0.1 * (2.5 - 0.5 * weight), rel=1e-5)
    with pytest.raises(ValueError, match='raw events'):
        training.process_minibatch(Fake('cpu'), _loader(1)[0], FakeTimer(), 'cpu', False, _LoopEvaluator(),
                                   [0.5, 1, 1], contrast_weight=0.25)
