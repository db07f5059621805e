"""The contrast term with several reference times and the polarities apart,
without a GPU (docs/CONTRAST_SPEC.md sections 11-15): the numpy restatement
loss.contrast_multi_fwd_host / contrast_multi_bwd_host, which the kernels of
csrc/contrast.hip are pinned to byte for byte
(tests/test_gpu_contrast_multi.py), against the existing restatement where
the two must agree, against the float64 definition within the derived bounds,
the exact identities (dyadic cases, the mirrored window, the polarities), the
use of the term, and the two flags."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import loss as L, options, training
from tests import contrast_cases as cc, contrast_multi_cases as mc

ALL = [(mask, pol) for mask in mc.MASKS for pol in (False, True)]
_done, _device_cases = {}, {}


def run(name, mask, pol):
    """(case, restatement forward, gradient, fixed-point sums), once per case and options."""
    key = (name, mask, pol)
    if key not in _done:
        c = mc.case(name)
        fwd = L.contrast_multi_fwd_host(*mc.args_of(c), mask, pol)
        grad, sums = L.contrast_multi_bwd_host(*mc.args_of(c), fwd)
        _done[key] = (c, fwd, grad, sums)
    return _done[key]


def same_forward(a, b):
    return np.array_equal(a['q'], b['q']) and np.array_equal(a['count'], b['count']) \
        and a['result'].tobytes() == b['result'].tobytes() and a['term'].tobytes() == b['term'].tobytes()


# ------------------------------------------- the term as it was, by new code
def _old_cases():
    if not _device_cases:
        _device_cases.update({k: cc.case(k) for k in cc.ORACLE_CASES})
        _device_cases.update(cc.device_cases())
    return _device_cases


@pytest.mark.parametrize('name', list(cc.ORACLE_CASES) + list(cc.device_cases()))
def test_start_without_polarity_is_the_existing_restatement_byte_for_byte(name):
    """rho = 0: sig has the bits of tau, b = 0, M = F.  q, count, the rows,
    term, the records, the sums and grad_flow; p is not read (None)."""
    c = _old_cases()[name]
    old = L.contrast_fwd_host(*cc.args_of(c))
    old_grad, old_sums = L.contrast_bwd_host(*cc.args_of(c), old, seed=-1.5, weight=0.25)
    new = L.contrast_multi_fwd_host(c['x'], c['y'], c['t'], None, c['s'], c['ts'], c['fs'], c['flow'])
    grad, sums = L.contrast_multi_bwd_host(c['x'], c['y'], c['t'], None, c['s'], c['ts'], c['fs'], c['flow'], new,
                                           seed=-1.5, weight=0.25)
    assert new['mask'] == 1 and new['R'] == new['C'] == 1
    assert same_forward(old, new)
    for k, k_old in (('mean', 'mean'), ('coef', 'coef'), ('unit', 'unit'), ('image_term', 'frame_term')):
        assert new[k].tobytes() == old[k_old].tobytes(), k
    assert np.array_equal(sums, old_sums) and grad.tobytes() == old_grad.tobytes()
    assert grad.dtype == old_grad.dtype == np.float32 and grad.shape == old_grad.shape


# ------------------------------------------------- against the definition
def test_the_generator_of_the_random_cases_terminates_on_the_committed_seeds():
    for name in cc.RANDOM_IDS:
        c, rounds = mc.make_case(name)
        print(name, 'resampling rounds', rounds)
        assert rounds < 32
        for rho in mc.RHO:
            for p in mc.pairs64(c, rho):
                for a in (p['xw'], p['yw']):
                    assert (np.abs(a - np.round(a)) >= mc.KINK).all()
        assert (c['p'] == 0).any() and (c['p'] > 0).any() and (c['p'] < 0).any()
        assert np.array_equal(c['x'], cc.case(name)['x']) and c['flow'] is cc.case(name)['flow']


_worst = {}


@pytest.mark.parametrize('mask,pol', ALL)
@pytest.mark.parametrize('name', cc.RANDOM_IDS)
def test_restatement_within_the_derived_bounds_of_the_float64_definition(name, mask, pol):
    c, fwd, grad, _ = run(name, mask, pol)
    o = mc.oracle64(c, mask, pol)
    assert fwd['count'].sum() > 100 and np.array_equal(fwd['count'], o['count'].astype(np.uint32))
    b_term, b_grad = mc.bounds(c, o)
    err_term, err_grad = abs(float(fwd['term']) - o['term']), np.abs(grad.astype(np.float64) - o['grad'])
    _worst[name, mask, pol] = max(err_term / b_term, (err_grad / b_grad).max())
    print(name, mask, pol, 'term', float(fwd['term']), 'error / bound', err_term / b_term, '| grad max',
          np.abs(o['grad']).max(), 'worst error / bound', (err_grad / b_grad).max(),
          '| worst share so far', max(_worst.values()))
    assert grad.dtype == np.float32 and fwd['term'].dtype == np.float32
    assert err_term <= b_term
    assert (err_grad <= b_grad).all()               # every element, none left out
    # the bounds say something: far below the quantities they bound
    live = o['grad'] != 0
    assert b_term < 1e-2 * abs(o['term']) and np.median(b_grad[live] / np.abs(o['grad'][live])) < 1e-2


def test_weight_and_seed_scale_the_gradient_within_the_bound():
    c, fwd, _, _ = run('random_16x16_F3', 7, True)
    o = mc.oracle64(c, 7, True)
    grad, _ = L.contrast_multi_bwd_host(*mc.args_of(c), fwd, seed=-1.5, weight=0.25)
    _, b_grad = mc.bounds(c, o, seed=-1.5, weight=0.25)
    assert (np.abs(grad.astype(np.float64) - (-1.5 * 0.25) * o['grad']) <= b_grad).all()


@pytest.mark.parametrize('pol', (False, True))
@pytest.mark.parametrize('name', cc.DYADIC_IDS)
def test_dyadic_cases_are_exact_at_every_reference(name, pol):
    """tau, u, v on a 2^-4 grid and rho on halves: sig, the warp and the
    weights are exact and q is the float64 image times 2^32, image by image."""
    c, fwd, _, _ = run(name, 7, pol)
    o = mc.oracle64(c, 7, pol)
    scaled = o['image'] * 2.0 ** 32
    assert np.array_equal(scaled, np.round(scaled)) and scaled.max() > 2.0 ** 32
    assert np.array_equal(fwd['q'], scaled.astype(np.int64))
    assert np.array_equal(fwd['count'], o['count'].astype(np.uint32))
    R, C = fwd['R'], fwd['C']
    for r in range(R):                              # every reference has an image of its own
        assert fwd['q'].reshape(-1, R, C, *c['shape'])[:, r].any()
    assert not np.array_equal(fwd['q'][0], fwd['q'][C])


@pytest.mark.parametrize('name', cc.DYADIC_IDS)
def test_a_mirrored_window_swaps_start_and_end(name):
    """t -> t0 + t1 - t and flow -> -flow, frame by frame: the events warped
    to the end of the window are then the events warped to its start, byte for
    byte, and the middle maps to the middle."""
    c = mc.case(name)
    seen = 0
    for f in range(len(c['fs'])):
        one = cc.single_frame(c, f)
        back = mc.mirrored(one)
        a = L.contrast_multi_fwd_host(*mc.args_of(one), 7, True)
        b = L.contrast_multi_fwd_host(*mc.args_of(back), 7, True)
        q_a, q_b = a['q'].reshape(3, 2, *c['shape']), b['q'].reshape(3, 2, *c['shape'])
        assert np.array_equal(q_a[2], q_b[0]) and np.array_equal(q_a[0], q_b[2]) and np.array_equal(q_a[1], q_b[1])
        assert np.array_equal(a['count'], b['count'])
        assert not np.array_equal(q_a[0], q_a[2])
        seen += int(a['count'].sum())
    assert seen > 100


# ------------------------------------------------------------- polarities
@pytest.mark.parametrize('name', ['random_16x16_F3', 'dyadic_33x31_F4'])
def test_a_channel_is_the_unseparated_image_of_its_events(name):
    c, fwd, _, _ = run(name, 7, True)
    F, (h, w) = len(c['fs']), c['shape']
    q, count = fwd['q'].reshape(F, 3, 2, h, w), fwd['count'].reshape(F, 3, 2, h, w)
    rows = fwd['result'].reshape(F, 3, 2)
    for ch, keep in enumerate((c['p'] > 0, c['p'] < 0)):
        part = L.contrast_multi_fwd_host(*mc.args_of(mc.restricted(c, keep)), 7, False)
        assert np.array_equal(part['q'].reshape(F, 3, h, w), q[:, :, ch])
        assert np.array_equal(part['count'].reshape(F, 3, h, w), count[:, :, ch])
        assert part['result'].reshape(F, 3).tobytes() == np.ascontiguousarray(rows[:, :, ch]).tobytes()
        assert part['count'].sum() > 100
    # the count image is the same bytes for every reference
    assert all(np.array_equal(count[:, 0], count[:, r]) for r in (1, 2))


def test_an_event_of_polarity_zero_changes_no_byte():
    c, fwd, grad, sums = run('random_16x16_F3', 5, True)
    assert (c['p'] == 0).sum() > 50
    d = mc.restricted(c, c['p'] != 0)
    fwd_d = L.contrast_multi_fwd_host(*mc.args_of(d), 5, True)
    grad_d, sums_d = L.contrast_multi_bwd_host(*mc.args_of(d), fwd_d)
    assert same_forward(fwd, fwd_d) and np.array_equal(sums, sums_d) and grad.tobytes() == grad_d.tobytes()
    # without polarity the same events do take part
    plain = L.contrast_multi_fwd_host(*mc.args_of(c), 5, False)
    assert plain['count'].sum() > fwd['count'].sum()
    assert np.array_equal(plain['count'][0::2], plain['count'][1::2])      # R = 2: the count image twice per frame


# ------------------------------------------------------- exact identities
@pytest.mark.parametrize('mask,pol', [(7, True), (2, False)])
def test_zero_flow_gives_exactly_zero(mask, pol):
    for name in ('random_5x7_F1', 'random_33x31_F4'):
        c = mc.case(name)
        c = dict(c, flow=np.zeros_like(c['flow']))
        fwd = L.contrast_multi_fwd_host(*mc.args_of(c), mask, pol)
        assert fwd['count'].sum() > 100 and np.array_equal(fwd['q'], fwd['count'].astype(np.int64) << 32)
        assert fwd['term'].tobytes() == np.float32(0).tobytes()
        assert all(v == 0.0 for v in fwd['image_term'])


def test_images_without_contrast_contribute_nothing():
    """No events, and the same count on every pixel of a channel: var(c) = 0,
    the image's share of the term is 0 and it adds nothing to the sums."""
    base = mc.case('random_5x7_F1')
    h, w = base['shape']
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[:h, :w]
    n = 3 * h * w
    uniform = dict(x=np.tile(xx.ravel(), 3), y=np.tile(yy.ravel(), 3), s=np.ones(n, np.int64),
                   t=rng.uniform(0.3, 0.7, n).astype(np.float32), p=np.ones(n, np.int64))
    cols = {k: np.concatenate([base[k], uniform[k]]) for k in ('x', 'y', 's', 't', 'p')}
    # frame 0: the base case; frame 1: three ON events on every pixel; frame 2: a sample without events
    c = dict(cols, ts=np.tile(base['ts'], 3), fs=np.array([0, 1, 2], np.int64),
             flow=np.concatenate([base['flow'], rng.normal(0, 2, (2, 2, h, w)).astype(np.float32)]), shape=(h, w))
    fwd = L.contrast_multi_fwd_host(*mc.args_of(c), 7, True)
    grad, sums = L.contrast_multi_bwd_host(*mc.args_of(c), fwd)
    count, terms = fwd['count'].reshape(3, 3, 2, h, w), fwd['image_term'].reshape(3, 3, 2)
    assert (count[1, :, 0] == 3).all() and not count[1, :, 1].any() and not count[2].any()
    assert fwd['q'].reshape(3, 3, 2, h, w)[1, :, 0].any()
    assert terms[0].all() and not terms[1:].any() and not fwd['coef'].reshape(3, 6)[1:].any()
    assert grad[0].any() and not grad[1:].any() and not sums[1:].any()
    alone = L.contrast_multi_fwd_host(*mc.args_of(base), 7, True)
    assert float(fwd['term']) == pytest.approx(float(alone['term']) / 3, rel=1e-6)


@pytest.mark.parametrize('name', ['random_16x16_F3', 'dyadic_33x31_F4'])
def test_the_order_of_the_events_changes_no_byte(name):
    c, fwd, grad, sums = run(name, 7, True)
    p = mc.permuted(c)
    fwd_p = L.contrast_multi_fwd_host(*mc.args_of(p), 7, True)
    grad_p, sums_p = L.contrast_multi_bwd_host(*mc.args_of(p), fwd_p)
    assert same_forward(fwd, fwd_p)
    assert np.array_equal(sums_p, sums) and grad_p.tobytes() == grad.tobytes()


@pytest.mark.parametrize('mask,pol', [(7, True), (5, False)])
@pytest.mark.parametrize('name', ['random_16x16_F3', 'random_33x31_F4'])
def test_a_frame_alone_equals_the_frame_in_its_batch(name, mask, pol):
    """Images, records, the unit and the fixed-point sums of a frame do not
    depend on the batch: the unit is per frame and 1/M is applied after the sums."""
    c, fwd, _, sums = run(name, mask, pol)
    RC = fwd['R'] * fwd['C']
    for f in range(len(c['fs'])):
        one = cc.single_frame(c, f)
        fwd1 = L.contrast_multi_fwd_host(*mc.args_of(one), mask, pol)
        _, sums1 = L.contrast_multi_bwd_host(*mc.args_of(one), fwd1)
        mine = slice(f * RC, (f + 1) * RC)
        assert np.array_equal(fwd1['q'], fwd['q'][mine]) and np.array_equal(fwd1['count'], fwd['count'][mine])
        assert fwd1['result'].tobytes() == fwd['result'][mine].tobytes()
        for k in ('mean', 'coef', 'gmax', 'image_term'):
            assert fwd1[k].tobytes() == fwd[k][mine].tobytes(), k
        assert fwd1['unit'][0] == fwd['unit'][f]
        assert np.array_equal(sums1[0], sums[f]) and sums[f].any()


def test_the_unit_of_a_frame_comes_from_its_largest_image():
    c, fwd, _, sums = run('random_16x16_F3', 7, True)
    gmax = fwd['gmax'].reshape(3, 6)
    assert (gmax > 0).all() and len({float(v) for v in gmax[0]}) == 6
    for f in range(3):
        e = np.frexp(gmax[f].max())[1]
        assert fwd['unit'][f] == 2.0 ** (40 - 2 - e)
    # one addend is below 2^39 (1 + 2^-22) units; the events of a pixel stay far below 2^63
    assert np.abs(sums).max() < 2.0 ** 39 * 1.001 * fwd['count'].reshape(3, 6, 16, 16).sum(1).max()
    one = L.contrast_multi_fwd_host(*mc.args_of(c), 2, True)        # R = 1: the unit of the existing term
    for f in range(3):
        assert one['unit'][f] == 2.0 ** (40 - np.frexp(one['gmax'].reshape(3, 2)[f].max())[1])


# ------------------------------------------------------------ sign and use
def test_other_references_cut_the_reward_of_a_collapsing_flow():
    """The sink flow u = x - w/2, v = y - h/2 carries every event onto the
    centre.  Warped to the start it is paid in full; at the middle and the
    end it is not, and the mean over the three references pays about a third.
    Reduced, not removed: the mean is still negative."""
    c = mc.sink_case()
    terms = {mask: mc.oracle64(c, mask)['term'] for mask in (1, 2, 4, 7)}
    got = {mask: float(L.contrast_multi_fwd_host(*mc.args_of(c), mask, False)['term']) for mask in (1, 7)}
    print('sink flow, float64 definition: start', terms[1], 'middle', terms[2], 'end', terms[4],
          'mean of the three', terms[7], '| restatement', got)
    assert terms[1] < terms[7] < 0 and got[1] < got[7] < 0
    assert terms[7] == pytest.approx((terms[1] + terms[2] + terms[4]) / 3, rel=1e-12)
    assert 0.25 < terms[7] / terms[1] < 0.4 and terms[1] < -30
    assert got[1] == pytest.approx(terms[1], rel=1e-5) and got[7] == pytest.approx(terms[7], rel=1e-5)


def test_the_true_flow_stays_the_minimum_at_every_reference():
    true = np.array([3.0, -2.0])
    p = mc.with_polarity(cc.translating_pattern(flow=tuple(true)))
    for mask in (1, 2, 4):
        terms = {s: mc.oracle64(dict(p, flow=cc.constant_flow(p['shape'], tuple(true * s))), mask)['term']
                 for s in (0.0, 0.5, 1.0, 1.5)}
        print('reference mask', mask, terms)
        assert terms[1.0] < -0.15 and all(terms[s] >= 0 for s in (0.0, 0.5, 1.5))


def test_gradient_steps_on_a_translating_pattern_sharpen_it():
    """contrast_cases.translating_pattern, all three references, the polarities
    apart: a constant flow started at half the true one follows the
    restatement's gradient for twenty steps of 0.25.  The term falls at every
    step and the flow ends nearer the true one."""
    true = np.array([3.0, -2.0])
    p = mc.with_polarity(cc.translating_pattern(flow=tuple(true)))
    uv = (true / 2).astype(np.float32)
    terms = []
    for step in range(21):
        c = dict(p, flow=cc.constant_flow(p['shape'], uv))
        fwd = L.contrast_multi_fwd_host(*mc.args_of(c), ('start', 'middle', 'end'), True)
        terms.append(float(fwd['term']))
        if step == 20:
            break
        grad, _ = L.contrast_multi_bwd_host(*mc.args_of(c), fwd)
        uv = (uv - np.float32(0.25) * grad[0].sum((1, 2))).astype(np.float32)
    print('terms', terms, 'flow', uv)
    assert all(b < a for a, b in zip(terms, terms[1:]))
    assert np.linalg.norm(uv - true) < np.linalg.norm(true / 2)


# ------------------------------------------------------------ host plumbing
def test_reference_names_make_the_mask():
    assert L.contrast_reference_mask(('start',)) == 1 and L.contrast_reference_mask(['end', 'start']) == 5
    assert L.contrast_reference_mask('middle,end,start') == 7 and L.contrast_reference_mask(4) == 4
    for bad, what in (((), 'no reference'), (('start', 'start'), 'twice'), (('begin',), 'unknown'), (0, r'\[1, 7\]'),
                      (8, r'\[1, 7\]')):
        with pytest.raises(ValueError, match=what):
            L.contrast_reference_mask(bad)


def _parser():
    from argparse import ArgumentParser
    return options.add_preprocessed_dataset_arguments(options.add_train_arguments(ArgumentParser()))


def _parse(*extra):
    return options.validate_train_args(_parser().parse_args(['-m', '/tmp/m'] + list(extra)))


def test_the_two_flags_parse_and_need_a_weight():
    a = _parse()
    assert a.contrast_references == ('start',) and a.contrast_polarity is False and a.contrast_weight == 0.0
    a = _parse('--contrast-weight', '0.25')
    assert a.contrast_references == ('start',) and a.contrast_polarity is False
    a = _parse('--contrast-weight', '0.25', '--contrast-references', 'end,start', '--contrast-polarity')
    assert a.contrast_references == ('start', 'end') and a.contrast_polarity is True
    a = _parse('--contrast-weight', '0.25', '--contrast-references', 'start,middle,end')
    assert a.contrast_references == ('start', 'middle', 'end')
    for extra, what in ((['--contrast-references', 'start,end'], 'contrast-weight'),
                        (['--contrast-polarity'], 'contrast-weight'),
                        (['--contrast-weight', '0', '--contrast-polarity'], 'contrast-weight'),
                        (['--contrast-weight', '0.5', '--contrast-references', 'start,start'], 'twice'),
                        (['--contrast-weight', '0.5', '--contrast-references', 'start,centre'], 'unknown'),
                        (['--contrast-weight', '0.5', '--contrast-references', ''], 'unknown'),
                        (['--contrast-weight', '0.5', '--contrast-polarity', '--ev_images'], 'ev_images'),
                        (['--contrast-weight', '0.5', '--contrast-polarity', '--compact-events'], 'compact-events')):
        with pytest.raises(SystemExit, match=what):
            _parse(*extra)
    # naming the default is no option
    assert _parse('--contrast-references', 'start').contrast_references == ('start',)


class _Evaluator:
    def __init__(self):
        self.calls = []

    def __call__(self, flows, *rest, **kw):
        return tuple(tuple(torch.tensor(float(10 * t + k)) for k in range(len(flows))) for t in range(3))

    def contrast(self, flows, flow_ts, flow_sample_idx, events, weight=None, **options_):
        self.calls.append((weight, options_))
        return torch.tensor(-0.5 * weight), torch.tensor(-0.5)


def test_combined_loss_hands_the_options_on_and_the_defaults_not_at_all():
    flows = (torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 4, 4))
    ev, events = _Evaluator(), {'x': None}
    call = (ev, flows, None, None, None, None, None, None)
    training.combined_loss(*call, contrast_weight=0.25, events=events)
    training.combined_loss(*call, contrast_weight=0.25, events=events, contrast_references=('start',),
                           contrast_polarity=False)
    training.combined_loss(*call, contrast_weight=0.25, events=events, contrast_references=('start', 'end'))
    loss, terms = training.combined_loss(*call, contrast_weight=0.5, events=events,
                                         contrast_references=('start', 'middle', 'end'), contrast_polarity=True)
    assert ev.calls == [(0.25, {}), (0.25, {}), (0.25, {'references': ('start', 'end')}),
                        (0.5, {'references': ('start', 'middle', 'end'), 'polarity': True})]
    assert float(terms.contrast) == -0.5
    training.combined_loss(*call, contrast_references=('end',), contrast_polarity=True)     # weight 0: nothing
    assert len(ev.calls) == 4


class _LoopEvaluator:
    """CPU stand-in with the Losses call signature; records what the term was asked for."""
    seen = []

    def __call__(self, flows, flow_ts, fsi, images, ts, si):
        return (tuple(f.mean() for f in flows), tuple(2 * f.mean() for f in flows),
                tuple(0 * f.mean() for f in flows))

    def contrast(self, flows, flow_ts, flow_sample_idx, events, weight=None, references=('start',),
                 polarity=False):
        assert events['polarity'].numel() == events['x'].numel() > 0
        self.seen.append((tuple(references), polarity))
        term = -0.5 * flows[-1].mean()
        return term * weight, term.detach()


class _Logger:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, v, x):
        self.rows.append((tag, float(v), x))


def test_train_validate_and_the_hook_pass_the_options_through():
    import sys
    from pathlib import Path
    from dvs_of_training_framework_amd import hooks, synthetic
    from dvs_of_training_framework_amd.timer import FakeTimer
    sys.path.insert(0, str(Path(__file__).parent))
    from fake_flownet.net import Model as Fake
    sys.path.pop(0)

    def loader(n):
        return [synthetic.to_torch(synthetic.make_batch(i, 2, 16, 16, 10)) for i in range(n)]
    opts = dict(contrast_weight=0.25, contrast_references=('start', 'middle', 'end'), contrast_polarity=True)
    ev = _LoopEvaluator()
    ev.seen.clear()
    log = _Logger()
    training.validate(Fake('cpu'), 'cpu', loader(2), 7, log, ev, **opts)
    assert ev.seen == [(('start', 'middle', 'end'), True)] * 2
    assert {t: v for t, v, _ in log.rows}['Validation/contrast'] == pytest.approx(-0.5)
    ev.seen.clear()
    model = Fake('cpu')
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
    log = _Logger()
    training.train(model, 'cpu', loader(2), opt, num_steps=1, scheduler=sch, logger=log, evaluator=ev,
                   accumulation_steps=2, timers=FakeTimer(), max_events_per_batch=10 ** 6, **opts)
    assert ev.seen == [(('start', 'middle', 'end'), True)] * 2
    assert {t: v for t, v, _ in log.rows}['Train/contrast'] == pytest.approx(-0.5)
    ev.seen.clear()
    log = _Logger()
    hooks.ValidationHook(Fake('cpu'), 'cpu', loader(1), log, ev, [0.5, 1, 1], True, **opts)(1, 2)
    assert ev.seen == [(('start', 'middle', 'end'), True)]
    assert 'Validation/contrast' in {t for t, _, _ in log.rows}
    ev.seen.clear()
    hooks.ValidationHook(Fake('cpu'), 'cpu', loader(1), _Logger(), ev, [0.5, 1, 1], True)(1, 2)
    assert not ev.seen                              # no weight: the term is not asked for


def test_capture_refusal_still_names_the_weight():
    class Optimizer:
        def begin_capture(self): pass
        def advance(self): pass
        def end_capture(self): pass
    why = training.capture_refusal(Optimizer(), True, None, 0.25)
    assert '--contrast-weight' in why and '0.25' in why
