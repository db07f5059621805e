"""The average-timestamp term on every flow scale without a GPU
(docs/AVG_TIMESTAMP_SPEC.md sections 11-15): the restatement
loss.avg_timestamp_pyramid_fwd_host / _bwd_host against the one-level
restatement it is made of, what the device cases of
tests/contrast_pyramid_cases.py reach on every level, and the front end --
``Losses.avg_timestamp_scales``, the keyword down the chain only where it
differs from the default, the flag and its refusal, and what is logged.  Every
comparison of numbers is of bytes."""
import inspect

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import hooks, loss as L, options, training
from tests import avg_timestamp_pyramid_cases as apc, contrast_multi_cases as mc, contrast_pyramid_cases as pc

F32 = np.float32


# ------------------------------------------------------------ the restatement
@pytest.mark.parametrize('shape', apc.SHAPES)
@pytest.mark.parametrize('mask,pol', [(5, False), (7, True)])
def test_one_level_of_shift_zero_is_the_one_level_restatement(shape, mask, pol):
    full = pc.device_case(shape)
    c = dict(full, level_shapes=full['level_shapes'][:1], flows=full['flows'][:1])
    w = [F32(0.25)]
    fwd = L.avg_timestamp_pyramid_fwd_host(*pc.host_args(c), c['shape'], w, mask, pol)
    one = L.avg_timestamp_fwd_host(*mc.args_of(dict(c, flow=c['flows'][0])), mask, pol)
    assert fwd['shifts'] == [0] and set(fwd['levels'][0]) == set(one)
    for key, v in one.items():
        got = fwd['levels'][0][key]
        got, v = np.asarray(got), np.asarray(v)
        assert got.tobytes() == v.tobytes() and got.dtype == v.dtype, key
    assert fwd['terms'].tobytes() == np.asarray([one['term']]).tobytes()
    assert fwd['value'].tobytes() == F32(np.float64(F32(0.25)) * fwd['terms64'][0]).tobytes()
    (grad, sums), = L.avg_timestamp_pyramid_bwd_host(*pc.host_args(c), fwd, seed=-1.5)
    want, want_sums = L.avg_timestamp_bwd_host(*mc.args_of(dict(c, flow=c['flows'][0])), one, seed=-1.5, weight=w[0])
    assert grad.tobytes() == want.tobytes() and np.array_equal(sums, want_sums) and want.any()


def test_the_combination_is_the_stated_one():
    c = pc.device_case((21, 37))
    w = np.asarray([0.5, 0.0, -2.0, 0.125], F32)
    fwd = L.avg_timestamp_pyramid_fwd_host(*pc.host_args(c), c['shape'], w, 7, True)
    total = np.float64(0)
    for k, lev in enumerate(fwd['levels']):
        s = np.float64(0)
        for v in lev['image_value']:
            s = s + v
        assert fwd['terms64'][k] == s / np.float64(18) and fwd['terms'][k].tobytes() == F32(s / 18).tobytes()
        total = total + np.float64(w[k]) * (s / np.float64(18))
    assert fwd['value'].tobytes() == F32(total).tobytes() and fwd['value'].dtype == F32
    assert fwd['shifts'] == [0, 1, 2, 3]
    default = L.avg_timestamp_pyramid_fwd_host(*pc.host_args(c), c['shape'])
    assert default['weights'].tobytes() == np.asarray([F32(1) / F32(4)] * 4, F32).tobytes()
    assert default['levels'][0]['mask'] == 5 and default['levels'][0]['C'] == 1        # start,end, no polarity
    with pytest.raises(ValueError, match='levels'):
        L.avg_timestamp_pyramid_fwd_host(*pc.host_args(c)[:-1], [], c['shape'])
    with pytest.raises(ValueError, match='halving'):
        L.avg_timestamp_pyramid_fwd_host(*pc.host_args(c)[:-1], [np.zeros((3, 2, 10, 19), F32)], c['shape'])


@pytest.mark.parametrize('shape', apc.SHAPES)
def test_at_zero_flow_every_level_gives_exactly_one(shape):
    full = pc.device_case(shape)
    c = dict(full, flows=[np.zeros_like(f) for f in full['flows']])
    for mask, pol in pc.OPTIONS:
        fwd = L.avg_timestamp_pyramid_fwd_host(*pc.host_args(c), c['shape'], None, mask, pol)
        for k, lev in enumerate(fwd['levels']):
            held = lev['count'].reshape(len(lev['rec']), -1).sum(1) > 0
            live = lev['rec']['S0'] > 0         # an image whose events all sit on its reference has no distance
            assert held.any() and (lev['image_value'][live] == 1.0).all() and not lev['image_value'][~live].any(), k
            assert not (live & ~held).any()
            if live.all():
                assert fwd['terms'][k] == 1.0, (mask, pol, k)
        if all((lev['rec']['S0'] > 0).all() for lev in fwd['levels']):
            assert fwd['value'].tobytes() == F32(sum(np.float64(w) for w in fwd['weights'])).tobytes()


def test_events_on_the_far_edges_stay_out_of_every_level():
    """21x37: x == w and y == h shift to columns inside the coarser grids; the
    inside test comes before the shift."""
    c = pc.device_case((21, 37))
    h, w = c['shape']
    edge = ((c['x'] == w) & (c['y'] >= 0) & (c['y'] <= h)) | ((c['y'] == h) & (c['x'] >= 0) & (c['x'] <= w))
    assert ((c['x'] == w) & (c['y'] < h) & (c['y'] >= 0)).any() and ((c['y'] == h) & (c['x'] < w) & (c['x'] >= 0)).any()
    assert 37 >> 1 < 19 and 21 >> 1 < 11 and 37 >> 2 < 10 and 21 >> 2 < 6      # they would land inside
    without = {k: (v[~edge] if k in ('x', 'y', 't', 'p', 's') else v) for k, v in c.items()}
    for mask, pol in ((5, False), (7, True)):
        a = L.avg_timestamp_pyramid_fwd_host(*pc.host_args(c), c['shape'], None, mask, pol)
        b = L.avg_timestamp_pyramid_fwd_host(*pc.host_args(without), c['shape'], None, mask, pol)
        for k in range(4):
            for key in ('q', 's', 'base', 'count', 'rec', 'unit'):
                assert a['levels'][k][key].tobytes() == b['levels'][k][key].tobytes(), (k, key)
        assert a['value'].tobytes() == b['value'].tobytes()
        inside = (c['x'] >= 0) & (c['x'] < w) & (c['y'] >= 0) & (c['y'] < h)
        xs, ys = L.contrast_level_columns(c['x'], c['y'], c['shape'], 2)
        assert (xs[~inside] == -1).all() and (ys[~inside] == -1).all() and (xs[inside] == c['x'][inside] >> 2).all()


@pytest.mark.parametrize('shape', apc.SHAPES)
def test_the_device_cases_reach_every_level(shape):
    """What tests/test_gpu_avg_timestamp_pyramid.py relies on, checked on the
    host: under every option every level has events, a frame that has events has
    an image with n > 0 and n0 > 0, the gradient is finite and not zero, and the
    term is finite and not exactly 1."""
    c = pc.device_case(shape)
    F = len(c['fs'])
    for mask, pol in pc.OPTIONS:
        fwd = L.avg_timestamp_pyramid_fwd_host(*pc.host_args(c), c['shape'], None, mask, pol)
        bwd = L.avg_timestamp_pyramid_bwd_host(*pc.host_args(c), fwd)
        assert len(fwd['levels']) == len(pc.LEVELS[shape]) in (3, 4)
        for k, lev in enumerate(fwd['levels']):
            RC = lev['R'] * lev['C']
            per_frame = lev['count'].reshape(F, RC, -1).sum((1, 2))
            assert lev['count'].sum() > 0, (mask, pol, k)
            n, n0 = lev['rec']['n'].reshape(F, RC), lev['rec']['n0'].reshape(F, RC)
            for f in range(F):
                if per_frame[f]:
                    assert ((n[f] > 0) & (n0[f] > 0)).any(), (mask, pol, k, f)
            assert per_frame.all()          # here every frame has events
            grad = bwd[k][0]
            assert np.isfinite(grad).all() and grad.any(), (mask, pol, k)
            assert np.isfinite(fwd['terms'][k]) and fwd['terms'][k] != 1.0, (mask, pol, k)
        assert np.isfinite(fwd['value'])


# ------------------------------------------------- Losses.avg_timestamp_scales
class _Recorder:
    def __init__(self, out):
        self.calls, self.out = [], out

    def __call__(self, *args):
        self.calls.append(args)
        return self.out


@pytest.fixture
def recorders(monkeypatch):
    one = _Recorder((torch.tensor(0.4), torch.tensor(0.8)))
    pyramid = _Recorder((torch.tensor(0.3), torch.tensor([0.5, 0.75, 1.0])))
    other = _Recorder(None)
    monkeypatch.setattr(L._AvgTimestamp, 'apply', one)
    monkeypatch.setattr(L._AvgTimestampPyramid, 'apply', pyramid)
    monkeypatch.setattr(L._ContrastPyramid, 'apply', other)
    monkeypatch.setattr(L._lib, 'require_cuda', lambda *a: None)
    return one, pyramid, other


SHAPES = [(6, 10), (12, 20), (24, 40)]


def _call(shapes=SHAPES, **kw):
    ev = L.Losses(shapes, 3, 'cpu')
    flows = [torch.zeros(3, 2, *s) for s in shapes]
    events = {k: torch.zeros(5, dtype=torch.long) for k in ('x', 'y', 'polarity', 'sample_index')}
    events['timestamp'] = torch.zeros(5)
    return flows, ev.avg_timestamp_scales(flows, torch.zeros(3, 2), torch.zeros(3, dtype=torch.long), events, **kw)


def test_finest_is_the_call_as_it_is_and_constructs_nothing_new(recorders):
    one, pyramid, other = recorders
    for kw in ({}, {'scales': 'finest'}, {'weight': 0.25}, {'weight': 0.25, 'scales': 'finest'}):
        _, out = _call(**kw)
        assert (isinstance(out, tuple) and len(out) == 2) == ('weight' in kw)
    assert len(one.calls) == 4 and not pyramid.calls and not other.calls
    for args in one.calls:
        assert len(args) == 11 and args[0].shape[-2:] == (24, 40) and args[8] in (1.0, 0.25) and args[9:] == (5, False)
    # the signature of the one-level method is held as it is; the new one adds the keyword
    assert list(inspect.signature(L.Losses.avg_timestamp).parameters) == [
        'self', 'flows', 'flow_ts', 'flow_sample_idx', 'events', 'weight', 'references', 'polarity']
    p = inspect.signature(L.Losses.avg_timestamp_scales).parameters
    assert list(p)[:8] == list(inspect.signature(L.Losses.avg_timestamp).parameters) and list(p)[8:] == ['scales']
    assert p['scales'].default == 'finest' and p['references'].default == ('start', 'end')


def test_all_goes_through_the_pyramid_function_with_every_flow(recorders):
    one, pyramid, other = recorders
    flows, out = _call(weight=0.25, scales='all', references=('start', 'middle', 'end'), polarity=True)
    assert not one.calls and not other.calls and len(pyramid.calls) == 1
    args = pyramid.calls[0]
    assert args[7] == (24, 40) and args[9:11] == (7, True)
    assert [w.tobytes() for w in args[8]] == [(F32(0.25) / F32(3)).tobytes()] * 3
    assert all(a is b for a, b in zip(args[11:], flows)) and len(args) == 11 + 3
    value, terms = out
    assert float(value) == pytest.approx(0.3) and terms.tolist() == [0.5, 0.75, 1.0]
    _, alone = _call(scales='all')
    assert float(alone) == pytest.approx(0.3)
    assert pyramid.calls[1][9:11] == (5, False) and pyramid.calls[1][3] is None       # start,end; p not handed on
    assert [w.tobytes() for w in pyramid.calls[1][8]] == [(F32(1) / F32(3)).tobytes()] * 3


def test_refusals_of_the_keyword_come_before_any_call(recorders):
    one, pyramid, _ = recorders
    with pytest.raises(ValueError, match='unknown avg-timestamp scales "coarse"'):
        _call(scales='coarse')
    with pytest.raises(ValueError, match='unknown reference'):
        _call(scales='all', references=('begin',))
    with pytest.raises(ValueError, match='halving'):
        _call(shapes=[(6, 10), (12, 21), (24, 40)], scales='all')
    _call(shapes=[(6, 10), (12, 21), (24, 40)])                # the finest alone is fine
    assert len(one.calls) == 1 and not pyramid.calls


# ----------------------------------------------------------------- the flag
def _parse(*extra):
    from argparse import ArgumentParser
    parser = options.add_preprocessed_dataset_arguments(options.add_train_arguments(ArgumentParser()))
    return options.validate_train_args(parser.parse_args(['-m', '/tmp/m'] + list(extra)))


def test_the_flag_parses_needs_a_weight_and_travels_only_where_it_differs():
    assert not hasattr(_parse(), 'avg_timestamp_scales')        # absent unless given
    assert not hasattr(_parse('--avg-timestamp-weight', '0.5'), 'avg_timestamp_scales')
    on = _parse('--avg-timestamp-weight', '0.5', '--avg-timestamp-scales', 'all')
    assert on.avg_timestamp_scales == 'all'
    assert _parse('--avg-timestamp-scales', 'finest').avg_timestamp_scales == 'finest'   # the default is no option
    for extra, what in ((['--avg-timestamp-scales', 'all'],
                         '--avg-timestamp-scales needs a positive --avg-timestamp-weight'),
                        (['--avg-timestamp-weight', '0', '--avg-timestamp-scales', 'all'],
                         '--avg-timestamp-scales needs a positive --avg-timestamp-weight'),
                        (['--contrast-weight', '0.5', '--avg-timestamp-scales', 'all'],
                         '--avg-timestamp-scales needs a positive --avg-timestamp-weight'),
                        (['--avg-timestamp-weight', '0.5', '--avg-timestamp-scales', 'all', '--ev_images'],
                         'ev_images'),
                        (['--avg-timestamp-weight', '-1', '--avg-timestamp-scales', 'all'], 'negative')):
        with pytest.raises(SystemExit, match=what):
            _parse(*extra)
    with pytest.raises(SystemExit):
        _parse('--avg-timestamp-weight', '0.5', '--avg-timestamp-scales', 'coarse')
    today = {'avg_timestamp_weight': 0.5, 'avg_timestamp_references': ('start', 'end'),
             'avg_timestamp_polarity': False}
    assert options.avg_timestamp_keywords(_parse('--avg-timestamp-weight', '0.5')) == today
    assert options.avg_timestamp_keywords(
        _parse('--avg-timestamp-weight', '0.5', '--avg-timestamp-scales', 'finest')) == today
    assert options.avg_timestamp_keywords(on) == dict(today, avg_timestamp_scales='all')
    assert options.avg_timestamp_keywords(_parse()) == {}
    # the dicts down the chain, which are the capture signature's loss_options
    assert training._avg_timestamp_keywords(0.5, ('start', 'end'), False) == {'avg_timestamp_weight': 0.5}
    assert training._avg_timestamp_keywords(0.5, ('start', 'end'), False, 'finest') == {'avg_timestamp_weight': 0.5}
    assert training._avg_timestamp_keywords(0.5, ('end',), True, 'all') == {
        'avg_timestamp_weight': 0.5, 'avg_timestamp_references': ('end',), 'avg_timestamp_polarity': True,
        'avg_timestamp_scales': 'all'}
    assert training._avg_timestamp_keywords(0.0, ('end',), True, 'all') == {}
    assert training._avg_timestamp_options(('start', 'end'), False) == {}
    assert training._avg_timestamp_options(('start', 'end'), False, 'all') == {'scales': 'all'}


# -------------------------------------------------------------- down the chain
class _Evaluator:
    def __init__(self):
        self.calls = []

    def __call__(self, flows, *rest, **kw):
        return tuple(tuple(torch.tensor(float(10 * t + k)) for k in range(len(flows))) for t in range(3))

    def avg_timestamp(self, flows, flow_ts, flow_sample_idx, events, weight=None, **options_):
        self.calls.append(('avg_timestamp', weight, options_))
        return torch.tensor(0.75 * weight), torch.tensor(0.75)

    def avg_timestamp_scales(self, flows, flow_ts, flow_sample_idx, events, weight=None, **options_):
        self.calls.append(('avg_timestamp_scales', weight, options_))
        assert options_['scales'] == 'all'
        terms = torch.tensor([0.5 * (k + 1) for k in range(len(flows))])
        return terms.mean() * weight, terms


def test_combined_loss_hands_the_keyword_on_only_where_it_differs():
    flows = (torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 4, 4))
    ev, events = _Evaluator(), {'x': None}
    call = (ev, flows, None, None, None, None, None, None)
    plain, _ = training.combined_loss(*call)
    training.combined_loss(*call, avg_timestamp_weight=0.25, events=events)
    training.combined_loss(*call, avg_timestamp_weight=0.25, events=events, avg_timestamp_scales='finest')
    loss, terms = training.combined_loss(*call, avg_timestamp_weight=0.5, events=events, avg_timestamp_scales='all',
                                         avg_timestamp_references=('end',))
    assert ev.calls == [('avg_timestamp', 0.25, {}), ('avg_timestamp', 0.25, {}),
                        ('avg_timestamp_scales', 0.5, {'references': ('end',), 'scales': 'all'})]
    assert terms.avg_timestamp.tolist() == [0.5, 1.0] and terms.contrast is None
    assert float(loss) == float(plain) + 0.375
    back = training.TermReadback(terms)
    assert back.avg_timestamp_levels() == [0.5, 1.0] and back.avg_timestamp() == 0.75 and back.contrast() is None
    one = training.TermReadback(training.combined_loss(*call, avg_timestamp_weight=0.25, events=events)[1])
    assert one.avg_timestamp() == 0.75 and one.avg_timestamp_levels() is None
    training.combined_loss(*call, avg_timestamp_scales='all')   # weight 0: nothing
    assert len(ev.calls) == 4
    for fn in (training.combined_loss, training.process_minibatch, training.train, training.validate,
               hooks.ValidationHook.__init__):
        p = inspect.signature(fn).parameters
        assert p['avg_timestamp_scales'].default == 'finest', fn
        assert tuple(p)[-3:] == ('avg_timestamp_weight', 'avg_timestamp_references', 'avg_timestamp_polarity'), fn


class _LoopEvaluator:
    """CPU stand-in with the Losses call signature; records what the term was asked for."""

    def __init__(self):
        self.seen = []

    def __call__(self, flows, flow_ts, fsi, images, ts, si):
        return (tuple(f.mean() for f in flows), tuple(2 * f.mean() for f in flows),
                tuple(0 * f.mean() for f in flows))

    def avg_timestamp(self, flows, flow_ts, flow_sample_idx, events, weight=None, **rest):
        self.seen.append(('avg_timestamp', dict(rest)))
        term = 0.75 + 0 * flows[-1].mean()
        return term * weight, term.detach()

    def avg_timestamp_scales(self, flows, flow_ts, flow_sample_idx, events, weight=None, **rest):
        self.seen.append(('avg_timestamp_scales', dict(rest)))
        terms = torch.stack([0.5 * (k + 1) + 0 * f.mean() for k, f in enumerate(flows)])
        return terms.mean() * weight, terms.detach()


class _Logger:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, v, x):
        self.rows.append((tag, float(v), x))


def test_train_validate_and_the_hook_pass_the_keyword_through_and_log_the_levels():
    import sys
    from pathlib import Path
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.timer import FakeTimer
    sys.path.insert(0, str(Path(__file__).parent))
    from fake_flownet.net import Model as Fake
    sys.path.pop(0)

    def loader(n):
        return [synthetic.to_torch(synthetic.make_batch(i, 2, 16, 16, 10)) for i in range(n)]

    def train(**opts):
        model = Fake('cpu')
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
        log = _Logger()
        training.train(model, 'cpu', loader(2), opt, num_steps=1, scheduler=sch, logger=log, evaluator=ev,
                       accumulation_steps=2, timers=FakeTimer(), max_events_per_batch=10 ** 6, **opts)
        return {t: v for t, v, _ in log.rows}
    ev = _LoopEvaluator()
    rows = train(avg_timestamp_weight=0.25, avg_timestamp_scales='all')
    assert ev.seen == [('avg_timestamp_scales', {'scales': 'all'})] * 2
    tags = sorted(t for t in rows if t.startswith('Train/avg timestamp/'))
    K = len(tags)
    assert K >= 2
    assert {t.split('/')[-1] for t in tags} == {t.split('/')[-1] for t in rows
                                                if t.startswith('Train/smoothness loss/')}
    assert sorted(rows[t] for t in tags) == pytest.approx(sorted(0.5 * (k + 1) for k in range(K)))
    assert rows['Train/avg timestamp'] == pytest.approx(np.mean([0.5 * (k + 1) for k in range(K)]))
    # at the default nothing new is asked for and nothing new is logged
    ev.seen.clear()
    for opts in (dict(avg_timestamp_weight=0.25), dict(avg_timestamp_weight=0.25, avg_timestamp_scales='finest')):
        rows = train(**opts)
        assert rows['Train/avg timestamp'] == pytest.approx(0.75)
        assert not [t for t in rows if t.startswith('Train/avg timestamp/')]
    assert ev.seen == [('avg_timestamp', {})] * 4
    ev.seen.clear()
    log = _Logger()
    training.validate(Fake('cpu'), 'cpu', loader(2), 7, log, ev, avg_timestamp_weight=0.25,
                      avg_timestamp_scales='all')
    assert ev.seen == [('avg_timestamp_scales', {'scales': 'all'})] * 2
    rows = {t: v for t, v, _ in log.rows}
    assert rows['Validation/avg timestamp'] == pytest.approx(np.mean([0.5 * (k + 1) for k in range(K)]))
    assert sorted(v for t, v in rows.items() if t.startswith('Validation/avg timestamp/')) == pytest.approx(
        sorted(0.5 * (k + 1) for k in range(K)))
    ev.seen.clear()
    make = lambda **kw: hooks.ValidationHook(Fake('cpu'), 'cpu', loader(1), _Logger(), ev, [0.5, 1, 1], True, **kw)
    make(avg_timestamp_weight=0.25, avg_timestamp_scales='all')(1, 2)
    make(avg_timestamp_weight=0.25)(1, 2)
    make(avg_timestamp_weight=0.25, avg_timestamp_scales='finest')(1, 2)
    make(avg_timestamp_scales='all')(1, 2)                      # no weight: the term is not asked for
    assert ev.seen == [('avg_timestamp_scales', {'scales': 'all'}), ('avg_timestamp', {}), ('avg_timestamp', {})]
    assert make(avg_timestamp_weight=0.25).extra == {'avg_timestamp_weight': 0.25,
                                                     'avg_timestamp_references': ('start', 'end'),
                                                     'avg_timestamp_polarity': False}


def test_the_captured_step_is_asked_for_the_method_the_run_will_call():
    class Finest:
        contrast = avg_timestamp = frameless = staticmethod(lambda *a, **k: None)
    assert training.event_terms_capture_refusal(Finest(), True, ['avg_timestamp']) is None
    assert 'avg_timestamp_scales' in training.event_terms_capture_refusal(Finest(), True, ['avg_timestamp_scales'])
    assert training.EVENT_TERM_METHODS == ('contrast', 'avg_timestamp', 'frameless')
