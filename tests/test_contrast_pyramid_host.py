"""The front end of the contrast term on every flow scale, without a GPU
(docs/CONTRAST_SPEC.md section 23): ``Losses.contrast(..., scales=...)`` takes
the path it took at the default and the new autograd function only at 'all',
the keyword is handed down the chain only where it differs from the default,
the flag and its refusals, and what is logged."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import hooks, loss as L, options, training


# ------------------------------------------------------------ Losses.contrast
class _Recorder:
    """Stands in for an autograd function's ``apply``: records, returns what the real one returns."""

    def __init__(self, out):
        self.calls, self.out = [], out

    def __call__(self, *args):
        self.calls.append(args)
        return self.out


@pytest.fixture
def recorders(monkeypatch):
    one = _Recorder((torch.tensor(-0.125), torch.tensor(-0.5)))
    pyramid = _Recorder((torch.tensor(-0.25), torch.tensor([-0.5, -1.0, -1.5])))
    monkeypatch.setattr(L._Contrast, 'apply', one)
    monkeypatch.setattr(L._ContrastPyramid, 'apply', pyramid)
    monkeypatch.setattr(L._lib, 'require_cuda', lambda *a: None)
    return one, pyramid


SHAPES = [(6, 10), (12, 20), (24, 40)]


def _call(**kw):
    ev = L.Losses(SHAPES, 3, 'cpu')
    flows = [torch.zeros(3, 2, *s) for s in SHAPES]
    events = {k: torch.zeros(5, dtype=torch.long) for k in ('x', 'y', 'polarity', 'sample_index')}
    events['timestamp'] = torch.zeros(5)
    return flows, ev.contrast(flows, torch.zeros(3, 2), torch.zeros(3, dtype=torch.long), events, **kw)


def test_the_default_takes_the_path_it_took_and_constructs_nothing_new(recorders):
    one, pyramid = recorders
    for kw in ({}, {'scales': 'finest'}, {'weight': 0.25}, {'weight': 0.25, 'scales': 'finest'}):
        flows, out = _call(**kw)
        assert (isinstance(out, tuple) and len(out) == 2) == ('weight' in kw)
    assert len(one.calls) == 4 and not pyramid.calls           # the pyramid function is never entered
    for args in one.calls:
        assert len(args) == 11 and args[0].shape[-2:] == (24, 40)          # the finest flow alone
        assert args[8] in (1.0, 0.25) and args[9:] == (1, False)


def test_all_goes_through_the_pyramid_function_with_every_flow(recorders):
    one, pyramid = recorders
    flows, out = _call(weight=0.25, scales='all', references=('start', 'end'), polarity=True)
    assert not one.calls and len(pyramid.calls) == 1
    args = pyramid.calls[0]
    assert args[7] == (24, 40) and args[9:11] == (5, True)
    assert [w.tobytes() for w in args[8]] == [(np.float32(0.25) / np.float32(3)).tobytes()] * 3
    assert all(a is b for a, b in zip(args[11:], flows)) and len(args) == 11 + 3
    value, terms = out
    assert float(value) == -0.25 and terms.tolist() == [-0.5, -1.0, -1.5]
    _, alone = _call(scales='all')                              # without a weight: the value alone, at weight 1
    assert float(alone) == -0.25
    assert [w.tobytes() for w in pyramid.calls[1][8]] == [(np.float32(1) / np.float32(3)).tobytes()] * 3


def test_refusals_of_the_keyword_come_before_any_call(recorders):
    one, pyramid = recorders
    with pytest.raises(ValueError, match='unknown contrast scales "coarse"'):
        _call(scales='coarse')
    with pytest.raises(ValueError, match='unknown reference'):
        _call(scales='all', references=('begin',))
    ev = L.Losses([(6, 10), (12, 21), (24, 40)], 3, 'cpu')     # 12x21 is no halving of 24x40
    flows = [torch.zeros(3, 2, *s) for s in ev.shapes]
    events = {k: torch.zeros(5, dtype=torch.long) for k in ('x', 'y', 'polarity', 'sample_index')}
    events['timestamp'] = torch.zeros(5)
    with pytest.raises(ValueError, match='halving'):
        ev.contrast(flows, torch.zeros(3, 2), torch.zeros(3, dtype=torch.long), events, scales='all')
    ev.contrast(flows, torch.zeros(3, 2), torch.zeros(3, dtype=torch.long), events)       # the finest alone is fine
    assert len(one.calls) == 1 and not pyramid.calls


# ----------------------------------------------------------------- the flag
def _parser():
    from argparse import ArgumentParser
    return options.add_preprocessed_dataset_arguments(options.add_train_arguments(ArgumentParser()))


def _parse(*extra):
    return options.validate_train_args(_parser().parse_args(['-m', '/tmp/m'] + list(extra)))


def test_the_flag_parses_and_needs_a_weight():
    assert not hasattr(_parse(), 'contrast_scales')            # absent unless given: the namespace is as it was
    assert not hasattr(_parse('--contrast-weight', '0.25'), 'contrast_scales')
    assert _parse('--contrast-weight', '0.25', '--contrast-scales', 'all').contrast_scales == 'all'
    assert _parse('--contrast-weight', '0.25', '--contrast-scales', 'finest').contrast_scales == 'finest'
    assert _parse('--contrast-scales', 'finest').contrast_scales == 'finest'       # naming the default is no option
    for extra, what in ((['--contrast-scales', 'all'], '--contrast-scales needs a positive --contrast-weight'),
                        (['--contrast-weight', '0', '--contrast-scales', 'all'], 'contrast-weight'),
                        # the refusals of the weight and of the other options stay
                        (['--contrast-weight', '0.5', '--contrast-scales', 'all', '--ev_images'], 'ev_images'),
                        (['--contrast-weight', '0.5', '--contrast-scales', 'all', '--compact-events'],
                         'compact-events'),
                        (['--contrast-weight', '-1', '--contrast-scales', 'all'], 'negative'),
                        (['--contrast-scales', 'all', '--contrast-polarity'], 'contrast-weight')):
        with pytest.raises(SystemExit, match=what):
            _parse(*extra)
    with pytest.raises(SystemExit):
        _parse('--contrast-weight', '0.5', '--contrast-scales', 'coarse')


# -------------------------------------------------------------- down the chain
class _Evaluator:
    def __init__(self):
        self.calls = []

    def __call__(self, flows, *rest, **kw):
        return tuple(tuple(torch.tensor(float(10 * t + k)) for k in range(len(flows))) for t in range(3))

    def contrast(self, flows, flow_ts, flow_sample_idx, events, weight=None, **options_):
        self.calls.append((weight, options_))
        if options_.get('scales') == 'all':
            terms = torch.tensor([-0.5 * (k + 1) for k in range(len(flows))])
            return terms.mean() * weight, terms
        return torch.tensor(-0.5 * weight), torch.tensor(-0.5)


def test_combined_loss_hands_the_keyword_on_only_where_it_differs():
    flows = (torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 4, 4))
    ev, events = _Evaluator(), {'x': None}
    call = (ev, flows, None, None, None, None, None, None)
    training.combined_loss(*call, contrast_weight=0.25, events=events)
    training.combined_loss(*call, contrast_weight=0.25, events=events, contrast_scales='finest')
    loss, terms = training.combined_loss(*call, contrast_weight=0.5, events=events, contrast_scales='all',
                                         contrast_references=('start', 'end'))
    assert ev.calls == [(0.25, {}), (0.25, {}), (0.5, {'references': ('start', 'end'), 'scales': 'all'})]
    assert terms.contrast.tolist() == [-0.5, -1.0]
    back = training.TermReadback(terms)
    assert back.contrast_levels() == [-0.5, -1.0] and back.contrast() == -0.75
    plain = training.TermReadback(training.combined_loss(*call, contrast_weight=0.25, events=events)[1])
    assert plain.contrast() == -0.5 and plain.contrast_levels() is None
    training.combined_loss(*call, contrast_scales='all')        # weight 0: nothing
    assert len(ev.calls) == 4
    assert training._contrast_keywords(0.25, ('start',), False) == {'contrast_weight': 0.25}
    assert training._contrast_keywords(0.25, ('start',), False, 'finest') == {'contrast_weight': 0.25}
    assert training._contrast_keywords(0.25, ('start',), False, 'all') == {'contrast_weight': 0.25,
                                                                          'contrast_scales': 'all'}
    assert training._contrast_keywords(0.0, ('start',), False, 'all') == {}


class _LoopEvaluator:
    """CPU stand-in with the Losses call signature; records what the term was asked for."""
    seen = []

    def __call__(self, flows, flow_ts, fsi, images, ts, si):
        return (tuple(f.mean() for f in flows), tuple(2 * f.mean() for f in flows),
                tuple(0 * f.mean() for f in flows))

    def contrast(self, flows, flow_ts, flow_sample_idx, events, weight=None, references=('start',),
                 polarity=False, **rest):
        self.seen.append(dict(rest))
        if rest.get('scales') == 'all':
            terms = torch.stack([-0.5 * (k + 1) + 0 * f.mean() for k, f in enumerate(flows)])
            return terms.mean() * weight, terms.detach()
        term = -0.5 + 0 * flows[-1].mean()
        return term * weight, term.detach()


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
    ev.seen.clear()
    rows = train(contrast_weight=0.25, contrast_scales='all')
    assert ev.seen == [{'scales': 'all'}] * 2
    tags = sorted(t for t in rows if t.startswith('Train/contrast/'))
    K = len(tags)
    assert K >= 2 and all(t.split('/')[-1].count('x') == 1 for t in tags)
    assert {t.split('/')[-1] for t in tags} == {t.split('/')[-1] for t in rows if t.startswith('Train/smoothness loss/')}
    assert sorted(rows[t] for t in tags) == pytest.approx(sorted(-0.5 * (k + 1) for k in range(K)))
    assert rows['Train/contrast'] == pytest.approx(np.mean([-0.5 * (k + 1) for k in range(K)]))
    # at the default nothing new is asked for and nothing new is logged
    ev.seen.clear()
    for opts in (dict(contrast_weight=0.25), dict(contrast_weight=0.25, contrast_scales='finest')):
        rows = train(**opts)
        assert rows['Train/contrast'] == pytest.approx(-0.5)
        assert not [t for t in rows if t.startswith('Train/contrast/')]
    assert ev.seen == [{}] * 4
    ev.seen.clear()
    log = _Logger()
    training.validate(Fake('cpu'), 'cpu', loader(2), 7, log, ev, contrast_weight=0.25, contrast_scales='all')
    assert ev.seen == [{'scales': 'all'}] * 2
    assert {t: v for t, v, _ in log.rows}['Validation/contrast'] == pytest.approx(
        np.mean([-0.5 * (k + 1) for k in range(K)]))
    ev.seen.clear()
    hooks.ValidationHook(Fake('cpu'), 'cpu', loader(1), _Logger(), ev, [0.5, 1, 1], True, contrast_weight=0.25,
                         contrast_scales='all')(1, 2)
    hooks.ValidationHook(Fake('cpu'), 'cpu', loader(1), _Logger(), ev, [0.5, 1, 1], True, contrast_weight=0.25)(1, 2)
    hooks.ValidationHook(Fake('cpu'), 'cpu', loader(1), _Logger(), ev, [0.5, 1, 1], True, contrast_weight=0.25,
                         contrast_scales='finest')(1, 2)
    hooks.ValidationHook(Fake('cpu'), 'cpu', loader(1), _Logger(), ev, [0.5, 1, 1], True,
                         contrast_scales='all')(1, 2)          # no weight: the term is not asked for
    assert ev.seen == [{'scales': 'all'}, {}, {}]


def test_capture_refusal_is_unchanged():
    class Optimizer:
        def begin_capture(self): pass
        def advance(self): pass
        def end_capture(self): pass
    why = training.capture_refusal(Optimizer(), True, None, 0.25)
    assert '--contrast-weight' in why and '0.25' in why
    import inspect
    assert list(inspect.signature(training.capture_refusal).parameters) == ['optimizer', 'is_raw', 'model',
                                                                           'contrast_weight']
