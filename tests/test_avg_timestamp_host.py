"""The front end of the average-timestamp term, without a GPU
(docs/AVG_TIMESTAMP_SPEC.md section 10): the flags, their grammar and their
refusals, a namespace that holds no new key unless a flag is given,
``Losses.avg_timestamp`` and ``combined_loss`` down to the autograd function,
what ``train``, ``validate`` and the validation hook hand on and log, and a
run that asks to be captured."""
import inspect

import pytest
import torch

from dvs_of_training_framework_amd import hooks, loss as L, options, training

KEYS = ('avg_timestamp_weight', 'avg_timestamp_references', 'avg_timestamp_polarity')


# ---------------------------------------------------------------- the flags
def _parser():
    from argparse import ArgumentParser
    return options.add_preprocessed_dataset_arguments(options.add_train_arguments(ArgumentParser()))


def _parse(*extra):
    return options.validate_train_args(_parser().parse_args(['-m', '/tmp/m'] + list(extra)))


def test_the_namespace_holds_no_new_key_unless_a_flag_is_given():
    for extra in ((), ('--contrast-weight', '0.25'), ('--contrast-weight', '0.25', '--contrast-references', 'end')):
        args = _parse(*extra)
        assert not [k for k in vars(args) if 'avg' in k or 'timestamp' in k], extra
        assert options.avg_timestamp_keywords(args) == {}
    args = _parse('--avg-timestamp-weight', '0.5')
    assert [k for k in vars(args) if k.startswith('avg_')] == ['avg_timestamp_weight']
    assert options.avg_timestamp_keywords(args) == dict(avg_timestamp_weight=0.5, avg_timestamp_polarity=False,
                                                        avg_timestamp_references=('start', 'end'))


def test_the_grammar_of_the_flags():
    args = _parse('--avg-timestamp-weight', '0.5', '--avg-timestamp-references', 'end,middle',
                  '--avg-timestamp-polarity')
    assert args.avg_timestamp_references == ('middle', 'end') and args.avg_timestamp_polarity is True
    assert options.avg_timestamp_keywords(args) == dict(avg_timestamp_weight=0.5, avg_timestamp_polarity=True,
                                                        avg_timestamp_references=('middle', 'end'))
    assert _parse('--avg-timestamp-weight', '0.5', '--avg-timestamp-references',
                  'start').avg_timestamp_references == ('start',)
    # beside the contrast term, whose options stay its own
    both = _parse('--avg-timestamp-weight', '0.5', '--contrast-weight', '0.25', '--contrast-references', 'start')
    assert both.contrast_references == ('start',) and not hasattr(both, 'avg_timestamp_references')
    assert _parse('--avg-timestamp-weight', '0').avg_timestamp_weight == 0.0


@pytest.mark.parametrize('extra,what', [
    (['--avg-timestamp-references', 'start,end'], '--avg-timestamp-references needs a positive --avg-timestamp-weight'),
    (['--avg-timestamp-polarity'], '--avg-timestamp-polarity needs a positive --avg-timestamp-weight'),
    (['--avg-timestamp-weight', '0', '--avg-timestamp-polarity'], '--avg-timestamp-polarity needs'),
    (['--avg-timestamp-weight', '-1'], '--avg-timestamp-weight must not be negative'),
    (['--avg-timestamp-weight', 'nan'], '--avg-timestamp-weight must not be negative'),
    (['--avg-timestamp-weight', '0.5', '--avg-timestamp-references', 'begin'],
     '--avg-timestamp-references: unknown reference time "begin"'),
    (['--avg-timestamp-weight', '0.5', '--avg-timestamp-references', 'end,end'],
     '--avg-timestamp-references: "end" is given twice'),
    (['--avg-timestamp-weight', '0.5', '--ev_images'], '--avg-timestamp-weight cannot be combined with --ev_images'),
    (['--avg-timestamp-weight', '0.5', '--compact-events'],
     '--avg-timestamp-weight cannot be combined with --compact-events'),
    # the pinned refusals of the contrast term stay, and come first
    (['--avg-timestamp-weight', '0.5', '--contrast-weight', '0.5', '--ev_images'], '--contrast-weight cannot'),
    (['--avg-timestamp-weight', '0.5', '--contrast-weight', '0.5', '--compact-events'], '--contrast-weight cannot'),
    # a frameless run still needs the contrast term: this one is an additional term there
    (['--avg-timestamp-weight', '0.5', '--recording', '/tmp/r.h5', '--window-duration', '0.04'],
     '--recording needs --contrast-weight > 0'),
])
def test_the_refusals_name_their_flag(extra, what):
    with pytest.raises(SystemExit, match=what):
        _parse(*extra)


# ------------------------------------------------------ Losses.avg_timestamp
class _Recorder:
    def __init__(self, out):
        self.calls, self.out = [], out

    def __call__(self, *args):
        self.calls.append(args)
        return self.out


def test_losses_avg_timestamp_acts_on_the_finest_flow_and_returns_what_contrast_returns(monkeypatch):
    rec, other = _Recorder((torch.tensor(0.4), torch.tensor(0.8))), _Recorder(None)
    monkeypatch.setattr(L._AvgTimestamp, 'apply', rec)
    monkeypatch.setattr(L._Contrast, 'apply', other)
    monkeypatch.setattr(L._lib, 'require_cuda', lambda *a: None)
    shapes = [(6, 10), (12, 20)]
    ev = L.Losses(shapes, 3, 'cpu')
    flows = [torch.zeros(3, 2, *s) for s in shapes]
    events = {k: torch.zeros(5, dtype=torch.long) for k in ('x', 'y', 'polarity', 'sample_index')}
    events['timestamp'] = torch.zeros(5)
    call = (flows, torch.zeros(3, 2), torch.zeros(3, dtype=torch.long), events)
    assert float(ev.avg_timestamp(*call)) == pytest.approx(0.4)
    value, term = ev.avg_timestamp(*call, weight=0.5, references=('end', 'middle', 'start'), polarity=True)
    assert float(value) == pytest.approx(0.4) and float(term) == pytest.approx(0.8)
    assert not other.calls and len(rec.calls) == 2
    first, second = rec.calls
    assert first[0] is flows[-1] and first[4] is None and first[8:] == (1.0, 5, False)     # start,end; p not handed on
    assert second[4] is events['polarity'] and second[8:] == (0.5, 7, True)
    with pytest.raises(ValueError, match='unknown reference'):
        ev.avg_timestamp(*call, references=('begin',))
    assert list(inspect.signature(L.Losses.avg_timestamp).parameters) == [
        'self', 'flows', 'flow_ts', 'flow_sample_idx', 'events', 'weight', 'references', 'polarity']
    assert inspect.signature(L.Losses.avg_timestamp).parameters['references'].default == ('start', 'end')


# ------------------------------------------------------------ combined_loss
class _Evaluator:
    """Records what it is asked for; the three frame terms are 0 + k, 10 + k, 20 + k."""

    def __init__(self):
        self.calls = []

    def __call__(self, flows, *rest, **kw):
        return tuple(tuple(torch.tensor(float(10 * t + k)) for k in range(len(flows))) for t in range(3))

    def contrast(self, flows, flow_ts, flow_sample_idx, events, weight=None, **options_):
        self.calls.append(('contrast', weight, options_))
        return torch.tensor(-0.5 * weight), torch.tensor(-0.5)

    def avg_timestamp(self, flows, flow_ts, flow_sample_idx, events, weight=None, **options_):
        assert events is not None
        self.calls.append(('avg_timestamp', weight, options_))
        return torch.tensor(0.75 * weight), torch.tensor(0.75)


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f'events.{name} was looked at')


def test_combined_loss_at_weight_zero_asks_for_nothing():
    flows = (torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 4, 4))
    ev = _Evaluator()
    call = (ev, flows, None, None, None, None, None, None)
    plain, terms = training.combined_loss(*call)
    for kw in (dict(avg_timestamp_weight=0.0), dict(avg_timestamp_weight=0, events=_Untouchable()),
               dict(avg_timestamp_references=('middle',), avg_timestamp_polarity=True, events=_Untouchable())):
        loss, terms_ = training.combined_loss(*call, **kw)
        assert float(loss) == float(plain) and type(terms_) is type(terms) is tuple
        assert not hasattr(terms_, 'avg_timestamp')
    assert not ev.calls
    assert training._avg_timestamp_keywords(0.0, ('middle',), True) == {}
    assert training._avg_timestamp_keywords(0.5, ('start', 'end'), False) == {'avg_timestamp_weight': 0.5}
    assert training._avg_timestamp_keywords(0.5, ('end',), True) == {
        'avg_timestamp_weight': 0.5, 'avg_timestamp_references': ('end',), 'avg_timestamp_polarity': True}


def test_combined_loss_adds_the_value_and_carries_the_term():
    flows = (torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 4, 4))
    ev, events = _Evaluator(), {'x': None}
    call = (ev, flows, None, None, None, None, None, None)
    plain, _ = training.combined_loss(*call)
    loss, terms = training.combined_loss(*call, avg_timestamp_weight=0.5, events=events)
    assert float(loss) == float(plain) + 0.375
    assert float(terms.avg_timestamp) == 0.75 and terms.contrast is None and len(terms) == 3
    back = training.TermReadback(terms)
    assert back.avg_timestamp() == 0.75 and back.contrast() is None and back.host()[1] == [10.0, 11.0]
    assert ev.calls == [('avg_timestamp', 0.5, {})]
    # both terms together, each with its own options
    ev.calls.clear()
    loss, terms = training.combined_loss(*call, contrast_weight=0.25, contrast_references=('start', 'end'),
                                         avg_timestamp_weight=0.5, avg_timestamp_references=('middle',),
                                         avg_timestamp_polarity=True, events=events)
    assert float(loss) == float(plain) - 0.125 + 0.375
    assert float(terms.contrast) == -0.5 and float(terms.avg_timestamp) == 0.75
    assert ev.calls == [('contrast', 0.25, {'references': ('start', 'end')}),
                        ('avg_timestamp', 0.5, {'references': ('middle',), 'polarity': True})]
    # the contrast term alone is what it was
    _, alone = training.combined_loss(*call, contrast_weight=0.25, events=events)
    assert float(alone.contrast) == -0.5 and alone.avg_timestamp is None
    assert training.TermReadback(alone).avg_timestamp() is None
    with pytest.raises(ValueError, match='avg_timestamp_weight must not be negative'):
        training.combined_loss(*call, avg_timestamp_weight=-1.0, events=events)
    with pytest.raises(ValueError, match='avg_timestamp_weight > 0 needs the raw events'):
        training.combined_loss(*call, avg_timestamp_weight=0.5)


def test_a_frameless_batch_still_needs_the_contrast_term():
    class Frameless(_Evaluator):
        def frameless(self, flows, weights):
            return torch.tensor(1.0), torch.zeros(3, len(flows))
    flows = (torch.zeros(1, 2, 2, 2),)
    call = (Frameless(), flows, None, None, None, None, None, None)
    with pytest.raises(ValueError, match='images=None needs contrast_weight > 0'):
        training.combined_loss(*call, avg_timestamp_weight=0.5, events={'x': None})
    loss, terms = training.combined_loss(*call, contrast_weight=0.25, avg_timestamp_weight=0.5, events={'x': None})
    assert float(loss) == 1.0 - 0.125 + 0.375 and float(terms.avg_timestamp) == 0.75


def test_the_new_keywords_stand_at_the_end():
    for fn in (training.combined_loss, training.process_minibatch, training.train, training.validate,
               hooks.ValidationHook.__init__):
        assert tuple(inspect.signature(fn).parameters)[-3:] == KEYS, fn
        p = inspect.signature(fn).parameters
        assert p['avg_timestamp_weight'].default == 0.0 and p['avg_timestamp_references'].default == ('start', 'end')
        assert p['avg_timestamp_polarity'].default is False


# ------------------------------------------------- train, validate, the hook
class _LoopEvaluator:
    """CPU stand-in with the Losses call signature; records what the terms were asked for."""

    def __init__(self):
        self.seen = []

    def __call__(self, flows, flow_ts, fsi, images, ts, si):
        return (tuple(f.mean() for f in flows), tuple(2 * f.mean() for f in flows),
                tuple(0 * f.mean() for f in flows))

    def contrast(self, flows, flow_ts, flow_sample_idx, events, weight=None, **rest):
        self.seen.append(('contrast', dict(rest)))
        term = -0.5 + 0 * flows[-1].mean()
        return term * weight, term.detach()

    def avg_timestamp(self, flows, flow_ts, flow_sample_idx, events, weight=None, **rest):
        self.seen.append(('avg_timestamp', dict(rest)))
        term = 0.75 + 0 * flows[-1].mean()
        return term * weight, term.detach()


class _Logger:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, v, x):
        self.rows.append((tag, float(v), x))


class _CaptureOptimizer(torch.optim.SGD):
    def begin_capture(self): pass
    def advance(self): pass
    def end_capture(self): pass


def _fake_model():
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).parent))
    from fake_flownet.net import Model as Fake
    sys.path.pop(0)
    return Fake('cpu')


def _loader(n):
    from dvs_of_training_framework_amd import synthetic
    return [synthetic.to_torch(synthetic.make_batch(i, 2, 16, 16, 10)) for i in range(n)]


def _train(ev, optimizer=torch.optim.SGD, **opts):
    from dvs_of_training_framework_amd.timer import FakeTimer
    model = _fake_model()
    opt = optimizer(model.parameters(), lr=0.1)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
    log = _Logger()
    training.train(model, 'cpu', _loader(2), opt, num_steps=1, scheduler=sch, logger=log, evaluator=ev,
                   accumulation_steps=2, timers=FakeTimer(), max_events_per_batch=10 ** 6, **opts)
    return {t: v for t, v, _ in log.rows}


def test_train_validate_and_the_hook_pass_the_keywords_on_and_log_the_term():
    ev = _LoopEvaluator()
    plain = _train(ev)
    assert not ev.seen and 'Train/avg timestamp' not in plain and 'Train/contrast' not in plain
    rows = _train(ev, avg_timestamp_weight=0.5)                 # under accumulation: the mean of two micro-batches
    assert ev.seen == [('avg_timestamp', {})] * 2
    assert rows['Train/avg timestamp'] == pytest.approx(0.75) and 'Train/contrast' not in rows
    assert rows['General/Train loss'] == pytest.approx(plain['General/Train loss'] + 0.375)
    ev.seen.clear()
    rows = _train(ev, avg_timestamp_weight=0.5, avg_timestamp_references=('start', 'middle', 'end'),
                  avg_timestamp_polarity=True, contrast_weight=0.25)
    assert ev.seen == [('contrast', {}), ('avg_timestamp', {'references': ('start', 'middle', 'end'),
                                                           'polarity': True})] * 2
    assert rows['Train/avg timestamp'] == pytest.approx(0.75) and rows['Train/contrast'] == pytest.approx(-0.5)
    ev.seen.clear()
    log = _Logger()
    training.validate(_fake_model(), 'cpu', _loader(2), 7, log, ev, avg_timestamp_weight=0.5,
                      avg_timestamp_references=('end',))
    assert ev.seen == [('avg_timestamp', {'references': ('end',)})] * 2
    assert {t: v for t, v, _ in log.rows}['Validation/avg timestamp'] == pytest.approx(0.75)
    assert 'Validation/contrast' not in {t for t, _, _ in log.rows}
    ev.seen.clear()
    log = _Logger()
    hooks.ValidationHook(_fake_model(), 'cpu', _loader(1), log, ev, [0.5, 1, 1], True, avg_timestamp_weight=0.5,
                         avg_timestamp_polarity=True)(1, 2)
    hooks.ValidationHook(_fake_model(), 'cpu', _loader(1), _Logger(), ev, [0.5, 1, 1], True,
                         avg_timestamp_polarity=True)(1, 2)     # no weight: the term is not asked for
    assert ev.seen == [('avg_timestamp', {'polarity': True})]
    assert 'Validation/avg timestamp' in {t for t, _, _ in log.rows}
    with pytest.raises(ValueError, match='avg_timestamp_weight > 0 needs raw events'):
        training.process_minibatch(_fake_model(), _loader(1)[0], None, 'cpu', False, ev, [0.5, 1, 1],
                                   avg_timestamp_weight=0.5)


def test_a_run_that_asks_for_capture_with_the_term_runs_eagerly_and_says_why(capsys):
    ev = _LoopEvaluator()
    rows = _train(ev, optimizer=_CaptureOptimizer, capture=True, avg_timestamp_weight=0.5)
    err = capsys.readouterr().err
    assert 'capture: not used, the loop runs eagerly' in err and '--avg-timestamp-weight 0.5' in err
    assert 'contrast-weight' not in err
    assert ev.seen == [('avg_timestamp', {})] * 2 and rows['Train/avg timestamp'] == pytest.approx(0.75)
    assert training.avg_timestamp_capture_refusal() is None and training.avg_timestamp_capture_refusal(0.0) is None
    assert '--avg-timestamp-weight 0.5' in training.avg_timestamp_capture_refusal(0.5)


def test_capture_refusal_is_untouched():
    assert list(inspect.signature(training.capture_refusal).parameters) == ['optimizer', 'is_raw', 'model',
                                                                           'contrast_weight']
    opt = _CaptureOptimizer([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    assert training.capture_refusal(opt, True) is None
    assert training.capture_refusal(opt, True, None, 0.0) is None
    why = training.capture_refusal(opt, True, None, 0.25)
    assert '--contrast-weight 0.25' in why and 'avg' not in why
    assert 'is_raw=False' in training.capture_refusal(opt, False)
    assert 'SGD' in training.capture_refusal(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), True)
