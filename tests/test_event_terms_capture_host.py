"""The opt-in that lets the captured step carry the events-only terms, without
a GPU: the flag ``--capture-event-terms`` and its refusals, what ``train``
decides with and without the keyword ``capture_event_terms`` (the default is the
parent's refusal, word for word), what it hands ``capture.CapturedLoop`` as
``loss_options``, ``event_terms_capture_refusal``, and the signature of framed
and frameless batches."""
import inspect

import pytest
import torch

from dvs_of_training_framework_amd import capture, options, synthetic, training
from tests.test_avg_timestamp_host import _CaptureOptimizer, _LoopEvaluator, _train


# ---------------------------------------------------------------- the flag
def _parser():
    from argparse import ArgumentParser
    return options.add_preprocessed_dataset_arguments(options.add_train_arguments(ArgumentParser()))


def _parse(*extra):
    return options.validate_train_args(_parser().parse_args(['-m', 'm'] + list(extra)))


def test_the_flag_is_absent_from_the_namespace_unless_given():
    for extra in ((), ('--capture',), ('--capture', '--contrast-weight', '0.25'),
                  ('--capture', '--avg-timestamp-weight', '0.5')):
        assert 'capture_event_terms' not in vars(_parse(*extra)), extra
    args = _parse('--capture', '--contrast-weight', '0.25', '--capture-event-terms')
    assert args.capture_event_terms is True and args.capture is True
    assert _parse('--capture', '--avg-timestamp-weight', '0.5', '--capture-event-terms').capture_event_terms is True


@pytest.mark.parametrize('extra,what', [
    (['--capture-event-terms', '--contrast-weight', '0.25'], '--capture-event-terms needs --capture'),
    (['--capture-event-terms'], '--capture-event-terms needs --capture'),
    (['--capture-event-terms', '--capture'], '--contrast-weight'),
    (['--capture-event-terms', '--capture'], '--avg-timestamp-weight'),
    (['--capture-event-terms', '--capture', '--contrast-weight', '0'], 'needs a positive --contrast-weight or'),
    (['--capture-event-terms', '--capture', '--avg-timestamp-weight', '0'], '--avg-timestamp-weight'),
])
def test_the_flag_is_refused_without_what_it_needs(extra, what):
    with pytest.raises(SystemExit) as e:
        _parse(*extra)
    assert what in str(e.value), e.value


def test_the_flag_is_accepted_on_a_frameless_run_and_the_other_refusals_stay():
    args = _parse('--recording', 'r.npz', '--window-duration', '0.05', '--contrast-weight', '0.25', '--capture',
                  '--capture-event-terms')
    assert args.capture_event_terms and args.capture and args.contrast_weight == 0.25
    run = ['--contrast-weight', '0.25', '--capture', '--capture-event-terms']
    for flag, what in (('--ev_images', '--contrast-weight cannot be combined with --ev_images'),
                       ('--compact-events', '--contrast-weight cannot be combined with --compact-events')):
        with pytest.raises(SystemExit) as e:
            _parse(*run, flag)
        assert what in str(e.value)
    with pytest.raises(SystemExit) as e:
        _parse('--recording', 'r.npz', '--window-duration', '0.05', *run, '--device-feeder')
    assert '--recording cannot be combined with --device-feeder' in str(e.value)


# ------------------------------------------------------------------- train
class _Recorder:
    """Stands where ``capture.CapturedLoop`` stands and keeps what it was given."""
    made = []

    def __init__(self, *args, **kwargs):
        self.args, self.kwargs, self.runs, self.failed, self.closed = args, kwargs, [], None, 0
        _Recorder.made.append(self)

    def run(self, batch, micro_in_step, timers=None):
        self.runs.append(micro_in_step)
        zero = torch.zeros(())
        return torch.ones(()), training.TermReadback(((zero,), (zero,), (zero,))), ['16x16']

    def close(self):
        self.closed += 1


@pytest.fixture
def recorder(monkeypatch):
    _Recorder.made = []
    monkeypatch.setattr(capture, 'CapturedLoop', _Recorder)
    return _Recorder


PARENT_LINES = {
    'avg_timestamp_weight': ('capture: not used, the loop runs eagerly: --avg-timestamp-weight 0.5: the captured '
                             'step does not carry the average-timestamp term (dvsof_avg_timestamp_fwd / '
                             'dvsof_avg_timestamp_bwd)\n', 0.5),
    'contrast_weight': ('capture: not used, the loop runs eagerly: --contrast-weight 0.25: the captured step does '
                        'not carry the contrast-maximisation term (dvsof_contrast_fwd / dvsof_contrast_bwd)\n', 0.25),
}


@pytest.mark.parametrize('keyword', sorted(PARENT_LINES))
@pytest.mark.parametrize('spelled', [False, True])
def test_the_default_is_the_parents_refusal_word_for_word(recorder, capsys, keyword, spelled):
    line, weight = PARENT_LINES[keyword]
    ev = _LoopEvaluator()
    _train(ev, optimizer=_CaptureOptimizer, capture=True, **{keyword: weight},
           **({'capture_event_terms': False} if spelled else {}))
    assert capsys.readouterr().err == line
    assert recorder.made == [] and len(ev.seen) == 2          # no loop constructed: two eager micro-batches
    assert inspect.signature(training.train).parameters['capture_event_terms'].default is False


def test_the_keyword_without_capture_or_without_a_term_changes_nothing(recorder, capsys):
    ev = _LoopEvaluator()
    _train(ev, optimizer=_CaptureOptimizer, capture=False, capture_event_terms=True, contrast_weight=0.25)
    assert recorder.made == [] and len(ev.seen) == 2 and capsys.readouterr().err == ''
    _train(ev, optimizer=_CaptureOptimizer, capture=True, capture_event_terms=True)
    assert len(recorder.made) == 1 and recorder.made[0].kwargs == {}      # the parent's call: no loss_options


@pytest.mark.parametrize('opts,want', [
    (dict(contrast_weight=0.25), {'contrast_weight': 0.25}),
    (dict(avg_timestamp_weight=0.5), {'avg_timestamp_weight': 0.5}),
    (dict(contrast_weight=0.25, contrast_references=('start',), contrast_polarity=False, contrast_scales='finest',
          avg_timestamp_weight=0.5, avg_timestamp_references=('start', 'end'), avg_timestamp_polarity=False),
     {'contrast_weight': 0.25, 'avg_timestamp_weight': 0.5}),
    (dict(contrast_weight=0.25, contrast_scales='all', contrast_references=('start', 'middle', 'end'),
          contrast_polarity=True, avg_timestamp_weight=0.5, avg_timestamp_polarity=True,
          avg_timestamp_references=('end',)),
     {'contrast_weight': 0.25, 'contrast_scales': 'all', 'contrast_references': ('start', 'middle', 'end'),
      'contrast_polarity': True, 'avg_timestamp_weight': 0.5, 'avg_timestamp_polarity': True,
      'avg_timestamp_references': ('end',)}),
])
def test_opted_in_the_loop_is_made_once_with_the_merged_keywords(recorder, capsys, opts, want):
    ev = _LoopEvaluator()
    _train(ev, optimizer=_CaptureOptimizer, capture=True, capture_event_terms=True, **opts)
    assert capsys.readouterr().err == ''
    assert len(recorder.made) == 1
    loop = recorder.made[0]
    assert loop.kwargs == {'loss_options': want}
    # ... which is what train hands process_minibatch in the eager loop
    assert want == dict(training._contrast_keywords(
        opts.get('contrast_weight', 0.0), opts.get('contrast_references', ('start',)),
        opts.get('contrast_polarity', False), opts.get('contrast_scales', 'finest')),
        **training._avg_timestamp_keywords(opts.get('avg_timestamp_weight', 0.0),
                                           opts.get('avg_timestamp_references', ('start', 'end')),
                                           opts.get('avg_timestamp_polarity', False)))
    assert loop.args[1] is ev and loop.args[5] == 2           # evaluator, accumulation steps
    assert loop.runs == [0, 1] and loop.closed == 1           # one run per micro-batch (_train: two of them)
    assert ev.seen == []                                      # nothing ran eagerly beside the loop


def test_what_still_refuses_opted_in(recorder, capsys):
    ev = _LoopEvaluator()
    _train(ev, capture=True, capture_event_terms=True, contrast_weight=0.25)     # torch.optim.SGD: no protocol
    err = capsys.readouterr().err
    assert err.startswith('capture: not used, the loop runs eagerly: optimizer SGD has no begin_capture')
    assert recorder.made == [] and len(ev.seen) == 2

    class NoTerms:
        def __call__(self, *a):
            raise AssertionError

    why = training.event_terms_capture_refusal(NoTerms(), True)
    assert 'NoTerms' in why and 'contrast' in why and 'avg_timestamp' in why and 'frameless' not in why.split('(')[0]
    assert 'frameless' in training.event_terms_capture_refusal(ev, True, needs=training.EVENT_TERM_METHODS)
    assert training.event_terms_capture_refusal(ev, True) is None
    assert 'is_raw=False' in training.event_terms_capture_refusal(ev, False)
    assert list(inspect.signature(training.event_terms_capture_refusal).parameters)[:2] == ['evaluator', 'is_raw']

    class OnlyContrast(_LoopEvaluator):
        avg_timestamp = None
    one = OnlyContrast()
    _train(one, optimizer=_CaptureOptimizer, capture=True, capture_event_terms=True, contrast_weight=0.25)
    assert len(recorder.made) == 1 and capsys.readouterr().err == ''          # the term it lacks is not asked for
    with pytest.raises(TypeError):      # ... and where it is, the run is eager and says why, then meets the None
        _train(one, optimizer=_CaptureOptimizer, capture=True, capture_event_terms=True, avg_timestamp_weight=0.5)
    err = capsys.readouterr().err
    assert 'capture: not used, the loop runs eagerly: evaluator OnlyContrast has no avg_timestamp' in err
    assert len(recorder.made) == 1


def test_the_pinned_refusals_are_as_they_were():
    assert list(inspect.signature(training.capture_refusal).parameters) == ['optimizer', 'is_raw', 'model',
                                                                           'contrast_weight']
    assert list(inspect.signature(training.avg_timestamp_capture_refusal).parameters) == ['avg_timestamp_weight']
    opt = _CaptureOptimizer([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    assert training.capture_refusal(opt, True, None, 0.25) == PARENT_LINES['contrast_weight'][0].split(': ', 2)[2][:-1]
    assert training.avg_timestamp_capture_refusal(0.5) == PARENT_LINES['avg_timestamp_weight'][0].split(': ', 2)[2][:-1]


# ------------------------------------------------------------- signatures
def _frameless(batch, shape):
    out = dict(batch, images=None)
    out['shape'] = shape
    return out


def test_signatures_of_framed_and_frameless_batches():
    sig = capture.CapturedTrainStep._signature
    framed = synthetic.to_torch(synthetic.make_batch(3, 2, 16, 24, 10))
    assert sig(framed) == (2, tuple(framed['images'].shape), tuple(framed['timestamps'].shape), False)
    bare = _frameless(framed, (16, 24))
    assert sig(bare) == (2, ('frameless', 16, 24), tuple(framed['timestamps'].shape), False)
    assert sig(bare) != sig(framed)
    assert sig(_frameless(framed, (24, 16))) != sig(bare) and sig(_frameless(framed, (16, 32))) != sig(bare)
    assert sig(_frameless(framed, torch.Size([16, 24]))) == sig(bare)        # whatever sequence type holds it
    # loss_options are a constructor keyword of the step, the loop and the fall-back body
    for cls in (capture.CapturedTrainStep, capture.CapturedLoop, capture._EagerBody):
        assert inspect.signature(cls.__init__).parameters['loss_options'].default is None
