"""Train / validate loops behind the reference's surface (utils/training.py).

Public names, signatures, return structures, hook protocol and TensorBoard
tags are the reference's: ``combined_loss`` (:12-24), ``make_hook_periodic``
(:27-30), ``process_minibatch`` (:37-86), ``train`` (:89-235), ``validate``
(:244-271).  The organisation underneath is this build's:

  * ``TermReadback``   the 3 x n_scales loss terms of one micro-batch as host
                       floats, fetched by ONE packed device->host copy at first
                       use (the reference makes 12 ``.item()`` syncs, :77);
  * ``ScaleSums``      per-scale running sums between optimizer steps and the
                       scalar tags they are written under;
  * ``_StepClock``     micro-batch / optimizer-step / sample counters and the
                       oversize-batch bookkeeping (:141-150);
  * ``train``          drives them; ``reducer`` (parallel.GradReducer) adds
                       the data-parallel gradient exchange: buckets are
                       all-reduced on a side stream during backward and joined
                       before ``optimizer.step()``; micro-batches that only
                       accumulate do not exchange;
  * ``HostGuard``      gradient clipping and the skip of a non-finite step
                       for an optimizer that has no device-side guard
                       (``torch.optim`` on the CPU); the fused optimizers
                       carry their own (optim.set_guard,
                       docs/STEP_GUARD_SPEC.md).  ``train`` reads either at
                       logging steps only.
"""
import torch

from .common import mean
from .loss import unit_backward
from .timer import EventTimer, FakeTimer

TERM_NAMES = ('smoothness', 'photometric', 'out_reg')       # order of :171
STAGES = ('batch_construction', 'batch2gpu', 'forward', 'loss', 'backprop',
          'optimizer_step', 'logging')


# --------------------------------------------------------------------- loss
class _Terms(tuple):
    """((smooth_k), (photo_k), (border_k)) of 0-dim tensors that are views of
    one [3,K] tensor (``packed``): host readers fetch it in one copy."""
    def __new__(cls, packed):
        self = super().__new__(cls, (tuple(r.unbind(0))
                                     for r in packed.unbind(0)))
        self.packed = packed
        return self


class _TermsAndContrast(tuple):
    """The terms structure as it is, carrying the contrast-maximisation term
    of the micro-batch beside it (``contrast``: a 0-dim device tensor) and,
    where the loss has one, the average-timestamp term (``avg_timestamp``,
    likewise; either is None where the loss has none, and the [K] tensor of
    the levels' terms where it is taken on every scale)."""
    def __new__(cls, terms, contrast, avg_timestamp=None):
        self = super().__new__(cls, terms)
        self.packed = getattr(terms, 'packed', None)
        self.contrast = contrast
        self.avg_timestamp = avg_timestamp
        return self


def _contrast_options(references, polarity, scales='finest'):
    """The keywords of ``Losses.contrast`` that differ from its defaults, so
    that a run without them makes the call it always made."""
    out = {}
    if scales != 'finest':
        out['scales'] = scales
    if tuple(references) != ('start',):
        out['references'] = tuple(references)
    if polarity:
        out['polarity'] = True
    return out


def _contrast_keywords(weight, references, polarity, scales='finest'):
    """What a call down the chain gets: nothing at weight 0, and the options
    only where they differ from the defaults."""
    if not weight:
        return {}
    return dict({'contrast_weight': weight},
                **{'contrast_' + k: v for k, v in _contrast_options(references, polarity, scales).items()})


AVG_TIMESTAMP_REFERENCES = ('start', 'end')


def _avg_timestamp_options(references, polarity, scales='finest'):
    """The keywords of ``Losses.avg_timestamp`` that differ from its defaults;
    with 'scales' among them the call goes to ``Losses.avg_timestamp_scales``."""
    out = {}
    if scales != 'finest':
        out['scales'] = scales
    if tuple(references) != AVG_TIMESTAMP_REFERENCES:
        out['references'] = tuple(references)
    if polarity:
        out['polarity'] = True
    return out


def _avg_timestamp_keywords(weight, references, polarity, scales='finest'):
    """What a call down the chain gets: nothing at weight 0, and the options
    only where they differ from the defaults."""
    if not weight:
        return {}
    return dict({'avg_timestamp_weight': weight},
                **{'avg_timestamp_' + k: v
                   for k, v in _avg_timestamp_options(references, polarity, scales).items()})


def combined_loss(evaluator, flows, flow_ts, flow_sample_idx, images,
                  timestamps, sample_idx, features, weights=[0.5, 1, 1],
                  frame_indices=None, contrast_weight=0.0, events=None,
                  contrast_references=('start',), contrast_polarity=False,
                  contrast_scales='finest', avg_timestamp_scales='finest',
                  avg_timestamp_weight=0.0,
                  avg_timestamp_references=AVG_TIMESTAMP_REFERENCES,
                  avg_timestamp_polarity=False):
    """-> (sum_t weights[t] * mean_k term[t][k], terms).  With an evaluator
    that has ``fused`` and flows that need gradients the value and the flow
    gradients come out of one sweep (loss.Losses.fused).

    contrast_weight > 0: plus contrast_weight * the contrast-maximisation term
    of the finest flow over ``events``, the wire columns on the device or the
    compact ones (voxel.is_compact; the same bytes either way, CONTRAST_SPEC
    section 24) (loss.Losses.contrast, docs/CONTRAST_SPEC.md); the term rides on the
    returned terms as ``.contrast``.  At 0 nothing of that is constructed and
    ``events`` is not looked at.  contrast_references, contrast_polarity: the
    reference times of the term and whether ON and OFF events are kept apart
    (``Losses.contrast``); the defaults are the term of one image per frame.
    contrast_scales='all': the term of every flow, each level weighing
    contrast_weight / K (CONTRAST_SPEC sections 19-23); ``.contrast`` is then
    the [K] tensor of the levels' terms.  'finest', the default, is the call
    as it was.

    avg_timestamp_weight > 0: plus avg_timestamp_weight * the average-timestamp
    term of the finest flow over ``events`` (loss.Losses.avg_timestamp,
    docs/AVG_TIMESTAMP_SPEC.md), beside the contrast term or without it; the
    term rides on the returned terms as ``.avg_timestamp``.  At 0 nothing of
    that is constructed and ``events`` is not looked at.
    avg_timestamp_scales='all': the term of every flow, each level weighing
    avg_timestamp_weight / K (loss.Losses.avg_timestamp_scales,
    AVG_TIMESTAMP_SPEC sections 11-15); ``.avg_timestamp`` is then the [K]
    tensor of the levels' terms.  'finest', the default, is the call as it was.

    images=None with an evaluator that has ``frameless`` (loss.Losses): a
    frameless batch (docs/FRAMELESS_SPEC.md).  That method gives smoothness
    and out-of-border with the weights (weights[0], weights[2]) and a
    photometric row of zeros; ``timestamps``
    and ``sample_idx`` are not looked at; the contrast term is added as above
    and has to be there (ValueError at contrast_weight 0: smoothness alone has
    no data term)."""
    extra = {} if frame_indices is None else {'frame_indices': frame_indices}
    call = (flows, flow_ts, flow_sample_idx, images, timestamps, sample_idx)
    trainable = torch.is_grad_enabled() and \
        any(f.requires_grad for f in flows)
    if images is None and hasattr(evaluator, 'frameless'):
        # a frameless batch (docs/FRAMELESS_SPEC.md): smoothness and
        # out-of-border alone, no frame is read; the contrast term below is
        # the data term.  (An evaluator without ``frameless`` is handed the
        # None as before: what it makes of it is its own business.)
        if not contrast_weight:
            raise ValueError('images=None needs contrast_weight > 0: without frames the '
                             'contrast-maximisation term is the only data term, smoothness '
                             'alone has none')
        loss, packed = evaluator.frameless(flows, weights=(weights[0], weights[2]))
        terms = _Terms(packed)
    elif trainable and hasattr(evaluator, 'fused'):
        loss, packed = evaluator.fused(*call, weights=weights, **extra)
        terms = _Terms(packed)
    else:
        terms = evaluator(*call, **extra)
        loss = 0
        for weight, per_scale in zip(weights, terms):
            loss = loss + weight * mean(per_scale)
    if not contrast_weight and not avg_timestamp_weight:
        return loss, terms
    term = avg_term = None
    if contrast_weight:
        if contrast_weight < 0:
            raise ValueError(f'contrast_weight must not be negative, got {contrast_weight}')
        if events is None:
            raise ValueError('contrast_weight > 0 needs the raw events of the batch on the device '
                             '(is_raw=True); preprocessed voxel grids carry none')
        value, term = evaluator.contrast(flows, flow_ts, flow_sample_idx, events,
                                         weight=contrast_weight, **_contrast_options(
                                             contrast_references, contrast_polarity, contrast_scales))
        loss = loss + value
    if avg_timestamp_weight:
        if avg_timestamp_weight < 0:
            raise ValueError(f'avg_timestamp_weight must not be negative, got {avg_timestamp_weight}')
        if events is None:
            raise ValueError('avg_timestamp_weight > 0 needs the raw events of the batch on the device '
                             '(is_raw=True); preprocessed voxel grids carry none')
        options = _avg_timestamp_options(avg_timestamp_references, avg_timestamp_polarity, avg_timestamp_scales)
        method = evaluator.avg_timestamp_scales if 'scales' in options else evaluator.avg_timestamp
        value, avg_term = method(flows, flow_ts, flow_sample_idx, events, weight=avg_timestamp_weight, **options)
        loss = loss + value
    return loss, _TermsAndContrast(terms, term, avg_term)


class TermReadback:
    """Host view of the loss terms of one micro-batch.

    Iterating yields one iterator of floats per term (smoothness,
    photometric, out-of-border) -- the structure ``process_minibatch``
    returns in the reference -- and ``host()`` the whole table.  Nothing is
    copied until a value is asked for; then everything is, once."""

    def __init__(self, terms):
        self._terms = terms
        self.n_terms = len(terms)
        self.n_scales = len(terms[0]) if self.n_terms else 0
        self._table = None
        self._contrast = getattr(terms, 'contrast', None)
        self._contrast_levels = None
        self._avg_timestamp = getattr(terms, 'avg_timestamp', None)
        self._avg_timestamp_levels = None

    def avg_timestamp(self):
        """The average-timestamp term as a host float (one small copy), None
        when the loss has none; with the term on every scale the mean of the
        levels' terms."""
        if isinstance(self._avg_timestamp, torch.Tensor):
            if self._avg_timestamp.dim() == 1:
                self._avg_timestamp_levels = self._avg_timestamp.tolist()
                self._avg_timestamp = sum(self._avg_timestamp_levels) / len(self._avg_timestamp_levels)
            else:
                self._avg_timestamp = float(self._avg_timestamp)
        return self._avg_timestamp

    def avg_timestamp_levels(self):
        """The levels' average-timestamp terms as host floats, coarsest first;
        None unless the term is taken on every scale."""
        self.avg_timestamp()
        return self._avg_timestamp_levels

    def contrast(self):
        """The contrast-maximisation term as a host float (one small copy),
        None when the loss has none; with the term on every scale the mean of
        the levels' terms."""
        if isinstance(self._contrast, torch.Tensor):
            if self._contrast.dim() == 1:
                self._contrast_levels = self._contrast.tolist()
                self._contrast = sum(self._contrast_levels) / len(self._contrast_levels)
            else:
                self._contrast = float(self._contrast)
        return self._contrast

    def contrast_levels(self):
        """The levels' terms as host floats, coarsest first; None unless the
        term is taken on every scale."""
        self.contrast()
        return self._contrast_levels

    def host(self):
        if self._table is None:
            packed = getattr(self._terms, 'packed', None)
            if packed is None:
                packed = torch.stack([torch.stack(list(t))
                                      for t in self._terms])
            self._table = packed.detach().cpu().tolist()
            self._terms = None
        return self._table

    def row(self, t):
        """Floats of term ``t``, one per scale (a generator: still lazy)."""
        return (self.host()[t][k] for k in range(self.n_scales))

    def __len__(self):
        return self.n_terms

    def __iter__(self):
        # row(t) binds t per call: unpacking all rows first and reading them
        # afterwards gives three different rows
        return iter([self.row(t) for t in range(self.n_terms)])


def _lazy_items(terms):
    return TermReadback(terms)


def make_hook_periodic(hook, checkpointing_interval):
    def periodic(step, *args):
        if step % checkpointing_interval == 0:
            return hook(step, *args)
        return None
    return periodic


def predictions2tag(predictions):
    return (f'{p.shape[-2]}x{p.shape[-1]}' for p in predictions)


# ---------------------------------------------------------------- one batch
def _to_device(batch, device, is_raw):
    def put(t):
        return t.to(device, non_blocking=True)
    frames = tuple(put(batch[k]) for k in ('timestamps', 'sample_idx'))
    # (a frameless batch carries 'images': None and its size as 'shape')
    frames += (None if batch['images'] is None else put(batch['images']),)
    if not is_raw:
        return frames + (put(batch['data']),)
    events = batch['events']
    for name in [k for k in events if k != 'size']:
        events[name] = put(events[name])
    return frames + (events,)


def process_minibatch(model, batch, timers, device, is_raw, evaluator,
                      weights, return_prediction=False, contrast_weight=0.0,
                      contrast_references=('start',), contrast_polarity=False,
                      contrast_scales='finest', avg_timestamp_scales='finest',
                      avg_timestamp_weight=0.0,
                      avg_timestamp_references=AVG_TIMESTAMP_REFERENCES,
                      avg_timestamp_polarity=False):
    """batch (SURVEY 8b wire format, or compact event columns:
    voxel.is_compact) -> (loss, terms, tags[, outputs]).
    contrast_weight > 0 (raw events only, in either column form), contrast_references,
    contrast_polarity, contrast_scales, and avg_timestamp_weight > 0 (raw
    events only) with its references, polarity and scales: see ``combined_loss``.  A frameless batch
    (``'images': None``, ``'shape': (h, w)``; sequence.EventWindowLoader) takes
    the frame size from ``'shape'`` and the loss that reads no frame."""
    contrast = _contrast_keywords(contrast_weight, contrast_references, contrast_polarity, contrast_scales)
    if contrast and not is_raw:
        raise ValueError('contrast_weight > 0 needs raw events (is_raw=True)')
    avg = _avg_timestamp_keywords(avg_timestamp_weight, avg_timestamp_references, avg_timestamp_polarity,
                                  avg_timestamp_scales)
    if avg and not is_raw:
        raise ValueError('avg_timestamp_weight > 0 needs raw events (is_raw=True)')
    if avg:
        contrast = dict(contrast, **avg)
    with _timed(timers, 'batch2gpu'):
        timestamps, sample_idx, images, payload = _to_device(batch, device,
                                                             is_raw)
    with _timed(timers, 'forward'):
        hints = {}
        if hasattr(model, 'last_frame_indices') and 'size' in batch:
            hints['batch_size'] = int(batch['size'])    # B without a device sync
        shape = tuple(batch['shape']) if images is None else images.size()[-2:]
        flows, flow_ts, flow_sample_idx, features = model(
            payload, timestamps, sample_idx, shape, raw=is_raw,
            intermediate=True, **hints)
        tags = predictions2tag(flows)
    with _timed(timers, 'loss'):
        loss, terms = combined_loss(
            evaluator, flows, flow_ts, flow_sample_idx, images, timestamps,
            sample_idx, features, weights=weights,
            frame_indices=getattr(model, 'last_frame_indices', None),
            **(dict(contrast, events=payload) if contrast else {}))
        terms = TermReadback(terms)
    if not return_prediction:
        return loss, terms, tags
    return loss, terms, tags, {'prediction': flows, 'flow_ts': flow_ts,
                               'flow_sample_idx': flow_sample_idx,
                               'features': features}


class _timed:
    """``with _timed(timers, name):`` = timers(name).start() / .stop()."""
    def __init__(self, timers, name):
        self.t = timers(name)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *exc):
        self.t.stop()
        return False


# ------------------------------------------------------------- bookkeeping
class ScaleSums:
    """Per-scale sums of the three terms and of the loss since the last
    optimizer step (train) or over a whole pass (validate)."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.per_term = None        # [term][scale]
        self.loss = 0.0
        self.contrast = None        # sum of the contrast-maximisation term, if the loss has one
        self.contrast_levels = None  # and per level, if it is taken on every scale
        self.avg_timestamp = None   # sum of the average-timestamp term, if the loss has one
        self.avg_timestamp_levels = None    # and per level, if it is taken on every scale
        self.tags = None

    def add(self, loss, readback, tags):
        rows = [list(r) for r in readback]
        if self.per_term is None:
            self.per_term = rows
        else:
            self.per_term = [[a + b for a, b in zip(acc, new)]
                             for acc, new in zip(self.per_term, rows)]
        self.loss += loss.item()
        extra = readback.contrast() if hasattr(readback, 'contrast') else None
        if extra is not None:
            self.contrast = (self.contrast or 0.0) + extra
            levels = readback.contrast_levels() if hasattr(readback, 'contrast_levels') else None
            if levels is not None:
                self.contrast_levels = [a + b for a, b in zip(self.contrast_levels or [0.0] * len(levels), levels)]
        extra = readback.avg_timestamp() if hasattr(readback, 'avg_timestamp') else None
        if extra is not None:
            self.avg_timestamp = (self.avg_timestamp or 0.0) + extra
            levels = readback.avg_timestamp_levels() if hasattr(readback, 'avg_timestamp_levels') else None
            if levels is not None:
                self.avg_timestamp_levels = [a + b for a, b in
                                             zip(self.avg_timestamp_levels or [0.0] * len(levels), levels)]
        self.tags = list(tags)

    def write(self, logger, x, divisor, families):
        """families: per term the tag prefix, in TERM_NAMES order."""
        for k, tag in enumerate(self.tags):
            for t, family in families:
                logger.add_scalar(f'{family}/{tag}',
                                  self.per_term[t][k] / divisor, x)


_TRAIN_FAMILIES = ((1, 'Train/photometric loss'), (0, 'Train/smoothness loss'),
                   (2, 'Train/out regularization'))
_VALID_FAMILIES = ((0, 'Validation/smoothness loss'),
                   (1, 'Validation/photometric loss'),
                   (2, 'Validation/out regularization loss'))


class _StepClock:
    """Counts micro-batches (``micro``), derives optimizer steps and keeps
    ``samples_passed``; knows which micro-batch closes an optimizer step."""

    def __init__(self, init_step, accumulation_steps, num_steps,
                 init_samples_passed):
        self.accum = accumulation_steps
        self.first = self.micro = init_step * accumulation_steps
        self.last = num_steps * accumulation_steps
        self.samples = init_samples_passed
        self.skipped = 0

    def finished(self):
        return self.micro == self.last

    def admit(self, batch):
        self.micro += 1
        self.samples += batch['size']
        return self.micro % self.accum == 0

    @property
    def step(self):
        return self.micro // self.accum

    def skip(self, num_events, batch):
        self.skipped += 1
        done = self.micro - self.first
        print(f'batch of {num_events} events exceeds max_events_per_batch: '
              f'skipped (augmentation {batch.get("augmentation_params")}); '
              f'{done / (done + self.skipped):.2f} of the batches seen so far '
              'were processed')


# -------------------------------------------------------------------- loops
# what capture.CapturedTrainStep asks of an optimizer (optim._FusedBase)
CAPTURE_PROTOCOL = ('begin_capture', 'advance', 'end_capture')


class HostGuard:
    """The step guard of docs/STEP_GUARD_SPEC.md for an optimizer without a
    device-side one: ``torch.nn.utils.clip_grad_norm_`` and a finite check
    before ``optimizer.step()``, with a host synchronisation per step (fine
    on the CPU).  ``admit(optimizer)`` -> may the step update?  Counters as in
    the device record (``state()``)."""

    def __init__(self, max_norm=None, skip_nonfinite=True):
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.record = dict(scale=1.0, skip=False, norm=0.0, bad=0, skipped=0,
                           clipped=0, consecutive=0)

    def admit(self, optimizer):
        grads = [p.grad for g in optimizer.param_groups for p in g['params']
                 if p.grad is not None and p.grad.numel()]
        r = self.record
        r['bad'] = int(sum(int((~torch.isfinite(g)).sum()) for g in grads))
        r['skip'] = bool(r['bad']) and self.skip_nonfinite
        r['scale'] = 1.0
        if r['bad']:
            r['norm'] = float('nan')
        else:
            r['norm'] = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads))) \
                if grads else 0.0
            if self.max_norm is not None:
                r['scale'] = min(1.0, self.max_norm / (r['norm'] + 1e-6))
                torch.nn.utils.clip_grad_norm_(
                    [p for g in optimizer.param_groups for p in g['params']],
                    self.max_norm)
        r['skipped'] += int(r['skip'])
        r['clipped'] += int(r['scale'] < 1.0)
        r['consecutive'] = r['consecutive'] + 1 if r['skip'] else 0
        return not r['skip']

    def state(self):
        return dict(self.record)


def guard_readout(optimizer, host_guard=None):
    """The guard record of this run as a dict, or None without a guard: the
    device record of a fused optimizer (one 32-byte copy, which waits for the
    device) or the HostGuard's."""
    if getattr(optimizer, '_guard', None) is not None:
        return optimizer.guard_state()
    return host_guard.state() if host_guard is not None else None


def capture_refusal(optimizer, is_raw, model=None, contrast_weight=0.0):
    """Why ``train(capture=True)`` cannot replay its steps (None: it can)."""
    if contrast_weight:
        return (f'--contrast-weight {contrast_weight}: the captured step does not carry the '
                'contrast-maximisation term (dvsof_contrast_fwd / dvsof_contrast_bwd)')
    if not all(hasattr(optimizer, m) for m in CAPTURE_PROTOCOL):
        return (f'optimizer {type(optimizer).__name__} has no begin_capture / advance / '
                'end_capture (optim.FusedAdamW, FusedRAdam and FusedRanger do)')
    if not is_raw:
        return 'is_raw=False batches (preprocessed voxel grids) are not captured'
    layer = getattr(model, 'quantization_layer', None)
    if layer is not None and any(True for _ in layer.parameters()) and \
            not getattr(layer, 'capture_ready', False):
        # (capture_ready: net.LearnedVoxelGrid.make_resident -- the gradient of the knots
        # lives in a persistent slot the captured kernels write, strictly opt-in)
        return ('the event representation has parameters (net.LearnedVoxelGrid): the '
                'captured step does not carry their gradient and update')
    return None


def avg_timestamp_capture_refusal(avg_timestamp_weight=0.0):
    """Why ``train(capture=True)`` cannot replay a step that holds the
    average-timestamp term (None: there is none); asked before
    ``capture_refusal``."""
    if avg_timestamp_weight:
        return (f'--avg-timestamp-weight {avg_timestamp_weight}: the captured step does not carry the '
                'average-timestamp term (dvsof_avg_timestamp_fwd / dvsof_avg_timestamp_bwd)')
    return None


EVENT_TERM_METHODS = ('contrast', 'avg_timestamp', 'frameless')


def event_terms_capture_refusal(evaluator, is_raw, needs=EVENT_TERM_METHODS[:2]):
    """Why ``train(capture=True, capture_event_terms=True)`` cannot replay a
    step that holds an events-only term (None: it can), beyond what
    ``capture_refusal(optimizer, is_raw, model)`` says.  needs: the evaluator's
    methods the run will call, among ``EVENT_TERM_METHODS`` (``train`` names
    those of the terms whose weight is positive; 'frameless' for a caller that
    knows its batches carry no frames)."""
    if not is_raw:
        return ('is_raw=False batches (preprocessed voxel grids) carry no events: the '
                'events-only terms cannot be computed, let alone captured')
    missing = [m for m in needs if not callable(getattr(evaluator, m, None))]
    if missing:
        return (f'evaluator {type(evaluator).__name__} has no {" / ".join(missing)} '
                '(loss.Losses has contrast, avg_timestamp and frameless): the captured step '
                'records the evaluator\'s own kernels')
    return None


def train(model, device, loader, optimizer, num_steps: int, scheduler, logger,
          evaluator, weights=[0.5, 1, 1], is_raw=True, accumulation_steps=1,
          timers=None, hooks={}, init_step=0, init_samples_passed=0,
          max_events_per_batch: int = 350000, reducer=None,
          log_every: int = 1, capture=False, guard=None,
          max_skipped_steps: int = 32, guard_agreement_every: int = 0,
          contrast_weight: float = 0.0, contrast_references=('start',),
          contrast_polarity: bool = False, contrast_scales: str = 'finest',
          capture_event_terms: bool = False, avg_timestamp_scales: str = 'finest',
          avg_timestamp_weight: float = 0.0, avg_timestamp_references=AVG_TIMESTAMP_REFERENCES,
          avg_timestamp_polarity: bool = False):
    """Semantics of utils/training.py:89-235: ``accumulation_steps``
    micro-batches per optimizer step (each loss scaled by 1/accumulation_steps),
    batches above ``max_events_per_batch`` events are skipped and not counted,
    optimizer + scheduler step on the boundary, per-scale scalars against
    ``samples_passed``, then ``hooks[name](step, samples_passed)``.

    reducer:   parallel.GradReducer (data parallelism)
    log_every: write scalars every n-th optimizer step (1 = the reference)
    capture:   replay the loop body from ONE C call per micro-batch
               (capture.CapturedLoop / the step executor) once a batch
               signature has been seen: raw events (wire or compact columns),
               with or without accumulation, with or without a reducer (the
               gradient exchange is then issued by the executor).  A batch of
               another signature runs the same body eagerly; more events than
               the captured buffers hold re-records at a larger capacity; if
               recording fails training continues eagerly.  An optimizer
               without begin_capture / advance / end_capture, is_raw=False
               or a model whose event representation has parameters (unless
               it is resident: net.LearnedVoxelGrid.make_resident) runs the
               eager loop and says so on stderr
    guard:     HostGuard for an optimizer without a device-side step guard
               (a fused optimizer carries its own: optim.set_guard).  With
               either, ``General/gradient norm`` and ``General/skipped steps``
               are written at logging steps -- the record is read only there,
               so a step that is not logged never waits for the device -- and
               the run ends with a RuntimeError once ``max_skipped_steps``
               steps in a row were skipped
    guard_agreement_every:  under data parallelism, compare the guard's
               counters across ranks at logged steps that are multiples of
               this (the checkpointing interval; 0: never)
    contrast_weight:  > 0 adds this times the contrast-maximisation term of
               the finest flow to the loss (docs/CONTRAST_SPEC.md; raw events
               only), logged as ``Train/contrast``; such a run is
               captured with ``capture_event_terms`` only.  0: the step
               launches what it launches without it
    contrast_references, contrast_polarity:  the reference times of that term
               ('start', 'middle', 'end') and whether ON and OFF events are
               accumulated apart (``loss.Losses.contrast``)
    contrast_scales:  'all' takes that term on every flow scale, each level
               weighing contrast_weight / K; ``Train/contrast`` is then the
               mean of the levels' terms and ``Train/contrast/<tag>`` each
               level's.  'finest' (the default): the finest flow alone
    avg_timestamp_weight:  > 0 adds this times the average-timestamp term of
               the finest flow to the loss (docs/AVG_TIMESTAMP_SPEC.md; raw
               events only), logged as ``Train/avg timestamp``, beside the
               contrast term or without it; such a run is captured with
               ``capture_event_terms`` only.  0:
               the step launches what it launches without it
    avg_timestamp_references, avg_timestamp_polarity:  the reference times of
               that term (default: both ends of the window) and whether ON
               and OFF events are accumulated apart
    avg_timestamp_scales:  'all' takes that term on every flow scale, each
               level weighing avg_timestamp_weight / K; ``Train/avg
               timestamp`` is then the mean of the levels' terms and
               ``Train/avg timestamp/<tag>`` each level's.  'finest' (the
               default): the finest flow alone.  (By name, like
               ``capture_event_terms`` beside which it stands)
    capture_event_terms:  with ``capture`` and a positive contrast_weight or
               avg_timestamp_weight: the captured step carries those terms
               (their keywords travel as ``CapturedLoop(loss_options=...)``)
               and frameless batches, instead of refusing for the weights;
               ``Train/contrast``, ``Train/contrast/<tag>`` and ``Train/avg
               timestamp`` are then logged from replays.  What
               ``capture_refusal(optimizer, is_raw, model)`` and
               ``event_terms_capture_refusal`` name still runs the eager loop
               and says so.  False (the default): every decision, line on
               stderr and launch as without the keyword.  (Pass it by name: it
               stands in front of the avg_timestamp keywords, whose place at
               the end is held by a test)

    A loader of frameless batches (sequence.EventWindowLoader: is_raw=True,
    ``'images': None``) needs contrast_weight > 0; the photometric rows are
    then logged as 0 (docs/FRAMELESS_SPEC.md).
    """
    if timers is None:
        on_gpu = torch.device(device).type == 'cuda'
        timers = EventTimer() if on_gpu else FakeTimer()
    clock = _StepClock(init_step, accumulation_steps, num_steps,
                       init_samples_passed)
    sums = ScaleSums()
    captured = None
    # the opt-in: the captured step carries the events-only terms that are asked for
    event_terms = {}
    if capture and capture_event_terms:
        event_terms = dict(
            _contrast_keywords(contrast_weight, contrast_references, contrast_polarity, contrast_scales),
            **_avg_timestamp_keywords(avg_timestamp_weight, avg_timestamp_references,
                                      avg_timestamp_polarity, avg_timestamp_scales))
    if event_terms:
        avg_method = 'avg_timestamp' if avg_timestamp_scales == 'finest' else 'avg_timestamp_scales'
        refused = capture_refusal(optimizer, is_raw, model) or event_terms_capture_refusal(
            evaluator, is_raw, [m for m, w in zip((EVENT_TERM_METHODS[0], avg_method),
                                                  (contrast_weight, avg_timestamp_weight)) if w])
    else:
        refused = (avg_timestamp_capture_refusal(avg_timestamp_weight)
                   or capture_refusal(optimizer, is_raw, model, contrast_weight)) if capture else None
    if refused:
        import sys
        print(f'capture: not used, the loop runs eagerly: {refused}', file=sys.stderr)
    elif capture:
        from .capture import CapturedLoop
        captured = CapturedLoop(model, evaluator, optimizer, weights, device,
                                accumulation_steps, reducer,
                                **({'loss_options': event_terms} if event_terms else {}))
    model.train()
    optimizer.zero_grad(set_to_none=True)

    timers('batch_construction').start()
    for batch in loader:
        if clock.finished():
            break
        if is_raw:
            # (a feed.DeviceFeeder batch is padded to its slot's capacity)
            num_events = batch.get('num_events', batch['events']['x'].numel())
            if num_events > max_events_per_batch:
                clock.skip(num_events, batch)
                continue
        timers('batch_construction').stop()
        closes_step = clock.admit(batch)
        if reducer is not None:
            reducer.enabled = closes_step
        if hasattr(optimizer, 'fused_active'):      # optim.fuse_into_backward
            optimizer.fused_active = closes_step

        replayed = False
        if captured is not None and captured.failed is None:
            # the whole body of this micro-batch -- model, loss, backward and,
            # when it closes the step, exchange + optimizer -- replayed,
            # recorded (its first occurrence runs eagerly) or run eagerly
            loss, terms, tags = captured.run(
                batch, (clock.micro - 1) % accumulation_steps, timers)
            replayed = True
        if not replayed:
            loss, terms, tags = process_minibatch(
                model, batch, timers, device, is_raw, evaluator, weights,
                **_contrast_keywords(contrast_weight, contrast_references, contrast_polarity,
                                     contrast_scales),
                **_avg_timestamp_keywords(avg_timestamp_weight, avg_timestamp_references,
                                          avg_timestamp_polarity, avg_timestamp_scales))
            with _timed(timers, 'backprop'):
                if accumulation_steps == 1:
                    unit_backward(loss)     # seed 1.0: no fill, no scaling pass
                else:
                    loss /= accumulation_steps
                    loss.backward()
            if hasattr(model, 'strict'):
                model.strict = False        # layout was validated on batch one

        if not closes_step:
            with _timed(timers, 'logging'):
                sums.add(loss, terms, tags)
        else:
            with _timed(timers, 'optimizer_step'):
                if not replayed:        # a captured / replayed step holds the update
                    if reducer is not None:
                        reducer.wait()
                    if guard is None or guard.admit(optimizer):
                        optimizer.step()
                    optimizer.zero_grad(set_to_none=True)
            scheduler.step()
            with _timed(timers, 'logging'):
                wanted = clock.step % log_every == 0
                if wanted or accumulation_steps > 1:
                    sums.add(loss, terms, tags)
                if wanted and logger is not None:
                    x = clock.samples
                    sums.write(logger, x, accumulation_steps, _TRAIN_FAMILIES)
                    logger.add_scalar('General/Train loss', sums.loss, x)
                    if sums.contrast is not None:
                        logger.add_scalar('Train/contrast',
                                          sums.contrast / accumulation_steps, x)
                        for tag, level in zip(sums.tags, sums.contrast_levels or ()):
                            logger.add_scalar(f'Train/contrast/{tag}',
                                              level / accumulation_steps, x)
                    if sums.avg_timestamp is not None:
                        logger.add_scalar('Train/avg timestamp',
                                          sums.avg_timestamp / accumulation_steps, x)
                        for tag, level in zip(sums.tags, sums.avg_timestamp_levels or ()):
                            logger.add_scalar(f'Train/avg timestamp/{tag}',
                                              level / accumulation_steps, x)
                    for g, group in enumerate(optimizer.param_groups):
                        logger.add_scalar(f'General/learning rate/{g}',
                                          group['lr'], x)
                record = guard_readout(optimizer, guard) if wanted else None
                if record is not None:
                    if logger is not None:
                        logger.add_scalar('General/gradient norm', record['norm'], clock.samples)
                        logger.add_scalar('General/skipped steps', record['skipped'],
                                          clock.samples)
                    world = reducer.world if reducer is not None else 1
                    if world > 1 and guard_agreement_every > 0 and \
                            clock.step % guard_agreement_every == 0:
                        from .parallel import check_guard_agreement
                        check_guard_agreement(record, group=reducer.group)
                    if record['consecutive'] >= max_skipped_steps:
                        raise RuntimeError(
                            f'step {clock.step}: the last {record["consecutive"]} optimizer '
                            'steps were skipped for non-finite gradients '
                            f'(--max-skipped-steps {max_skipped_steps})')
                sums.clear()
            for name, hook in hooks.items():
                with _timed(timers, name):
                    hook(clock.step, clock.samples)
            model.train()               # a hook may have switched to eval()

        timers.log(names=list(STAGES) + list(hooks))
        timers('batch_construction').start()
    timers('batch_construction').stop()
    if captured is not None:
        captured.close()


def validate(model, device, loader, samples_passed, logger, evaluator,
             weights=[0.5, 1, 1], is_raw=True, contrast_weight=0.0,
             contrast_references=('start',), contrast_polarity=False,
             contrast_scales='finest', avg_timestamp_scales='finest', avg_timestamp_weight=0.0,
             avg_timestamp_references=AVG_TIMESTAMP_REFERENCES, avg_timestamp_polarity=False):
    """Mean loss and per-scale mean terms over ``loader`` (eval mode,
    no_grad), written against ``samples_passed``; with contrast_weight > 0
    the loss holds the contrast-maximisation term (of those reference times
    and polarity setting), written as ``Validation/contrast``; with
    contrast_scales='all' that is the mean of the levels' terms; with
    avg_timestamp_weight > 0 it holds the average-timestamp term as well,
    written as ``Validation/avg timestamp``; with avg_timestamp_scales='all'
    that is the mean of the levels' terms, each written as ``Validation/avg
    timestamp/<tag>`` beside it."""
    model.eval()
    sums, quiet = ScaleSums(), FakeTimer()
    n_batches = len(loader)
    with torch.no_grad():
        for batch in loader:
            loss, terms, tags = process_minibatch(
                model, batch, quiet, device, is_raw, evaluator, weights,
                **_contrast_keywords(contrast_weight, contrast_references, contrast_polarity,
                                     contrast_scales),
                **_avg_timestamp_keywords(avg_timestamp_weight, avg_timestamp_references,
                                          avg_timestamp_polarity, avg_timestamp_scales))
            sums.add(loss, terms, tags)
    logger.add_scalar('General/Validation loss', sums.loss / n_batches,
                      samples_passed)
    sums.write(logger, samples_passed, n_batches, _VALID_FAMILIES)
    if sums.contrast is not None:
        logger.add_scalar('Validation/contrast', sums.contrast / n_batches,
                          samples_passed)
    if sums.avg_timestamp is not None:
        logger.add_scalar('Validation/avg timestamp', sums.avg_timestamp / n_batches,
                          samples_passed)
        for tag, level in zip(sums.tags, sums.avg_timestamp_levels or ()):
            logger.add_scalar(f'Validation/avg timestamp/{tag}', level / n_batches, samples_passed)
