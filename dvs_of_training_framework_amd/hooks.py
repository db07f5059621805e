"""The two hooks of the reference's training script (utils/hooks/):
``SerializationHook`` checkpoints, ``ValidationHook`` runs a validation pass;
``VisualizationHook`` (an addition) draws what the model predicts,
``EvaluationHook`` (another) measures it against ground truth and
``SharpnessHook`` without any (the flow warp loss of the warped events).
``training.train`` calls ``hook(step, samples_passed)`` after an optimizer
step and times each under its dictionary name."""
from contextlib import contextmanager
from copy import deepcopy
from pathlib import Path

import numpy as np
import torch
import yaml

from .timer import FakeTimer
from .training import process_minibatch, validate
from .visualization import sample_picture, write_png


def gather_loader_states(state):
    """Loader states of every rank as a list indexed by rank, on rank 0
    (None elsewhere); one process: ``[state]``.  Host-side object gather, a
    few hundred bytes."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or \
            dist.get_world_size() == 1:
        return [state]
    out = [None] * dist.get_world_size() if dist.get_rank() == 0 else None
    dist.gather_object(state, out, dst=0)
    return out


class SerializationHook:
    """Checkpoints ``model`` and ``optimizer`` with ``samples_passed`` and
    whatever ``extra_state()`` returns (a dict; ``loader_state`` in it is
    gathered over the ranks and written as a list indexed by rank).  Every
    rank calls the hook, rank 0 alone writes."""

    def __init__(self, serializer, model, optimizer, logger, extra_state=None,
                 rank=0):
        self.serializer, self.model, self.optimizer = serializer, model, optimizer
        self.logger, self.extra_state, self.rank = logger, extra_state, rank

    def __call__(self, steps, samples):
        extra = dict(self.extra_state()) if self.extra_state is not None else {}
        if 'loader_state' in extra:
            extra['loader_state'] = gather_loader_states(extra['loader_state'])
        if self.rank != 0:
            return
        self.serializer.checkpoint_model(self.model, self.optimizer, steps,
                                         samples_passed=samples, **extra)
        if hasattr(self.logger, 'flush'):
            self.logger.flush()


_KEPT = ('strict', 'last_frame_indices', '_fast')


@contextmanager
def model_left_as_found(m):
    """What a hook that runs the model between two training steps must put
    back: train / eval mode, ``strict``, the layout cache a captured step
    reads from, the gradient tensors (the resident slot of a learnable
    representation among them)."""
    mode = m.training
    kept = {k: getattr(m, k) for k in _KEPT if hasattr(m, k)}
    cache = dict(m._layout_cache) if hasattr(m, '_layout_cache') else None
    grads = [(p, p.grad) for p in m.parameters()]
    try:
        yield m
    finally:
        for k, v in kept.items():
            setattr(m, k, v)
        if cache is not None:
            m._layout_cache.clear()
            m._layout_cache.update(cache)
        for p, g in grads:
            if p.grad is not g:
                p.grad = g
        m.train(mode)


class ValidationHook:
    """A validation pass (training.validate) that leaves the model as it found
    it (``model_left_as_found``)."""

    def __init__(self, model, device, loader, logger, losses, weights, is_raw,
                 contrast_weight=0.0, contrast_references=('start',), contrast_polarity=False,
                 contrast_scales='finest', avg_timestamp_scales='finest', avg_timestamp_weight=0.0,
                 avg_timestamp_references=('start', 'end'), avg_timestamp_polarity=False):
        self.model, self.device, self.loader = model, device, loader
        self.logger, self.losses = logger, losses
        self.weights = deepcopy(weights)
        self.is_raw = is_raw
        self.extra = {'contrast_weight': contrast_weight, 'contrast_references': tuple(contrast_references),
                      'contrast_polarity': bool(contrast_polarity)} if contrast_weight else {}
        if contrast_weight and contrast_scales != 'finest':
            self.extra['contrast_scales'] = contrast_scales
        if avg_timestamp_weight:
            self.extra.update(avg_timestamp_weight=avg_timestamp_weight,
                              avg_timestamp_references=tuple(avg_timestamp_references),
                              avg_timestamp_polarity=bool(avg_timestamp_polarity))
            if avg_timestamp_scales != 'finest':
                self.extra['avg_timestamp_scales'] = avg_timestamp_scales

    def __call__(self, steps, samples):
        with model_left_as_found(self.model):
            validate(self.model, self.device, self.loader, samples, self.logger,
                     self.losses, weights=self.weights, is_raw=self.is_raw, **self.extra)


def evaluation_frames(image_ts, gt_timestamps, last_event_time, step=1):
    """The frames an evaluation runs over (test.py:85-100 of the reference
    with the grid's start and stop unset) -> (frames [(start, stop)], the index
    of every frame's closing image).  The range begins at the first image (not
    before the first ground-truth timestamp) and stops at min(last event time,
    gt timestamps[-2]); a frame spans ``step`` images:
    zip(image_ts[b : e - step], image_ts[b + step : e])."""
    image_ts = np.asarray(image_ts, np.float64).reshape(-1)
    gt_timestamps = np.asarray(gt_timestamps, np.float64).reshape(-1)
    step = int(step)
    if step < 1:
        raise ValueError(f'a frame spans at least one image, not {step}')
    start = max(image_ts[0], gt_timestamps[0])
    stop = min(float(last_event_time), gt_timestamps[-2])
    b, e = (int(i) for i in np.searchsorted(image_ts, [start, stop]))
    n = max(e - step - b, 0)
    frames = list(zip(image_ts[b:b + n].tolist(), image_ts[b + step:b + step + n].tolist()))
    return frames, list(range(b + step, b + step + n))


def picture_indices(n_frames, pictures):
    """Which frames are drawn: ``(k * F) // pictures``, k = 0 .. pictures - 1
    (at most one picture per frame)."""
    pictures = max(min(int(pictures), int(n_frames)), 0)
    return [(k * n_frames) // pictures for k in range(pictures)]


class _Crop:
    """A box crop as ``testing.fold_box`` reads it (utils/data.py:24-42)."""

    def __init__(self, box):
        self.box = [int(b) for b in box]


class EvaluationHook:
    """Endpoint error of the live weights against ground truth
    (``testing.evaluate_frames`` on a device-resident ``FrameSequence``, events
    and ground truth cropped centrally to ``shape``), and for ``pictures``
    frames the four panels of ``visualization.eval_panels``.  Logs
    ``Evaluation/mean AEE`` and ``Evaluation/mean %AEE`` (x 100, as the
    reference's test.py does), writes ``<directory>/step_<N>/<k>.png`` + ``.yml``
    and hands the pictures to ``logger.add_image`` where there is one.  Only
    rank 0 evaluates, and nothing in here is a collective.  The model is left
    as it was found.

    gt: dict with 'timestamps', 'x_flow_dist', 'y_flow_dist' on the clock of
    the sequence's image timestamps."""

    def __init__(self, model, sequence, gt, logger, shape, directory, frame_step=1,
                 pictures=4, is_car=False, rank=0, batch_size=8):
        self.model, self.sequence, self.gt, self.logger = model, sequence, gt, logger
        self.shape = (int(shape[0]), int(shape[1]))
        self.directory, self.rank = Path(directory), rank
        self.is_car, self.batch_size = bool(is_car), int(batch_size)
        self.frames = self.closing = self.chosen = ()
        if rank != 0:
            return
        if getattr(model, 'prefix_length', 0) or getattr(model, 'suffix_length', 0):
            raise ValueError('the evaluation runs the model on one window per frame: '
                             'prefix_length = suffix_length = 0')
        from .sequence import central_box
        self.crop = _Crop(central_box(sequence.shape, self.shape))
        last = sequence.t[-1] if len(sequence) else -np.inf
        self.frames, self.closing = evaluation_frames(sequence.image_ts, gt['timestamps'],
                                                      last, frame_step)
        if not self.frames:
            raise ValueError('no frame of the validation sequence lies inside the ground truth')
        self.chosen = picture_indices(len(self.frames), pictures)

    def evaluate(self):
        """-> (result rows of every frame, [(frame, picture, its statistics)])
        with the model as it stands; pictures and statistics on the device."""
        from . import testing, visualization as vis
        from .of import OpticalFlow
        of = OpticalFlow.from_model(self.model, self.shape)
        y0, x0, h, w = self.crop.box
        drawn = []

        def observer(first, pred, gt_u, gt_v, max_row, count2):
            mine = [i for i in self.chosen if first <= i < first + pred.shape[0]]
            if not mine:
                return
            local = torch.tensor([i - first for i in mine], device=pred.device)
            closing = torch.tensor([self.closing[i] for i in mine], device=pred.device)
            grey = self.sequence.images[closing, y0:y0 + h, x0:x0 + w]
            image, stats = vis.eval_panels(pred[local], gt_u[local], gt_v[local], count2()[local],
                                           grey, max_row, return_stats=True)
            drawn.append((mine, image, stats))
        rows = testing.evaluate_frames(of, self.sequence, self.frames, self.gt, self.crop, None,
                                       self.crop, self.is_car, self.batch_size, observer=observer)
        return rows, drawn

    def __call__(self, steps, samples):
        if self.rank != 0:
            return
        from . import eval as dev_eval, testing, visualization as vis
        with model_left_as_found(self.model) as m:
            m.eval()
            with torch.no_grad():
                rows, drawn = self.evaluate()
        mean_aee, mean_percent = testing.summarize(rows)
        self.logger.add_scalar('Evaluation/mean AEE', float(mean_aee[-1]), samples)
        self.logger.add_scalar('Evaluation/mean %AEE', float(mean_percent[-1]) * 100, samples)
        aee, percent = dev_eval.derive(rows)
        out = self.directory / f'step_{steps}'
        k = 0
        for mine, images, stats in drawn:
            images, stats = vis._host(images), vis.read_panel_stats(stats)
            for i, image, s in zip(mine, images, stats):
                statistics = {
                    'frame': i, 'start': float(self.frames[i][0]), 'stop': float(self.frames[i][1]),
                    'AEE': float(aee[i]), 'n_points': int(rows['n_points'][i]),
                    'share_under_3px': float(percent[i]),
                    'prediction': {'lo': float(s['pred_lo']), 'hi': float(s['pred_hi']),
                                   'nonfinite': int(s['pred_nonfinite'])},
                    'ground_truth': {'lo': float(s['gt_lo']), 'hi': float(s['gt_hi']),
                                     'nonfinite': int(s['gt_nonfinite'])},
                    'm': float(vis.panel_scale(s))}
                if hasattr(self.logger, 'add_image'):
                    self.logger.add_image(f'Evaluation/{k}', image, samples, dataformats='HWC')
                out.mkdir(parents=True, exist_ok=True)
                write_png(out / f'{k:04d}.png', image)
                (out / f'{k:04d}.yml').write_text(yaml.dump(statistics))
                k += 1


def sharpness_frames(image_ts, last_event_time, step=1):
    """The frames a label-free validation runs over: ``evaluation_frames``
    without the ground-truth bounds.  The range begins at the first image and
    stops at the last event; a frame spans ``step`` images:
    zip(image_ts[b : e - step], image_ts[b + step : e])."""
    image_ts = np.asarray(image_ts, np.float64).reshape(-1)
    step = int(step)
    if step < 1:
        raise ValueError(f'a frame spans at least one image, not {step}')
    b, e = (int(i) for i in np.searchsorted(image_ts, [image_ts[0], float(last_event_time)]))
    n = max(e - step - b, 0)
    return list(zip(image_ts[b:b + n].tolist(), image_ts[b + step:b + step + n].tolist()))


class SharpnessHook:
    """Flow warp loss of the live weights, no ground truth needed
    (``testing.flow_warp_loss`` on a device-resident ``FrameSequence``, the
    events cropped centrally to ``shape``; docs/IWE_SPEC.md).  Logs
    ``Sharpness/mean FWL`` (the mean over the frames whose count image has a
    variance; NaN if none has), ``Sharpness/mean kept mass`` and
    ``Sharpness/frames without events``, draws ``pictures`` frames (count image
    | image of warped events) into ``<directory>/step_<N>/<k>.png`` + ``.yml``
    and hands them to ``logger.add_image`` where there is one.  Only rank 0
    evaluates, and nothing in here is a collective.  The model is left as it
    was found.

    references, polarity: the reference times the events are warped to (names
    among start, middle, end, or a mask) and whether ON and OFF events get
    images of their own (docs/IWE_SPEC.md sections 8-13): a frame then has
    R C images.  The three scalars keep their tags: the mean FWL is taken over
    all images that have one, the mean kept mass over the images with events,
    and a frame is without events when every image of it is empty.  With
    anything but the defaults the hook also logs ``Sharpness/mean FWL/<reference>``
    for every chosen reference and, with ``polarity``, ``Sharpness/mean FWL/ON``
    and ``/OFF``; a drawn frame is one picture of its images below one another
    in image order, and its ``.yml`` lists the statistics per image.

    rsat: beside the flow warp loss the ratio of squared average timestamps
    (``testing.event_alignment``, ``eval.derive_rsat``; docs/IWE_SPEC.md
    sections 14-21), from one splat for both.  The tags above carry the values
    they carry without it; the hook adds ``Sharpness/mean RSAT`` (the mean over
    the images that have one; NaN if none has) and, with anything but the
    default references and polarity, ``Sharpness/mean RSAT/<reference>``,
    ``/ON`` and ``/OFF``.  A drawn image row becomes count image | image of
    warped events | average timestamp at zero flow | average timestamp after
    the warp, and the ``.yml`` gains ``RSAT``, ``pixels_with_events`` and
    ``pixels_with_warped_events`` per image.  Off: nothing of it is built."""

    def __init__(self, model, sequence, logger, shape, directory, frame_step=1, pictures=4,
                 rank=0, batch_size=8, references=('start',), polarity=False, rsat=False):
        from .eval import iwe_image_names
        from .loss import contrast_reference_mask
        self.model, self.sequence, self.logger = model, sequence, logger
        self.reference_mask, self.polarity = contrast_reference_mask(references), bool(polarity)
        self.image_names = iwe_image_names(self.reference_mask, self.polarity)
        self.shape = (int(shape[0]), int(shape[1]))
        self.directory, self.rank = Path(directory), rank
        self.batch_size = int(batch_size)
        self.rsat = bool(rsat)
        self.frames = self.chosen = ()
        if rank != 0:
            return
        if getattr(model, 'prefix_length', 0) or getattr(model, 'suffix_length', 0):
            raise ValueError('the sharpness hook runs the model on one window per frame: '
                             'prefix_length = suffix_length = 0')
        from .sequence import central_box
        self.box = tuple(central_box(sequence.shape, self.shape))
        last = sequence.t[-1] if len(sequence) else -np.inf
        self.frames = sharpness_frames(sequence.image_ts, last, frame_step)
        if not self.frames:
            raise ValueError('no frame of the validation sequence holds events')
        self.chosen = picture_indices(len(self.frames), pictures)

    def evaluate(self):
        """-> (result rows of every image, [(frames, their pictures)]) with the
        model as it stands; pictures on the device.  With ``rsat`` a third
        entry, the average-timestamp rows of every image."""
        from . import eval as dev_eval, testing
        from .of import OpticalFlow
        of = OpticalFlow.from_model(self.model, self.shape)
        drawn = []
        per = len(self.image_names)

        def draw(first, q, count, results, more=None):
            mine = [i for i in self.chosen if first <= i < first + q.shape[0] // per]
            if not mine:
                return
            local = torch.tensor([(i - first) * per + k for i in mine for k in range(per)], device=q.device)
            canvas = dev_eval.iwe_render(q[local], count[local], results[local])
            if more is not None:
                s, base = more
                canvas = torch.cat([canvas, dev_eval.iwe_avg_timestamp_render(
                    q[local], s[local], base[local], count[local])], 2)
            # the images of a frame are contiguous: below one another, one picture
            drawn.append((mine, canvas.view(len(mine), per * canvas.shape[1], *canvas.shape[2:])))
        if self.rsat:
            rows, avg_rows = testing.event_alignment(
                of, self.sequence, self.frames, self.box, self.batch_size,
                observer=lambda first, images, results, _: draw(first, images[0], images[3], results, images[1:3]),
                references=self.reference_mask, polarity=self.polarity)
            return rows, drawn, avg_rows
        rows = testing.flow_warp_loss(of, self.sequence, self.frames, self.box, self.batch_size,
                                      observer=draw, references=self.reference_mask,
                                      polarity=self.polarity)
        return rows, drawn

    def __call__(self, steps, samples):
        if self.rank != 0:
            return
        from . import eval as dev_eval, visualization as vis
        with model_left_as_found(self.model) as m:
            m.eval()
            with torch.no_grad():
                rows, drawn, *avg_rows = self.evaluate()
        fwl, kept = dev_eval.derive_fwl(rows, self.shape[0] * self.shape[1])
        valid = ~np.isnan(fwl)
        has_events = rows['count_sum'] > 0
        names, per = self.image_names, len(self.image_names)

        def mean_fwl(pick):
            return float(fwl[valid & pick].mean()) if (valid & pick).any() else float('nan')
        self.logger.add_scalar('Sharpness/mean FWL', mean_fwl(True), samples)
        self.logger.add_scalar('Sharpness/mean kept mass',
                               float(kept[has_events].mean()) if has_events.any() else float('nan'),
                               samples)
        self.logger.add_scalar('Sharpness/frames without events',
                               int((~has_events).reshape(-1, per).all(1).sum()), samples)
        multi = self.reference_mask != 1 or self.polarity
        if multi:
            kind = np.arange(len(rows)) % per       # the image's place in its frame
            groups = list(dict.fromkeys(r for r, _ in names)) + (['ON', 'OFF'] if self.polarity else [])
            for group in groups:
                pick = np.isin(kind, [k for k, (r, c) in enumerate(names) if group in (r, c)])
                self.logger.add_scalar(f'Sharpness/mean FWL/{group}', mean_fwl(pick), samples)
        if self.rsat:
            avg_rows, = avg_rows
            rsat = dev_eval.derive_rsat(avg_rows)
            has_rsat = ~np.isnan(rsat)

            def mean_rsat(pick):
                return float(rsat[has_rsat & pick].mean()) if (has_rsat & pick).any() else float('nan')
            self.logger.add_scalar('Sharpness/mean RSAT', mean_rsat(True), samples)
            if multi:
                for group in groups:
                    pick = np.isin(kind, [k for k, (r, c) in enumerate(names) if group in (r, c)])
                    self.logger.add_scalar(f'Sharpness/mean RSAT/{group}', mean_rsat(pick), samples)

        def image_statistics(m):
            more = {'RSAT': float(rsat[m]), 'pixels_with_events': int(avg_rows['n0'][m]),
                    'pixels_with_warped_events': int(avg_rows['n'][m])} if self.rsat else {}
            return {'FWL': float(fwl[m]), 'kept_mass': float(kept[m]), 'count_max': int(rows['count_max'][m]),
                    'iwe_max': float(rows['max_q'][m]) * 2.0 ** -32, **more}
        out = self.directory / f'step_{steps}'
        k = 0
        for mine, images in drawn:
            for i, image in zip(mine, vis._host(images)):
                statistics = {'frame': i, 'start': float(self.frames[i][0]), 'stop': float(self.frames[i][1])}
                if multi:
                    statistics['images'] = [
                        {'reference': r, **({'channel': c} if c else {}), **image_statistics(i * per + j)}
                        for j, (r, c) in enumerate(names)]
                else:
                    statistics.update(image_statistics(i))
                if hasattr(self.logger, 'add_image'):
                    self.logger.add_image(f'Sharpness/{k}', image, samples, dataformats='HWC')
                out.mkdir(parents=True, exist_ok=True)
                write_png(out / f'{k:04d}.png', image)
                (out / f'{k:04d}.yml').write_text(yaml.dump(statistics))
                k += 1


class VisualizationHook:
    """Renders the first ``samples`` samples of ``loader`` (visualization.py:
    the frames on top, the predicted pyramid below) and leaves the model as it
    found it.  Each picture goes to ``logger.add_image`` where the logger has
    one and, on rank 0, to ``<directory>/step_<N>/<sample>.png`` + ``.yml``."""

    def __init__(self, model, device, loader, logger, losses, weights, is_raw,
                 args, directory, samples=4, rank=0):
        self.model, self.device, self.loader = model, device, loader
        self.logger, self.losses = logger, losses
        self.weights = deepcopy(weights)
        self.is_raw, self.args = is_raw, args
        self.directory, self.samples, self.rank = Path(directory), samples, rank

    def pictures(self):
        """-> [(image, statistics)] of the first ``samples`` samples."""
        out = []
        with torch.no_grad():
            for batch in self.loader:
                loss, parts, _, prediction = process_minibatch(
                    self.model, batch, FakeTimer(), self.device, self.is_raw,
                    self.losses, self.weights, return_prediction=True)
                for s in range(int(prediction['prediction'][-1].shape[0])):
                    out.append(sample_picture(self.args, batch, loss, parts,
                                              prediction, s))
                    if len(out) == self.samples:
                        return out
        return out

    def __call__(self, steps, samples):
        if self.rank != 0 and not hasattr(self.logger, 'add_image'):
            return      # nobody would see the pictures of this rank
        with model_left_as_found(self.model) as m:
            m.eval()
            pictures = self.pictures()
        for k, (image, statistics) in enumerate(pictures):
            if hasattr(self.logger, 'add_image'):
                self.logger.add_image(f'Visualization/{k}', image, samples,
                                      dataformats='HWC')
            if self.rank == 0:
                out = self.directory / f'step_{steps}'
                out.mkdir(parents=True, exist_ok=True)
                write_png(out / f'{k:04d}.png', image)
                (out / f'{k:04d}.yml').write_text(yaml.dump(statistics))
