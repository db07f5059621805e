"""The two hooks of the reference's training script (utils/hooks/):
``SerializationHook`` checkpoints, ``ValidationHook`` runs a validation pass;
``VisualizationHook`` (an addition) draws what the model predicts.
``training.train`` calls ``hook(step, samples_passed)`` after an optimizer
step and times each under its dictionary name."""
from contextlib import contextmanager
from copy import deepcopy
from pathlib import Path

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

    def __init__(self, model, device, loader, logger, losses, weights, is_raw):
        self.model, self.device, self.loader = model, device, loader
        self.logger, self.losses = logger, losses
        self.weights = deepcopy(weights)
        self.is_raw = is_raw

    def __call__(self, steps, samples):
        with model_left_as_found(self.model):
            validate(self.model, self.device, self.loader, samples, self.logger,
                     self.losses, weights=self.weights, is_raw=self.is_raw)


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
