"""The two hooks of the reference's training script (utils/hooks/):
``SerializationHook`` checkpoints, ``ValidationHook`` runs a validation pass.
``training.train`` calls ``hook(step, samples_passed)`` after an optimizer
step and times each under its dictionary name."""
from copy import deepcopy

from .training import validate


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


class ValidationHook:
    """A validation pass (training.validate) that leaves the model as it found
    it: train / eval mode, ``strict``, the layout cache a captured step reads
    from, the gradient tensors (the resident slot of a learnable
    representation among them)."""
    _KEPT = ('strict', 'last_frame_indices', '_fast')

    def __init__(self, model, device, loader, logger, losses, weights, is_raw):
        self.model, self.device, self.loader = model, device, loader
        self.logger, self.losses = logger, losses
        self.weights = deepcopy(weights)
        self.is_raw = is_raw

    def __call__(self, steps, samples):
        m = self.model
        mode = m.training
        kept = {k: getattr(m, k) for k in self._KEPT if hasattr(m, k)}
        cache = dict(m._layout_cache) if hasattr(m, '_layout_cache') else None
        grads = [(p, p.grad) for p in m.parameters()]
        try:
            validate(m, self.device, self.loader, samples, self.logger,
                     self.losses, weights=self.weights, is_raw=self.is_raw)
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
