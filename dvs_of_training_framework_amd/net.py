"""``Model`` -- the plugin class the reference's loader instantiates.

Boundary (reference): ``utils.model.init_model`` imports
``<flownet_path.name>.net`` and calls ``Model(device, **kwargs)`` with kwargs
filtered by this signature (utils/model.py:10-47, utils/options.py:332-347).
``forward(events, timestamps, sample_idx, imsize, raw=True,
intermediate=False)`` returns ``(flows[4] coarse->fine, flow_ts[P,2],
flow_sample_idx[P])`` plus ``(features,)`` iff ``intermediate``
(utils/training.py:59-64; witness DummyNet/net.py:42-80).  ``quantize`` is the
voxeliser entry used by scripts/quantize_preprocessed.py:87-91;
``quantization_layer`` / ``predictor`` are the attribute names
train_flownet.py:50-54,79-85 splits parameter groups on.
"""
import torch
from torch import nn

from . import learned_voxel, voxel
from .predictor import Predictor


def get_local_idx(shard_idx):
    """Local index of every element inside its shard and the shard sizes
    (reference DummyNet/net.py:5-39; example [0,0,1,1,2,1,2,2,2] ->
    [0,1,0,1,0,2,1,2,3], [2,3,4]).  Device-side, no host sync except the
    shard count."""
    assert shard_idx.dtype == torch.long
    n = shard_idx.numel()
    bs = int(shard_idx.max()) + 1 if n else 0
    order = torch.argsort(shard_idx, stable=True)
    sizes = torch.bincount(shard_idx, minlength=bs)
    starts = torch.cumsum(sizes, 0) - sizes
    ranks = torch.arange(n, device=shard_idx.device) - starts[shard_idx[order]]
    local = torch.empty_like(ranks)
    local[order] = ranks
    return local, sizes


class VoxelGrid(nn.Module):
    """Event representation (docs/VOXEL_SPEC.md): polarity-signed,
    time-bilinear voxel grid with ``depth`` bins.  No parameters."""

    def __init__(self, depth):
        super().__init__()
        self.depth = depth

    def forward(self, events, t0, t1, batch, height, width):
        """events: the int64 wire columns (utils/dataset.py:961-1020) or the
        compact 9 B/event columns (voxel.is_compact)."""
        if voxel.is_compact(events):
            return voxel.voxelize_compact(events, t0, t1, batch, self.depth,
                                          height, width)
        return voxel.voxelize(events, t0, t1, batch, self.depth, height, width)


class LearnedVoxelGrid(nn.Module):
    """Learnable event representation (docs/LEARNED_VOXEL_SPEC.md): the voxel
    grid with a learnable temporal kernel, a piecewise-linear lookup table of
    ``2 * radius * knots_per_bin + 1`` knots (the form Gehrig et al., ICCV
    2019, deploy their learned kernel in).  One parameter, ``kernel``,
    initialised to the triangle kernel: an untrained layer gives ``VoxelGrid``.
    Under ``no_grad`` (``Model.quantize``, offline quantisation, inference)
    only the forward kernel runs.

    RESIDENT mode (``make_resident``, off by default): ``kernel.grad`` lives in
    one persistent device slot the backward kernel writes or accumulates into
    (dvsof_learned_voxelize_bwd_into) instead of in a fresh tensor autograd
    adds up.  That is what a captured step (capture.py) and the data-parallel
    exchange need, and ``capture_ready`` says so.  The arithmetic is the
    default mode's, bit for bit.  ``reducer`` (parallel.GradReducer) is read
    when the backward runs, as the predictor reads its own: the layer's own
    attribute, or -- inside a ``Model`` -- the predictor's (``exchange_with``).

    ``deterministic`` (off by default): every forward of the layer -- training,
    ``Model.quantize``, inference, evaluation -- sums in 64-bit fixed point
    (dvsof_learned_voxelize_tiled): the same events give the same bits in any
    order, so two runs from one seed, and a replayed step and its eager twin,
    agree bit for bit on every input.  The backward is fixed-order already."""

    capture_ready = False

    def __init__(self, depth, radius=2, knots_per_bin=8, deterministic=False):
        super().__init__()
        self.depth, self.radius, self.knots_per_bin = depth, radius, knots_per_bin
        self.deterministic = bool(deterministic)
        self.kernel = nn.Parameter(
            learned_voxel.initial_kernel(radius, knots_per_bin))
        self.resident = None
        self._reducer, self._exchange_owner = None, ()

    def exchange_with(self, owner):
        """The knots' gradient joins the exchange of ``owner.reducer`` (the
        predictor: whatever reducer it has when the backward runs).  Kept in a
        tuple: the owner is no submodule of this layer."""
        self._exchange_owner = (owner,)

    @property
    def reducer(self):
        """parallel.GradReducer the slot is handed to as the step's last bucket."""
        for owner in self._exchange_owner:
            return owner.reducer
        return self._reducer

    @reducer.setter
    def reducer(self, value):
        assert not self._exchange_owner, 'the reducer is the predictor\'s: set it there'
        self._reducer = value

    def make_resident(self, event_capacity=None):
        """Allocate the gradient slot [K] and the reduction workspace (for
        ``event_capacity`` events; regrown between steps when a batch brings
        more) on the parameter's device, once.  -> self."""
        if not self.kernel.is_cuda:
            raise RuntimeError(
                'the resident gradient of a learnable representation lives on the GPU '
                f'(the layer is on {self.kernel.device}): there is no CPU implementation')
        if self.resident is None:
            self.resident = learned_voxel.ResidentGrad(
                self.radius, self.knots_per_bin, self.kernel.device, event_capacity)
            self.capture_ready = True
        elif event_capacity:
            self.resident.reserve(event_capacity)
        return self

    def attach_grad(self):
        """``kernel.grad`` = the slot where it is unset: the counterpart of
        ``Predictor.attach_bucket_grads`` for a replayed micro-batch."""
        if self.resident is not None and self.kernel.requires_grad:
            self.resident.attach(self.kernel)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        r = self.resident
        if r is not None and r.slot.device != self.kernel.device:
            # moved to another device: the slot follows (a gradient in flight does not);
            # off the GPU there is no resident mode
            self.kernel.grad = None
            self.resident, self.capture_ready = None, False
            if self.kernel.is_cuda:
                self.make_resident(r.capacity)
        return out

    def forward(self, events, t0, t1, batch, height, width):
        """events: the int64 wire columns or the compact 9 B/event columns."""
        return learned_voxel.apply(self.kernel, events, t0, t1, self.radius,
                                   self.knots_per_bin, batch, self.depth,
                                   height, width, resident=self.resident,
                                   reducer_of=self._reducer_now,
                                   deterministic=self.deterministic)

    def _reducer_now(self):
        return self.reducer


class Model(nn.Module):
    def __init__(self, device, prefix_length=0, suffix_length=0,
                 max_sequence_length=1, dynamic_sample_length=False,
                 event_representation_depth=9, activation=None,
                 compute_dtype='f32', learnable_representation=False,
                 representation_radius=2, representation_knots=8,
                 representation_resident=False,
                 representation_deterministic=False):
        super().__init__()
        self.prefix_length = prefix_length
        self.suffix_length = suffix_length
        self.max_sequence_length = max_sequence_length
        self.dynamic_sample_length = dynamic_sample_length
        self.event_representation_depth = event_representation_depth
        assert learnable_representation or not representation_deterministic, \
            'representation_deterministic needs learnable_representation'
        self.quantization_layer = LearnedVoxelGrid(
            event_representation_depth, representation_radius,
            representation_knots, representation_deterministic) \
            if learnable_representation \
            else VoxelGrid(event_representation_depth)
        self.predictor = Predictor(event_representation_depth, activation,
                                   compute_dtype)
        # strict=True reproduces the reference's host-side assertions (one
        # device sync per call); the train loop turns it off after step one.
        self.strict = True
        self.last_frame_indices = None
        self._layout_cache, self._fast = {}, None
        self.to(device)
        if representation_resident:
            assert learnable_representation, \
                'representation_resident needs learnable_representation'
            self.quantization_layer.make_resident()
            # its gradient joins the predictor's exchange (model.predictor.reducer)
            self.quantization_layer.exchange_with(self.predictor)

    # ---- host/device bookkeeping -------------------------------------
    def _select(self, timestamps, sample_idx, batch):
        """Predicted element = element ``prefix_length`` of every sample
        (DummyNet/net.py:70-78).  -> start, stop frame indices [B] (sorted by
        position), per-sample window t0/t1."""
        D = sample_idx.numel()
        dev = sample_idx.device
        local, sizes = None, None
        if D == batch * (2 + self.prefix_length + self.suffix_length) and \
                not self.strict:
            # uniform, sample-major layout: every index vector is a constant
            # of (D, batch): built once, then ONE gather per step
            key = (D, batch, self.prefix_length, str(dev))
            c = self._layout_cache.get(key)
            if c is None:
                T = D // batch
                first = torch.arange(batch, device=dev) * T
                start = first + self.prefix_length
                c = dict(start=start, stop=start + 1,
                         gather=torch.cat([first, first + T - 1, start,
                                           start + 1]),
                         start32=start.to(torch.int32),
                         stop32=(start + 1).to(torch.int32))
                if len(self._layout_cache) >= 8:
                    self._layout_cache.clear()
                self._layout_cache[key] = c
            g = timestamps[c['gather']]
            self._fast = (c, g)
            return c['start'], c['stop'], g[:batch], g[batch:2 * batch]
        self._fast = None
        local, sizes = get_local_idx(sample_idx)
        if self.strict and not self.dynamic_sample_length:
            assert bool((sizes == (2 + self.prefix_length +
                                   self.suffix_length)).all()), \
                'every sample needs 2 + prefix + suffix timestamps'
        pos = torch.arange(D, device=dev)

        def pick(k):
            key = torch.where(local == k, pos, pos + D)
            return torch.sort(key)[0][:batch]
        start, stop = pick(self.prefix_length), pick(self.prefix_length + 1)
        t0 = torch.full((batch,), float('inf'), device=dev).scatter_reduce(
            0, sample_idx, timestamps, 'amin')
        t1 = torch.full((batch,), float('-inf'), device=dev).scatter_reduce(
            0, sample_idx, timestamps, 'amax')
        return start, stop, t0, t1

    @staticmethod
    def _padded(imsize):
        h, w = int(imsize[0]), int(imsize[1])
        return h, w, (h + 15) // 16 * 16, (w + 15) // 16 * 16

    def _voxels(self, events, t0, t1, batch, imsize):
        h, w, hp, wp = self._padded(imsize)
        return self.quantization_layer(events, t0, t1, batch, hp, wp)

    def quantize(self, events, timestamps, sample_idx, imsize,
                 batch_size=None):
        """events -> float32 [B,C,H,W] (reference caller
        scripts/quantize_preprocessed.py:87-91)."""
        batch = batch_size or int(sample_idx[-1]) + 1
        _, _, t0, t1 = self._select(timestamps, sample_idx, batch)
        h, w, _, _ = self._padded(imsize)
        return self._voxels(events, t0, t1, batch, imsize)[:, :, :h, :w]

    def forward(self, events, timestamps, sample_idx, imsize, raw=True,
                intermediate=False, batch_size=None):
        batch = batch_size or int(sample_idx[-1]) + 1
        if raw and torch.is_grad_enabled() and timestamps.is_cuda:
            self.predictor.mark_step_begin(timestamps.device)
        start, stop, t0, t1 = self._select(timestamps, sample_idx, batch)
        h, w, hp, wp = self._padded(imsize)
        if raw:
            grid = self._voxels(events, t0, t1, batch, imsize)
        else:
            grid = events.float()
            assert grid.shape[0] == batch
            if (hp, wp) != (h, w):
                grid = nn.functional.pad(grid, (0, wp - w, 0, hp - h))
        flows = self.predictor(grid)
        if (hp, wp) != (h, w):      # shrink to the requested size
            flows = tuple(f[:, :, :h // 2 ** i, :w // 2 ** i]
                          for f, i in zip(flows, (3, 2, 1, 0)))
        with torch.no_grad():
            if self._fast is not None:
                c, g = self._fast
                flow_ts = g[2 * batch:].view(2, batch).t()
                self.last_frame_indices = (c['start32'], c['stop32'])
            else:
                flow_ts = torch.stack([timestamps[start], timestamps[stop]], 1)
                self.last_frame_indices = (start.to(torch.int32),
                                           stop.to(torch.int32))
            flow_sample_idx = sample_idx[start]
        add_info = (tuple(), ) if intermediate else tuple()
        return (tuple(flows), flow_ts, flow_sample_idx) + add_info
