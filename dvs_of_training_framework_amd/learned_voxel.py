"""Learnable event representation (HIP, csrc/learned_voxel.hip): the voxel
grid of docs/VOXEL_SPEC.md with the triangle kernel replaced by a
piecewise-linear lookup table ``theta[2*R*S + 1]`` -- docs/LEARNED_VOXEL_SPEC.md.

Upstream's learnable quantization layer lives in the absent EV_FlowNet
submodule; what the reference tree fixes is the wiring around it (parameter
group ``quantization_layer``, its own LR factor that stays 0 until
``training_steps * rs``: train_flownet.py:50-54,79-99).
"""
import torch

from . import _lib
from .voxel import WS_CLEAN, _WS_ROUND, is_compact

MAX_RADIUS, MAX_KNOTS_PER_BIN = 3, 16


def num_knots(radius, knots_per_bin):
    return 2 * radius * knots_per_bin + 1


def initial_kernel(radius, knots_per_bin):
    """theta[j] = max(0, 1 - |j/S - R|) (float64, rounded once): the triangle
    kernel -- an untrained layer gives the fixed voxel grid."""
    assert 1 <= radius <= MAX_RADIUS and 1 <= knots_per_bin <= MAX_KNOTS_PER_BIN
    d = torch.arange(num_knots(radius, knots_per_bin), dtype=torch.float64) \
        / knots_per_bin - radius
    return (1 - d.abs()).clamp_(min=0).float()


def _columns(events, device):
    """-> (x, y, t, polarity, sample, encoded) contiguous device tensors; sample
    is sample_index (wire columns) or sample_event_offsets (compact columns)."""
    if is_compact(events):
        cols = (events['x'].to(device, torch.short).contiguous(),
                events['y'].to(device, torch.short).contiguous(),
                events['timestamp'].to(device, torch.float32).contiguous(),
                events['polarity'].to(device, torch.uint8).contiguous(),
                events['sample_event_offsets'].to(device, torch.long).contiguous())
        return cols + (1,)
    x, y, p, s = (events[k].contiguous() for k in
                  ('x', 'y', 'polarity', 'sample_index'))
    for v in (x, y, p, s):
        assert v.dtype == torch.long, 'event columns are int64 on the wire'
    return x, y, events['timestamp'].contiguous().float(), p, s, 0


def _check(theta, radius, knots_per_bin, t0, t1, B):
    _lib.require_cuda(theta, t0, t1)
    assert theta.dtype == torch.float32 and theta.is_contiguous() and \
        theta.numel() == num_knots(radius, knots_per_bin)
    assert t0.numel() == B and t1.numel() == B


# Workspaces of the order-independent forward (dvsof_learned_voxelize_tiled): the
# pattern of voxel._workspace -- zero-filled once per shape and device, reused
# with WS_CLEAN, forgotten after a failed call.
_WORKSPACES = {}


def _forget_workspace(ws):
    for k in [k for k, v in _WORKSPACES.items() if v is ws]:
        del _WORKSPACES[k]


def _workspace(n, B, C, H, W, device):
    """-> (tensor, nbytes, flags) for the order-independent forward.  Tiled
    path: control words zero-filled ONCE, then WS_CLEAN (the kernels clean up
    after themselves); a workspace first met inside a stream capture is
    graph-owned scratch with flags 0 (a fill kernel node zeroes its control
    words).  Three-kernel path: the int64 scratch grid, no control words.  One
    call of a given shape at a time per device, as voxel._workspace."""
    lib = _lib.lib()
    control = lib.dvsof_learned_voxelize_tiled_control_bytes(n, B, C, H, W, 0)
    n_up = (n + _WS_ROUND - 1) // _WS_ROUND * _WS_ROUND if control else n
    nbytes = max(lib.dvsof_learned_voxelize_tiled_workspace_bytes(n_up, B, C, H, W, 0),
                 lib.dvsof_learned_voxelize_tiled_workspace_bytes(n, B, C, H, W, 0))
    flags = WS_CLEAN if control else 0
    key = (n_up if control else 0, control, B, C, H, W, str(device))
    ws = _WORKSPACES.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            return (torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device),
                    nbytes, 0)
        if len(_WORKSPACES) >= 16:
            _WORKSPACES.pop(next(iter(_WORKSPACES)))    # forget the oldest
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        ws[:control].zero_()
        _WORKSPACES[key] = ws
    return ws, nbytes, flags


def voxelize(events, t0, t1, theta, radius, knots_per_bin, B, C, H, W,
             deterministic=False):
    """events: wire or compact columns on the device; t0/t1: float32[B];
    theta: float32[2*R*S+1].  -> grid float32 [B,C,H,W].
    deterministic: the order-independent forward (64-bit fixed-point sums,
    LEARNED_VOXEL_SPEC "Order-independent forward"): the same events give the
    same bits in any order.  Off: float atomics in arrival order."""
    _check(theta, radius, knots_per_bin, t0, t1, B)
    x, y, t, p, s, encoded = _columns(events, t0.device)
    _lib.require_cuda(x, y, t, p, s)
    if encoded:
        assert s.numel() == B + 1, 'one offset per sample plus the end'
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=t0.device)
    lib = _lib.lib()
    if deterministic:
        n = x.numel()
        ws, nbytes, flags = _workspace(n, B, C, H, W, t0.device) if n else (None, 0, 0)
        rc = lib.dvsof_learned_voxelize_tiled(
            x.data_ptr(), y.data_ptr(), t.data_ptr(), p.data_ptr(), s.data_ptr(),
            encoded, n, t0.contiguous().data_ptr(), t1.contiguous().data_ptr(),
            theta.data_ptr(), radius, knots_per_bin, B, C, H, W, out.data_ptr(),
            _lib.ptr(ws), nbytes, flags, _lib.stream())
        if rc != 0:
            _forget_workspace(ws)
        _lib.check(rc, 'dvsof_learned_voxelize_tiled')
        return out
    fn, what = (lib.dvsof_learned_voxelize_encoded, 'dvsof_learned_voxelize_encoded') \
        if encoded else (lib.dvsof_learned_voxelize_fwd, 'dvsof_learned_voxelize_fwd')
    _lib.check(fn(x.data_ptr(), y.data_ptr(), t.data_ptr(), p.data_ptr(),
                  s.data_ptr(), x.numel(), t0.contiguous().data_ptr(),
                  t1.contiguous().data_ptr(), theta.data_ptr(), radius,
                  knots_per_bin, B, C, H, W, out.data_ptr(), _lib.stream()), what)
    return out


def voxelize_bwd(events, t0, t1, radius, knots_per_bin, grad_grid):
    """grad_grid: float32 [B,C,H,W] -> gradient of theta, float32[2*R*S+1]
    (fixed-order reduction: the same inputs give the same bits)."""
    B, C, H, W = grad_grid.shape
    _lib.require_cuda(grad_grid, t0, t1)
    x, y, t, p, s, encoded = _columns(events, t0.device)
    _lib.require_cuda(x, y, t, p, s)
    gv = grad_grid.contiguous().float()
    n = x.numel()
    lib = _lib.lib()
    gtheta = torch.empty(num_knots(radius, knots_per_bin), dtype=torch.float32,
                         device=t0.device)
    nbytes = lib.dvsof_learned_voxelize_bwd_workspace_bytes(n, radius, knots_per_bin)
    ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=t0.device)
    _lib.check(lib.dvsof_learned_voxelize_bwd(
        x.data_ptr(), y.data_ptr(), t.data_ptr(), p.data_ptr(), s.data_ptr(),
        encoded, n, t0.contiguous().data_ptr(), t1.contiguous().data_ptr(),
        radius, knots_per_bin, B, C, H, W, gv.data_ptr(), gtheta.data_ptr(),
        ws.data_ptr(), ws.numel() * 4, _lib.stream()), 'dvsof_learned_voxelize_bwd')
    return gtheta


def workspace_floats(n_events, radius, knots_per_bin):
    """Floats of reduction scratch ``voxelize_bwd_into`` needs for ``n_events``
    (non-decreasing in ``n_events``)."""
    nbytes = _lib.lib().dvsof_learned_voxelize_bwd_workspace_bytes(
        int(n_events), radius, knots_per_bin)
    return max(nbytes // 4, 4)


def voxelize_bwd_into(events, t0, t1, radius, knots_per_bin, grad_grid, gtheta,
                      accumulate, workspace):
    """The gradient of ``voxelize_bwd`` into the caller's persistent
    ``gtheta`` (float32[2*R*S+1]): written (``accumulate`` false: the bits of
    ``voxelize_bwd``) or added to what it holds by one float32 add.
    ``workspace``: float32 scratch of at least ``workspace_floats(n, R, S)``
    elements, the caller's too.  Allocates nothing and enqueues kernels only."""
    B, C, H, W = grad_grid.shape
    _lib.require_cuda(grad_grid, t0, t1, gtheta, workspace)
    x, y, t, p, s, encoded = _columns(events, t0.device)
    _lib.require_cuda(x, y, t, p, s)
    assert grad_grid.dtype == torch.float32 and grad_grid.is_contiguous()
    assert gtheta.dtype == torch.float32 and gtheta.is_contiguous() and \
        gtheta.numel() == num_knots(radius, knots_per_bin)
    assert workspace.dtype == torch.float32 and workspace.is_contiguous()
    _lib.check(_lib.lib().dvsof_learned_voxelize_bwd_into(
        x.data_ptr(), y.data_ptr(), t.data_ptr(), p.data_ptr(), s.data_ptr(),
        encoded, x.numel(), t0.contiguous().data_ptr(), t1.contiguous().data_ptr(),
        radius, knots_per_bin, B, C, H, W, grad_grid.data_ptr(), gtheta.data_ptr(),
        1 if accumulate else 0, workspace.data_ptr(), workspace.numel() * 4,
        _lib.stream()), 'dvsof_learned_voxelize_bwd_into')


def reduction_chain(n_events, knots_per_bin):
    """``m`` of docs/LEARNED_VOXEL_SPEC.md: the longest chain of float32
    roundings a term of the table's gradient passes through."""
    blocks = _lib.lib().dvsof_learned_voxelize_bwd_blocks(n_events)
    per_thread = -(-n_events // (blocks * 128)) if n_events else 0
    return (2 if knots_per_bin == 1 else 1) * per_thread + 11


class _LearnedVoxelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, events, t0, t1, radius, knots_per_bin, B, C, H, W,
                deterministic=False):
        ctx.args = (events, t0, t1, radius, knots_per_bin)
        return voxelize(events, t0, t1, theta.detach(), radius, knots_per_bin,
                        B, C, H, W, deterministic)

    @staticmethod
    def backward(ctx, grad_grid):
        events, t0, t1, radius, knots_per_bin = ctx.args
        g = voxelize_bwd(events, t0, t1, radius, knots_per_bin, grad_grid) \
            if ctx.needs_input_grad[0] else None
        return (g,) + (None,) * 10


class ResidentGrad:
    """Persistent home of the table's gradient (net.LearnedVoxelGrid.
    make_resident): ``slot`` float32[K], the SAME tensor every step -- what
    ``theta.grad`` is, what the optimizer's pointer table, a captured step and
    the gradient exchange point at -- and the reduction ``workspace``, regrown
    eagerly (never inside a stream capture) when a batch outgrows it."""

    def __init__(self, radius, knots_per_bin, device, event_capacity=None):
        self.radius, self.knots_per_bin = radius, knots_per_bin
        self.slot = torch.zeros(num_knots(radius, knots_per_bin),
                                dtype=torch.float32, device=device)
        self.workspace, self.capacity = None, 0
        self.reserve(event_capacity or 4096)

    def reserve(self, n_events):
        """Room for the reduction over ``n_events`` events."""
        need = workspace_floats(n_events, self.radius, self.knots_per_bin)
        if self.workspace is None or self.workspace.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(
                    f'the resident reduction workspace holds {self.capacity} events and the '
                    f'captured batch brings {n_events}: reserve() before recording')
            self.workspace = torch.empty(need, dtype=torch.float32,
                                         device=self.slot.device)
        self.capacity = max(self.capacity, int(n_events))

    def owns(self, grad):
        return grad is not None and grad.data_ptr() == self.slot.data_ptr()

    def attach(self, theta):
        """``theta.grad`` = the slot where it is unset (Python's view of what a
        replayed micro-batch that only wrote or accumulated gradients did)."""
        if theta.grad is None:
            theta.grad = self.slot

    def tensors(self):
        return [self.slot, self.workspace]

    def backward(self, theta, events, t0, t1, grad_grid, reducer=None):
        accumulate = self.owns(theta.grad)
        assert accumulate or theta.grad is None, \
            'a resident representation owns kernel.grad (found a foreign gradient tensor)'
        self.reserve(events['x'].numel())
        voxelize_bwd_into(events, t0, t1, self.radius, self.knots_per_bin,
                          grad_grid.contiguous().float(), self.slot, accumulate,
                          self.workspace)
        if not accumulate:
            theta.grad = self.slot
        # the last bucket of the step, behind enc.0's: every rank hands it over in every
        # launch mode (the reducer leaves a mark under capture), whatever its batch held
        if reducer is not None and reducer.active():
            reducer.bucket_ready(self.slot)


class _ResidentVoxelFn(torch.autograd.Function):
    """The learned grid with the table's gradient kept by ``resident``
    (ResidentGrad): backward writes / accumulates ``theta.grad`` itself and
    hands autograd nothing."""

    @staticmethod
    def forward(ctx, theta, resident, reducer_of, events, t0, t1, B, C, H, W,
                deterministic=False):
        ctx.args = (theta, resident, reducer_of, events, t0, t1)
        return voxelize(events, t0, t1, theta.detach(), resident.radius,
                        resident.knots_per_bin, B, C, H, W, deterministic)

    @staticmethod
    def backward(ctx, grad_grid):
        theta, resident, reducer_of, events, t0, t1 = ctx.args
        if ctx.needs_input_grad[0]:
            # the reducer in effect NOW, as the predictor's backward reads its own
            reducer = reducer_of() if reducer_of is not None else None
            resident.backward(theta, events, t0, t1, grad_grid, reducer)
        return (None,) * 11


def apply(theta, events, t0, t1, radius, knots_per_bin, B, C, H, W,
          resident=None, reducer_of=None, deterministic=False):
    """Differentiable with respect to ``theta`` only (no gradient to event
    coordinates or timestamps).  Without grad mode only the forward runs.
    resident: ResidentGrad -- the gradient goes to its persistent slot (and
    from there to the parallel.GradReducer that ``reducer_of()`` returns when
    the backward runs) instead of to autograd.
    deterministic: the order-independent forward (``voxelize``); the backward
    is fixed-order either way."""
    if resident is not None and torch.is_grad_enabled() and theta.requires_grad:
        assert (resident.radius, resident.knots_per_bin) == (radius, knots_per_bin)
        return _ResidentVoxelFn.apply(theta, resident, reducer_of, events, t0, t1,
                                      B, C, H, W, deterministic)
    if torch.is_grad_enabled() and theta.requires_grad:
        return _LearnedVoxelFn.apply(theta, events, t0, t1, radius,
                                     knots_per_bin, B, C, H, W, deterministic)
    return voxelize(events, t0, t1, theta.detach(), radius, knots_per_bin,
                    B, C, H, W, deterministic)
