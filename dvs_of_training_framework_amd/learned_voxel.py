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
from .voxel import is_compact

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


def voxelize(events, t0, t1, theta, radius, knots_per_bin, B, C, H, W):
    """events: wire or compact columns on the device; t0/t1: float32[B];
    theta: float32[2*R*S+1].  -> grid float32 [B,C,H,W]."""
    _check(theta, radius, knots_per_bin, t0, t1, B)
    x, y, t, p, s, encoded = _columns(events, t0.device)
    _lib.require_cuda(x, y, t, p, s)
    if encoded:
        assert s.numel() == B + 1, 'one offset per sample plus the end'
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=t0.device)
    lib = _lib.lib()
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


def reduction_chain(n_events, knots_per_bin):
    """``m`` of docs/LEARNED_VOXEL_SPEC.md: the longest chain of float32
    roundings a term of the table's gradient passes through."""
    blocks = _lib.lib().dvsof_learned_voxelize_bwd_blocks(n_events)
    per_thread = -(-n_events // (blocks * 128)) if n_events else 0
    return (2 if knots_per_bin == 1 else 1) * per_thread + 11


class _LearnedVoxelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, events, t0, t1, radius, knots_per_bin, B, C, H, W):
        ctx.args = (events, t0, t1, radius, knots_per_bin)
        return voxelize(events, t0, t1, theta.detach(), radius, knots_per_bin,
                        B, C, H, W)

    @staticmethod
    def backward(ctx, grad_grid):
        events, t0, t1, radius, knots_per_bin = ctx.args
        g = voxelize_bwd(events, t0, t1, radius, knots_per_bin, grad_grid) \
            if ctx.needs_input_grad[0] else None
        return (g,) + (None,) * 9


def apply(theta, events, t0, t1, radius, knots_per_bin, B, C, H, W):
    """Differentiable with respect to ``theta`` only (no gradient to event
    coordinates or timestamps).  Without grad mode only the forward runs."""
    if torch.is_grad_enabled() and theta.requires_grad:
        return _LearnedVoxelFn.apply(theta, events, t0, t1, radius,
                                     knots_per_bin, B, C, H, W)
    return voxelize(events, t0, t1, theta.detach(), radius, knots_per_bin,
                    B, C, H, W)
