"""Loss evaluator with the reference's surface, computed by HIP kernels.

Mirrors /root/reference/utils/loss.py: ``Loss`` (:38-171), ``Losses``
(:174-214), ``init_losses`` (:217-240), ``interpolate`` (:20-21).  Same call
signatures, same return structure ``((smooth_k), (photo_k), (border_k))`` of
0-dim tensors, same assertions on shapes and on frame resolution.

Differences that are deliberate (MI355X-first):
  * all scales are evaluated by ONE forward launch (+ a 1-workgroup finalize)
    and ONE backward launch (csrc/loss.hip) instead of ~15 ATen ops per scale;
  * frames are not gathered (``images[start_indices]``): kernels index the
    pyramid level through the start/stop index vectors;
  * ``Losses.fused`` is a training fast path (forward + gradient in one sweep);
  * ``Losses.frameless`` is the loss of a batch without frames: smoothness and
    out-of-border alone, no pyramid and no frame read (csrc/loss_frameless.hip,
    docs/FRAMELESS_SPEC.md);
  * ``Losses.contrast`` and ``Losses.avg_timestamp`` are training terms from the
    events alone, on the finest flow or, with ``scales='all'``
    (``Losses.avg_timestamp_scales`` for the second), on every flow
    (csrc/contrast.hip, csrc/avg_timestamp.hip; docs/CONTRAST_SPEC.md,
    docs/AVG_TIMESTAMP_SPEC.md).
"""
import ctypes

import numpy as np
import torch

from . import _lib, voxel
from .timer import FakeTimer


def interpolate(img, shape):
    """Bilinear resize, align_corners=True (reference utils/loss.py:20-21).
    img: [..., H, W] float32 device tensor."""
    _lib.require_cuda(img)
    img = img.contiguous().float()
    hin, win = img.shape[-2:]
    hout, wout = int(shape[0]), int(shape[1])
    n = img.numel() // (hin * win) if hin * win else 0
    out = torch.empty(img.shape[:-2] + (hout, wout), dtype=torch.float32,
                      device=img.device)
    _lib.check(_lib.lib().dvsof_resize_bilinear_ac(
        img.data_ptr(), out.data_ptr(), n, hin, win, hout, wout,
        _lib.stream()), 'dvsof_resize_bilinear_ac')
    return out


def resolve_frames(flow_ts, flow_sample_idx, timestamps, sample_idx):
    """Start/stop frame of every prediction (reference utils/loss.py:182-206):
    exact float equality of timestamps AND equal sample id, exactly one hit.
    Returns int32 device vectors; raises AssertionError like the reference."""
    same = sample_idx.view(1, -1, 1) == flow_sample_idx.view(1, 1, -1)
    ts = timestamps.view(1, -1, 1) == flow_ts.T.reshape(2, 1, -1)
    mask = torch.logical_and(ts, same)                      # [2, D, P]
    assert bool((mask.sum(1) == 1).all()), \
        'for each prediction has to be exactly one image in data'
    idx = mask.to(torch.uint8).argmax(dim=1).to(torch.int32)  # [2, P]
    return idx[0].contiguous(), idx[1].contiguous()


def _scale_array(frames, flows, grads):
    arr = (_lib.LossScale * len(flows))()
    for k, f in enumerate(flows):
        arr[k].frames = frames[k].data_ptr()
        arr[k].flow = f.data_ptr()
        arr[k].grad_flow = grads[k].data_ptr() if grads is not None else None
        arr[k].h, arr[k].w = f.shape[-2], f.shape[-1]
    return arr


def _workspace(arr, K, N, device):
    nbytes = _lib.lib().dvsof_loss_workspace_bytes(arr, K, N)
    if nbytes == 0:
        raise RuntimeError('dvsof_loss_workspace_bytes: invalid scales')
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device), nbytes


class _LossTerms(torch.autograd.Function):
    """terms[3,K] = f(flow_0..flow_{K-1}); gradient flows into the flows only
    (frames are no_grad in the reference, utils/loss.py:209-210)."""

    @staticmethod
    def forward(ctx, frames, start, stop, *flows):
        K, N = len(flows), flows[0].shape[0]
        dev = flows[0].device
        flows = tuple(f.detach().contiguous().float() for f in flows)
        arr = _scale_array(frames, flows, None)
        ws, nbytes = _workspace(arr, K, N, dev)
        terms = torch.empty(3, K, dtype=torch.float32, device=dev)
        oob = torch.empty(K * N, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().dvsof_loss_fwd(
            arr, K, N, start.data_ptr(), stop.data_ptr(), terms.data_ptr(),
            oob.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()),
            'dvsof_loss_fwd')
        ctx.frames, ctx.start, ctx.stop = frames, start, stop
        ctx.flows, ctx.oob = flows, oob
        return terms

    @staticmethod
    def backward(ctx, grad_terms):
        flows = ctx.flows
        K, N = len(flows), flows[0].shape[0]
        grads = tuple(torch.empty_like(f) for f in flows)
        arr = _scale_array(ctx.frames, flows, grads)
        seeds = grad_terms.contiguous().float()
        _lib.check(_lib.lib().dvsof_loss_bwd(
            arr, K, N, ctx.start.data_ptr(), ctx.stop.data_ptr(),
            seeds.data_ptr(), ctx.oob.data_ptr(), _lib.stream()),
            'dvsof_loss_bwd')
        return (None, None, None) + grads


_UNIT = {}


def unit_backward(loss):
    """``loss.backward()`` with a cached device-resident 1.0 as the seed: the
    fused loss recognises it (by address, no host sync) and hands out its flow
    gradients without the x1.0 multi-tensor pass and without the ones_like
    fill of every step."""
    one = _UNIT.get(loss.device)
    if one is None:
        one = _UNIT[loss.device] = torch.ones((), dtype=loss.dtype,
                                              device=loss.device)
    torch.autograd.backward(loss, grad_tensors=one)


class _FusedLoss(torch.autograd.Function):
    """loss = sum_t w_t * mean_k term[t,k] * scale with the flow gradients
    produced in the same sweep (dvsof_loss_fused).  ``images`` not None: the
    frame pyramid is built into ``frames`` by the same call
    (dvsof_loss_fused_pyramid)."""

    @staticmethod
    def forward(ctx, frames, images, start, stop, weights, scale, *flows):
        K, N = len(flows), flows[0].shape[0]
        dev = flows[0].device
        flows = tuple(f.detach().contiguous().float() for f in flows)
        grads = tuple(torch.empty_like(f) for f in flows)
        arr = _scale_array(frames, flows, grads)
        ws, nbytes = _workspace(arr, K, N, dev)
        terms = torch.empty(3, K, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        oob = torch.empty(K * N, dtype=torch.int32, device=dev)
        w = (ctypes.c_float * 3)(*[float(x) for x in weights])
        if images is None:
            _lib.check(_lib.lib().dvsof_loss_fused(
                arr, K, N, start.data_ptr(), stop.data_ptr(), w, float(scale),
                terms.data_ptr(), loss.data_ptr(), oob.data_ptr(),
                ws.data_ptr(), nbytes, _lib.stream()), 'dvsof_loss_fused')
        else:
            D, H, W = images.shape
            _lib.check(_lib.lib().dvsof_loss_fused_pyramid(
                images.data_ptr(), D, H, W, arr, K, N, start.data_ptr(),
                stop.data_ptr(), w, float(scale), terms.data_ptr(),
                loss.data_ptr(), oob.data_ptr(), ws.data_ptr(), nbytes,
                _lib.stream()), 'dvsof_loss_fused_pyramid')
        ctx.grads = grads
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return loss, terms

    @staticmethod
    def backward(ctx, g_loss, _g_terms):
        if g_loss is None:
            return (None,) * (6 + len(ctx.grads))
        one = _UNIT.get(g_loss.device)
        if one is not None and g_loss.data_ptr() == one.data_ptr():
            return (None,) * 6 + tuple(ctx.grads)      # seed is exactly 1.0
        # one multi-tensor launch for all scales
        return (None,) * 6 + tuple(torch._foreach_mul(list(ctx.grads), g_loss))


class _FramelessLoss(torch.autograd.Function):
    """loss = (w_s sum_k smooth_k + w_o sum_k border_k) / K * scale with the
    flow gradients produced in the same sweep (dvsof_loss_frameless,
    docs/FRAMELESS_SPEC.md): no frame is read, the photometric row of the
    terms is +0."""

    @staticmethod
    def forward(ctx, weights, scale, *flows):
        K, N = len(flows), flows[0].shape[0]
        dev = flows[0].device
        flows = tuple(f.detach().contiguous().float() for f in flows)
        grads = tuple(torch.empty_like(f) for f in flows)
        arr = (_lib.LossScale * K)()
        for k, (f, g) in enumerate(zip(flows, grads)):
            arr[k].frames, arr[k].flow, arr[k].grad_flow = None, f.data_ptr(), g.data_ptr()
            arr[k].h, arr[k].w = f.shape[-2], f.shape[-1]
        lib = _lib.lib()
        nbytes = lib.dvsof_loss_frameless_workspace_bytes(arr, K, N)
        if nbytes == 0:
            raise RuntimeError('dvsof_loss_frameless_workspace_bytes: invalid scales')
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        terms = torch.empty(3, K, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        oob = torch.empty(K * N, dtype=torch.int32, device=dev)
        w = (ctypes.c_float * 2)(*[float(x) for x in weights])
        _lib.check(lib.dvsof_loss_frameless(
            arr, K, N, w, float(scale), terms.data_ptr(), loss.data_ptr(), oob.data_ptr(),
            ws.data_ptr(), nbytes, _lib.stream()), 'dvsof_loss_frameless')
        ctx.grads = grads
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return loss, terms

    @staticmethod
    def backward(ctx, g_loss, _g_terms):
        if g_loss is None:
            return (None,) * (2 + len(ctx.grads))
        one = _UNIT.get(g_loss.device)
        if one is not None and g_loss.data_ptr() == one.data_ptr():
            return (None,) * 2 + tuple(ctx.grads)      # seed is exactly 1.0
        return (None,) * 2 + tuple(torch._foreach_mul(list(ctx.grads), g_loss))


# ---------------------------------------------------------------------------
# Contrast-maximisation term (csrc/contrast.hip, docs/CONTRAST_SPEC.md)
# ---------------------------------------------------------------------------
_F32 = np.float32
CONTRAST_UNIT_BITS = 40


def _contrast_pairs(x, y, t, sample_index, frame_ts, frame_sample, flow):
    """The (event, frame) pairs that take part, frame by frame, and their warp
    (steps 1-6 of IWE_SPEC section 2 in numpy float32).  -> dict of per-pair
    arrays: f, x, y, tau, inside (the inside test), cx, cy, wx [2], wy [2]
    (the last four only meaningful where ``inside``)."""
    x, y = np.asarray(x, np.int64).reshape(-1), np.asarray(y, np.int64).reshape(-1)
    t = np.asarray(t, _F32).reshape(-1)
    s = np.asarray(sample_index, np.int64).reshape(-1)
    ts = np.asarray(frame_ts, _F32).reshape(-1)
    fs = np.asarray(frame_sample, np.int64).reshape(-1)
    flow = np.asarray(flow, _F32)
    F, _, h, w = flow.shape
    assert ts.size == 2 * F and fs.size == F and x.size == y.size == t.size == s.size
    inb = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    sel = [np.flatnonzero(inb & (s == fs[f]) & (ts[2 * f] <= t) & (t <= ts[2 * f + 1]))
           for f in range(F)]
    e = np.concatenate(sel) if F else np.zeros(0, np.int64)
    f = np.concatenate([np.full(k.size, i, np.int64) for i, k in enumerate(sel)]) if F \
        else np.zeros(0, np.int64)
    x, y, t = x[e], y[e], t[e]
    t0 = ts[2 * f]
    d = ts[2 * f + 1] - t0
    with np.errstate(all='ignore'):
        tau = np.where(d > 0, np.fmin(np.fmax((t - t0) / d, _F32(0)), _F32(1)), _F32(0)).astype(_F32)
        xw = x.astype(_F32) - tau * flow[f, 0, y, x]
        yw = y.astype(_F32) - tau * flow[f, 1, y, x]
        inside = (xw > _F32(-1)) & (xw < _F32(w)) & (yw > _F32(-1)) & (yw < _F32(h))
        xw, yw = np.where(inside, xw, _F32(0)), np.where(inside, yw, _F32(0))
    flx, fly = np.floor(xw), np.floor(yw)
    fx, fy = xw - flx, yw - fly
    return dict(f=f, x=x, y=y, tau=tau, inside=inside, cx=flx.astype(np.int64), cy=fly.astype(np.int64),
                wx=(_F32(1) - fx, fx), wy=(_F32(1) - fy, fy))


def contrast_fwd_host(x, y, t, sample_index, frame_ts, frame_sample, flow):
    """CONTRAST_SPEC sections 2-4 on the host: what ``dvsof_contrast_fwd`` is
    pinned to, byte for byte.  x, y, sample_index int64 [n], t float32 [n],
    frame_ts float32 [2F] (or [F,2]), frame_sample int64 [F], flow float32
    [F,2,h,w] -> dict: q int64 [F,h,w], count uint32 [F,h,w], result (rows of
    eval.IWE_RESULT_DTYPE, sum_sq in the kernels' order), term float32, and
    the per-frame float64 records mean, coef, unit, frame_term."""
    from . import eval as ev
    flow = np.asarray(flow, _F32)
    F, _, h, w = flow.shape
    p = _contrast_pairs(x, y, t, sample_index, frame_ts, frame_sample, flow)
    q = np.zeros((F, h, w), np.int64)
    count = np.zeros((F, h, w), np.uint32)
    np.add.at(count, (p['f'], p['y'], p['x']), 1)
    k = p['inside']
    f, cx, cy = p['f'][k], p['cx'][k], p['cy'][k]
    for j in range(2):
        for i in range(2):
            xx, yy = cx + i, cy + j
            Q = ((p['wy'][j][k] * p['wx'][i][k]).astype(_F32) * _F32(ev.IWE_ONE)).astype(np.int64)
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h) & (Q > 0)
            np.add.at(q, (f[ok], yy[ok], xx[ok]), Q[ok])
    res = ev.iwe_stats_host(q, count)
    res['sum_sq'] = ev.iwe_sum_sq_kernel_order(q)
    # the closing wave, in float64
    N = np.float64(h) * np.float64(w)
    mean = res['sum_q'].astype(np.float64) * 2.0 ** -32 / N
    var_i = res['sum_sq'] / N - mean * mean
    cmean = res['count_sum'].astype(np.float64) / N
    var_c = res['count_sq'].astype(np.float64) / N - cmean * cmean
    live = var_c > 0
    with np.errstate(all='ignore'):
        coef = np.where(live, -2.0 / (N * var_c), 0.0)
        frame_term = np.where(live, 1.0 - var_i / var_c, 0.0)
    gmax = np.abs(coef) * np.fmax(res['max_q'].astype(np.float64) * 2.0 ** -32 - mean, mean)
    e = np.where(gmax > 0, np.frexp(gmax)[1], 0)
    unit = np.ldexp(1.0, CONTRAST_UNIT_BITS - e)
    total = np.float64(0)
    for v in frame_term:                # in frame order
        total = total + v
    with np.errstate(all='ignore'):
        term = _F32(total / np.float64(F))
    return dict(q=q, count=count, result=res, term=term, mean=mean, coef=coef, unit=unit,
                frame_term=frame_term)


def contrast_bwd_host(x, y, t, sample_index, frame_ts, frame_sample, flow, fwd, seed=1.0, weight=1.0):
    """CONTRAST_SPEC section 5 on the host: what ``dvsof_contrast_bwd`` is
    pinned to.  fwd: the dict of ``contrast_fwd_host`` for the same input.
    -> (grad_flow float32 [F,2,h,w] = seed * weight * d term / d flow,
    sums int64 [F,2,h,w], the fixed-point sums in units of 1/unit[f])."""
    flow = np.asarray(flow, _F32)
    F, _, h, w = flow.shape
    p = _contrast_pairs(x, y, t, sample_index, frame_ts, frame_sample, flow)
    k = p['inside'] & (fwd['coef'][p['f']] != 0)
    f, cx, cy, px, py = p['f'][k], p['cx'][k], p['cy'][k], p['x'][k], p['y'][k]
    coef, mean, unit = fwd['coef'][f], fwd['mean'][f], fwd['unit'][f]
    G = [[None, None], [None, None]]
    for j in range(2):
        for i in range(2):
            xx, yy = cx + i, cy + j
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            Q = fwd['q'][f, np.where(ok, yy, 0), np.where(ok, xx, 0)]
            G[j][i] = np.where(ok, coef * (Q.astype(np.float64) * 2.0 ** -32 - mean), 0.0)
    wx = [a[k].astype(np.float64) for a in p['wx']]
    wy = [a[k].astype(np.float64) for a in p['wy']]
    gx = wy[0] * (G[0][1] - G[0][0]) + wy[1] * (G[1][1] - G[1][0])
    gy = wx[0] * (G[1][0] - G[0][0]) + wx[1] * (G[1][1] - G[0][1])
    mt = -p['tau'][k].astype(np.float64)
    sums = np.zeros((F, 2, h, w), np.int64)
    np.add.at(sums, (f, 0, py, px), np.trunc(mt * gx * unit).astype(np.int64))
    np.add.at(sums, (f, 1, py, px), np.trunc(mt * gy * unit).astype(np.int64))
    value = sums.astype(np.float64) / fwd['unit'].reshape(F, 1, 1, 1) / np.float64(max(F, 1))
    sw = _F32(seed) * _F32(weight)
    return sw * value.astype(_F32), sums


# Several reference times, ON and OFF events apart (csrc/contrast.hip,
# CONTRAST_SPEC sections 11-15)
CONTRAST_REFERENCES = {'start': 0.0, 'middle': 0.5, 'end': 1.0}     # name -> rho, in the order of the mask's bits
CONTRAST_SHARED_BITS = 2


def contrast_reference_mask(references):
    """('end', 'start') -> 5: bit 0 start, bit 1 middle, bit 2 end.  Names in
    any order; an empty list, an unknown name and a duplicate are refused.  An
    int in [1, 7] is taken as the mask it is."""
    if isinstance(references, (int, np.integer)):
        if not 1 <= references <= 7:
            raise ValueError(f'reference mask {references} is outside [1, 7]')
        return int(references)
    if isinstance(references, str):
        references = references.split(',')
    names = list(CONTRAST_REFERENCES)
    mask = 0
    for name in references:
        if name not in names:
            raise ValueError(f'unknown reference time "{name}": one of {", ".join(names)}')
        if mask >> names.index(name) & 1:
            raise ValueError(f'reference time "{name}" is given twice')
        mask |= 1 << names.index(name)
    if not mask:
        raise ValueError('no reference time given')
    return mask


def _contrast_rhos(mask):
    return [_F32(rho) for b, rho in enumerate(CONTRAST_REFERENCES.values()) if mask >> b & 1]


def _contrast_multi_pairs(x, y, t, p, sample_index, frame_ts, frame_sample, flow, polarity):
    """The (event, frame) pairs that take part, frame by frame: dict of
    per-pair arrays f, c (the channel), x, y, tau, u, v (the flow at the
    event's own pixel).  With ``polarity`` an event with p == 0 takes no part;
    without it p is not read."""
    x, y = np.asarray(x, np.int64).reshape(-1), np.asarray(y, np.int64).reshape(-1)
    t = np.asarray(t, _F32).reshape(-1)
    s = np.asarray(sample_index, np.int64).reshape(-1)
    ts = np.asarray(frame_ts, _F32).reshape(-1)
    fs = np.asarray(frame_sample, np.int64).reshape(-1)
    F, _, h, w = flow.shape
    assert ts.size == 2 * F and fs.size == F and x.size == y.size == t.size == s.size
    inb = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    chan = np.zeros(x.size, np.int64)
    if polarity:
        p = np.asarray(p, np.int64).reshape(-1)
        assert p.size == x.size
        inb &= p != 0
        chan = (p < 0).astype(np.int64)
    sel = [np.flatnonzero(inb & (s == fs[f]) & (ts[2 * f] <= t) & (t <= ts[2 * f + 1]))
           for f in range(F)]
    e = np.concatenate(sel) if F else np.zeros(0, np.int64)
    f = np.concatenate([np.full(k.size, i, np.int64) for i, k in enumerate(sel)]) if F \
        else np.zeros(0, np.int64)
    x, y, t = x[e], y[e], t[e]
    t0 = ts[2 * f]
    d = ts[2 * f + 1] - t0
    with np.errstate(all='ignore'):
        tau = np.where(d > 0, np.fmin(np.fmax((t - t0) / d, _F32(0)), _F32(1)), _F32(0)).astype(_F32)
    return dict(f=f, c=chan[e], x=x, y=y, tau=tau, u=flow[f, 0, y, x], v=flow[f, 1, y, x])


def _contrast_warp_to(p, rho, h, w):
    """``warp_event_to`` of csrc/frame_common.h for the pairs p and one
    reference: sig = tau - rho in float32, then steps 2-6 of IWE_SPEC section
    2 with sig in place of tau -> dict sig, inside, cx, cy, wx [2], wy [2]."""
    with np.errstate(all='ignore'):
        sig = (p['tau'] - _F32(rho)).astype(_F32)
        xw = p['x'].astype(_F32) - sig * p['u']
        yw = p['y'].astype(_F32) - sig * p['v']
        inside = (xw > _F32(-1)) & (xw < _F32(w)) & (yw > _F32(-1)) & (yw < _F32(h))
        xw, yw = np.where(inside, xw, _F32(0)), np.where(inside, yw, _F32(0))
    flx, fly = np.floor(xw), np.floor(yw)
    fx, fy = xw - flx, yw - fly
    return dict(sig=sig, inside=inside, cx=flx.astype(np.int64), cy=fly.astype(np.int64),
                wx=(_F32(1) - fx, fx), wy=(_F32(1) - fy, fy))


def contrast_multi_fwd_host(x, y, t, p, sample_index, frame_ts, frame_sample, flow, references=('start',),
                            polarity=False):
    """CONTRAST_SPEC sections 11-13 on the host: what
    ``dvsof_contrast_multi_fwd`` is pinned to, byte for byte.  The arguments of
    ``contrast_fwd_host`` and the column p int64 [n] (None without
    ``polarity``); references: names or a mask.  With M = F R C images,
    m = (f R + r) C + c -> dict: q int64 [M,h,w], count uint32 [M,h,w], result
    (M rows), term float32, the per-image float64 records mean, coef, gmax,
    image_term [M], the per-frame unit [F], and mask, R, C."""
    from . import eval as ev
    flow = np.asarray(flow, _F32)
    F, _, h, w = flow.shape
    mask = contrast_reference_mask(references)
    rhos, C = _contrast_rhos(mask), 2 if polarity else 1
    R = len(rhos)
    M = F * R * C
    pr = _contrast_multi_pairs(x, y, t, p, sample_index, frame_ts, frame_sample, flow, polarity)
    q = np.zeros((M, h, w), np.int64)
    count = np.zeros((M, h, w), np.uint32)
    for r, rho in enumerate(rhos):
        m = (pr['f'] * R + r) * C + pr['c']
        np.add.at(count, (m, pr['y'], pr['x']), 1)
        wp = _contrast_warp_to(pr, rho, h, w)
        k = wp['inside']
        mk, cx, cy = m[k], wp['cx'][k], wp['cy'][k]
        for j in range(2):
            for i in range(2):
                xx, yy = cx + i, cy + j
                Q = ((wp['wy'][j][k] * wp['wx'][i][k]).astype(_F32) * _F32(ev.IWE_ONE)).astype(np.int64)
                ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h) & (Q > 0)
                np.add.at(q, (mk[ok], yy[ok], xx[ok]), Q[ok])
    res = ev.iwe_stats_host(q, count)
    res['sum_sq'] = ev.iwe_sum_sq_kernel_order(q)
    # the closing wave, in float64
    N = np.float64(h) * np.float64(w)
    mean = res['sum_q'].astype(np.float64) * 2.0 ** -32 / N
    var_i = res['sum_sq'] / N - mean * mean
    cmean = res['count_sum'].astype(np.float64) / N
    var_c = res['count_sq'].astype(np.float64) / N - cmean * cmean
    live = var_c > 0
    with np.errstate(all='ignore'):
        coef = np.where(live, -2.0 / (N * var_c), 0.0)
        image_term = np.where(live, 1.0 - var_i / var_c, 0.0)
    gmax = np.abs(coef) * np.fmax(res['max_q'].astype(np.float64) * 2.0 ** -32 - mean, mean)
    frame_gmax = gmax.reshape(F, R * C).max(1) if F else np.zeros(0)
    e = np.where(frame_gmax > 0, np.frexp(frame_gmax)[1], 0)
    unit = np.ldexp(1.0, CONTRAST_UNIT_BITS - (CONTRAST_SHARED_BITS if R > 1 else 0) - e)
    total = np.float64(0)
    for v in image_term:                # in image order
        total = total + v
    with np.errstate(all='ignore'):
        term = _F32(total / np.float64(M))
    return dict(q=q, count=count, result=res, term=term, mean=mean, coef=coef, gmax=gmax,
                image_term=image_term, unit=unit, mask=mask, R=R, C=C)


def contrast_multi_bwd_host(x, y, t, p, sample_index, frame_ts, frame_sample, flow, fwd, seed=1.0, weight=1.0):
    """CONTRAST_SPEC section 14 on the host: what ``dvsof_contrast_multi_bwd``
    is pinned to.  fwd: the dict of ``contrast_multi_fwd_host`` for the same
    input; references and polarity are read from it.  -> (grad_flow float32
    [F,2,h,w] = seed * weight * d term / d flow, sums int64 [F,2,h,w], the
    fixed-point sums of all images of a frame in units of 1/unit[f])."""
    flow = np.asarray(flow, _F32)
    F, _, h, w = flow.shape
    R, C = fwd['R'], fwd['C']
    M = F * R * C
    pr = _contrast_multi_pairs(x, y, t, p, sample_index, frame_ts, frame_sample, flow, C == 2)
    sums = np.zeros((F, 2, h, w), np.int64)
    for r, rho in enumerate(_contrast_rhos(fwd['mask'])):
        m = (pr['f'] * R + r) * C + pr['c']
        wp = _contrast_warp_to(pr, rho, h, w)
        k = wp['inside'] & (fwd['coef'][m] != 0)
        m, f, cx, cy, px, py = m[k], pr['f'][k], wp['cx'][k], wp['cy'][k], pr['x'][k], pr['y'][k]
        coef, mean, unit = fwd['coef'][m], fwd['mean'][m], fwd['unit'][f]
        G = [[None, None], [None, None]]
        for j in range(2):
            for i in range(2):
                xx, yy = cx + i, cy + j
                ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                Q = fwd['q'][m, np.where(ok, yy, 0), np.where(ok, xx, 0)]
                G[j][i] = np.where(ok, coef * (Q.astype(np.float64) * 2.0 ** -32 - mean), 0.0)
        wx = [a[k].astype(np.float64) for a in wp['wx']]
        wy = [a[k].astype(np.float64) for a in wp['wy']]
        gx = wy[0] * (G[0][1] - G[0][0]) + wy[1] * (G[1][1] - G[1][0])
        gy = wx[0] * (G[1][0] - G[0][0]) + wx[1] * (G[1][1] - G[0][1])
        ms = -wp['sig'][k].astype(np.float64)
        np.add.at(sums, (f, 0, py, px), np.trunc(ms * gx * unit).astype(np.int64))
        np.add.at(sums, (f, 1, py, px), np.trunc(ms * gy * unit).astype(np.int64))
    value = sums.astype(np.float64) / fwd['unit'].reshape(F, 1, 1, 1) / np.float64(max(M, 1))
    sw = _F32(seed) * _F32(weight)
    return sw * value.astype(_F32), sums


def wire_event_columns(events):
    """The wire columns a compact event dict (voxel.is_compact) stands for, on
    the dict's device, by the definition of include/dvsof_event_terms_encoded.h:
    x, y widened to int64, polarity ? +1 : -1, and sample_index[i] the largest
    b in [0, B) with sample_event_offsets[b] <= i (empty samples are repeated
    offsets; a slot at or past the last offset falls to sample B - 1).  -> dict
    of x, y, timestamp, polarity, sample_index.  A wire dict is returned as it
    is.  For the host restatements and the tests: the encoded entry points give
    the bytes of their wire twins on these columns."""
    if not voxel.is_compact(events):
        return events
    off = torch.as_tensor(events['sample_event_offsets']).long().reshape(-1)
    x = torch.as_tensor(events['x'])
    B = off.numel() - 1
    assert B >= 1 or x.numel() == 0, 'one offset per sample plus the end'
    index = torch.arange(x.numel(), dtype=torch.long, device=x.device)
    sample = (torch.searchsorted(off[:max(B, 0)].to(x.device), index, right=True) - 1).clamp_(min=0)
    return {'x': x.long(), 'y': torch.as_tensor(events['y']).long(),
            'timestamp': torch.as_tensor(events['timestamp']).float(),
            'polarity': torch.as_tensor(events['polarity']).bool().long() * 2 - 1,
            'sample_index': sample}


def _as_bytes(polarity):
    """The bool polarity column as the uint8 the entry points read: a view of
    the same bytes (no launch, which matters inside a captured step); another
    dtype is cast as voxel.voxelize_compact casts it."""
    return polarity.view(torch.uint8) if polarity.dtype == torch.bool else polarity.to(torch.uint8)


def _term_columns(events, polarity):
    """-> (x, y, timestamp, polarity or None, sample) of an event dict for the
    four autograd functions below: the wire columns as they are, or the compact
    ones (voxel.is_compact) with the casts of voxel.voxelize_compact, where
    ``sample`` is sample_event_offsets and x is int16, which is how the
    functions tell the two forms apart."""
    if not voxel.is_compact(events):
        cols = tuple(events[k] for k in ('x', 'y', 'timestamp', 'sample_index'))
        return cols[:3] + (events['polarity'] if polarity else None, cols[3])
    return (events['x'].to(torch.short).contiguous(), events['y'].to(torch.short).contiguous(),
            events['timestamp'].to(torch.float32).contiguous(),
            _as_bytes(events['polarity']).contiguous() if polarity else None,
            events['sample_event_offsets'].to(torch.long).contiguous())


def _bind_columns(x, y, t, p, sample, polarity):
    """The event-column arguments of an entry point and of its encoded twin
    (include/dvsof_event_terms_encoded.h) -> (suffix of the entry point's name,
    the leading arguments up to and including n_events, the tensors they point
    into).  int16 x: the compact columns, ``sample`` their B + 1 offsets."""
    cols = tuple(c.contiguous() for c in (x, y, t, sample))
    pol = p.contiguous() if polarity else None
    n = cols[0].numel()
    assert cols[0].numel() == cols[1].numel() == cols[2].numel() and cols[2].dtype == torch.float32
    assert pol is None or pol.numel() == n
    if cols[0].dtype == torch.short:
        assert cols[1].dtype == torch.short and cols[3].dtype == torch.long
        assert pol is None or pol.dtype == torch.uint8
        B = cols[3].numel() - 1
        assert B >= 1, 'one offset per sample plus the end'
        return '_encoded', [c.data_ptr() for c in cols[:3]] + [_lib.ptr(pol), cols[3].data_ptr(), B, n], (cols, pol)
    assert cols[0].dtype == cols[1].dtype == cols[3].dtype == torch.long and cols[3].numel() == n
    assert pol is None or pol.dtype == torch.long
    return '', [c.data_ptr() for c in cols[:3]] + [_lib.ptr(pol), cols[3].data_ptr(), n], (cols, pol)


class _Contrast(torch.autograd.Function):
    """(weight * term, term) of the finest flow; the gradient of the first
    enters the flow (dvsof_contrast_multi_fwd / dvsof_contrast_multi_bwd, with
    the reference times of ``mask`` and the polarities apart or not).  The
    weight is applied inside the backward's closing kernel."""

    @staticmethod
    def forward(ctx, flow, x, y, t, p, sample_index, frame_ts, frame_sample, weight, mask, polarity):
        from .eval import IWE_RESULT_DTYPE
        dev = flow.device
        flow = flow.detach().contiguous().float()
        F, _, h, w = flow.shape
        lib = _lib.lib()
        M = F * bin(mask).count('1') * (2 if polarity else 1)
        q = torch.empty(M, h, w, dtype=torch.long, device=dev)
        count = torch.empty(M, h, w, dtype=torch.int32, device=dev)
        result = torch.empty(M, IWE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        term = torch.zeros((), dtype=torch.float32, device=dev) if F == 0 else \
            torch.empty((), dtype=torch.float32, device=dev)
        nbytes = lib.dvsof_contrast_multi_workspace_bytes(F, mask, int(polarity), h, w)
        ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.long, device=dev)
        tables = (frame_ts.contiguous().float(), frame_sample.contiguous().long())
        assert tables[0].numel() == 2 * F and tables[1].numel() == F, (flow.shape, frame_ts.shape)
        ctx.form, head, (cols, pol) = _bind_columns(x, y, t, p, sample_index, polarity)
        ctx.args = (head + [tables[0].data_ptr(), tables[1].data_ptr(),
                       flow.data_ptr(), F, h, w, mask, int(polarity)])
        _lib.check(getattr(lib, 'dvsof_contrast_multi_fwd' + ctx.form)(
            *ctx.args, q.data_ptr(), count.data_ptr(), result.data_ptr(), term.data_ptr(), ws.data_ptr(),
            nbytes, _lib.stream()), 'dvsof_contrast_multi_fwd' + ctx.form)
        ctx.held = (cols, pol, tables, flow, q, ws, nbytes)
        ctx.weight = float(weight)
        ctx.mark_non_differentiable(term)
        ctx.set_materialize_grads(False)
        return term * ctx.weight, term

    @staticmethod
    def backward(ctx, g_value, _g_term):
        if g_value is None:
            return (None,) * 11
        flow, q, ws, nbytes = ctx.held[3:]
        grad = torch.empty_like(flow)
        seed = g_value.contiguous().float()
        _lib.check(getattr(_lib.lib(), 'dvsof_contrast_multi_bwd' + ctx.form)(
            *ctx.args, q.data_ptr(), ws.data_ptr(), nbytes, seed.data_ptr(), ctx.weight, grad.data_ptr(),
            _lib.stream()), 'dvsof_contrast_multi_bwd' + ctx.form)
        return (grad,) + (None,) * 10


# The term on every flow scale (csrc/contrast.hip, CONTRAST_SPEC sections 19-23)
CONTRAST_SCALES = ('finest', 'all')
CONTRAST_MAX_LEVELS = 8
CONTRAST_MAX_SHIFT = 15


def contrast_level_shift(shape, level_shape):
    """The shift s of a level of shape ``level_shape`` under the frame
    ``shape`` the event coordinates live in: the smallest s in [0, 15] with
    h_k == ceil(h / 2^s) and w_k == ceil(w / 2^s), the chain of stride-2
    halvings.  An event at x < w sits at level column x >> s < w_k.  A level
    with no such s is refused."""
    (h, w), (hk, wk) = (int(v) for v in shape), (int(v) for v in level_shape)
    for s in range(CONTRAST_MAX_SHIFT + 1):
        if hk == -(-h // 2 ** s) and wk == -(-w // 2 ** s):
            return s
    raise ValueError(f'a level of shape {(hk, wk)} is no halving of the frame {(h, w)}: '
                     f'no shift s in [0, {CONTRAST_MAX_SHIFT}] gives ceil(h / 2^s), ceil(w / 2^s)')


def contrast_level_columns(x, y, shape, shift):
    """The columns x, y quantised to a level's grid: x >> shift, y >> shift
    for an event inside the full-resolution frame, -1 for one outside it (the
    inside test is made before the shift)."""
    x, y = np.asarray(x, np.int64).reshape(-1), np.asarray(y, np.int64).reshape(-1)
    h, w = shape
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    return np.where(inside, x >> shift, -1), np.where(inside, y >> shift, -1)


def contrast_level_weights(weight, K):
    """One float32 weight per level: float32(weight) / float32(K), one
    division (the reference's mean over scales)."""
    return [_F32(weight) / _F32(K)] * K


def contrast_pyramid_fwd_host(x, y, t, p, sample_index, frame_ts, frame_sample, flows, shape, weights=None,
                              references=('start',), polarity=False):
    """CONTRAST_SPEC sections 19-21 on the host: what
    ``dvsof_contrast_pyramid_fwd`` is pinned to, byte for byte.  flows: one
    float32 [F,2,h_k,w_k] per level; shape: the frame (h, w) of the event
    coordinates; weights: one per level (default ``contrast_level_weights(1,
    K)``).  Per level ``contrast_multi_fwd_host`` on the quantised columns,
    then the combination -> dict: levels (the K dicts of that function),
    shifts, weights float32 [K], terms float32 [K] (unweighted), terms64,
    value float32."""
    K = len(flows)
    if not 1 <= K <= CONTRAST_MAX_LEVELS:
        raise ValueError(f'{K} levels: the level table holds 1 to {CONTRAST_MAX_LEVELS}')
    flows = [np.asarray(f, _F32) for f in flows]
    shifts = [contrast_level_shift(shape, f.shape[-2:]) for f in flows]
    weights = np.asarray(contrast_level_weights(1.0, K) if weights is None else weights, _F32)
    assert weights.shape == (K,)
    levels = []
    for flow, s in zip(flows, shifts):
        xs, ys = contrast_level_columns(x, y, shape, s)
        levels.append(contrast_multi_fwd_host(xs, ys, t, p, sample_index, frame_ts, frame_sample, flow,
                                              references, polarity))
    terms64 = np.zeros(K, np.float64)
    total = np.float64(0)
    with np.errstate(all='ignore'):
        for k, lev in enumerate(levels):        # in level order
            s = np.float64(0)
            for v in lev['image_term']:         # in image order
                s = s + v
            terms64[k] = s / np.float64(len(lev['image_term']))
            total = total + np.float64(weights[k]) * terms64[k]
        return dict(levels=levels, shifts=shifts, weights=weights, terms=terms64.astype(_F32), terms64=terms64,
                    value=_F32(total), shape=tuple(int(v) for v in shape))


def contrast_pyramid_bwd_host(x, y, t, p, sample_index, frame_ts, frame_sample, flows, fwd, seed=1.0):
    """CONTRAST_SPEC section 22 on the host: what ``dvsof_contrast_pyramid_bwd``
    is pinned to.  fwd: the dict of ``contrast_pyramid_fwd_host`` for the same
    input.  -> one (grad_flow_k float32 [F,2,h_k,w_k] = seed * weight_k *
    d term_k / d flow_k, sums int64 [F,2,h_k,w_k]) per level."""
    out = []
    for flow, s, lev, weight in zip(flows, fwd['shifts'], fwd['levels'], fwd['weights']):
        xs, ys = contrast_level_columns(x, y, fwd['shape'], s)
        out.append(contrast_multi_bwd_host(xs, ys, t, p, sample_index, frame_ts, frame_sample, flow, lev,
                                           seed=seed, weight=weight))
    return out


def contrast_level_table(shape, level_shapes, F, M, weights, flows=None, grads=None):
    """The by-value level table of include/dvsof_contrast_pyramid.h with the
    packed offsets: shapes, shifts (``contrast_level_shift``: ValueError for a
    level that is no halving), weights and, where given, the addresses of the
    flows and of the gradient buffers."""
    K = len(level_shapes)
    if not 1 <= K <= CONTRAST_MAX_LEVELS:
        raise ValueError(f'{K} levels: the level table holds 1 to {CONTRAST_MAX_LEVELS}')
    table = _lib.ContrastLevels()
    table.K = K
    pixels = 0
    for k, (hk, wk) in enumerate(level_shapes):
        lev = table.level[k]
        lev.h, lev.w, lev.shift = int(hk), int(wk), contrast_level_shift(shape, (hk, wk))
        lev.weight = float(weights[k])
        lev.image_offset, lev.row_offset, lev.sums_offset = M * pixels, k * M, 2 * F * pixels
        lev.flow = flows[k] if flows is not None else None
        lev.grad_flow = grads[k] if grads is not None else None
        pixels += int(hk) * int(wk)
    return table


class _ContrastPyramid(torch.autograd.Function):
    """(sum_k weight_k term_k, terms [K]) of all flows; the gradient of the
    first enters every flow (dvsof_contrast_pyramid_fwd /
    dvsof_contrast_pyramid_bwd: one splat and one backward for all levels).
    The weights are applied inside the kernels."""

    @staticmethod
    def forward(ctx, x, y, t, p, sample_index, frame_ts, frame_sample, shape, weights, mask, polarity, *flows):
        from .eval import IWE_RESULT_DTYPE
        dev = flows[0].device
        flows = tuple(f.detach().contiguous().float() for f in flows)
        K, F = len(flows), flows[0].shape[0]
        assert all(f.shape[0] == F and f.shape[1] == 2 for f in flows)
        lib = _lib.lib()
        M = F * bin(mask).count('1') * (2 if polarity else 1)
        shapes = [tuple(f.shape[-2:]) for f in flows]
        table = contrast_level_table(shape, shapes, F, M, weights, [f.data_ptr() for f in flows])
        terms = torch.zeros(K, dtype=torch.float32, device=dev) if F == 0 else \
            torch.empty(K, dtype=torch.float32, device=dev)
        value = torch.zeros((), dtype=torch.float32, device=dev) if F == 0 else \
            torch.empty((), dtype=torch.float32, device=dev)
        result = torch.empty(K * M, IWE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        h, w = (int(v) for v in shape)
        nbytes = lib.dvsof_contrast_pyramid_workspace_bytes(F, mask, int(polarity), h, w, table)
        ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.long, device=dev)
        tables = (frame_ts.contiguous().float(), frame_sample.contiguous().long())
        assert tables[0].numel() == 2 * F and tables[1].numel() == F, (flows[0].shape, frame_ts.shape)
        ctx.form, head, (cols, pol) = _bind_columns(x, y, t, p, sample_index, polarity)
        ctx.args = (head + [tables[0].data_ptr(), tables[1].data_ptr(),
                       F, h, w, mask, int(polarity)])
        _lib.check(getattr(lib, 'dvsof_contrast_pyramid_fwd' + ctx.form)(
            *ctx.args, table, result.data_ptr(), terms.data_ptr(), value.data_ptr(), ws.data_ptr(), nbytes,
            _lib.stream()), 'dvsof_contrast_pyramid_fwd' + ctx.form)
        ctx.held = (cols, pol, tables, flows, ws, nbytes, table)
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return value, terms

    @staticmethod
    def backward(ctx, g_value, _g_terms):
        flows, ws, nbytes, table = ctx.held[3:]
        if g_value is None:
            return (None,) * (11 + len(flows))
        grads = tuple(torch.empty_like(f) for f in flows)
        for k, g in enumerate(grads):
            table.level[k].grad_flow = g.data_ptr()
        seed = g_value.contiguous().float()
        _lib.check(getattr(_lib.lib(), 'dvsof_contrast_pyramid_bwd' + ctx.form)(
            *ctx.args, table, ws.data_ptr(), nbytes, seed.data_ptr(), _lib.stream()),
            'dvsof_contrast_pyramid_bwd' + ctx.form)
        return (None,) * 11 + grads


# ---------------------------------------------------------------------------
# Average-timestamp term (csrc/avg_timestamp.hip, docs/AVG_TIMESTAMP_SPEC.md)
# ---------------------------------------------------------------------------
AVG_TIMESTAMP_EPS = 2.0 ** -10
AVG_TIMESTAMP_REC_DTYPE = np.dtype([(k, '<f8') for k in ('S', 'S0', 'n', 'n0', 'peak', 'value', 'k2', 'gmax')])
AVG_TIMESTAMP_ROW_DTYPE = np.dtype([('S', '<f8'), ('S0', '<f8'), ('peak', '<f8'), ('n', '<u4'), ('n0', '<u4')])


def avg_timestamp_layout(F, M, h, w):
    """The byte offsets of include/dvsof_avg_timestamp.h -> dict: q, s, base,
    sums, count, zeroed_bytes, rec, unit, rows, part, bytes, nb."""
    from . import eval as ev
    P, S, nb = M * h * w, 2 * F * h * w, ev.partial_blocks(h * w)
    o = dict(q=0, s=8 * P, base=16 * P, sums=24 * P, count=24 * P + 8 * S, nb=nb)
    o['zeroed_bytes'] = o['count'] + 4 * P
    o['rec'] = (o['zeroed_bytes'] + 7) // 8 * 8
    o['unit'] = o['rec'] + 64 * M
    o['rows'] = o['unit'] + 8 * F
    o['part'] = o['rows'] + 32 * M
    o['bytes'] = o['part'] + 32 * M * nb
    return o


def _avg_timestamp_pixels(q, s):
    """T = A / (I + eps) and D = 1 / (I + eps) in float64, as both kernels form them."""
    den = q.astype(np.float64) * 2.0 ** -32 + AVG_TIMESTAMP_EPS
    return s.astype(np.float64) * 2.0 ** -32 / den, 1.0 / den


def avg_timestamp_splat_host(pr, mask, polarity, F, h, w):
    """AVG_TIMESTAMP_SPEC section 2, steps 1-3 (``avgts_splat_event`` of
    csrc/avg_timestamp_images.h) for the (event, frame) pairs pr that take part
    (the dict of ``_contrast_multi_pairs``; which pairs those are is the
    caller's frame rule) -> q, s, base int64 [M,h,w], count uint32 [M,h,w]."""
    from . import eval as ev
    rhos, C = _contrast_rhos(mask), 2 if polarity else 1
    R = len(rhos)
    M = F * R * C
    q, s, base = (np.zeros((M, h, w), np.int64) for _ in range(3))
    count = np.zeros((M, h, w), np.uint32)
    one = _F32(ev.IWE_ONE)
    for r, rho in enumerate(rhos):
        m = (pr['f'] * R + r) * C + pr['c']
        wp = _contrast_warp_to(pr, rho, h, w)
        a = np.abs(wp['sig'])
        np.add.at(count, (m, pr['y'], pr['x']), 1)
        np.add.at(base, (m, pr['y'], pr['x']), (a * one).astype(np.int64))
        k = wp['inside']
        mk, cx, cy, ak = m[k], wp['cx'][k], wp['cy'][k], a[k]
        for j in range(2):
            for i in range(2):
                xx, yy = cx + i, cy + j
                wgt = (wp['wy'][j][k] * wp['wx'][i][k]).astype(_F32)
                Q = (wgt * one).astype(np.int64)
                QA = ((wgt * ak).astype(_F32) * one).astype(np.int64)
                ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                np.add.at(q, (mk[ok], yy[ok], xx[ok]), Q[ok])
                np.add.at(s, (mk[ok], yy[ok], xx[ok]), QA[ok])
    return q, s, base, count


def avg_timestamp_pixels_host(q, s, base, count):
    """AVG_TIMESTAMP_SPEC section 3 per pixel, in float64 -> (T, D, T0), each
    of the images' shape: ``avgts_pixel`` of csrc/avg_timestamp_images.h."""
    T, D = _avg_timestamp_pixels(q, s)
    T0 = base.astype(np.float64) * 2.0 ** -32 / (count.astype(np.float64) + AVG_TIMESTAMP_EPS)
    return T, D, T0


def avg_timestamp_rows_host(q, s, base, count):
    """The statistics rows of M images (AVG_TIMESTAMP_ROW_DTYPE), the sums in
    the kernels' order (``eval.kernel_order_sum``): the bits
    ``avgts_stats_partial_kernel`` and the closing reduction store."""
    from . import eval as ev
    M, h, w = q.shape
    N, nb = h * w, ev.partial_blocks(h * w)
    T, D, T0 = avg_timestamp_pixels_host(q.reshape(M, N), s.reshape(M, N), base.reshape(M, N),
                                         count.reshape(M, N))
    rows = np.zeros(M, AVG_TIMESTAMP_ROW_DTYPE)
    if M:
        rows['S'], rows['S0'] = ev.kernel_order_sum(T * T, nb), ev.kernel_order_sum(T0 * T0, nb)
        rows['peak'] = (2.0 * T * D).max(1)
        rows['n'], rows['n0'] = (q.reshape(M, N) > 0).sum(1), (count.reshape(M, N) > 0).sum(1)
    return rows


def avg_timestamp_fwd_host(x, y, t, p, sample_index, frame_ts, frame_sample, flow, references=('start', 'end'),
                           polarity=False):
    """AVG_TIMESTAMP_SPEC sections 2-5 on the host: what
    ``dvsof_avg_timestamp_fwd`` is pinned to, byte for byte.  The arguments of
    ``contrast_multi_fwd_host``.  With M = F R C images, m = (f R + r) C + c ->
    dict: q, s, base int64 [M,h,w], count uint32 [M,h,w], rows (M statistics
    rows, AVG_TIMESTAMP_ROW_DTYPE, the sums in the kernels' order), rec (M
    records, AVG_TIMESTAMP_REC_DTYPE), image_value float64 [M], unit float64
    [F], term float32, and mask, R, C."""
    flow = np.asarray(flow, _F32)
    F, _, h, w = flow.shape
    mask = contrast_reference_mask(references)
    rhos, C = _contrast_rhos(mask), 2 if polarity else 1
    R = len(rhos)
    M = F * R * C
    pr = _contrast_multi_pairs(x, y, t, p, sample_index, frame_ts, frame_sample, flow, polarity)
    q, s, base, count = avg_timestamp_splat_host(pr, mask, polarity, F, h, w)
    rows = avg_timestamp_rows_host(q, s, base, count)
    # the closing wave
    rec = np.zeros(M, AVG_TIMESTAMP_REC_DTYPE)
    for k_ in ('S', 'S0', 'n', 'n0', 'peak'):
        rec[k_] = rows[k_]
    live, stayed = rec['S0'] > 0, rec['n'] > 0
    with np.errstate(all='ignore'):
        rec['value'] = np.where(live, np.where(stayed, (rec['S'] / rec['n']) / (rec['S0'] / rec['n0']), 1.0), 0.0)
        rec['k2'] = np.where(live & stayed, 2.0 * (rec['n0'] / (rec['n'] * rec['S0'])), 0.0)
    rec['gmax'] = 0.5 * rec['k2'] * rec['peak']
    frame_gmax = rec['gmax'].reshape(F, R * C).max(1) if F else np.zeros(0)
    e = np.where(frame_gmax > 0, np.frexp(frame_gmax)[1], 0)
    unit = np.ldexp(1.0, CONTRAST_UNIT_BITS - (CONTRAST_SHARED_BITS if R > 1 else 0) - e)
    total = np.float64(0)
    for v in rec['value']:              # in image order
        total = total + v
    with np.errstate(all='ignore'):
        term = _F32(total / np.float64(M))
    return dict(q=q, s=s, base=base, count=count, rows=rows, rec=rec, image_value=rec['value'].copy(), unit=unit,
                term=term, mask=mask, R=R, C=C)


def avg_timestamp_bwd_host(x, y, t, p, sample_index, frame_ts, frame_sample, flow, fwd, seed=1.0, weight=1.0):
    """AVG_TIMESTAMP_SPEC section 6 on the host: what ``dvsof_avg_timestamp_bwd``
    is pinned to.  fwd: the dict of ``avg_timestamp_fwd_host`` for the same
    input; references and polarity are read from it.  -> (grad_flow float32
    [F,2,h,w] = seed * weight * d term / d flow, sums int64 [F,2,h,w], the
    fixed-point sums of all images of a frame in units of 1/unit[f])."""
    flow = np.asarray(flow, _F32)
    F, _, h, w = flow.shape
    R, C = fwd['R'], fwd['C']
    M = F * R * C
    pr = _contrast_multi_pairs(x, y, t, p, sample_index, frame_ts, frame_sample, flow, C == 2)
    T, D = _avg_timestamp_pixels(fwd['q'], fwd['s'])
    sums = np.zeros((F, 2, h, w), np.int64)
    for r, rho in enumerate(_contrast_rhos(fwd['mask'])):
        m = (pr['f'] * R + r) * C + pr['c']
        wp = _contrast_warp_to(pr, rho, h, w)
        k = wp['inside'] & (fwd['rec']['k2'][m] != 0)
        m, f, cx, cy, px, py = m[k], pr['f'][k], wp['cx'][k], wp['cy'][k], pr['x'][k], pr['y'][k]
        k2, unit = fwd['rec']['k2'][m], fwd['unit'][f]
        a = np.abs(wp['sig'][k]).astype(np.float64)
        G = [[None, None], [None, None]]
        for j in range(2):
            for i in range(2):
                xx, yy = cx + i, cy + j
                ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                at = (m, np.where(ok, yy, 0), np.where(ok, xx, 0))
                G[j][i] = np.where(ok, k2 * T[at] * D[at] * (a - T[at]), 0.0)
        wx = [v[k].astype(np.float64) for v in wp['wx']]
        wy = [v[k].astype(np.float64) for v in wp['wy']]
        gx = wy[0] * (G[0][1] - G[0][0]) + wy[1] * (G[1][1] - G[1][0])
        gy = wx[0] * (G[1][0] - G[0][0]) + wx[1] * (G[1][1] - G[0][1])
        ms = -wp['sig'][k].astype(np.float64)
        np.add.at(sums, (f, 0, py, px), np.trunc(ms * gx * unit).astype(np.int64))
        np.add.at(sums, (f, 1, py, px), np.trunc(ms * gy * unit).astype(np.int64))
    value = sums.astype(np.float64) / fwd['unit'].reshape(F, 1, 1, 1) / np.float64(max(M, 1))
    sw = _F32(seed) * _F32(weight)
    return sw * value.astype(_F32), sums


class _AvgTimestamp(torch.autograd.Function):
    """(weight * term, term) of the finest flow; the gradient of the first
    enters the flow (dvsof_avg_timestamp_fwd / dvsof_avg_timestamp_bwd).  The
    images live in the workspace; the weight is applied inside the backward's
    closing kernel."""

    @staticmethod
    def forward(ctx, flow, x, y, t, p, sample_index, frame_ts, frame_sample, weight, mask, polarity):
        dev = flow.device
        flow = flow.detach().contiguous().float()
        F, _, h, w = flow.shape
        lib = _lib.lib()
        term = torch.zeros((), dtype=torch.float32, device=dev) if F == 0 else \
            torch.empty((), dtype=torch.float32, device=dev)
        nbytes = lib.dvsof_avg_timestamp_workspace_bytes(F, mask, int(polarity), h, w)
        ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.long, device=dev)
        tables = (frame_ts.contiguous().float(), frame_sample.contiguous().long())
        assert tables[0].numel() == 2 * F and tables[1].numel() == F, (flow.shape, frame_ts.shape)
        ctx.form, head, (cols, pol) = _bind_columns(x, y, t, p, sample_index, polarity)
        ctx.args = (head + [tables[0].data_ptr(), tables[1].data_ptr(),
                       flow.data_ptr(), F, h, w, mask, int(polarity)])
        _lib.check(getattr(lib, 'dvsof_avg_timestamp_fwd' + ctx.form)(
            *ctx.args, term.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()), 'dvsof_avg_timestamp_fwd' + ctx.form)
        ctx.held = (cols, pol, tables, flow, ws, nbytes)
        ctx.weight = float(weight)
        ctx.mark_non_differentiable(term)
        ctx.set_materialize_grads(False)
        return term * ctx.weight, term

    @staticmethod
    def backward(ctx, g_value, _g_term):
        if g_value is None:
            return (None,) * 11
        flow, ws, nbytes = ctx.held[3:]
        grad = torch.empty_like(flow)
        seed = g_value.contiguous().float()
        _lib.check(getattr(_lib.lib(), 'dvsof_avg_timestamp_bwd' + ctx.form)(
            *ctx.args, ws.data_ptr(), nbytes, seed.data_ptr(), ctx.weight, grad.data_ptr(), _lib.stream()),
            'dvsof_avg_timestamp_bwd' + ctx.form)
        return (grad,) + (None,) * 10


# The term on every flow scale (csrc/avg_timestamp.hip, AVG_TIMESTAMP_SPEC sections 11-15)
AVG_TIMESTAMP_SCALES = ('finest', 'all')


def avg_timestamp_pyramid_layout(F, M, level_shapes):
    """The byte offsets of include/dvsof_avg_timestamp_pyramid.h for levels of
    the shapes ``level_shapes`` -> dict: q, s, base, sums, count,
    zeroed_bytes, rec, unit, rows, part, bytes, nb (the largest level's),
    pixels (sum_k h_k w_k)."""
    from . import eval as ev
    K = len(level_shapes)
    pixels = sum(int(h) * int(w) for h, w in level_shapes)
    P, S = M * pixels, 2 * F * pixels
    nb = max(ev.partial_blocks(int(h) * int(w)) for h, w in level_shapes)
    o = dict(q=0, s=8 * P, base=16 * P, sums=24 * P, count=24 * P + 8 * S, nb=nb, pixels=pixels)
    o['zeroed_bytes'] = o['count'] + 4 * P
    o['rec'] = (o['zeroed_bytes'] + 7) // 8 * 8
    o['unit'] = o['rec'] + 64 * K * M
    o['rows'] = o['unit'] + 8 * K * F
    o['part'] = o['rows'] + 32 * K * M
    o['bytes'] = o['part'] + 32 * M * nb
    return o


def avg_timestamp_pyramid_fwd_host(x, y, t, p, sample_index, frame_ts, frame_sample, flows, shape, weights=None,
                                   references=('start', 'end'), polarity=False):
    """AVG_TIMESTAMP_SPEC sections 11-13 on the host: what
    ``dvsof_avg_timestamp_pyramid_fwd`` is pinned to, byte for byte.  The
    arguments of ``contrast_pyramid_fwd_host``.  Per level
    ``avg_timestamp_fwd_host`` on the quantised columns, then the combination
    -> dict: levels (the K dicts of that function), shifts, weights float32
    [K], terms float32 [K] (unweighted), terms64, value float32."""
    K = len(flows)
    if not 1 <= K <= CONTRAST_MAX_LEVELS:
        raise ValueError(f'{K} levels: the level table holds 1 to {CONTRAST_MAX_LEVELS}')
    flows = [np.asarray(f, _F32) for f in flows]
    shifts = [contrast_level_shift(shape, f.shape[-2:]) for f in flows]
    weights = np.asarray(contrast_level_weights(1.0, K) if weights is None else weights, _F32)
    assert weights.shape == (K,)
    levels = []
    for flow, s in zip(flows, shifts):
        xs, ys = contrast_level_columns(x, y, shape, s)
        levels.append(avg_timestamp_fwd_host(xs, ys, t, p, sample_index, frame_ts, frame_sample, flow,
                                             references, polarity))
    terms64 = np.zeros(K, np.float64)
    total = np.float64(0)
    with np.errstate(all='ignore'):
        for k, lev in enumerate(levels):        # in level order
            s = np.float64(0)
            for v in lev['image_value']:        # in image order
                s = s + v
            terms64[k] = s / np.float64(len(lev['image_value']))
            total = total + np.float64(weights[k]) * terms64[k]
        return dict(levels=levels, shifts=shifts, weights=weights, terms=terms64.astype(_F32), terms64=terms64,
                    value=_F32(total), shape=tuple(int(v) for v in shape))


def avg_timestamp_pyramid_bwd_host(x, y, t, p, sample_index, frame_ts, frame_sample, flows, fwd, seed=1.0):
    """AVG_TIMESTAMP_SPEC section 14 on the host: what
    ``dvsof_avg_timestamp_pyramid_bwd`` is pinned to.  fwd: the dict of
    ``avg_timestamp_pyramid_fwd_host`` for the same input.  -> one
    (grad_flow_k float32 [F,2,h_k,w_k] = seed * weight_k * d term_k / d flow_k,
    sums int64 [F,2,h_k,w_k]) per level."""
    out = []
    for flow, s, lev, weight in zip(flows, fwd['shifts'], fwd['levels'], fwd['weights']):
        xs, ys = contrast_level_columns(x, y, fwd['shape'], s)
        out.append(avg_timestamp_bwd_host(xs, ys, t, p, sample_index, frame_ts, frame_sample, flow, lev,
                                          seed=seed, weight=weight))
    return out


class _AvgTimestampPyramid(torch.autograd.Function):
    """(sum_k weight_k term_k, terms [K]) of all flows; the gradient of the
    first enters every flow (dvsof_avg_timestamp_pyramid_fwd /
    dvsof_avg_timestamp_pyramid_bwd: one splat and one backward for all
    levels).  The images live in the workspace; the weights are applied inside
    the kernels."""

    @staticmethod
    def forward(ctx, x, y, t, p, sample_index, frame_ts, frame_sample, shape, weights, mask, polarity, *flows):
        dev = flows[0].device
        flows = tuple(f.detach().contiguous().float() for f in flows)
        K, F = len(flows), flows[0].shape[0]
        assert all(f.shape[0] == F and f.shape[1] == 2 for f in flows)
        lib = _lib.lib()
        M = F * bin(mask).count('1') * (2 if polarity else 1)
        shapes = [tuple(f.shape[-2:]) for f in flows]
        table = contrast_level_table(shape, shapes, F, M, weights, [f.data_ptr() for f in flows])
        terms = torch.zeros(K, dtype=torch.float32, device=dev) if F == 0 else \
            torch.empty(K, dtype=torch.float32, device=dev)
        value = torch.zeros((), dtype=torch.float32, device=dev) if F == 0 else \
            torch.empty((), dtype=torch.float32, device=dev)
        h, w = (int(v) for v in shape)
        nbytes = lib.dvsof_avg_timestamp_pyramid_workspace_bytes(F, mask, int(polarity), h, w, table)
        ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.long, device=dev)
        tables = (frame_ts.contiguous().float(), frame_sample.contiguous().long())
        assert tables[0].numel() == 2 * F and tables[1].numel() == F, (flows[0].shape, frame_ts.shape)
        ctx.form, head, (cols, pol) = _bind_columns(x, y, t, p, sample_index, polarity)
        ctx.args = (head + [tables[0].data_ptr(), tables[1].data_ptr(),
                       F, h, w, mask, int(polarity)])
        _lib.check(getattr(lib, 'dvsof_avg_timestamp_pyramid_fwd' + ctx.form)(
            *ctx.args, table, terms.data_ptr(), value.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()),
            'dvsof_avg_timestamp_pyramid_fwd' + ctx.form)
        ctx.held = (cols, pol, tables, flows, ws, nbytes, table)
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return value, terms

    @staticmethod
    def backward(ctx, g_value, _g_terms):
        flows, ws, nbytes, table = ctx.held[3:]
        if g_value is None:
            return (None,) * (11 + len(flows))
        grads = tuple(torch.empty_like(f) for f in flows)
        for k, g in enumerate(grads):
            table.level[k].grad_flow = g.data_ptr()
        seed = g_value.contiguous().float()
        _lib.check(getattr(_lib.lib(), 'dvsof_avg_timestamp_pyramid_bwd' + ctx.form)(
            *ctx.args, table, ws.data_ptr(), nbytes, seed.data_ptr(), _lib.stream()),
            'dvsof_avg_timestamp_pyramid_bwd' + ctx.form)
        return (None,) * 11 + grads


class Loss:
    """Single-scale evaluator (reference utils/loss.py:38-171)."""

    def __init__(self, pred_shape, batch_size, device, timers=FakeTimer()):
        self.N = batch_size
        self.H, self.W = pred_shape
        self.device = torch.device(device)
        self.timers = timers

    def _check(self, prev_images, next_images, flow):
        N, C, H, W = prev_images.size()
        assert self.N >= N, 'This object should be used for batch of ' \
            f'at most {self.N} samples, but {N} samples are given'
        assert self.H == H, 'This object should be used for images of ' \
            f'height {self.H}, but image of height {H} are given'
        assert self.W == W, 'This object should be used for images of ' \
            f'width {self.W}, but image of width {W} are given'
        assert tuple(next_images.size()) == (N, C, H, W)
        assert C == 1, 'frames are single-channel'
        FN, FC, FH, FW = flow.size()
        assert FN == N, f'Number of images and flows should be the same ' \
            f'{N} vs {FN}'
        assert FC == 2, 'Flow should contain 2 channels (dx and dy)'
        assert FH == H and FW == W, 'images and flows should have the ' \
            f'same size {(H, W)} vs {(FH, FW)}'

    def __call__(self, prev_images, next_images, flow):
        self._check(prev_images, next_images, flow)
        _lib.require_cuda(prev_images, next_images, flow)
        N = flow.shape[0]
        frames = torch.cat([prev_images.reshape(N, self.H, self.W),
                            next_images.reshape(N, self.H, self.W)]) \
            .contiguous().float()
        start = torch.arange(N, dtype=torch.int32, device=flow.device)
        terms = _LossTerms.apply((frames,), start, start + N, flow)
        return terms[0, 0], terms[1, 0], terms[2, 0]


class Losses:
    """Multi-scale evaluator (reference utils/loss.py:174-214)."""

    def __init__(self, shapes, batch_size, device, timers=FakeTimer()):
        self.shapes = [tuple(int(v) for v in s) for s in shapes]
        self.N = batch_size
        self.device = torch.device(device)
        self.timers = timers
        self.losses = [Loss(s, batch_size, device, timers)
                       for s in self.shapes]

    def _check_flows(self, flows):
        assert len(flows) == len(self.shapes)
        for flow, shape in zip(flows, self.shapes):
            assert tuple(flow.shape[-2:]) == shape, \
                f'flow of size {tuple(flow.shape[-2:])} given to the ' \
                f'evaluator of scale {shape}'
            assert flow.shape[1] == 2, \
                'Flow should contain 2 channels (dx and dy)'
            assert flow.shape[0] <= self.N, 'This object should be used ' \
                f'for batch of at most {self.N} samples'

    def _level_buffers(self, images):
        img = images.detach().contiguous().float()
        img = img.reshape(img.shape[0], img.shape[-2], img.shape[-1])
        frames = tuple(torch.empty(img.shape[0], h, w, dtype=torch.float32,
                                   device=img.device) for h, w in self.shapes)
        return img, frames

    def _pyramid(self, flows, images):
        """CASCADE: level k resamples level k-1 (utils/loss.py:207-210), all
        levels by one call (dvsof_loss_pyramid)."""
        self._check_flows(flows)
        img, frames = self._level_buffers(images)
        K = len(frames)
        ptrs = (ctypes.c_void_p * K)(*[f.data_ptr() for f in frames])
        hs = (ctypes.c_int * K)(*[s[0] for s in self.shapes])
        ws = (ctypes.c_int * K)(*[s[1] for s in self.shapes])
        D, H, W = img.shape
        _lib.check(_lib.lib().dvsof_loss_pyramid(
            img.data_ptr(), D, H, W, ptrs, hs, ws, K, _lib.stream()),
            'dvsof_loss_pyramid')
        return frames

    def _prepare(self, flows, flow_ts, flow_sample_idx, images, timestamps,
                 sample_idx, frame_indices):
        _lib.require_cuda(images, *flows)
        if frame_indices is None:
            frame_indices = resolve_frames(flow_ts, flow_sample_idx,
                                           timestamps, sample_idx)
        start, stop = frame_indices
        assert start.numel() == flows[0].shape[0]
        return self._pyramid(flows, images), start, stop

    def __call__(self, flows, flow_ts, flow_sample_idx, images, timestamps,
                 sample_idx, frame_indices=None):
        frames, start, stop = self._prepare(flows, flow_ts, flow_sample_idx,
                                            images, timestamps, sample_idx,
                                            frame_indices)
        terms = _LossTerms.apply(frames, start, stop, *flows)
        return tuple(tuple(row.unbind(0)) for row in terms.unbind(0))

    def fused(self, flows, flow_ts, flow_sample_idx, images, timestamps,
              sample_idx, weights=(0.5, 1, 1), loss_scale=1.0,
              frame_indices=None):
        """-> (loss, terms[3,K]); same value as combined_loss
        (reference utils/training.py:12-24) times loss_scale.  Pyramid,
        out-of-border count, terms and flow gradients: 4 launches."""
        _lib.require_cuda(images, *flows)
        if frame_indices is None:
            frame_indices = resolve_frames(flow_ts, flow_sample_idx,
                                           timestamps, sample_idx)
        start, stop = frame_indices
        assert start.numel() == flows[0].shape[0]
        self._check_flows(flows)
        img, frames = self._level_buffers(images)
        return _FusedLoss.apply(frames, img, start, stop, tuple(weights),
                                loss_scale, *flows)

    def frameless(self, flows, weights=(0.5, 1), loss_scale=1.0):
        """The loss of a batch that has no frames (docs/FRAMELESS_SPEC.md):
        weights = (smoothness, out-of-border) -> (loss, terms[3,K]) with
        loss = (w_s sum_k smooth_k + w_o sum_k border_k) / K * loss_scale; the
        photometric row of the terms is 0.  Out-of-border count, terms and flow
        gradients: 3 launches, no pyramid, no frame read."""
        _lib.require_cuda(*flows)
        self._check_flows(flows)
        weights = tuple(weights)
        assert len(weights) == 2, 'weights = (smoothness, out-of-border)'
        return _FramelessLoss.apply(weights, loss_scale, *flows)

    def contrast(self, flows, flow_ts, flow_sample_idx, events, weight=None,
                 references=('start',), polarity=False, scales='finest'):
        """The contrast-maximisation term of the finest flow ``flows[-1]``
        (docs/CONTRAST_SPEC.md): the mean over the predictions of
        1 - var(image of warped events) / var(count image), negative where the
        flow sharpens the events of its own window.  events: the wire columns
        on the device, or the compact ones (voxel.is_compact), which go to the
        encoded entry points as they are and give the same bytes
        (``wire_event_columns``).  -> the 0-dim term, differentiable with respect to
        ``flows[-1]``; with a ``weight`` -> (weight * term, term), the first
        differentiable (the weight is applied inside the backward kernel), the
        second detached for logging.  Nothing waits for the device.

        references: names among 'start', 'middle', 'end', the times of the
        window the events are warped to, one image each; polarity: ON and OFF
        events in images of their own (``events['polarity']``; an event of
        polarity 0 takes no part).  The term is the mean over all images
        (CONTRAST_SPEC sections 11-15).  The defaults are the term as it was:
        the same kernels, through the general entry point.

        scales='all': the term of every flow on the events quantised to that
        flow's grid (CONTRAST_SPEC sections 19-23), one splat and one backward
        for all levels; each level weighs float32(weight) / float32(K), the
        mean over the scales.  -> the 0-dim weighted sum, differentiable with
        respect to every flow (without a ``weight``: the mean of the levels'
        terms); with a ``weight`` -> (that, terms [K]), the levels' unweighted
        terms detached for logging.  'finest', the default, is the call above
        and constructs nothing else."""
        if scales != 'finest':
            if scales not in CONTRAST_SCALES:
                raise ValueError(f'unknown contrast scales "{scales}": one of {", ".join(CONTRAST_SCALES)}')
            return self._contrast_all(flows, flow_ts, flow_sample_idx, events, weight, references, polarity)
        flow = flows[-1]
        assert tuple(flow.shape[-2:]) == self.shapes[-1] and flow.shape[1] == 2, \
            f'flow of size {tuple(flow.shape)} given to the contrast term of scale {self.shapes[-1]}'
        *cols, pol, sample = _term_columns(events, polarity)
        cols.append(sample)
        _lib.require_cuda(flow, flow_ts, flow_sample_idx, *cols)
        mask = contrast_reference_mask(references)
        weight_ = 1.0 if weight is None else float(weight)
        _lib.require_cuda(pol)
        value, term = _Contrast.apply(flow, *cols[:3], pol, cols[3], flow_ts, flow_sample_idx, weight_, mask,
                                      bool(polarity))
        return value if weight is None else (value, term)

    def avg_timestamp(self, flows, flow_ts, flow_sample_idx, events, weight=None,
                      references=('start', 'end'), polarity=False):
        """The average-timestamp term of the finest flow ``flows[-1]``
        (docs/AVG_TIMESTAMP_SPEC.md): per image the mean over the pixels that
        hold events of the squared average distance in time between the events
        warped onto a pixel and the reference time, over the same at zero
        flow; the mean over all images.  1 at zero flow, below 1 where the flow
        brings events of the same edge together.  The arguments and what is
        returned are those of ``contrast``: the 0-dim term, differentiable with
        respect to ``flows[-1]``; with a ``weight`` -> (weight * term, term),
        the second detached for logging.  Nothing waits for the device.

        references: names among 'start', 'middle', 'end'; the default warps
        to both ends of the window (Zhu et al., CVPR 2019): at one end alone
        the events that need no warp carry no distance.  polarity: ON and OFF
        events in images of their own.  The term on every flow scale is
        ``avg_timestamp_scales``."""
        flow = flows[-1]
        assert tuple(flow.shape[-2:]) == self.shapes[-1] and flow.shape[1] == 2, \
            f'flow of size {tuple(flow.shape)} given to the average-timestamp term of scale {self.shapes[-1]}'
        *cols, pol, sample = _term_columns(events, polarity)
        cols.append(sample)
        _lib.require_cuda(flow, flow_ts, flow_sample_idx, *cols)
        mask = contrast_reference_mask(references)
        weight_ = 1.0 if weight is None else float(weight)
        _lib.require_cuda(pol)
        value, term = _AvgTimestamp.apply(flow, *cols[:3], pol, cols[3], flow_ts, flow_sample_idx, weight_, mask,
                                          bool(polarity))
        return value if weight is None else (value, term)

    def avg_timestamp_scales(self, flows, flow_ts, flow_sample_idx, events, weight=None,
                             references=('start', 'end'), polarity=False, scales='finest'):
        """``avg_timestamp`` with the choice of the flow scales (a method of
        its own: the signature of ``avg_timestamp`` is held as it is).
        scales='all': the term of every flow on the events quantised to that
        flow's grid (AVG_TIMESTAMP_SPEC sections 11-15), one splat and one
        backward for all levels; each level weighs float32(weight) /
        float32(K), the mean over the scales.  -> the 0-dim weighted sum,
        differentiable with respect to every flow (without a ``weight``: the
        mean of the levels' terms); with a ``weight`` -> (that, terms [K]),
        the levels' unweighted terms detached for logging.  A level that is no
        halving of the finest is refused (``contrast_level_shift``).
        'finest', the default, is ``avg_timestamp`` and constructs nothing
        else; any other name raises ValueError."""
        if scales == 'finest':
            return self.avg_timestamp(flows, flow_ts, flow_sample_idx, events, weight, references, polarity)
        if scales not in AVG_TIMESTAMP_SCALES:
            raise ValueError(f'unknown avg-timestamp scales "{scales}": one of {", ".join(AVG_TIMESTAMP_SCALES)}')
        return self._event_term_all(_AvgTimestampPyramid, flows, flow_ts, flow_sample_idx, events, weight,
                                    references, polarity)

    def _contrast_all(self, flows, flow_ts, flow_sample_idx, events, weight, references, polarity):
        return self._event_term_all(_ContrastPyramid, flows, flow_ts, flow_sample_idx, events, weight,
                                    references, polarity)

    def _event_term_all(self, function, flows, flow_ts, flow_sample_idx, events, weight, references, polarity):
        self._check_flows(flows)
        *cols, pol, sample = _term_columns(events, polarity)
        cols.append(sample)
        _lib.require_cuda(flow_ts, flow_sample_idx, *flows, *cols)
        mask = contrast_reference_mask(references)
        for shape in self.shapes:                       # a level that is no halving is refused here
            contrast_level_shift(self.shapes[-1], shape)
        weights = contrast_level_weights(1.0 if weight is None else weight, len(flows))
        _lib.require_cuda(pol)
        value, terms = function.apply(*cols[:3], pol, cols[3], flow_ts, flow_sample_idx,
                                      self.shapes[-1], weights, mask, bool(polarity), *flows)
        return value if weight is None else (value, terms)


def init_losses(shape, batch_size, model, device, sequence_length,
                timers=FakeTimer()):
    """Shape discovery by calling the model with ZERO events
    (reference utils/loss.py:217-240)."""
    def empty(dtype):
        return torch.tensor([], dtype=dtype, device=device)
    events = {'x': empty(torch.long), 'y': empty(torch.long),
              'timestamp': empty(torch.float32),
              'polarity': empty(torch.long),
              'element_index': empty(torch.long),
              'sample_index': empty(torch.long)}
    with torch.no_grad():
        num_timestamps = sequence_length + 1
        out = model(events,
                    torch.tensor([0.04 * i for i in range(num_timestamps)],
                                 dtype=torch.float32, device=device),
                    torch.tensor([0] * num_timestamps, dtype=torch.long,
                                 device=device),
                    shape, raw=True)
    out_shapes = tuple(tuple(flow.shape[2:]) for flow in out[0])
    return Losses(out_shapes, batch_size, device, timers=timers)
