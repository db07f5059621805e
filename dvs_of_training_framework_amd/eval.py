"""Evaluation against ground-truth flow on the device (HIP, csrc/eval.hip;
arithmetic in docs/EVAL_SPEC.md).

``flow_error_dense`` and ``estimate_corresponding_gt_flow`` keep the
reference's names and arguments (utils/eval.py:6-50, 84-184): numpy in, numpy
out, the work done by the kernels.  The batched device functions underneath
(``propagate``, ``flow_error``, ``count_image_batched``) are what
``testing.evaluate`` drives; ``plan_gt_steps`` is the host-side part of the
propagation (which maps, which scale factors) and needs no GPU.

Without ground truth: ``iwe_splat``, ``iwe_stats``, ``iwe_render`` and
``derive_fwl`` (csrc/iwe.hip, docs/IWE_SPEC.md), the image of warped events
and its flow warp loss, driven by ``testing.flow_warp_loss``; for host arrays
they run the numpy float32 restatement ``iwe_*_host`` the kernels are pinned to.
Beside it ``iwe_avg_timestamp``, ``iwe_avg_timestamp_render`` and
``derive_rsat`` (IWE_SPEC sections 14-21): the average-timestamp images of the
same events and the ratio of squared average timestamps, from one splat that
serves both metrics; ``testing.event_alignment`` drives them.
"""
import numpy as np
import torch

from . import _lib
from ._abi import dtype_of

F32, F64 = _lib.CONSTANTS['DVSOF_EVAL_F32'], _lib.CONSTANTS['DVSOF_EVAL_F64']
DIRECT, PROPAGATE = 1, 0
CAR_ROWS = 190          # utils/eval.py:18-19: the hood of the car is below

RESULT_DTYPE = dtype_of('dvsof_eval_result_t')   # sum_ee, n_points, n_below, pred_max, pred_min
assert RESULT_DTYPE.itemsize == 32


def check_in_frame(x, y, shape):
    # np.ravel_multi_index of the reference's get_count_image raises for these
    if x.size and (x.min() < 0 or x.max() >= shape[1] or
                   y.min() < 0 or y.max() >= shape[0]):
        raise ValueError('invalid entry in coordinates array')


def plan_gt_steps(gt_timestamps, start, stop):
    """Which ground-truth maps the interval [start, stop] walks through and
    by how much of each (utils/eval.py:118-172, literally: searchsorted
    'right' - 1, the strict ``<`` of the loop, float64 scale factors).

    -> (mode, maps, scales).  PROPAGATE: one entry per ``prop_flow`` call.
    DIRECT (the interval is shorter than the ground-truth gap it starts in):
    maps = [k, k], scales = [dt, gt_dt]."""
    ts = np.asarray(gt_timestamps)
    k = int(np.searchsorted(ts, start, side='right')) - 1
    if k < 0:
        raise ValueError('the interval starts before the first ground-truth '
                         'timestamp')
    gap = ts[k + 1] - ts[k]
    span = stop - start
    if gap > span:
        return DIRECT, [k, k], [float(span), float(gap)]
    # the rest of the gap the interval starts in, whole gaps, a last share
    maps, scales = [k], [float((ts[k + 1] - start) / gap)]
    k += 1
    while ts[k + 1] < stop:
        maps.append(k)
        scales.append(1.0)
        k += 1
    maps.append(k)
    scales.append(float((stop - ts[k]) / (ts[k + 1] - ts[k])))
    return PROPAGATE, maps, scales


def step_table(plans, map_offset=0):
    """Plans of F frames -> the kernel's table: frame_step_begin int32[F+1],
    step_map int32[S] (minus ``map_offset``, the first map that is on the
    device), step_scale float64[S], frame_mode int32[F]."""
    begin = np.zeros(len(plans) + 1, np.int32)
    begin[1:] = np.cumsum([len(p[1]) for p in plans])
    maps = np.array([m - map_offset for p in plans for m in p[1]], np.int32)
    scales = np.array([s for p in plans for s in p[2]], np.float64)
    mode = np.array([p[0] for p in plans], np.int32)
    return begin, maps, scales, mode


def map_dtype(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise TypeError(f'ground-truth maps are float32 or float64, not {t.dtype}')


class StepTable:
    """The step table of a batch on the device, sent in ONE copy: the int32
    parts ride in front of the float64 scales in one byte buffer.  ``begin``,
    ``maps``, ``scales``, ``mode`` are the device addresses the C ABI takes;
    F frames, S table entries."""

    def __init__(self, plans, map_offset, device):
        begin, maps, scales, mode = step_table(plans, map_offset)
        self.F, self.S = len(plans), len(maps)
        ints = np.concatenate([begin, mode, maps])
        pad = (-ints.nbytes) % 8
        raw = ints.tobytes() + b'\0' * pad + scales.tobytes()
        self.buffer = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        base = self.buffer.data_ptr()
        self.begin = base
        self.mode = base + 4 * (self.F + 1)
        self.maps = base + 4 * (2 * self.F + 1)
        self.scales = base + ints.nbytes + pad


def propagate(x_flow, y_flow, plans, window=None, map_offset=0):
    """x_flow, y_flow: device tensors [K,H,W] (float32 or float64), map
    ``map_offset + k`` of the sequence at index k; plans: one
    ``plan_gt_steps`` result per frame; window: (y0, x0, h, w) on the full
    frame, default the full frame.  -> u, v float32 [F,h,w] on the device."""
    _lib.require_cuda(x_flow, y_flow)
    x_flow, y_flow = x_flow.contiguous(), y_flow.contiguous()
    assert x_flow.dim() == 3 and x_flow.shape == y_flow.shape \
        and x_flow.dtype == y_flow.dtype
    K, H, W = x_flow.shape
    y0, x0, h, w = (0, 0, H, W) if window is None else map(int, window)
    dev = x_flow.device
    table = StepTable(plans, map_offset, dev)
    u = torch.empty(table.F, max(h, 0), max(w, 0), dtype=torch.float32, device=dev)
    v = torch.empty_like(u)
    rc = _lib.lib().dvsof_gt_flow_propagate(
        x_flow.data_ptr(), y_flow.data_ptr(), map_dtype(x_flow), K, H, W,
        table.begin, table.maps, table.scales, table.mode, table.F, table.S,
        y0, x0, h, w, u.data_ptr(), v.data_ptr(), _lib.stream())
    _lib.check(rc, 'dvsof_gt_flow_propagate')
    return u, v


def flow_error(gt_u, gt_v, pred, count=None, max_row=None):
    """gt_u, gt_v float32 [F,h,w]; pred float32 [F,2,h,w]; count uint32/int32
    [F,h,w] or None (dense); max_row default h.  -> device uint8 [F,32], one
    dvsof_eval_result_t per frame (``read_results`` copies it to the host)."""
    _lib.require_cuda(gt_u, gt_v, pred, count)
    gt_u, gt_v, pred = gt_u.contiguous(), gt_v.contiguous(), pred.contiguous()
    for t in (gt_u, gt_v, pred):
        assert t.dtype == torch.float32
    F, h, w = gt_u.shape
    assert gt_v.shape == gt_u.shape and tuple(pred.shape) == (F, 2, h, w), \
        (gt_u.shape, gt_v.shape, pred.shape)
    if count is not None:
        count = count.contiguous()
        assert tuple(count.shape) == (F, h, w) and count.element_size() == 4
    max_row = h if max_row is None else int(max_row)
    lib = _lib.lib()
    out = torch.empty(F, RESULT_DTYPE.itemsize, dtype=torch.uint8,
                      device=gt_u.device)
    nbytes = lib.dvsof_flow_error_workspace_bytes(F, h, w)
    ws = torch.empty(max(nbytes, 32), dtype=torch.uint8, device=gt_u.device)
    _lib.check(lib.dvsof_flow_error(
        gt_u.data_ptr(), gt_v.data_ptr(), pred.data_ptr(), _lib.ptr(count),
        F, h, w, max_row, out.data_ptr(), ws.data_ptr(), nbytes,
        _lib.stream()), 'dvsof_flow_error')
    return out


def read_results(results):
    """Device rows of ``flow_error`` -> numpy structured array [F]
    (RESULT_DTYPE): the one device-to-host copy of a batch."""
    return results.cpu().numpy().view(RESULT_DTYPE).reshape(-1)


def derive(res):
    """-> (AEE, percent_AEE) float64 arrays of per-frame results: AEE =
    sum_ee / n_points (NaN for an empty mask, the reference's mean of
    nothing), percent_AEE = n_below / (n_points + 1e-5)."""
    n = res['n_points'].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        aee = res['sum_ee'] / n
    return aee, res['n_below'].astype(np.float64) / (n + 1e-5)


def count_image_batched(x, y, frame_event_begin, shape, box=None):
    """x, y: int64 device columns of a batch of frames; frame_event_begin:
    int64[F+1] (device or host), the first event of every frame; box:
    (y0, x0, h, w) with EventCrop's semantics (utils/data.py:24-42), default
    (0, 0) + shape.  Events outside the box are dropped.
    -> int32 device tensor [F,h,w] holding the uint32 counts."""
    _lib.require_cuda(x, y)
    x, y = x.contiguous(), y.contiguous()
    assert x.dtype == torch.long and y.dtype == torch.long \
        and x.numel() == y.numel()
    begin = torch.as_tensor(frame_event_begin, dtype=torch.long) \
        .to(x.device).contiguous()
    F = begin.numel() - 1
    h, w = int(shape[0]), int(shape[1])
    y0, x0 = (0, 0) if box is None else (int(box[0]), int(box[1]))
    if box is not None:
        assert (int(box[2]), int(box[3])) == (h, w), (box, shape)
    out = torch.empty(max(F, 0), h, w, dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().dvsof_count_image_batched(
        x.data_ptr(), y.data_ptr(), x.numel(), begin.data_ptr(), F, y0, x0,
        h, w, out.data_ptr(), _lib.stream()), 'dvsof_count_image_batched')
    return out


def count_image_polarity_batched(x, y, p, frame_event_begin, shape, box=None):
    """``count_image_batched`` by polarity: p is the int64 wire polarity
    column.  -> int32 device tensor [F,2,h,w] holding the uint32 counts, plane
    0 the events with p > 0, plane 1 those with p <= 0; the planes add up to
    ``count_image_batched`` of the same columns."""
    _lib.require_cuda(x, y, p)
    x, y, p = x.contiguous(), y.contiguous(), p.contiguous()
    assert x.dtype == y.dtype == p.dtype == torch.long \
        and x.numel() == y.numel() == p.numel()
    begin = torch.as_tensor(frame_event_begin, dtype=torch.long) \
        .to(x.device).contiguous()
    F = begin.numel() - 1
    h, w = int(shape[0]), int(shape[1])
    y0, x0 = (0, 0) if box is None else (int(box[0]), int(box[1]))
    if box is not None:
        assert (int(box[2]), int(box[3])) == (h, w), (box, shape)
    out = torch.empty(max(F, 0), 2, h, w, dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().dvsof_count_image_polarity_batched(
        x.data_ptr(), y.data_ptr(), p.data_ptr(), x.numel(), begin.data_ptr(),
        F, y0, x0, h, w, out.data_ptr(), _lib.stream()),
        'dvsof_count_image_polarity_batched')
    return out


def _upload_maps(a, device):
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def flow_error_dense(flow_gt, flow_pred, event_img, is_car=False,
                     is_dense=False, device='cuda'):
    """utils/eval.py:6-50 on the device: flow_gt, flow_pred [h,w,2],
    event_img [h,w] event counts -> (AEE, percent_AEE, n_points)."""
    flow_gt, flow_pred = np.asarray(flow_gt), np.asarray(flow_pred)
    h, w = flow_gt.shape[:2]
    with np.errstate(over='ignore'):
        gt = torch.from_numpy(np.ascontiguousarray(
            np.moveaxis(flow_gt, 2, 0), dtype=np.float32)).to(device)
        pred = torch.from_numpy(np.ascontiguousarray(
            np.moveaxis(flow_pred, 2, 0), dtype=np.float32)).to(device)
    count = None
    if not is_dense:
        mask = np.squeeze(np.asarray(event_img)).reshape(h, w) > 0
        count = torch.from_numpy(mask.astype(np.int32)[None]).to(device)
    res = read_results(flow_error(gt[0:1], gt[1:2], pred[None], count,
                                  min(CAR_ROWS, h) if is_car else h))
    aee, percent = derive(res)
    return aee[0], float(percent[0]), int(res['n_points'][0])


def estimate_corresponding_gt_flow(x_flow_in, y_flow_in, gt_timestamps,
                                   start_time, end_time, device='cuda'):
    """utils/eval.py:84-184 on the device -> (x_shift, y_shift) numpy [H,W].
    Only the maps the interval touches are uploaded.  The values are the
    kernel's float32; on the direct-scale branch, where the reference returns
    the maps' own dtype, they are widened to it."""
    mode, maps, scales = plan = plan_gt_steps(gt_timestamps, start_time,
                                              end_time)
    lo, hi = min(maps), max(maps) + 1
    H, W = np.squeeze(x_flow_in[lo]).shape
    xd = _upload_maps(np.reshape(x_flow_in[lo:hi], (hi - lo, H, W)), device)
    yd = _upload_maps(np.reshape(y_flow_in[lo:hi], (hi - lo, H, W)), device)
    u, v = propagate(xd, yd, [plan], None, lo)
    u, v = u[0].cpu().numpy(), v[0].cpu().numpy()
    if mode == DIRECT:
        dt = np.result_type(np.asarray(x_flow_in[lo]).dtype, np.float64)
        return u.astype(dt), v.astype(dt)
    return u, v


# ---------------------------------------------------------------------------
# Image of warped events and flow warp loss (csrc/iwe.hip, docs/IWE_SPEC.md)
# ---------------------------------------------------------------------------
# sum_sq, sum_q, max_q, count_sum, count_sq, count_max
IWE_RESULT_DTYPE = dtype_of('dvsof_iwe_result_t')
assert IWE_RESULT_DTYPE.itemsize == 48
IWE_ONE = 1 << 32       # the fixed-point unit of q
_F = np.float32


def _on_device(t):
    return isinstance(t, torch.Tensor) and t.is_cuda


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _counts(count):
    """A count image as the kernels read it: the uint32 bits, as int64."""
    c = np.ascontiguousarray(_np(count))
    assert c.dtype.itemsize == 4, c.dtype
    return c.view(np.uint32).astype(np.int64)


def iwe_splat_host(x, y, t, frame_event_begin, frame_ts, flow):
    """IWE_SPEC section 2 in numpy float32: what ``iwe_splat`` runs without a
    GPU and what the kernel is pinned to, byte for byte.  x, y int64 [n], t
    float32 [n], frame_event_begin int64 [F+1], frame_ts float32 [2F], flow
    float32 [F,2,h,w] -> q int64 [F,h,w]."""
    x, y = np.asarray(x, np.int64).reshape(-1), np.asarray(y, np.int64).reshape(-1)
    t = np.asarray(t, _F).reshape(-1)
    begin = np.asarray(frame_event_begin, np.int64).reshape(-1)
    ts = np.asarray(frame_ts, _F).reshape(-1)
    flow = np.asarray(flow, _F)
    F, _, h, w = flow.shape
    assert begin.size == F + 1 and ts.size == 2 * F and x.size == y.size == t.size
    q = np.zeros((F, h, w), np.int64)
    if F == 0 or x.size == 0:
        return q
    e = np.arange(x.size, dtype=np.int64)
    keep = (e >= begin[0]) & (e < begin[F]) & (x >= 0) & (x < w) & (y >= 0) & (y < h)
    e = e[keep]
    f = np.searchsorted(begin[:F], e, side='right') - 1     # the last f with begin[f] <= e
    x, y, t = x[keep], y[keep], t[keep]
    t0 = ts[2 * f]
    d = ts[2 * f + 1] - t0
    with np.errstate(all='ignore'):
        tau = np.where(d > 0, np.fmin(np.fmax((t - t0) / d, _F(0)), _F(1)), _F(0)).astype(_F)
        u, v = flow[f, 0, y, x], flow[f, 1, y, x]
        xw = x.astype(_F) - tau * u
        yw = y.astype(_F) - tau * v
        inside = (xw > _F(-1)) & (xw < _F(w)) & (yw > _F(-1)) & (yw < _F(h))
    f, xw, yw = f[inside], xw[inside], yw[inside]
    flx, fly = np.floor(xw), np.floor(yw)
    fx, fy = xw - flx, yw - fly
    cx, cy = flx.astype(np.int64), fly.astype(np.int64)
    for j, wy in enumerate((_F(1) - fy, fy)):
        for i, wx in enumerate((_F(1) - fx, fx)):
            xx, yy = cx + i, cy + j
            Q = ((wy * wx).astype(_F) * _F(IWE_ONE)).astype(np.int64)    # truncates
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h) & (Q > 0)
            np.add.at(q, (f[ok], yy[ok], xx[ok]), Q[ok])
    return q


IWE_REFERENCES = (('start', 0.0), ('middle', 0.5), ('end', 1.0))    # in the order of the mask's bits
IWE_CHANNELS = ('ON', 'OFF')


def iwe_image_names(mask, polarity):
    """[(reference name, channel name or None)] of the R C images of a frame, in image order."""
    refs = [name for b, (name, _) in enumerate(IWE_REFERENCES) if mask >> b & 1]
    return [(r, c) for r in refs for c in (IWE_CHANNELS if polarity else (None,))]


def iwe_splat_multi_host(x, y, t, p, frame_event_begin, frame_ts, flow, references=('start',), polarity=False):
    """IWE_SPEC sections 8-9 in numpy float32: what ``iwe_splat_multi`` runs
    without a GPU and what ``dvsof_iwe_splat_multi`` is pinned to, byte for
    byte.  The arguments of ``iwe_splat_host`` and the column p int64 [n]
    (not read without ``polarity``; may be None); references: names or a mask.
    With M = F R C images, m = (f R + r) C + c -> (q int64 [M,h,w], count
    uint32 [M,h,w])."""
    from .loss import contrast_reference_mask
    mask = contrast_reference_mask(references)
    rhos = [_F(rho) for b, (_, rho) in enumerate(IWE_REFERENCES) if mask >> b & 1]
    R, C = len(rhos), 2 if polarity else 1
    x, y = np.asarray(x, np.int64).reshape(-1), np.asarray(y, np.int64).reshape(-1)
    t = np.asarray(t, _F).reshape(-1)
    begin = np.asarray(frame_event_begin, np.int64).reshape(-1)
    ts = np.asarray(frame_ts, _F).reshape(-1)
    flow = np.asarray(flow, _F)
    F, _, h, w = flow.shape
    assert begin.size == F + 1 and ts.size == 2 * F and x.size == y.size == t.size
    q = np.zeros((F * R * C, h, w), np.int64)
    count = np.zeros((F * R * C, h, w), np.uint32)
    if F == 0 or x.size == 0:
        return q, count
    e = np.arange(x.size, dtype=np.int64)
    keep = (e >= begin[0]) & (e < begin[F]) & (x >= 0) & (x < w) & (y >= 0) & (y < h)
    chan = np.zeros(x.size, np.int64)
    if polarity:
        p = np.asarray(p, np.int64).reshape(-1)
        assert p.size == x.size
        keep &= p != 0
        chan = (p < 0).astype(np.int64)
    e = e[keep]
    f = np.searchsorted(begin[:F], e, side='right') - 1     # the last f with begin[f] <= e
    x, y, t, chan = x[keep], y[keep], t[keep], chan[keep]
    t0 = ts[2 * f]
    d = ts[2 * f + 1] - t0
    with np.errstate(all='ignore'):
        tau = np.where(d > 0, np.fmin(np.fmax((t - t0) / d, _F(0)), _F(1)), _F(0)).astype(_F)
    u, v = flow[f, 0, y, x], flow[f, 1, y, x]
    for r, rho in enumerate(rhos):
        m = (f * R + r) * C + chan
        np.add.at(count, (m, y, x), 1)
        with np.errstate(all='ignore'):
            sig = (tau - rho).astype(_F)
            xw = x.astype(_F) - sig * u
            yw = y.astype(_F) - sig * v
            inside = (xw > _F(-1)) & (xw < _F(w)) & (yw > _F(-1)) & (yw < _F(h))
        mi, xi, yi = m[inside], xw[inside], yw[inside]
        flx, fly = np.floor(xi), np.floor(yi)
        fx, fy = xi - flx, yi - fly
        cx, cy = flx.astype(np.int64), fly.astype(np.int64)
        for j, wy in enumerate((_F(1) - fy, fy)):
            for i, wx in enumerate((_F(1) - fx, fx)):
                xx, yy = cx + i, cy + j
                Q = ((wy * wx).astype(_F) * _F(IWE_ONE)).astype(np.int64)    # truncates
                ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h) & (Q > 0)
                np.add.at(q, (mi[ok], yy[ok], xx[ok]), Q[ok])
    return q, count


def iwe_stats_host(q, count):
    """IWE_SPEC section 3 on the host -> structured array [F]
    (IWE_RESULT_DTYPE).  The integer fields are exact; sum_sq is a float64 sum
    of the kernel's terms in numpy's order, not the kernel's."""
    q = np.asarray(_np(q), np.int64)
    c = _counts(count)
    F = q.shape[0]
    assert q.ndim == 3 and c.shape == q.shape, (q.shape, c.shape)
    res = np.zeros(F, IWE_RESULT_DTYPE)
    qf, cf = q.reshape(F, -1), c.reshape(F, -1)
    image = qf.astype(np.float64) * 2.0 ** -32
    res['sum_sq'] = (image * image).sum(1)
    res['sum_q'], res['max_q'] = qf.sum(1), qf.max(1, initial=0)
    res['count_sum'], res['count_sq'] = cf.sum(1), (cf * cf).sum(1)
    res['count_max'] = cf.max(1, initial=0)
    return res


def _wave_tree(a):
    """Lane 0 of the kernels' shuffle tree over the last axis (64 lanes)."""
    a = a.copy()
    off = 32
    while off:
        a[..., :off] = a[..., :off] + a[..., off:2 * off]
        off >>= 1
    return a[..., 0]


def partial_blocks(n):
    """Partials per frame of n pixels: partial_blocks of csrc/frame_common.h."""
    return min(max((n + 1023) // 1024, 1), 128)


def kernel_order_sum(terms, nb):
    """The per-frame float64 sum of csrc/frame_common.h with the kernels' own
    order of additions (thread: strided pixels ascending; wave: shuffle tree;
    block: waves 0..3; frame: partials ascending per lane, shuffle tree): the
    bits ``dvsof_flow_error`` and ``dvsof_iwe_stats`` store.  terms float64
    [F,n], a pixel that adds nothing as +0; nb partials -> float64 [F]."""
    terms = np.asarray(terms, np.float64)
    F, n = terms.shape
    assert 1 <= nb <= 128
    per = nb * 256
    rounds = (n + per - 1) // per
    padded = np.zeros((F, rounds * per))
    padded[:, :n] = terms
    padded = padded.reshape(F, rounds, nb, 256)
    thread = np.zeros((F, nb, 256))
    for k in range(rounds):
        thread = thread + padded[:, k]
    waves = _wave_tree(thread.reshape(F, nb, 4, 64))
    part = waves[..., 0]
    for k in range(1, 4):
        part = part + waves[..., k]
    lanes = np.zeros((F, 128))
    lanes[:, :nb] = part
    return _wave_tree(lanes[:, :64] + lanes[:, 64:])


def iwe_sum_sq_kernel_order(q):
    """``sum_sq`` of IWE_SPEC section 3 in the kernels' order
    (``kernel_order_sum``): the bits ``dvsof_iwe_stats`` stores.
    q int64 [F,h,w] -> float64 [F]."""
    q = np.asarray(_np(q), np.int64)
    F, h, w = q.shape
    image = q.reshape(F, h * w).astype(np.float64) * 2.0 ** -32
    return kernel_order_sum(image * image, partial_blocks(h * w))


def _grey_host(value, m):
    """g = m > 0 ? min(255, (int)(value / m * 255.f + 0.5f)) : 0, float32."""
    if not m > 0:
        return np.zeros(value.shape, np.uint8)
    g = (value / _F(m) * _F(255) + _F(0.5)).astype(np.int64)
    return np.minimum(g, 255).astype(np.uint8)


def iwe_render_host(q, count, results):
    """IWE_SPEC section 4 in numpy float32 -> uint8 [F,h,2w,3]: the count image
    on the left, the image of warped events on the right, each grey on its own
    scale."""
    q = np.asarray(_np(q), np.int64)
    c = _counts(count)
    res = read_iwe_results(results)
    F, h, w = q.shape
    canvas = np.empty((F, h, 2 * w, 3), np.uint8)
    for f in range(F):
        canvas[f, :, :w] = _grey_host(c[f].astype(_F), _F(res['count_max'][f]))[..., None]
        image = (q[f].astype(np.float64) * 2.0 ** -32).astype(_F)
        m = _F(np.float64(res['max_q'][f]) * 2.0 ** -32)
        canvas[f, :, w:] = _grey_host(image, m)[..., None]
    return canvas


def iwe_splat(events, win_out, frame_ts, flow):
    """The image of warped events of a batch of frames.  events: the collated
    wire columns ('x', 'y' int64, 'timestamp' float32;
    ``EventSequence.collate_frames``), win_out int64 [F+1] the first slot of
    every frame, frame_ts float32 [2F] start and stop of every frame on the
    clock of the timestamps, flow float32 [F,2,h,w] -> int64 [F,h,w] in units
    of 2^-32, on the device; ``iwe_splat_host`` (a numpy array) for host
    input."""
    x, y, t = events['x'], events['y'], events['timestamp']
    if not _on_device(flow):
        return iwe_splat_host(_np(x), _np(y), _np(t), _np(win_out), _np(frame_ts), _np(flow))
    _lib.require_cuda(x, y, t, frame_ts)
    x, y, t = x.contiguous(), y.contiguous(), t.contiguous()
    flow, frame_ts = flow.contiguous(), frame_ts.contiguous()
    assert x.dtype == y.dtype == torch.long and t.dtype == flow.dtype == frame_ts.dtype == torch.float32
    assert x.numel() == y.numel() == t.numel()
    begin = torch.as_tensor(win_out, dtype=torch.long).to(flow.device).contiguous()
    F, two, h, w = flow.shape
    assert two == 2 and begin.numel() == F + 1 and frame_ts.numel() == 2 * F, \
        (flow.shape, begin.shape, frame_ts.shape)
    q = torch.empty(F, h, w, dtype=torch.long, device=flow.device)
    _lib.check(_lib.lib().dvsof_iwe_splat(
        x.data_ptr(), y.data_ptr(), t.data_ptr(), x.numel(), begin.data_ptr(),
        frame_ts.data_ptr(), flow.data_ptr(), F, h, w, q.data_ptr(), _lib.stream()),
        'dvsof_iwe_splat')
    return q


def iwe_splat_multi(events, win_out, frame_ts, flow, references=('start',), polarity=False):
    """``iwe_splat`` at several reference times of the window and with ON and
    OFF events apart (csrc/iwe.hip, IWE_SPEC sections 8-13).  events,
    win_out, frame_ts, flow as ``iwe_splat`` takes them, and the column
    'polarity' int64 with ``polarity``; references: names among start, middle,
    end, or a mask (``loss.contrast_reference_mask``).  With M = F R C images,
    m = (f R + r) C + c -> (q int64 [M,h,w] in units of 2^-32, count int32
    [M,h,w] holding the uint32 counts of the image's channel) on the device;
    ``iwe_splat_multi_host`` (numpy arrays, count uint32) for host input.
    ``iwe_stats`` and ``iwe_render`` take them as M frames."""
    from .loss import contrast_reference_mask
    mask, polarity = contrast_reference_mask(references), bool(polarity)
    x, y, t = events['x'], events['y'], events['timestamp']
    if polarity and events.get('polarity') is None:
        raise ValueError('polarity=True needs the events\' polarity column')
    p = events['polarity'] if polarity else None
    if not _on_device(flow):
        return iwe_splat_multi_host(_np(x), _np(y), _np(t), None if p is None else _np(p), _np(win_out),
                                    _np(frame_ts), _np(flow), mask, polarity)
    _lib.require_cuda(x, y, t, p, frame_ts)
    x, y, t = x.contiguous(), y.contiguous(), t.contiguous()
    flow, frame_ts = flow.contiguous(), frame_ts.contiguous()
    assert x.dtype == y.dtype == torch.long and t.dtype == flow.dtype == frame_ts.dtype == torch.float32
    assert x.numel() == y.numel() == t.numel()
    if p is not None:
        p = p.contiguous()
        assert p.dtype == torch.long and p.numel() == x.numel()
    begin = torch.as_tensor(win_out, dtype=torch.long).to(flow.device).contiguous()
    F, two, h, w = flow.shape
    assert two == 2 and begin.numel() == F + 1 and frame_ts.numel() == 2 * F, \
        (flow.shape, begin.shape, frame_ts.shape)
    lib = _lib.lib()
    M = lib.dvsof_iwe_multi_images(F, mask, int(polarity))
    if F > 0 and M == 0:
        raise ValueError(f'{F} frames at {bin(mask).count("1")} reference times'
                         f'{" and two polarities" if polarity else ""} are more than 65535 images')
    q = torch.empty(M, h, w, dtype=torch.long, device=flow.device)
    count = torch.empty(M, h, w, dtype=torch.int32, device=flow.device)
    _lib.check(lib.dvsof_iwe_splat_multi(
        x.data_ptr(), y.data_ptr(), t.data_ptr(), _lib.ptr(p), x.numel(), begin.data_ptr(),
        frame_ts.data_ptr(), flow.data_ptr(), F, h, w, mask, int(polarity), q.data_ptr(), count.data_ptr(),
        _lib.stream()), 'dvsof_iwe_splat_multi')
    return q, count


def iwe_stats(q, count):
    """q int64 [F,h,w] (``iwe_splat``), count uint32/int32 [F,h,w]
    (``count_image_batched`` of the same columns) -> device uint8 [F,48], one
    dvsof_iwe_result_t per frame (``read_iwe_results`` copies it to the host);
    for host input the rows of ``iwe_stats_host`` as a numpy uint8 [F,48]."""
    if not _on_device(q):
        return iwe_stats_host(q, count).view(np.uint8).reshape(-1, IWE_RESULT_DTYPE.itemsize)
    _lib.require_cuda(count)
    q, count = q.contiguous(), count.contiguous()
    F, h, w = q.shape
    assert q.dtype == torch.long and tuple(count.shape) == (F, h, w) and count.element_size() == 4
    lib = _lib.lib()
    out = torch.empty(F, IWE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=q.device)
    nbytes = lib.dvsof_iwe_stats_workspace_bytes(F, h, w)
    ws = torch.empty(max(nbytes, 48), dtype=torch.uint8, device=q.device)
    _lib.check(lib.dvsof_iwe_stats(q.data_ptr(), count.data_ptr(), F, h, w, out.data_ptr(),
                                   ws.data_ptr(), nbytes, _lib.stream()), 'dvsof_iwe_stats')
    return out


def iwe_render(q, count, results):
    """Per frame the count image beside the image of warped events, grey, each
    on its own scale -> uint8 [F,h,2w,3] on the device; ``iwe_render_host`` for
    host input.  results: the rows of ``iwe_stats`` (device uint8 [F,48])."""
    if not _on_device(q):
        return iwe_render_host(q, count, results)
    _lib.require_cuda(count, results)
    q, count, results = q.contiguous(), count.contiguous(), results.contiguous()
    F, h, w = q.shape
    assert q.dtype == torch.long and tuple(count.shape) == (F, h, w) and count.element_size() == 4
    assert results.dtype == torch.uint8 and results.numel() == F * IWE_RESULT_DTYPE.itemsize
    canvas = torch.empty(F, h, 2 * w, 3, dtype=torch.uint8, device=q.device)
    _lib.check(_lib.lib().dvsof_iwe_render(q.data_ptr(), count.data_ptr(), results.data_ptr(),
                                           F, h, w, canvas.data_ptr(), _lib.stream()),
               'dvsof_iwe_render')
    return canvas


def read_iwe_results(results):
    """Rows of ``iwe_stats`` -> numpy structured array [F] (IWE_RESULT_DTYPE):
    the one device-to-host copy of a batch."""
    a = _np(results)
    if a.dtype == IWE_RESULT_DTYPE:
        return a.reshape(-1)
    return np.ascontiguousarray(a).view(IWE_RESULT_DTYPE).reshape(-1)


def derive_fwl(res, n_pixels):
    """-> (FWL, kept mass) float64 arrays of per-frame rows: FWL = variance of
    the image of warped events / variance of the count image (NaN where the
    latter is 0: no events, or the same count everywhere), kept mass = the
    share of the events' weight that landed inside the image."""
    n = float(n_pixels)
    sum_i = res['sum_q'].astype(np.float64) * 2.0 ** -32
    count_sum = res['count_sum'].astype(np.float64)
    var_iwe = res['sum_sq'] / n - (sum_i / n) ** 2
    var_cnt = res['count_sq'].astype(np.float64) / n - (count_sum / n) ** 2
    with np.errstate(invalid='ignore', divide='ignore'):
        fwl = np.where(var_cnt == 0, np.nan, var_iwe / var_cnt)
        kept = res['sum_q'].astype(np.float64) / (count_sum * 2.0 ** 32)
    return fwl, kept


# ---------------------------------------------------------------------------
# Average-timestamp images of the warped events and their ratio (RSAT),
# csrc/iwe.hip, docs/IWE_SPEC.md sections 14-21
# ---------------------------------------------------------------------------
def _avg_timestamp_row_dtype():
    from .loss import AVG_TIMESTAMP_ROW_DTYPE      # S, S0, peak, n, n0: the row of the training term
    assert AVG_TIMESTAMP_ROW_DTYPE.itemsize == 32
    return AVG_TIMESTAMP_ROW_DTYPE


def iwe_avg_timestamp_image_bytes(M, h, w):
    """The region of include/dvsof_iwe_avg_timestamp.h: q, s, base int64 and count uint32, padded to 8."""
    return (28 * M * h * w + 7) // 8 * 8


def _avg_timestamp_views(buffer, M, h, w):
    """q, s, base (int64) and count (int32 on the device, uint32 on the host) [M,h,w] as views of the region."""
    P = M * h * w
    cut = [buffer[8 * k * P:8 * (k + 1) * P] for k in range(3)] + [buffer[24 * P:28 * P]]
    if isinstance(buffer, torch.Tensor):
        return tuple(c.view(torch.long).view(M, h, w) for c in cut[:3]) + (cut[3].view(torch.int32).view(M, h, w),)
    return tuple(c.view(np.int64).reshape(M, h, w) for c in cut[:3]) + (cut[3].view(np.uint32).reshape(M, h, w),)


def iwe_avg_timestamp_host(x, y, t, p, frame_event_begin, frame_ts, flow, references=('start',), polarity=False):
    """IWE_SPEC sections 14-16 in numpy float32: what ``iwe_avg_timestamp``
    runs without a GPU and what ``dvsof_iwe_avg_timestamp`` is pinned to, byte
    for byte.  The arguments of ``iwe_splat_multi_host``: the events of a frame
    are those of its slots (section 2), what each does to the images is
    AVG_TIMESTAMP_SPEC section 2 (``loss.avg_timestamp_splat_host``, which the
    training term's restatement runs).  With M = F R C images -> (q, s, base
    int64 [M,h,w], count uint32 [M,h,w]), views of one buffer laid out as
    include/dvsof_iwe_avg_timestamp.h lays the region out."""
    from .loss import avg_timestamp_splat_host, contrast_reference_mask
    mask = contrast_reference_mask(references)
    x, y = np.asarray(x, np.int64).reshape(-1), np.asarray(y, np.int64).reshape(-1)
    t = np.asarray(t, _F).reshape(-1)
    begin = np.asarray(frame_event_begin, np.int64).reshape(-1)
    ts = np.asarray(frame_ts, _F).reshape(-1)
    flow = np.asarray(flow, _F)
    F, _, h, w = flow.shape
    assert begin.size == F + 1 and ts.size == 2 * F and x.size == y.size == t.size
    e = np.arange(x.size, dtype=np.int64)
    keep = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    if F:
        keep &= (e >= begin[0]) & (e < begin[F])
    else:
        keep &= False
    chan = np.zeros(x.size, np.int64)
    if polarity:
        p = np.asarray(p, np.int64).reshape(-1)
        assert p.size == x.size
        keep &= p != 0
        chan = (p < 0).astype(np.int64)
    e = e[keep]
    f = np.searchsorted(begin[:F], e, side='right') - 1     # the last f with begin[f] <= e
    x, y, t = x[keep], y[keep], t[keep]
    t0 = ts[2 * f]
    d = ts[2 * f + 1] - t0
    with np.errstate(all='ignore'):
        tau = np.where(d > 0, np.fmin(np.fmax((t - t0) / d, _F(0)), _F(1)), _F(0)).astype(_F)
    pairs = dict(f=f, c=chan[keep], x=x, y=y, tau=tau, u=flow[f, 0, y, x], v=flow[f, 1, y, x])
    images = avg_timestamp_splat_host(pairs, mask, polarity, F, h, w)
    M = images[0].shape[0]
    buffer = np.zeros(iwe_avg_timestamp_image_bytes(M, h, w), np.uint8)
    views = _avg_timestamp_views(buffer, M, h, w)
    for view, image in zip(views, images):
        view[...] = image
    return views


def iwe_avg_timestamp_rows_host(q, s, base, count):
    """IWE_SPEC section 17 on the host -> the M statistics rows
    (loss.AVG_TIMESTAMP_ROW_DTYPE: S, S0, peak, n, n0), S and S0 through
    ``kernel_order_sum``: the bits ``dvsof_iwe_avg_timestamp`` stores, by
    ``loss.avg_timestamp_rows_host``, which the training term's restatement
    runs."""
    from .loss import avg_timestamp_rows_host
    q, s, base = (np.asarray(_np(a), np.int64) for a in (q, s, base))
    c = _counts(count)
    assert q.ndim == 3 and s.shape == base.shape == c.shape == q.shape
    return avg_timestamp_rows_host(q, s, base, c)


def iwe_avg_timestamp(events, win_out, frame_ts, flow, references=('start',), polarity=False):
    """The average-timestamp images of the warped events of a batch of frames
    and their statistics (csrc/iwe.hip, IWE_SPEC sections 14-18).  The
    arguments of ``iwe_splat_multi``.  With M = F R C images ->
    ((q, s, base int64 [M,h,w], count int32 [M,h,w] holding the uint32
    counts), rows uint8 [M,32]) on the device, the four images views of one
    buffer; q and count hold the bytes of ``iwe_splat_multi``, so that
    ``iwe_stats`` and ``iwe_render`` take them.  For host input the images of
    ``iwe_avg_timestamp_host`` (count uint32) and the rows of
    ``iwe_avg_timestamp_rows_host`` as a numpy uint8 [M,32]."""
    from .loss import contrast_reference_mask
    mask, polarity = contrast_reference_mask(references), bool(polarity)
    x, y, t = events['x'], events['y'], events['timestamp']
    if polarity and events.get('polarity') is None:
        raise ValueError('polarity=True needs the events\' polarity column')
    p = events['polarity'] if polarity else None
    if not _on_device(flow):
        images = iwe_avg_timestamp_host(_np(x), _np(y), _np(t), None if p is None else _np(p), _np(win_out),
                                        _np(frame_ts), _np(flow), mask, polarity)
        rows = iwe_avg_timestamp_rows_host(*images)
        return images, rows.view(np.uint8).reshape(-1, rows.dtype.itemsize)
    _lib.require_cuda(x, y, t, p, frame_ts)
    x, y, t = x.contiguous(), y.contiguous(), t.contiguous()
    flow, frame_ts = flow.contiguous(), frame_ts.contiguous()
    assert x.dtype == y.dtype == torch.long and t.dtype == flow.dtype == frame_ts.dtype == torch.float32
    assert x.numel() == y.numel() == t.numel()
    if p is not None:
        p = p.contiguous()
        assert p.dtype == torch.long and p.numel() == x.numel()
    begin = torch.as_tensor(win_out, dtype=torch.long).to(flow.device).contiguous()
    F, two, h, w = flow.shape
    assert two == 2 and begin.numel() == F + 1 and frame_ts.numel() == 2 * F, \
        (flow.shape, begin.shape, frame_ts.shape)
    lib = _lib.lib()
    M = lib.dvsof_iwe_multi_images(F, mask, int(polarity))
    if F > 0 and M == 0:
        raise ValueError(f'{F} frames at {bin(mask).count("1")} reference times'
                         f'{" and two polarities" if polarity else ""} are more than 65535 images')
    nbytes = lib.dvsof_iwe_avg_timestamp_image_bytes(F, h, w, mask, int(polarity))
    assert nbytes == iwe_avg_timestamp_image_bytes(M, h, w), (nbytes, M, h, w)
    # int64 storage: the region and the rows are 8-byte aligned
    buffer = torch.empty(nbytes // 8, dtype=torch.long, device=flow.device).view(torch.uint8)
    rows = torch.empty(M * 4, dtype=torch.long, device=flow.device).view(torch.uint8).view(M, 32)
    ws_bytes = lib.dvsof_iwe_avg_timestamp_workspace_bytes(F, h, w, mask, int(polarity))
    ws = torch.empty(max(ws_bytes, 32) // 8, dtype=torch.long, device=flow.device)
    _lib.check(lib.dvsof_iwe_avg_timestamp(
        x.data_ptr(), y.data_ptr(), t.data_ptr(), _lib.ptr(p), x.numel(), begin.data_ptr(),
        frame_ts.data_ptr(), flow.data_ptr(), F, h, w, mask, int(polarity), buffer.data_ptr(), nbytes,
        rows.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream()), 'dvsof_iwe_avg_timestamp')
    return _avg_timestamp_views(buffer, M, h, w), rows


def read_avg_timestamp_rows(rows):
    """Rows of ``iwe_avg_timestamp`` -> numpy structured array [M]
    (loss.AVG_TIMESTAMP_ROW_DTYPE): the one device-to-host copy of a batch."""
    dtype = _avg_timestamp_row_dtype()
    a = _np(rows)
    if a.dtype == dtype:
        return a.reshape(-1)
    return np.ascontiguousarray(a).view(dtype).reshape(-1)


def iwe_avg_timestamp_render_host(q, s, base, count):
    """IWE_SPEC section 19 in numpy -> uint8 [M,h,2w,3]: the average distance
    in time at zero flow T0 on the left, the average distance T after the warp
    on the right, float64 as the statistics form them, converted once to
    float32, grey on the fixed scale [0, 1)."""
    from .loss import avg_timestamp_pixels_host
    q, s, base = (np.asarray(_np(a), np.int64) for a in (q, s, base))
    c = _counts(count)
    M, h, w = q.shape
    T, _, T0 = avg_timestamp_pixels_host(q, s, base, c)
    canvas = np.empty((M, h, 2 * w, 3), np.uint8)
    canvas[:, :, :w] = _grey_host(T0.astype(_F), _F(1))[..., None]
    canvas[:, :, w:] = _grey_host(T.astype(_F), _F(1))[..., None]
    return canvas


def iwe_avg_timestamp_render(q, s, base, count):
    """Per image the average distance in time at zero flow beside that after
    the warp, grey on the fixed scale [0, 1) -> uint8 [M,h,2w,3] on the device;
    ``iwe_avg_timestamp_render_host`` for host input.  q, s, base, count: the
    images of ``iwe_avg_timestamp`` or a selection of them (gathered into one
    region of the layout the kernel reads)."""
    if not _on_device(q):
        return iwe_avg_timestamp_render_host(q, s, base, count)
    _lib.require_cuda(s, base, count)
    M, h, w = q.shape
    assert q.dtype == s.dtype == base.dtype == torch.long and count.element_size() == 4
    assert tuple(s.shape) == tuple(base.shape) == tuple(count.shape) == (M, h, w)
    nbytes = iwe_avg_timestamp_image_bytes(M, h, w)
    P = M * h * w
    contiguous = all(a.is_contiguous() for a in (q, s, base, count)) and \
        s.data_ptr() == q.data_ptr() + 8 * P and base.data_ptr() == q.data_ptr() + 16 * P and \
        count.data_ptr() == q.data_ptr() + 24 * P
    if contiguous:
        region = q
    else:
        region = torch.empty(nbytes // 8, dtype=torch.long, device=q.device).view(torch.uint8)
        for dst, src in zip(_avg_timestamp_views(region, M, h, w), (q, s, base, count)):
            dst.copy_(src.view(dst.dtype) if src.dtype != dst.dtype else src)
    canvas = torch.empty(M, h, 2 * w, 3, dtype=torch.uint8, device=q.device)
    # the images as M frames of one reference and no polarity: the kernel reads the layout alone
    _lib.check(_lib.lib().dvsof_iwe_avg_timestamp_render(region.data_ptr(), M, h, w, 1, 0, canvas.data_ptr(),
                                                          _lib.stream()), 'dvsof_iwe_avg_timestamp_render')
    return canvas


def derive_rsat(rows):
    """-> RSAT float64 [M] of per-image rows (``read_avg_timestamp_rows``): the
    ratio of the mean squared average timestamp of the warped events over that
    at zero flow, (S / n) / (S0 / n0), the per-image value of
    AVG_TIMESTAMP_SPEC section 1.  NaN where S0 <= 0 (no events, or all of them
    on the reference: left out of means, as the NaN of ``derive_fwl`` is); 1.0
    where S0 > 0 and n = 0 (every event left the image: never rewarded)."""
    rows = read_avg_timestamp_rows(rows)
    S, S0 = rows['S'].astype(np.float64), rows['S0'].astype(np.float64)
    n, n0 = rows['n'].astype(np.float64), rows['n0'].astype(np.float64)
    live, stayed = S0 > 0, rows['n'] > 0
    with np.errstate(all='ignore'):
        value = (S / n) / (S0 / n0)
    return np.where(live, np.where(stayed, value, 1.0), np.nan)
