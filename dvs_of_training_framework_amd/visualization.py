"""Predicted flow as colour images (HIP, csrc/render.hip; arithmetic and layout
in docs/RENDER_SPEC.md).

``flow2img`` keeps the reference's name and arguments
(utils/visualization.py:5-18): numpy in, BGR uint8 out.  ``render_flows`` and
``render_pyramid`` are the batched device functions underneath; ``visualize``
is visualize.py:130-140 of the reference without its text band.  A mosaic is
laid out once on the host (``Canvas``) and drawn by two kernel launches, or,
for sources that are not on a GPU, by the numpy float32 restatement of the
spec that lives here too (``flow2img_numpy``): it is what a CPU-only user
gets and what the tests pin the kernels against.  ``eval_panels`` (HIP,
csrc/eval_panels.hip; docs/EVAL_PANELS_SPEC.md) draws a prediction against its
ground truth: events, both flows on one scale, the endpoint error;
``eval_panels_numpy`` is its restatement.
"""
import struct
import zlib

import numpy as np
import torch

from . import _lib
from ._abi import dtype_of

FLOW, FRAME, FILL = (_lib.CONSTANTS['DVSOF_RENDER_' + k] for k in ('FLOW', 'FRAME', 'FILL'))
MAX_CHUNKS = _lib.CONSTANTS['DVSOF_RENDER_MAX_CHUNKS']
CHUNK_PIXELS = 2048

# src, dst_offset, dst_stride, kind, image, h, w, x0, y0, row0, rows, chunk, chunks
ITEM_DTYPE = dtype_of('dvsof_render_item_t')
STATS_DTYPE = dtype_of('dvsof_render_stats_t')       # lo, hi, nonfinite, reserved
assert ITEM_DTYPE.itemsize == 64 and STATS_DTYPE.itemsize == 16

_F = np.float32
# {b, g, r} -> index into tab = {v, 0, v*(1-f), v*f}, per hue sector
_SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


# ------------------------------------------------- the numpy restatement
def flow_stats_numpy(flow_x, flow_y):
    """-> (mag float32 [H,W], finite bool [H,W], lo, hi, nonfinite): RENDER_SPEC
    section 2, steps 1-2."""
    fx, fy = np.asarray(flow_x, _F), np.asarray(flow_y, _F)
    finite = np.isfinite(fx) & np.isfinite(fy)
    with np.errstate(all='ignore'):
        mag = np.sqrt(fx * fx + fy * fy)
    lo, hi = _F(np.inf), _F(-np.inf)
    if finite.any():
        lo, hi = mag[finite].min(), mag[finite].max()
    return mag, finite, lo, hi, int(finite.size - finite.sum())


def value_plane_numpy(mag, finite, lo, hi, max_magnitude=0.0):
    """Steps 3-4: the V plane, uint8; non-finite pixels 0."""
    m = _F(max_magnitude)
    with np.errstate(all='ignore'):
        if m > 0:
            mag, lo, hi = np.fmin(mag, m), _F(0), m
        scale = _F(255) / (hi - lo) if hi - lo > 0 else _F(0)
        v = np.trunc(np.fmin((mag - lo) * scale, _F(255)))
    return np.where(finite, v, 0).astype(np.uint8)


def hue_plane_numpy(flow_x, flow_y, finite):
    """Steps 5-6: the hue, int32 in [0, 180]; non-finite pixels 0."""
    fx, fy = np.asarray(flow_x, _F), np.asarray(flow_y, _F)
    with np.errstate(all='ignore'):
        a = (np.arctan2(fy, fx) + _F(np.pi)) * _F(180.0 / np.pi / 2.0)
    return np.where(finite, np.trunc(a), 0).astype(np.int32)


def hsv2bgr_numpy(hue, value):
    """Step 7: OpenCV's float formula for 8-bit input, hue range 180, S = 255.
    hue int [..] in [0, 180], value uint8 [..] -> uint8 [.., 3]."""
    hue = np.asarray(hue).astype(np.int32)
    sector = (hue // 30) % 6
    f = (hue % 30).astype(_F) / _F(30)
    v = np.asarray(value).astype(_F) / _F(255)
    tab = np.stack([v, np.zeros_like(v), v * (_F(1) - f), v * f], axis=-1)
    bgr = np.take_along_axis(tab, _SECTOR[sector], axis=-1)
    return np.rint(bgr * _F(255)).astype(np.uint8)


def flow2img_numpy(flow_x, flow_y, max_magnitude=0.0, return_stats=False):
    """The whole of RENDER_SPEC section 2 in numpy float32."""
    mag, finite, lo, hi, bad = flow_stats_numpy(flow_x, flow_y)
    value = value_plane_numpy(mag, finite, lo, hi, max_magnitude)
    image = hsv2bgr_numpy(hue_plane_numpy(flow_x, flow_y, finite), value)
    image[~finite] = 0
    if return_stats:
        return image, np.array([(lo, hi, bad, 0)], STATS_DTYPE)[0]
    return image


# --------------------------------------------------------------- layout
def chunk_rows(h, w):
    """Rows per item (ints or arrays): dvsof_flow_render_chunk_rows, restated
    (the library validates the table, so a disagreement is an error, not a
    wrong image)."""
    return np.maximum(-(-CHUNK_PIXELS // w), -(-h // MAX_CHUNKS))


def pyramid_layout(shapes):
    """shapes: (h, w) of the levels, coarse -> fine (the predictor's order).
    -> ((canvas_h, canvas_w), [(x0, y0) per level]): the finest level at
    (0, 0), the coarser ones in a row below it, next-finest first
    (visualize.py:96-112)."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    hf, wf = shapes[-1]
    height = hf + (shapes[-2][0] if len(shapes) > 1 else 0)
    at = [None] * len(shapes)
    at[-1] = (0, 0)
    x0 = 0
    for k in range(len(shapes) - 2, -1, -1):
        at[k] = (x0, hf)
        x0 += shapes[k][1]
    return (height, wf), at


def uncovered(height, width, rects):
    """The part of a height x width canvas that none of ``rects`` (x0, y0, w,
    h; disjoint) covers, as rectangles (x0, y0, w, h): a sweep over the bands
    between the rectangles' edges, vertically adjacent equals merged."""
    ys = sorted({0, height} | {y for _, y0, _, h in rects for y in (y0, y0 + h)})
    out, open_ = [], {}         # (x0, w) -> index in out of the piece it continues
    for top, bottom in zip(ys[:-1], ys[1:]):
        spans = sorted((x0, x0 + w) for x0, y0, w, h in rects if y0 <= top and bottom <= y0 + h)
        gaps, x = [], 0
        for a, b in spans:
            if a > x:
                gaps.append((x, a - x))
            x = max(x, b)
        if x < width:
            gaps.append((x, width - x))
        now = {}
        for g in gaps:
            if g in open_:
                k = open_[g]
                out[k] = (*out[k][:3], out[k][3] + bottom - top)
            else:
                k = len(out)
                out.append((g[0], top, g[1], bottom - top))
            now[g] = k
        open_ = now
    return out


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


class Canvas:
    """``n`` BGR canvases of height x width and what goes where.  ``render``
    draws them: two launches when the sources are on a GPU, numpy otherwise.
    Sources must not overlap; what they leave uncovered is 0."""

    def __init__(self, n, height, width):
        self.n, self.height, self.width = int(n), int(height), int(width)
        self.flows, self.frames = [], []

    def _check(self, h, w, x0, y0, index):
        if not (0 <= index < self.n and x0 >= 0 and y0 >= 0 and h >= 1 and w >= 1 and
                x0 + w <= self.width and y0 + h <= self.height):
            raise ValueError(f'a {h}x{w} source at ({x0}, {y0}) of canvas {index} does not lie '
                             f'inside {self.n} canvases of {self.height}x{self.width}')

    def put_flow(self, flow, x0=0, y0=0, index=0, max_magnitude=0.0):
        """flow [2,h,w] float32; -> its row in the statistics."""
        assert flow.ndim == 3 and flow.shape[0] == 2, tuple(flow.shape)
        self._check(flow.shape[1], flow.shape[2], x0, y0, index)
        self.flows.append((flow, int(x0), int(y0), int(index), float(max_magnitude)))
        return len(self.flows) - 1

    def put_frame(self, grey, x0=0, y0=0, index=0):
        """grey [h,w] uint8, replicated to three channels."""
        assert grey.ndim == 2, tuple(grey.shape)
        self._check(grey.shape[0], grey.shape[1], x0, y0, index)
        self.frames.append((grey, int(x0), int(y0), int(index)))

    def fills(self):
        """[(x0, y0, w, h, index)]: what nothing covers.  ValueError for
        sources that overlap (two workgroups would write the same bytes)."""
        rects = [[] for _ in range(self.n)]
        for s, x0, y0, index, *_ in self.flows + self.frames:
            rects[index].append((x0, y0, s.shape[-1], s.shape[-2]))
        out, seen = [], {}      # the canvases of a batch are mostly laid out alike
        for i, r in enumerate(rects):
            key = tuple(r)
            if key not in seen:
                for k, (ax, ay, aw, ah) in enumerate(r):
                    for bx, by, bw, bh in r[:k]:
                        if ax < bx + bw and bx < ax + aw and ay < by + bh and by < ay + ah:
                            raise ValueError(f'sources overlap on canvas {i}: {r[k]} and '
                                             f'{(bx, by, bw, bh)} (x0, y0, w, h)')
                seen[key] = uncovered(self.height, self.width, r)
            out += [(*u, i) for u in seen[key]]
        return out

    def on_device(self):
        sources = [s for s, *_ in self.flows + self.frames]
        return bool(sources) and all(isinstance(s, torch.Tensor) and s.is_cuda for s in sources)

    def render(self, out=None):
        """-> (uint8 [n,height,width,3], statistics): a device tensor and a
        device uint8 [n_flows,16] (``read_stats`` copies it back) when the
        sources are on a GPU, numpy arrays otherwise."""
        if self.on_device():
            return self._render_device(out)
        assert out is None, 'out= is for device rendering'
        self.fills()            # the same refusal of overlapping sources as on the device
        image = np.zeros((self.n, self.height, self.width, 3), np.uint8)
        stats = np.zeros(len(self.flows), STATS_DTYPE)
        for k, (flow, x0, y0, index, m) in enumerate(self.flows):
            f = _host(flow)
            img, stats[k] = flow2img_numpy(f[0], f[1], m, return_stats=True)
            image[index, y0:y0 + img.shape[0], x0:x0 + img.shape[1]] = img
        for grey, x0, y0, index in self.frames:
            g = _host(grey).astype(np.uint8)
            image[index, y0:y0 + g.shape[0], x0:x0 + g.shape[1]] = g[:, :, None]
        return image, stats

    # -- the item table (dvsof_render_item_t) and the two launches
    def _items(self, keep):
        """-> (items, n_flow): one head row per source, expanded into its
        chunks in one vectorised pass (a batch of 8 four-level pyramids is
        ~400 items)."""
        heads = []      # kind, src, h, w, x0, y0, index, image
        for k, (flow, x0, y0, index, _) in enumerate(self.flows):
            assert flow.dtype == torch.float32, flow.dtype
            flow = flow.contiguous()
            keep.append(flow)
            heads.append((FLOW, flow.data_ptr(), flow.shape[1], flow.shape[2], x0, y0, index, k))
        for grey, x0, y0, index in self.frames:
            assert grey.dtype == torch.uint8, grey.dtype
            grey = grey.contiguous()
            keep.append(grey)
            heads.append((FRAME, grey.data_ptr(), grey.shape[0], grey.shape[1], x0, y0, index, -1))
        for x0, y0, w, h, index in self.fills():
            heads.append((FILL, 0, h, w, x0, y0, index, -1))
        kind, src, h, w, x0, y0, index, image = np.array(heads, np.int64).reshape(-1, 8).T
        step = chunk_rows(h, w)
        chunks = -(-h // step)
        of = np.repeat(np.arange(len(heads)), chunks)           # the source of every item
        chunk = np.arange(len(of)) - (np.cumsum(chunks) - chunks)[of]
        items = np.zeros(len(of), ITEM_DTYPE)
        items['src'], items['kind'], items['image'] = src[of], kind[of], image[of]
        items['dst_offset'] = index[of] * (3 * self.width * self.height)
        items['dst_stride'] = 3 * self.width
        items['h'], items['w'], items['x0'], items['y0'] = h[of], w[of], x0[of], y0[of]
        items['row0'] = chunk * step[of]
        items['rows'] = np.minimum(step[of], h[of] - items['row0'])
        items['chunk'], items['chunks'] = chunk, chunks[of]
        return items, int(chunks[:len(self.flows)].sum())

    def _render_device(self, out=None):
        keep = []
        items, n_flow = self._items(keep)
        dev = keep[0].device
        shape = (self.n, self.height, self.width, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
        assert tuple(out.shape) == shape and out.dtype == torch.uint8 and out.is_contiguous() \
            and out.device == dev, (tuple(out.shape), out.dtype, out.device)
        stats = run_items(items, n_flow, len(self.flows),
                          [m for *_, m in self.flows], out)
        return out, stats


def run_items(items, n_flow, n_images, max_magnitude, canvas):
    """The two launches over an item table (numpy, ITEM_DTYPE) that draws into
    the device tensor ``canvas``.  -> device uint8 [n_images,16]."""
    lib = _lib.lib()
    dev = canvas.device
    items = np.ascontiguousarray(items)
    items_dev = torch.from_numpy(items.view(np.uint8).reshape(-1).copy()).to(dev)
    stats = torch.empty(max(n_images, 1), STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    nbytes = lib.dvsof_flow_render_workspace_bytes(n_images)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    mm = None
    if any(m > 0 for m in max_magnitude):
        mm = torch.tensor(max_magnitude, dtype=torch.float32).to(dev)
    host = items.ctypes.data if len(items) else None
    _lib.check(lib.dvsof_flow_render_stats(
        host, items_dev.data_ptr(), n_flow, n_images, ws.data_ptr(), nbytes,
        _lib.stream()), 'dvsof_flow_render_stats')
    _lib.check(lib.dvsof_flow_render(
        host, items_dev.data_ptr(), len(items), n_flow, n_images, _lib.ptr(mm),
        ws.data_ptr(), nbytes, canvas.data_ptr(), canvas.numel(), stats.data_ptr(),
        _lib.stream()), 'dvsof_flow_render')
    return stats[:n_images]


def read_stats(stats):
    """Statistics of a ``render`` -> numpy structured array (STATS_DTYPE): the
    one device-to-host copy."""
    if isinstance(stats, torch.Tensor):
        return stats.cpu().numpy().view(STATS_DTYPE).reshape(-1)
    return np.asarray(stats, STATS_DTYPE).reshape(-1)


# ------------------------------------------------------ public functions
def _magnitudes(max_magnitude, shape):
    if max_magnitude is None:
        return np.zeros(shape, np.float32)
    return np.broadcast_to(np.asarray(_host(max_magnitude), np.float32), shape)


def render_flows(flow, max_magnitude=None, out=None, return_stats=False):
    """flow [N,2,H,W] float32 (on the device: two launches for the batch) ->
    uint8 [N,H,W,3] BGR, every image on its own min / max unless
    ``max_magnitude`` (a scalar or [N]; <= 0: own) gives the scale."""
    n, two, h, w = flow.shape
    assert two == 2, tuple(flow.shape)
    mm = _magnitudes(max_magnitude, (n,))
    canvas = Canvas(n, h, w)
    for i in range(n):
        canvas.put_flow(flow[i], 0, 0, i, mm[i])
    image, stats = canvas.render(out)
    return (image, stats) if return_stats else image


def render_pyramid(flows, max_magnitude=None, out=None, return_stats=False):
    """flows: the levels [N,2,h,w], coarse -> fine -> uint8 [N,Hc,W,3], one
    pyramid mosaic per sample (``pyramid_layout``), every level on its own
    scale unless ``max_magnitude`` (broadcast to [N,levels]) says otherwise.
    Statistics: row ``i * levels + k`` is level k of sample i."""
    n = flows[0].shape[0]
    (height, width), at = pyramid_layout([f.shape[-2:] for f in flows])
    mm = _magnitudes(max_magnitude, (n, len(flows)))
    canvas = Canvas(n, height, width)
    for i in range(n):
        for k, f in enumerate(flows):
            canvas.put_flow(f[i], at[k][0], at[k][1], i, mm[i, k])
    image, stats = canvas.render(out)
    return (image, stats) if return_stats else image


def flow2img(flow_x, flow_y):
    """utils/visualization.py:5-18: numpy [H,W] x 2 -> uint8 [H,W,3] BGR, on
    the GPU when there is one, else by the numpy restatement."""
    fx, fy = np.asarray(flow_x, np.float32), np.asarray(flow_y, np.float32)
    if not torch.cuda.is_available():
        return flow2img_numpy(fx, fy)
    flow = torch.from_numpy(np.stack([fx, fy])[None]).cuda()
    return render_flows(flow)[0].cpu().numpy()


def sample_canvas(images, predictions, prefix_length=0):
    """The picture of ONE sample (visualize.py:115-140 without the text band):
    images uint8 [D,1,H,W] side by side on top; below them the pyramids of the
    sample's predictions (each a list of [2,h,w] levels, coarse -> fine) side
    by side, shifted right by prefix_length * W + W // 2."""
    d, _, h, w = images.shape
    (ph, pw), at = pyramid_layout([f.shape[-2:] for f in predictions[0]])
    canvas = Canvas(1, h + ph, d * w)
    for k in range(d):
        canvas.put_frame(images[k, 0], k * w, 0)
    shift = prefix_length * pw + pw // 2
    for p, levels in enumerate(predictions):
        for k, f in enumerate(levels):
            canvas.put_flow(f, shift + p * pw + at[k][0], h + at[k][1])
    return canvas


def event_statistics(args, batch, sequence_length, sample=0):
    """visualize.py:47-55 for one sample of the batch -> events of the prefix,
    of the predicted elements, of the suffix (zeros for a batch without raw
    events)."""
    events = batch.get('events') if hasattr(batch, 'get') else None
    if not events or 'element_index' not in events:
        return 0, 0, 0
    element = events['element_index']
    if 'sample_index' in events:
        element = element[events['sample_index'] == sample]
    prefix = int((element < args.prefix_length).sum())
    suffix = int((element >= sequence_length - args.suffix_length).sum())
    return prefix, int(element.numel()) - prefix - suffix, suffix


def sample_picture(args, batch, loss, parts, prediction, sample=0):
    """The picture and the statistics of sample ``sample`` of a batch of any
    size: its frames (``sample_idx``) on top, its predictions
    (``flow_sample_idx``) below.  ``loss`` and ``parts`` are the batch's.
    statistics: the reference's keys plus ``levels``, per prediction the
    lo / hi / nonfinite of every level, coarse -> fine."""
    flows = prediction['prediction']
    device = flows[-1].device
    images = torch.as_tensor(batch['images'])
    frames = torch.as_tensor(batch['sample_idx']).to(images.device) == sample
    images = images[frames].to(device).to(torch.uint8)         # join_images: astype(uint8)
    own = torch.nonzero(prediction['flow_sample_idx'] == sample).flatten().tolist()
    predictions = [[f[i] for f in flows] for i in own]
    canvas = sample_canvas(images, predictions, args.prefix_length)
    image, stats = canvas.render()
    stats = read_stats(stats).reshape(len(predictions), len(flows))
    parts = [[float(x) for x in row] for row in parts]
    sizes = event_statistics(args, batch, images.shape[0] - 1, sample)
    statistics = {'loss': float(loss), 'smoothness': parts[0], 'photometric': parts[1],
                  'border': parts[2], 'prefix_size': sizes[0], 'pred_size': sizes[1],
                  'suffix_size': sizes[2],
                  'levels': [[{'lo': float(s['lo']), 'hi': float(s['hi']),
                               'nonfinite': int(s['nonfinite'])} for s in row]
                             for row in stats]}
    return _host(image[0]), statistics


def visualize(args, batch, loss, parts, weights, prediction):
    """visualize.py:130-140 for a batch of ONE sample (``mbs = 1``) -> (image
    uint8 [H + Hc, D * W, 3] BGR as numpy, statistics).  ``prediction`` is what
    ``process_minibatch(..., return_prediction=True)`` returns.  ``weights`` is
    kept for the reference's signature: it only fed the text band."""
    return sample_picture(args, batch, loss, parts, prediction, 0)


# ------------------------------------------------------ evaluation panels
# pred_lo, pred_hi, pred_nonfinite, gt_lo, gt_hi, gt_nonfinite, n_counted, n_below
PANEL_STATS_DTYPE = dtype_of('dvsof_eval_panel_stats_t')
assert PANEL_STATS_DTYPE.itemsize == 32
UNCOUNTED = 64                  # grey of a pixel the metric does not count
PANELS = ('events', 'prediction', 'ground truth', 'endpoint error')


def counted_numpy(gt_u, gt_v, count2=None, max_row=None):
    """The pixels ``eval.flow_error`` counts (EVAL_SPEC section 3) -> bool
    [..,h,w]: row < max_row, an event of either polarity (count2 [..,2,h,w];
    None: dense), no infinite ground-truth component, its float32 norm > 0."""
    gu, gv = np.asarray(gt_u, _F), np.asarray(gt_v, _F)
    h = gu.shape[-2]
    rows = np.arange(h)[:, None] < (h if max_row is None else int(max_row))
    with np.errstate(all='ignore'):
        moving = np.sqrt(gu * gu + gv * gv) > 0
    ok = rows & ~np.isinf(gu) & ~np.isinf(gv) & moving
    if count2 is not None:
        c = np.asarray(count2).astype(np.int64) & 0xFFFFFFFF    # the uint32 counts
        ok = ok & (c[..., 0, :, :] + c[..., 1, :, :] > 0)
    return ok


def endpoint_error_numpy(pred, gt_u, gt_v):
    """EE of ``dvsof_flow_error``: sqrtf(du * du + dv * dv) with du = gt_u -
    pred_u, every operation rounded to float32.  pred [..,2,h,w]."""
    pred = np.asarray(pred, _F)
    with np.errstate(all='ignore'):
        du = np.asarray(gt_u, _F) - pred[..., 0, :, :]
        dv = np.asarray(gt_v, _F) - pred[..., 1, :, :]
        return np.sqrt(du * du + dv * dv)


def panel_scale(stats, flow_scale=0.0):
    """The ``max_magnitude`` both flow panels of a frame are drawn with:
    ``flow_scale`` when > 0, else the ground truth's ``hi`` when it is finite
    and > 0, else the prediction's ``hi``.  stats: one PANEL_STATS_DTYPE row."""
    if _F(flow_scale) > 0:
        return _F(flow_scale)
    hi = _F(stats['gt_hi'])
    return hi if np.isfinite(hi) and hi > 0 else _F(stats['pred_hi'])


def heat_numpy(ee, counted, err_max=6.0):
    """The error panel -> uint8 [..,3] BGR: black -> red -> yellow -> white
    over 0 .. err_max, a NaN at the maximum, an uncounted pixel (64, 64, 64)."""
    with np.errstate(all='ignore'):
        t = np.trunc(np.fmin(np.asarray(ee, _F) * (_F(255) / _F(err_max)), _F(255)))
    t3 = 3 * np.where(counted, t, 0).astype(np.int64)
    bgr = np.stack([np.clip(t3 - 510, 0, 255), np.clip(t3 - 255, 0, 255),
                    np.minimum(t3, 255)], -1).astype(np.uint8)
    bgr[~np.asarray(counted, bool)] = UNCOUNTED
    return bgr


def events_numpy(shape, count2=None, frames=None, gain=85):
    """The events panel -> uint8 shape + (3,) BGR: ON events red, OFF events
    blue, ``gain`` per event, over the grey frame (black without one)."""
    out = np.zeros(tuple(shape) + (3,), np.uint8)
    if frames is not None:
        out[:] = np.asarray(frames, np.uint8)[..., None]
    if count2 is not None:
        c = np.asarray(count2).astype(np.int64) & 0xFFFFFFFF
        on, off = c[..., 0, :, :], c[..., 1, :, :]
        hit = on + off > 0
        colour = np.stack([np.minimum(255, np.minimum(off, 255) * int(gain)), np.zeros_like(on),
                           np.minimum(255, np.minimum(on, 255) * int(gain))], -1)
        out[hit] = colour[hit].astype(np.uint8)
    return out


def eval_panels_numpy(pred, gt_u, gt_v, count2=None, frames=None, max_row=None, flow_scale=0.0,
                      err_max=6.0, gain=85, return_stats=False):
    """docs/EVAL_PANELS_SPEC.md in numpy float32: what ``eval_panels`` runs
    without a GPU and what the kernels are pinned to.  pred [F,2,h,w], gt_u,
    gt_v [F,h,w], count2 [F,2,h,w] or None, frames uint8 [F,h,w] or None ->
    uint8 [F,h,4w,3] BGR (events | prediction | ground truth | endpoint
    error) and, with return_stats, a PANEL_STATS_DTYPE array [F]."""
    pred, gu, gv = np.asarray(pred, _F), np.asarray(gt_u, _F), np.asarray(gt_v, _F)
    F, two, h, w = pred.shape
    assert two == 2 and gu.shape == gv.shape == (F, h, w), (pred.shape, gu.shape, gv.shape)
    counted = counted_numpy(gu, gv, count2, max_row)
    ee = endpoint_error_numpy(pred, gu, gv)
    image = np.empty((F, h, 4 * w, 3), np.uint8)
    stats = np.zeros(F, PANEL_STATS_DTYPE)
    image[:, :, :w] = events_numpy((F, h, w), count2, frames, gain)
    image[:, :, 3 * w:] = heat_numpy(ee, counted, err_max)
    for f in range(F):
        s = stats[f]
        _, _, s['pred_lo'], s['pred_hi'], s['pred_nonfinite'] = flow_stats_numpy(pred[f, 0], pred[f, 1])
        _, _, s['gt_lo'], s['gt_hi'], s['gt_nonfinite'] = flow_stats_numpy(gu[f], gv[f])
        s['n_counted'] = counted[f].sum()
        with np.errstate(invalid='ignore'):
            s['n_below'] = (ee[f][counted[f]] < _F(3)).sum()
        m = panel_scale(s, flow_scale)
        image[f, :, w:2 * w] = flow2img_numpy(pred[f, 0], pred[f, 1], m)
        image[f, :, 2 * w:3 * w] = flow2img_numpy(gu[f], gv[f], m)
    return (image, stats) if return_stats else image


def eval_panels(pred, gt_u, gt_v, count2=None, frames=None, max_row=None, flow_scale=0.0,
                err_max=6.0, gain=85, out=None, return_stats=False):
    """Per frame one picture of four panels, events | prediction | ground
    truth | endpoint error, the two flows on one colour scale: two launches
    for any F on the device, ``eval_panels_numpy`` for host arrays.

    pred float32 [F,2,h,w]; gt_u, gt_v float32 [F,h,w]; count2 [F,2,h,w]
    (``eval.count_image_polarity_batched``) or None (dense); frames uint8
    [F,h,w] or None; max_row: rows the metric counts (default h).  out: a
    device uint8 [F,h,4w,3] to draw into, contiguous or a strided view whose
    pixels are 3 and whose columns 1 byte apart.  -> uint8 [F,h,4w,3] BGR and,
    with return_stats, the statistics (device uint8 [F,32]: ``read_panel_stats``)."""
    if not (isinstance(pred, torch.Tensor) and pred.is_cuda):
        assert out is None, 'out= is for device rendering'
        return eval_panels_numpy(_host(pred), _host(gt_u), _host(gt_v),
                                 None if count2 is None else _host(count2),
                                 None if frames is None else _host(frames), max_row, flow_scale,
                                 err_max, gain, return_stats)
    _lib.require_cuda(gt_u, gt_v, count2, frames)
    pred, gt_u, gt_v = pred.contiguous(), gt_u.contiguous(), gt_v.contiguous()
    F, two, h, w = pred.shape
    assert two == 2 and tuple(gt_u.shape) == tuple(gt_v.shape) == (F, h, w) \
        and pred.dtype == gt_u.dtype == gt_v.dtype == torch.float32, \
        (pred.shape, gt_u.shape, gt_v.shape)
    if count2 is not None:
        count2 = count2.contiguous()
        assert tuple(count2.shape) == (F, 2, h, w) and count2.element_size() == 4
    if frames is not None:
        frames = frames.contiguous()
        assert tuple(frames.shape) == (F, h, w) and frames.dtype == torch.uint8
    dev = pred.device
    if out is None:
        out = torch.empty(F, h, 4 * w, 3, dtype=torch.uint8, device=dev)
    assert tuple(out.shape) == (F, h, 4 * w, 3) and out.dtype == torch.uint8 \
        and out.device == dev and out.stride(3) == 1 and out.stride(2) == 3, \
        (tuple(out.shape), out.stride(), out.dtype, out.device)
    lib = _lib.lib()
    stats = torch.empty(max(F, 1), PANEL_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    nbytes = lib.dvsof_eval_panels_workspace_bytes(F)
    ws = torch.empty(max(nbytes, 32), dtype=torch.uint8, device=dev)
    max_row = h if max_row is None else int(max_row)
    _lib.check(lib.dvsof_eval_panels_stats(
        pred.data_ptr(), gt_u.data_ptr(), gt_v.data_ptr(), _lib.ptr(count2), F, h, w, max_row,
        ws.data_ptr(), nbytes, _lib.stream()), 'dvsof_eval_panels_stats')
    _lib.check(lib.dvsof_eval_panels(
        pred.data_ptr(), gt_u.data_ptr(), gt_v.data_ptr(), _lib.ptr(count2), _lib.ptr(frames),
        F, h, w, max_row, float(flow_scale), float(err_max), int(gain), ws.data_ptr(), nbytes,
        out.data_ptr(), out.untyped_storage().nbytes() - out.storage_offset(),
        out.stride(0), out.stride(1), stats.data_ptr(), _lib.stream()), 'dvsof_eval_panels')
    return (out, stats[:F]) if return_stats else out


def read_panel_stats(stats):
    """Statistics of ``eval_panels`` -> numpy structured array
    (PANEL_STATS_DTYPE): the one device-to-host copy."""
    if isinstance(stats, torch.Tensor):
        return stats.cpu().numpy().view(PANEL_STATS_DTYPE).reshape(-1)
    return np.asarray(stats, PANEL_STATS_DTYPE).reshape(-1)


# ------------------------------------------------------------------ files
def write_png(path, array):
    """uint8 [H,W,3] (written as given: hand in RGB for a viewer's colours, or
    the BGR of this module as the reference's imwrite did) or [H,W] -> an
    8-bit PNG, filter 0 on every row; zlib and struct only."""
    a = np.ascontiguousarray(_host(array))
    assert a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)), \
        (a.dtype, a.shape)
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + a.size // h), np.uint8)
    raw[:, 1:] = a.reshape(h, -1)

    def chunk(tag, data):
        body = tag + data
        return struct.pack('>I', len(data)) + body + struct.pack('>I', zlib.crc32(body))
    header = struct.pack('>IIBBBBB', w, h, 8, 0 if a.ndim == 2 else 2, 0, 0, 0)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', header) +
                chunk(b'IDAT', zlib.compress(raw.tobytes(), 6)) + chunk(b'IEND', b''))
