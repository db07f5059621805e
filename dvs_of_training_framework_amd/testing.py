"""``evaluate`` with the reference's signature (utils/testing.py:10-108), the
per-frame work done on the device in batches of frames: one batched
inference, one count-image launch, one ground-truth propagation, one error
launch and one device-to-host copy per batch (kernels: csrc/eval.hip).
``frame_generator`` (utils/data.py:139-152), ``read_config`` and
``ravel_config`` (utils/testing.py:111-153) are restated beside it."""
import itertools
from types import SimpleNamespace

import numpy as np
import torch

from . import eval as dev_eval


def frame_generator(events, frames):
    """Cut a recording into frames.  events: the columns [x, y, t, p], sorted
    by t; frames: (start, stop) timestamp pairs.  Yields (columns of the
    frame, start, stop); a frame holds the events with start < t <= stop."""
    windows = np.asarray(frames).reshape(-1, 2)
    cuts = np.searchsorted(events[2], windows, side='right')
    for (t_begin, t_end), (lo, hi) in zip(windows, cuts):
        yield [column[lo:hi] for column in events], t_begin, t_end


def read_config(filename):
    """The YAML test grid as a dict; a malformed file raises yaml.YAMLError."""
    import yaml
    with open(filename) as stream:
        return yaml.safe_load(stream)


# axes of the test grid, slowest first
GRID_KEYS = ('start', 'stop', 'step', 'test_shape', 'crop_type', 'is_car')


def _grid_axis(key, value):
    """Values one grid axis runs over: a scalar is an axis of one; a test
    shape is itself a list, so only a list of lists is an axis of several."""
    if key != 'test_shape':
        return value if isinstance(value, list) else [value]
    if not isinstance(value, list) or not value:
        raise TypeError(f'test_shape is a [h, w] list or a list of them, not {value!r}')
    return value if isinstance(value[0], list) else [value]


def ravel_config(config):
    """Every combination of the grid's axes as a namespace with the fields
    GRID_KEYS, the last axis varying fastest."""
    axes = [_grid_axis(key, config[key]) for key in GRID_KEYS]
    for combination in itertools.product(*axes):
        yield SimpleNamespace(**dict(zip(GRID_KEYS, combination)))


def fold_box(fun, frame_shape):
    """The (y0, x0, h, w) window of a reference-style box crop (an object with
    a ``.box``, utils/data.py:24-42, 78-86) that lies inside the frame, as
    ints; None for anything else (applied on the host instead)."""
    box = getattr(fun, 'box', None)
    if box is None or len(box) != 4:
        return None
    try:
        y0, x0, h, w = (int(b) for b in box)
    except (TypeError, ValueError):
        return None
    if [y0, x0, h, w] != [b for b in box]:      # fractional boxes: not ours
        return None
    H, W = frame_shape
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        return None
    return y0, x0, h, w


class MapWindow:
    """The ground-truth maps [lo, hi) of a sequence on the device.  A batch
    asks for the range its frames touch; maps already there (consecutive
    batches overlap in at least one) are kept, only the new ones are
    uploaded.  ``uploaded`` counts maps sent to the device."""

    def __init__(self, x_maps, y_maps, device):
        self.src = (x_maps, y_maps)
        self.device = device
        self.lo = self.hi = 0
        self.dev = None
        self.uploaded = 0

    def _send(self, a, dst):
        a = np.asarray(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        dst.copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(dst.shape))

    def ensure(self, lo, hi):
        """-> (x, y, map_offset): device tensors [K,H,W] holding at least the
        maps [lo, hi), the first being map ``map_offset``."""
        if self.dev is not None and self.lo <= lo and hi <= self.hi:
            return self.dev[0], self.dev[1], self.lo
        first = np.asarray(self.src[0][lo])
        H, W = np.squeeze(first).shape
        dtype = torch.float32 if first.dtype == np.float32 else torch.float64
        k_lo, k_hi = max(lo, self.lo), min(hi, self.hi)     # kept maps
        new = []
        for src, old in zip(self.src, self.dev or (None, None)):
            t = torch.empty(hi - lo, H, W, dtype=dtype, device=self.device)
            if old is not None and k_lo < k_hi:
                t[k_lo - lo:k_hi - lo].copy_(old[k_lo - self.lo:k_hi - self.lo])
                if lo < k_lo:
                    self._send(src[lo:k_lo], t[:k_lo - lo])
                if k_hi < hi:
                    self._send(src[k_hi:hi], t[k_hi - lo:])
            else:
                self._send(src[lo:hi], t)
            new.append(t)
        kept = max(k_hi - k_lo, 0) if self.dev is not None else 0
        self.uploaded += hi - lo - kept
        self.dev, self.lo, self.hi = tuple(new), lo, hi
        return new[0], new[1], lo


def _device_of(of):
    return torch.device(getattr(of, '_device', 'cuda'))


_check_in_frame = dev_eval.check_in_frame


def evaluate_frames(of, events, frames, gt, event_preproc_fun=None,
                    pred_postproc_fun=None, gt_proc_fun=None, is_car=False,
                    batch_size=8, fold=True, *, observer=None):
    """The per-frame results behind ``evaluate``: a numpy structured array
    (eval.RESULT_DTYPE: sum_ee, n_points, n_below, pred_max, pred_min), one
    row per frame.  fold=False applies box crops on the host like any other
    callable (same results; for tests).

    observer: called once per batch as ``observer(first, pred, gt_u, gt_v,
    max_row, count2)`` with the index of the batch's first frame, the device
    tensors the error kernel reads and a zero-argument callable that returns
    the polarity count image [F,2,h,w] of the batch
    (``eval.count_image_polarity_batched`` of the columns the count image was
    made of; launched only when called).  None: nothing more is launched.

    events: the columns [x, y, t, p], or a ``sequence.EventSequence`` holding
    them on the device: a batch of frames is then one window-kernel launch in
    front of the inference (``of.flow_sequence``), and the count image is made
    of the same collated columns; nothing but the window table is uploaded.
    ``event_preproc_fun`` must then be None or a box crop.  The events stay on
    the device, so whether one lies outside the ground-truth frame is decided
    by the shapes alone: a sensor (or box) larger than the ground truth raises
    the ValueError of the numpy-events path even when no event does."""
    from .sequence import EventSequence
    on_device = isinstance(events, EventSequence)
    if on_device:
        seq_box = fold_box(event_preproc_fun, events.shape)
        if event_preproc_fun is not None and seq_box is None:
            raise TypeError(
                'with an EventSequence event_preproc_fun is None or a box crop '
                '(an object with a .box inside the frame); any other callable '
                'needs the numpy-events path: pass events as [x, y, t, p]')
        if not hasattr(of, 'flow_sequence'):
            raise TypeError(
                'an EventSequence needs an `of` with flow_sequence '
                '(OpticalFlow); other callables take the numpy-events path')
    device = _device_of(of)
    frames = np.array(frames)
    if frames.size == 0:
        return np.zeros(0, dev_eval.RESULT_DTYPE)
    frames = frames.reshape(-1, 2)
    batch_size = max(int(batch_size), 1)
    if not on_device:
        t = events[2]
        idx = np.searchsorted(t, frames.ravel(), side='right').reshape(-1, 2)
    xg, yg, ts = gt['x_flow_dist'], gt['y_flow_dist'], gt['timestamps']
    H, W = np.squeeze(xg[0]).shape
    gt_box = fold_box(gt_proc_fun, (H, W)) if fold else None
    ev_box = fold_box(event_preproc_fun, (H, W)) if fold else None
    post_box = None
    maps = MapWindow(xg, yg, device)
    out = []
    for b0 in range(0, len(frames), batch_size):
        fr = frames[b0:b0 + batch_size]
        starts, stops = list(fr[:, 0]), list(fr[:, 1])
        if not on_device:
            raw = [[p[i0:i1] for p in events] for i0, i1 in idx[b0:b0 + batch_size]]
            # events as the network sees them (utils/testing.py:66)
            if event_preproc_fun is None:
                evs = [np.array(e) for e in raw]
            else:
                evs = [event_preproc_fun(np.array(e).T).T for e in raw]

        # one batched inference -> pred [F,2,h,w] on the device
        if on_device:
            pred, collated = of.flow_sequence(events, starts, stops, box=seq_box,
                                              return_events=True)
        elif hasattr(of, 'flow_device'):
            pred = of.flow_device(evs, starts, stops)
        else:
            pred = torch.from_numpy(np.ascontiguousarray(np.transpose(
                np.asarray(of(evs, starts, stops), dtype=np.float32),
                (0, 3, 1, 2)))).to(device)
        if pred_postproc_fun is not None:
            if fold:
                post_box = fold_box(pred_postproc_fun, pred.shape[-2:])
            if post_box is not None:
                y0, x0, h, w = post_box
                pred = pred[:, :, y0:y0 + h, x0:x0 + w]
            else:
                host = np.transpose(pred.cpu().numpy(), (0, 2, 3, 1))
                host = np.stack([pred_postproc_fun(f) for f in host])
                pred = torch.from_numpy(np.ascontiguousarray(np.transpose(
                    host, (0, 3, 1, 2)), dtype=np.float32)).to(device)
        pred = pred.to(torch.float32).contiguous()

        # ground truth over each frame's interval
        plans = [dev_eval.plan_gt_steps(ts, a, b) for a, b in zip(starts, stops)]
        lo = min(min(p[1]) for p in plans)
        hi = max(max(p[1]) for p in plans) + 1
        xd, yd, off = maps.ensure(lo, hi)
        if gt_proc_fun is None or gt_box is not None:
            gt_u, gt_v = dev_eval.propagate(xd, yd, plans, gt_box, off)
        else:
            u, v = dev_eval.propagate(xd, yd, plans, None, off)
            u, v = u.cpu().numpy(), v.cpu().numpy()
            host = np.stack([gt_proc_fun(np.dstack((a, b)))
                             for a, b in zip(u, v)])
            gt_u = torch.from_numpy(np.ascontiguousarray(host[..., 0])).to(device)
            gt_v = torch.from_numpy(np.ascontiguousarray(host[..., 1])).to(device)
        h, w = gt_u.shape[-2:]

        # event mask: count image of the frame's events
        if on_device:
            # the collated columns are already cropped and shifted; the -1
            # slots (outside the box, padding) fall outside (0, 0, h, w)
            eh, ew = seq_box[2:] if seq_box is not None else events.shape
            if eh > h or ew > w:    # events could lie outside the ground truth
                raise ValueError('invalid entry in coordinates array')
            count = dev_eval.count_image_batched(
                collated.events['x'], collated.events['y'], collated.win_out,
                (h, w), (0, 0, h, w))
            max_row = min(dev_eval.CAR_ROWS, h) if is_car else h
            res = dev_eval.flow_error(gt_u, gt_v, pred, count, max_row)
            out.append(dev_eval.read_results(res))
            if observer is not None:
                ev = collated.events
                observer(b0, pred, gt_u, gt_v, max_row,
                         lambda ev=ev, begin=collated.win_out, h=h, w=w:
                         dev_eval.count_image_polarity_batched(
                             ev['x'], ev['y'], ev['polarity'], begin, (h, w),
                             (0, 0, h, w)))
            continue
        if ev_box is not None and ev_box[2:] == (h, w):
            cols, box = raw, ev_box         # the kernel drops and shifts
        else:
            cols, box = evs, None
            for e in evs:
                _check_in_frame(np.asarray(e[0]).astype(np.int64),
                                np.asarray(e[1]).astype(np.int64), (h, w))
        begin = np.zeros(len(cols) + 1, np.int64)
        begin[1:] = np.cumsum([len(e[0]) for e in cols])
        xy = np.empty((2, begin[-1]), np.int64)
        for e, i0, i1 in zip(cols, begin[:-1], begin[1:]):
            xy[0, i0:i1] = np.asarray(e[0]).astype(int)
            xy[1, i0:i1] = np.asarray(e[1]).astype(int)
        xy = torch.from_numpy(xy).to(device)
        count = dev_eval.count_image_batched(xy[0], xy[1], begin, (h, w), box)

        max_row = min(dev_eval.CAR_ROWS, h) if is_car else h
        res = dev_eval.flow_error(gt_u, gt_v, pred, count, max_row)
        out.append(dev_eval.read_results(res))      # the batch's one copy back
        if observer is not None:
            def count2(cols=cols, xy=xy, begin=begin, h=h, w=w, box=box):
                pol = np.concatenate([np.asarray(e[3]).astype(np.int64)
                                      for e in cols] + [np.zeros(0, np.int64)])
                return dev_eval.count_image_polarity_batched(
                    xy[0], xy[1], torch.from_numpy(pol).to(device), begin,
                    (h, w), box)
            observer(b0, pred, gt_u, gt_v, max_row, count2)
    return np.concatenate(out)


def flow_warp_loss(of, sequence, frames, box=None, batch_size=8, observer=None, references=('start',),
                   polarity=False):
    """Label-free quality of ``of`` on a device-resident
    ``sequence.EventSequence``: per frame the statistics of the image of warped
    events and of the count image (docs/IWE_SPEC.md) as a numpy structured
    array (eval.IWE_RESULT_DTYPE); ``eval.derive_fwl`` makes the flow warp loss
    of them.  Per batch of frames: one ``of.flow_sequence``, one count image of
    the collated columns, one splat, one statistics call and one copy back of
    48 bytes per frame.

    frames: [(start, stop)]; box: None or a (y0, x0, h, w) inside the frame,
    the crop the events get (``of`` predicts at that size);
    observer(first, q, count, results): called once per batch with the index
    of its first frame and the device tensors.

    references, polarity: the reference times the events are warped to (names
    among start, middle, end, or a mask) and whether ON and OFF events get
    images of their own (IWE_SPEC sections 8-13).  With anything but the
    defaults a batch makes one ``eval.iwe_splat_multi`` call in place of the
    count image and the splat, and every frame has R C rows, in image order
    m = (f R + r) C + c (``eval.iwe_image_names``); the observer gets the
    tensors of the batch's images."""
    from .loss import contrast_reference_mask
    mask, polarity = contrast_reference_mask(references), bool(polarity)
    multi = mask != 1 or polarity
    out = []
    for b0, pred, collated, (h, w) in _warped_event_batches('flow_warp_loss', of, sequence, frames, box, batch_size):
        ev = collated.events
        if multi:
            q, count = dev_eval.iwe_splat_multi(ev, collated.win_out, collated.timestamps, pred, mask, polarity)
        else:
            count = dev_eval.count_image_batched(ev['x'], ev['y'], collated.win_out, (h, w),
                                                 (0, 0, h, w))
            q = dev_eval.iwe_splat(ev, collated.win_out, collated.timestamps, pred)
        res = dev_eval.iwe_stats(q, count)
        out.append(dev_eval.read_iwe_results(res))      # the batch's one copy back
        if observer is not None:
            observer(b0, q, count, res)
    return np.concatenate(out) if out else np.zeros(0, dev_eval.IWE_RESULT_DTYPE)


def event_alignment(of, sequence, frames, box=None, batch_size=8, observer=None, references=('start',),
                    polarity=False):
    """``flow_warp_loss`` and, from the same splat, the statistics of the
    average-timestamp images of the warped events (docs/IWE_SPEC.md sections
    14-21) -> (IWE rows, average-timestamp rows): numpy structured arrays
    (eval.IWE_RESULT_DTYPE, loss.AVG_TIMESTAMP_ROW_DTYPE) with R C rows per
    frame, in image order; ``eval.derive_fwl`` and ``eval.derive_rsat`` make
    the two metrics of them.  The IWE rows are those of ``flow_warp_loss`` with
    the same arguments, bit for bit.  Per batch of frames: one
    ``of.flow_sequence``, one ``eval.iwe_avg_timestamp`` (in place of the count
    image and the splat), one ``eval.iwe_stats`` on its q and count, and two
    copies back, of 48 and of 32 bytes per image.

    The arguments of ``flow_warp_loss``;
    observer(first, images, iwe_results, avg_rows): called once per batch with
    the index of its first frame and the device tensors, images = (q, s, base,
    count)."""
    from .loss import AVG_TIMESTAMP_ROW_DTYPE, contrast_reference_mask
    mask, polarity = contrast_reference_mask(references), bool(polarity)
    iwe, avg = [], []
    for b0, pred, collated, _ in _warped_event_batches('event_alignment', of, sequence, frames, box, batch_size):
        images, rows = dev_eval.iwe_avg_timestamp(collated.events, collated.win_out, collated.timestamps, pred,
                                                  mask, polarity)
        res = dev_eval.iwe_stats(images[0], images[3])
        iwe.append(dev_eval.read_iwe_results(res))          # the batch's two copies back
        avg.append(dev_eval.read_avg_timestamp_rows(rows))
        if observer is not None:
            observer(b0, images, res, rows)
    if not iwe:
        return np.zeros(0, dev_eval.IWE_RESULT_DTYPE), np.zeros(0, AVG_TIMESTAMP_ROW_DTYPE)
    return np.concatenate(iwe), np.concatenate(avg)


def _warped_event_batches(name, of, sequence, frames, box, batch_size):
    """The batch loop ``flow_warp_loss`` and ``event_alignment`` share: yields
    (index of the batch's first frame, pred float32 [F,2,h,w], the collated
    events, (h, w)) after one ``of.flow_sequence`` per batch of frames."""
    from .sequence import EventSequence, check_box
    if not isinstance(sequence, EventSequence):
        raise TypeError(f'{name} takes a sequence.EventSequence (the events stay on '
                        f'the device), not {type(sequence).__name__}')
    if not hasattr(of, 'flow_sequence'):
        raise TypeError(f'{name} needs an `of` with flow_sequence (OpticalFlow)')
    if box is not None:
        box = check_box(box, sequence.shape)
    frames = np.array(frames, dtype=np.float64)
    if frames.size == 0:
        return
    frames = frames.reshape(-1, 2)
    batch_size = max(int(batch_size), 1)
    for b0 in range(0, len(frames), batch_size):
        fr = frames[b0:b0 + batch_size]
        pred, collated = of.flow_sequence(sequence, list(fr[:, 0]), list(fr[:, 1]), box=box,
                                          return_events=True)
        pred = pred.to(torch.float32).contiguous()
        h, w = pred.shape[-2:]
        eh, ew = box[2:] if box is not None else sequence.shape
        if (eh, ew) != (h, w):
            raise ValueError(f'the flow is {(h, w)}, the events cover {(eh, ew)}')
        yield b0, pred, collated, (h, w)


def summarize(rows):
    """Per-frame result rows -> (running mean AEE, running mean share under
    3 px) float64 [F]: sums in frame order, so that a NaN (a frame without a
    counted pixel) spoils the mean from there on, as it does in the
    reference.  The last entries are what ``evaluate`` returns."""
    aee, percent = dev_eval.derive(rows)
    count = np.arange(1, len(rows) + 1)
    return np.cumsum(aee) / count, np.cumsum(percent) / count


def evaluate(of, events, frames, gt, event_preproc_fun=None,
             pred_postproc_fun=None, gt_proc_fun=None, is_car=False,
             log=False, batch_size=8):
    """Quality of the optical flow ``of`` on a sequence: (mean AEE, mean share
    of pixels with an endpoint error under 3 px) over the frames, like the
    reference's ``evaluate``.

    of: ``OpticalFlow`` (its ``flow_device`` keeps the flow on the device) or
    any callable with the reference contract (events, start, stop) -> numpy
    [B,H,W,2]; events: [x, y, t, p] sorted by t, or a
    ``sequence.EventSequence`` of them (device-resident: see
    ``evaluate_frames``); frames: [(start, stop)];
    gt: dict with 'timestamps', 'x_flow_dist', 'y_flow_dist'.  The three
    optional functions pre-/post-process events [n,4], predicted flow [H,W,2]
    and ground-truth flow [H,W,2]; box crops (objects with ``.box``) are
    folded into the kernels.  batch_size: frames per launch (the reference
    runs one)."""
    rows = evaluate_frames(of, events, frames, gt, event_preproc_fun,
                           pred_postproc_fun, gt_proc_fun, is_car, batch_size)
    if len(rows) == 0:
        raise ValueError('evaluate needs at least one frame')
    mean_aee, mean_percent = summarize(rows)
    if log:
        count = np.arange(1, len(rows) + 1)
        mean_max = np.cumsum(rows['pred_max'], dtype=np.float64) / count
        mean_min = np.cumsum(rows['pred_min'], dtype=np.float64) / count
        for k in range(99, len(rows), 100):
            print(f'[{k + 1} frames] AEE {mean_aee[k]:.2f}  share under 3 px '
                  f'{mean_percent[k]:.2f}  points in the last frame '
                  f'{rows["n_points"][k]}  flow range {mean_min[k]:.2f} .. '
                  f'{mean_max[k]:.2f} (means over the frames so far)')
        print(f'done: {len(rows)} frames, AEE {mean_aee[-1]:.6f}, '
              f'share under 3 px {mean_percent[-1]:.6f}')
    return float(mean_aee[-1]), float(mean_percent[-1])
