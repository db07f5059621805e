"""Event sequences that live on the device (HIP, csrc/sequence.hip; arithmetic
in docs/SEQUENCE_SPEC.md).

A recording is uploaded ONCE (int16 x / y, float64 t, int8 p: 13 B/event);
every batch after that is a table of windows -- a few hundred bytes -- and one
``dvsof_event_windows`` launch that writes the wire-format columns.

  ``EventSequence``   the events of a recording; ``frame_ranges`` is
                      ``frame_generator``'s rule (utils/data.py:139-152),
                      ``collate`` what ``OpticalFlow._collate`` makes of the
                      host-sliced, host-cropped frames (DummyNet/of.py:76-115)
  ``FrameSequence``   ... plus its images and their timestamps: the per-frame
                      dataset of the reference ({events, image1, image2, start,
                      stop} files, utils/dataset.py:647-662) as one object
  ``SequenceLoader``  wire-format training batches from it: the rules of
                      ``DatasetImpl.__getitem__`` (is_raw, static sequence
                      length, aligned timestamps; utils/dataset.py:671-796) and
                      ``collate_wrapper`` (:961-1020), then the device
                      augmentation (augment.augment_batch)

Planning (which events, which images, which origin) is numpy on the host and
needs no GPU; only the launch does.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .eval import check_in_frame

EVENT_KEYS = ('x', 'y', 'timestamp', 'polarity', 'element_index',
              'sample_index')
_OUT_DTYPES = {k: (torch.float32 if k == 'timestamp' else torch.long)
               for k in EVENT_KEYS}
_TORCH = {np.dtype(np.int64): torch.int64, np.dtype(np.float64): torch.float64,
          np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}
MAX_SIDE = 32767        # int16 coordinates


def check_box(box, shape):
    """(y0, x0, h, w) inside the frame as ints; None -> (0, 0, 0, 0), the
    kernel's "no crop"."""
    if box is None:
        return 0, 0, 0, 0
    y0, x0, h, w = (int(b) for b in box)
    H, W = int(shape[0]), int(shape[1])
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > H or x0 + w > W:
        raise ValueError(f'crop box {(y0, x0, h, w)} outside the frame {(H, W)}')
    return y0, x0, h, w


def check_window_table(n_events, win_begin, win_end, win_out=None):
    """The window table as the kernel reads it, validated while it is still a
    host array: 0 <= begin <= end <= n_events, win_out the prefix sum of the
    lengths (built when None).  -> begin int64[W], end int64[W],
    win_out int64[W+1]."""
    begin = np.ascontiguousarray(win_begin, dtype=np.int64).reshape(-1)
    end = np.ascontiguousarray(win_end, dtype=np.int64).reshape(-1)
    if begin.shape != end.shape:
        raise ValueError('win_begin and win_end differ in length')
    if begin.size and (begin.min() < 0 or (begin > end).any() or
                       end.max() > n_events):
        raise ValueError('window table: 0 <= begin <= end <= '
                         f'{n_events} does not hold')
    prefix = np.zeros(begin.size + 1, np.int64)
    np.cumsum(end - begin, out=prefix[1:])
    if win_out is None:
        return begin, end, prefix
    out = np.ascontiguousarray(win_out, dtype=np.int64).reshape(-1)
    if out.shape != prefix.shape or (out != prefix).any():
        raise ValueError('window table: win_out is not the prefix sum of the '
                         'window lengths')
    return begin, end, out


def _pack(arrays, device):
    """Host arrays -> device views of ONE uploaded byte buffer (every part
    starts on an 8-byte boundary)."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    raw, offsets = bytearray(), []
    for a in arrays:
        offsets.append(len(raw))
        raw += a.tobytes()
        raw += b'\0' * ((-len(raw)) % 8)
    if not raw:
        raw = bytearray(8)
    buf = torch.frombuffer(raw, dtype=torch.uint8).to(device)
    return [buf[o:o + a.nbytes].view(_TORCH[a.dtype]).reshape(a.shape)
            for o, a in zip(offsets, arrays)]


def _output_columns(capacity, out, device):
    if out is None:
        return {k: torch.empty(capacity, dtype=_OUT_DTYPES[k], device=device)
                for k in EVENT_KEYS}
    for k in EVENT_KEYS:
        v = out[k]
        if v.dtype != _OUT_DTYPES[k] or v.dim() != 1 or not v.is_contiguous() \
                or v.numel() < capacity or v.device != device:
            raise ValueError(f"out['{k}'] must be a contiguous {_OUT_DTYPES[k]} "
                             f'column of at least {capacity} slots on {device}')
    return {k: out[k] for k in EVENT_KEYS}


class EventSequence:
    """events = [x, y, t, p] sorted by t (the form ``evaluate`` takes);
    shape = (H, W) of the sensor.  The columns are uploaded once; ``t`` stays
    on the host as float64 too, for ``np.searchsorted`` only."""

    def __init__(self, events, shape, device='cuda'):
        x, y, t, p = (np.asarray(c).reshape(-1) for c in events[:4])
        if not (x.size == y.size == t.size == p.size):
            raise ValueError('event columns differ in length')
        H, W = int(shape[0]), int(shape[1])
        if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
            raise ValueError(f'frame sides lie in 1..{MAX_SIDE}, not {(H, W)}')
        t = np.ascontiguousarray(t, dtype=np.float64)
        if not np.isfinite(t).all() or (np.diff(t) < 0).any():
            raise ValueError('event timestamps are not sorted (or not finite)')
        xi, yi = x.astype(np.int64), y.astype(np.int64)
        check_in_frame(xi, yi, (H, W))
        if not np.isin(p, (-1, 0, 1)).all():
            raise ValueError('event polarities lie in {-1, 0, +1}')
        self.shape = (H, W)
        self.t = t
        self.n_events = int(t.size)
        self.x = torch.from_numpy(xi.astype(np.int16)).to(device)
        self.device = self.x.device     # with its index: 'cuda' -> 'cuda:0'
        self.y = torch.from_numpy(yi.astype(np.int16)).to(self.device)
        self.t_dev = torch.from_numpy(t).to(self.device)
        self.p = torch.from_numpy(p.astype(np.int64).astype(np.int8)).to(self.device)

    def __len__(self):
        return self.n_events

    def frame_ranges(self, frames):
        """frames: (start, stop) pairs -> int64 [F,2] event index ranges; a
        frame holds the events with start < t <= stop."""
        frames = np.asarray(frames).reshape(-1, 2)
        return np.searchsorted(self.t, frames, side='right').astype(np.int64) \
            .reshape(-1, 2)

    def windows(self, win_begin, win_end, win_origin, win_sample, win_element,
                win_out=None, box=None, capacity=None, out=None, extra=()):
        """One ``dvsof_event_windows`` launch over a host window table.
        -> (events dict of device columns with ``capacity`` slots, win_out on
        the device, the device views of the ``extra`` host arrays, which ride
        in the table's upload, the six table columns on the device).
        capacity: default n_out (``out``'s size when ``out`` is given); out:
        caller-owned columns to write into."""
        begin, end, prefix = check_window_table(self.n_events, win_begin,
                                                win_end, win_out)
        W = begin.size
        y0, x0, h, w = check_box(box, self.shape)
        origin = np.ascontiguousarray(win_origin, dtype=np.float64).reshape(-1)
        sample = np.ascontiguousarray(win_sample, dtype=np.int32).reshape(-1)
        element = np.ascontiguousarray(win_element, dtype=np.int32).reshape(-1)
        if not (origin.size == sample.size == element.size == W):
            raise ValueError('window table columns differ in length')
        n_out = int(prefix[-1])
        if capacity is None:
            capacity = n_out if out is None else int(out['x'].numel())
        capacity = int(capacity)
        if capacity < n_out:
            raise ValueError(f'capacity {capacity} < {n_out} events')
        cols = _output_columns(capacity, out, self.device)
        views = _pack([begin, end, prefix, origin, sample, element, *extra],
                      self.device)
        self.launch(views[:6], (y0, x0, h, w), cols, n_out, capacity)
        return cols, views[2], views[6:], views[:6]

    def launch(self, table, box, cols, n_out, capacity):
        """The C ABI call alone, nothing but device addresses in (what a
        stream capture may hold).  table: the device columns win_begin,
        win_end, win_out, win_origin, win_sample, win_element of a VALIDATED
        host table; box: (y0, x0, h, w), zeros for none; cols: the six output
        columns."""
        if not capacity:
            return
        _lib.require_cuda(self.x, *table, *cols.values())
        tb, te, to, tor, tsa, tel = table
        rc = _lib.lib().dvsof_event_windows(
            self.x.data_ptr(), self.y.data_ptr(), self.t_dev.data_ptr(),
            self.p.data_ptr(), self.n_events, tb.data_ptr(), te.data_ptr(),
            to.data_ptr(), tor.data_ptr(), tsa.data_ptr(), tel.data_ptr(),
            tb.numel(), box[0], box[1], box[2], box[3], cols['x'].data_ptr(),
            cols['y'].data_ptr(), cols['timestamp'].data_ptr(),
            cols['polarity'].data_ptr(), cols['sample_index'].data_ptr(),
            cols['element_index'].data_ptr(), n_out, capacity, _lib.stream())
        _lib.check(rc, 'dvsof_event_windows')

    def collate_frames(self, starts, stops, box=None, capacity=None, out=None,
                       buffers=None):
        """``collate`` with what its consumers need besides: a namespace with
        events, timestamps, sample_idx, win_out (device int64[F+1]: the first
        slot of every frame) and n_out.  buffers: a callable
        n_out -> (capacity, out), for a caller whose static columns depend on
        the event count (the frames are looked up once)."""
        starts = np.asarray(starts, dtype=np.float64).reshape(-1)
        stops = np.asarray(stops, dtype=np.float64).reshape(-1)
        F = starts.size
        assert stops.size == F
        ranges = self.frame_ranges(np.stack([starts, stops], 1))
        begin = ranges[:, 0]
        end = np.maximum(ranges[:, 1], begin)       # stop < start: an empty slice
        if buffers is not None:
            capacity, out = buffers(int((end - begin).sum()))
        timestamps = np.stack([starts, stops], 1).reshape(-1)
        min_t = timestamps.min() if F else 0.0
        sample_idx = np.repeat(np.arange(F, dtype=np.int64), 2)
        cols, win_out, (ts, sidx), _ = self.windows(
            begin, end, np.full(F, min_t), np.arange(F), np.zeros(F), box=box,
            capacity=capacity, out=out,
            extra=((timestamps - min_t).astype(np.float32), sample_idx))
        return SimpleNamespace(events=cols, timestamps=ts, sample_idx=sidx,
                               win_out=win_out,
                               n_out=int((end - begin).sum()))

    def collate(self, starts, stops, box=None, capacity=None, out=None):
        """The frames (start_i, stop_i] as one wire-format batch on the device
        -> (events dict, timestamps float32[2F], sample_idx int64[2F]): what
        ``OpticalFlow._collate`` returns for the host-sliced events of the
        same frames, with the events outside ``box`` = (y0, x0, h, w) kept in
        their slots as x = y = -1 instead of removed.  Times are relative to
        the smallest start / stop; element_index is 0, sample_index the frame
        number.  capacity > the event count pads (x = y = -1); out: static
        columns to write into (the graph path)."""
        c = self.collate_frames(starts, stops, box, capacity, out)
        return c.events, c.timestamps, c.sample_idx


class FrameSequence(EventSequence):
    """An ``EventSequence`` plus the n+1 images around its n samples (uint8
    [n+1,H,W]) and their float64 timestamps.  Sample i is the interval
    image_ts[i] .. image_ts[i+1] with the events
    [frame_event_begin[i], frame_event_begin[i+1])."""

    def __init__(self, events, images, image_ts, frame_event_begin=None,
                 device='cuda'):
        images = np.asarray(images)
        if images.ndim != 3 or images.dtype != np.uint8:
            raise ValueError('images are uint8 [n+1,H,W]')
        super().__init__(events, images.shape[-2:], device)
        image_ts = np.ascontiguousarray(image_ts, dtype=np.float64).reshape(-1)
        if image_ts.size != images.shape[0] or image_ts.size < 2:
            raise ValueError('one timestamp per image, at least two images')
        if (np.diff(image_ts) < 0).any():
            raise ValueError('image timestamps are not sorted')
        if frame_event_begin is None:
            feb = np.searchsorted(self.t, image_ts, side='right')
        else:
            feb = np.asarray(frame_event_begin)
        feb = np.ascontiguousarray(feb, dtype=np.int64).reshape(-1)
        if feb.size != image_ts.size or (np.diff(feb) < 0).any() or \
                feb[0] < 0 or feb[-1] > self.n_events:
            raise ValueError('frame_event_begin: n+1 ascending event indices '
                             f'within 0..{self.n_events}')
        self.image_ts = image_ts
        self.frame_event_begin = feb
        self.images = torch.from_numpy(np.ascontiguousarray(images)).to(self.device)
        self.image_ts_dev = torch.from_numpy(image_ts).to(self.device)

    @property
    def n_samples(self):
        return self.image_ts.size - 1

    @classmethod
    def from_samples(cls, samples, device='cuda'):
        """samples: consecutive {events [m,4] = x, y, t, p; image1; image2;
        start; stop} dicts, the content of the reference's per-frame files;
        every sample starts where the one before stops
        (utils/dataset.py:657)."""
        samples = list(samples)
        assert samples, 'no samples'
        events, images, ts, counts = [], [], [], []
        for i, s in enumerate(samples):
            start, stop = float(np.asarray(s['start'])), float(np.asarray(s['stop']))
            if i == 0:
                images.append(np.asarray(s['image1']))
                ts.append(start)
            else:
                assert ts[-1] == start, \
                    f'sample {i} starts at {start}, sample {i - 1} stops at {ts[-1]}'
            images.append(np.asarray(s['image2']))
            ts.append(stop)
            e = np.asarray(s['events']).reshape(-1, 4)
            events.append(e)
            counts.append(len(e))
        events = np.concatenate(events)
        feb = np.concatenate([[0], np.cumsum(counts)])
        return cls([events[:, c] for c in range(4)], np.stack(images), ts, feb,
                   device)

    @classmethod
    def from_directory(cls, path, device='cuda'):
        """The reference's per-frame dataset: ``<number>.hdf5`` files in
        numeric order (utils/dataset.py:617-618, 647-662)."""
        from pathlib import Path
        from . import hdf5io
        files = sorted(Path(path).glob('*.hdf5'), key=lambda f: int(f.stem))
        assert files, f'No hdf5 files found in {path}'

        def read(file):
            with hdf5io.File(file, 'r') as f:
                return {k: np.array(f[k][...])
                        for k in ('events', 'image1', 'image2', 'start', 'stop')}
        return cls.from_samples((read(f) for f in files), device)


def central_box(in_shape, out_shape):
    """Central crop (utils/data.py:14-21, 96-99) as (y0, x0, h, w)."""
    return [(int(i) - int(o)) // 2 for i, o in zip(in_shape, out_shape)] + \
        [int(out_shape[0]), int(out_shape[1])]


class SequenceLoader:
    """Training batches in the wire format straight from a ``FrameSequence``:
    an iterable for ``training.train``.

    Per sample the rules of ``DatasetImpl.__getitem__`` with is_raw=True,
    is_static_seq_length=True, is_align=True: the sample at ``idx`` with
    collapse length k is ``seq_length`` elements of k consecutive recorded
    samples each; element i carries element_index i, the images are
    idx + i*k for i = 0..seq_length, and all times are relative to
    image_ts[idx] (float64 subtraction, then float32).  The whole batch is one
    window-kernel launch and one ``index_select`` of the resident images;
    flip / rotation / crop follow on the device.

    shape: (h, w) of the crop; augmentation: draw k, flip, angle and crop
    corner at random (off: k = 1, no flip, angle 0, central crop); rng:
    numpy Generator; steps: batches per iteration (None: one pass over a
    permutation of the samples; incomplete batches are dropped)."""

    def __init__(self, seq, shape, batch_size, augmentation=False,
                 collapse_length=6, seq_length=1, angle=30, rng=None,
                 steps=None):
        assert isinstance(seq, FrameSequence)
        assert seq_length >= 1 and collapse_length >= 1 and batch_size >= 1
        self.seq, self.shape = seq, (int(shape[0]), int(shape[1]))
        self.batch_size, self.augmentation = int(batch_size), bool(augmentation)
        self.collapse_length, self.seq_length = int(collapse_length), int(seq_length)
        self.angle, self.steps = angle, steps
        self.rng = np.random.default_rng() if rng is None else rng
        check_box(central_box(seq.shape, self.shape), seq.shape)
        if self.num_samples < self.batch_size:
            raise ValueError(f'{self.num_samples} samples do not fill a batch '
                             f'of {self.batch_size}')

    @property
    def num_samples(self):          # DatasetImpl.__len__, static sequence length
        return self.seq.n_samples - self.seq_length + 1

    def __len__(self):
        if self.steps is not None:
            return int(self.steps)
        return self.num_samples // self.batch_size

    def draw_k(self, idx):
        """Collapse length of the sample at idx (utils/dataset.py:703-710)."""
        if not self.augmentation:
            return 1
        max_k = (self.seq.n_samples - int(idx)) // self.seq_length
        return int(self.rng.integers(min(self.collapse_length, max_k))) + 1

    def plan(self, idx, k):
        """Host side of a batch: idx, k int[B] -> dict of the window table
        (win_begin, win_end, win_origin, win_sample, win_element:
        B * seq_length windows, sample-major), image_index
        [B * (seq_length + 1)], timestamps float32 and sample_idx int64 of
        the images."""
        s, L = self.seq, self.seq_length
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        k = np.asarray(k, dtype=np.int64).reshape(-1)
        B = idx.size
        assert k.size == B
        assert (idx >= 0).all() and (k >= 1).all()
        assert (idx + k * L <= s.n_samples).all(), \
            'idx + collapse_length * seq_length exceeds the sequence'
        first = idx[:, None] + np.arange(L)[None, :] * k[:, None]       # [B,L]
        image_index = idx[:, None] + np.arange(L + 1)[None, :] * k[:, None]
        origin = s.image_ts[idx]
        return dict(
            win_begin=s.frame_event_begin[first].reshape(-1),
            win_end=s.frame_event_begin[first + k[:, None]].reshape(-1),
            win_origin=np.repeat(origin, L),
            win_sample=np.repeat(np.arange(B, dtype=np.int32), L),
            win_element=np.tile(np.arange(L, dtype=np.int32), B),
            image_index=image_index.reshape(-1),
            timestamps=(s.image_ts[image_index] - origin[:, None])
            .astype(np.float32).reshape(-1),
            sample_idx=np.repeat(np.arange(B, dtype=np.int64), L + 1))

    def batch(self, idx, k, is_flip, angle, box):
        """One batch from explicit per-sample parameters (idx, k int[B];
        is_flip bool[B]; angle float[B], degrees; box int[B,4])."""
        from .augment import augment_batch
        s = self.seq
        pl = self.plan(idx, k)
        B = np.asarray(idx).size
        cols, _, (img, ts, sidx), _ = s.windows(
            pl['win_begin'], pl['win_end'], pl['win_origin'], pl['win_sample'],
            pl['win_element'],
            extra=(pl['image_index'], pl['timestamps'], pl['sample_idx']))
        raw = {'events': cols, 'timestamps': ts, 'sample_idx': sidx,
               'images': s.images.index_select(0, img)[:, None],
               'augmentation_params': {
                   'idx': torch.from_numpy(np.asarray(idx, np.int64).reshape(-1).copy()),
                   'sequence_length': torch.full((B,), self.seq_length, dtype=torch.long),
                   'collapse_length': torch.from_numpy(np.asarray(k, np.int64).reshape(-1).copy())},
               'size': B}
        return augment_batch(raw, is_flip, angle, box, device=s.device)

    def draw_params(self, idx):
        """The host-side draws of one batch, in the order the generator is
        consumed -> (k, is_flip, angle, box)."""
        from .augment import random_params
        B = len(idx)
        k = [self.draw_k(i) for i in idx]
        if self.augmentation:
            is_flip, angle, box = random_params(B, self.seq.shape, self.shape,
                                                self.angle, self.rng)
        else:
            is_flip, angle = np.zeros(B, bool), np.zeros(B)
            box = np.tile(central_box(self.seq.shape, self.shape), (B, 1))
        return k, is_flip, angle, box

    def draw_batch(self, idx):
        """idx int[B] -> a batch with the per-sample parameters drawn (or,
        without augmentation, fixed) as the reference does."""
        return self.batch(idx, *self.draw_params(idx))

    # ---- position in the stream (docs/CHECKPOINT_SPEC.md) ---------------
    def state(self):
        """Where the stream stands: the generator's state at the start of the
        current permutation and the batches drawn from it since.  Plain ints,
        strings and dicts: loads under ``torch.load(weights_only=True)``."""
        if getattr(self, '_perm_state', None) is None:
            return {'rng': self.rng.bit_generator.state, 'drawn': 0}
        return {'rng': self._perm_state, 'drawn': int(self._drawn)}

    def restore(self, state):
        """The next iteration continues the stream ``state`` was taken from:
        the permutation and the draws of the batches already handed out are
        repeated on the host and discarded, nothing is launched."""
        self._resume = {'rng': state['rng'], 'drawn': int(state['drawn'])}
        self._perm_state = None

    def __iter__(self):
        B, done = self.batch_size, 0
        resume, self._resume = getattr(self, '_resume', None), None
        if resume is not None:
            self.rng.bit_generator.state = resume['rng']
        while True:
            self._perm_state, self._drawn = self.rng.bit_generator.state, 0
            order = self.rng.permutation(self.num_samples)
            for b0 in range(0, order.size - B + 1, B):
                if resume is not None and self._drawn < resume['drawn']:
                    self.draw_params(order[b0:b0 + B])
                    self._drawn += 1
                    continue
                if self.steps is not None and done >= self.steps:
                    return
                idx = order[b0:b0 + B]
                params = self.draw_params(idx)
                self._drawn += 1        # drawn: state() now belongs to this batch
                yield self.batch(idx, *params)
                done += 1
            resume = None
            if self.steps is None:
                return


# ---------------------------------------------------------------------------
# Recordings without frames (docs/FRAMELESS_SPEC.md)
# ---------------------------------------------------------------------------
RECORDING_KEYS = ('x', 'y', 't', 'p', 'shape')


class WindowedEvents(EventSequence):
    """An ``EventSequence`` plus n + 1 ascending window boundaries (float64):
    a recording that has no frames, cut into n samples.  Sample i is the
    interval image_ts[i] .. image_ts[i+1] with the events
    [frame_event_begin[i], frame_event_begin[i+1]) -- the names and the
    meaning ``FrameSequence`` gives them, so that what needs only those
    (``hooks.sharpness_frames``, ``testing.flow_warp_loss``) takes either.
    There are no ``images``.

    frame_event_begin None: ``np.searchsorted(t, boundaries, side='right')``,
    ``FrameSequence``'s rule: a window holds the events with
    start < t <= stop."""

    def __init__(self, events, shape, boundaries, frame_event_begin=None,
                 device='cuda'):
        super().__init__(events, shape, device)
        ts = np.ascontiguousarray(boundaries, dtype=np.float64).reshape(-1)
        if ts.size < 2:
            raise ValueError('a windowed recording needs at least two window '
                             f'boundaries (one window), got {ts.size}')
        if not np.isfinite(ts).all() or (np.diff(ts) < 0).any():
            raise ValueError('window boundaries are not sorted (or not finite)')
        if frame_event_begin is None:
            feb = np.searchsorted(self.t, ts, side='right')
        else:
            feb = np.asarray(frame_event_begin)
        feb = np.ascontiguousarray(feb, dtype=np.int64).reshape(-1)
        if feb.size != ts.size or (np.diff(feb) < 0).any() or \
                feb[0] < 0 or feb[-1] > self.n_events:
            raise ValueError('frame_event_begin: n+1 ascending event indices '
                             f'within 0..{self.n_events}')
        self.image_ts = ts
        self.frame_event_begin = feb

    @property
    def n_samples(self):
        return self.image_ts.size - 1

    @classmethod
    def cut(cls, events, shape, boundaries=None, duration=None,
            events_per_window=None, device='cuda'):
        """Exactly one of
          boundaries         the n + 1 window boundaries themselves;
          duration           seconds: boundaries t[0] + i * duration (float64),
                             the last one the last that is not beyond the last
                             event;
          events_per_window  N: boundary i is the time of event i * N and
                             frame_event_begin[i] = i * N, given explicitly
                             (ties in t cannot move an event to its neighbour);
                             the events from the last boundary on belong to no
                             window.
        In the two time modes frame_event_begin is searchsorted(side='right')."""
        given = [v is not None for v in (boundaries, duration, events_per_window)]
        if sum(given) != 1:
            raise ValueError('exactly one of boundaries, duration and '
                             'events_per_window cuts a recording')
        if boundaries is not None:
            return cls(events, shape, boundaries, None, device)
        t = np.ascontiguousarray(np.asarray(events[2]).reshape(-1), dtype=np.float64)
        if duration is not None:
            duration = float(duration)
            if not (duration > 0 and np.isfinite(duration)):
                raise ValueError(f'the window duration is positive and finite, not {duration}')
            ts = np.zeros(0)
            if t.size and np.isfinite(t[0]) and np.isfinite(t[-1]) and t[-1] >= t[0]:
                m = int(np.floor((t[-1] - t[0]) / duration))
                ts = t[0] + np.arange(m + 2, dtype=np.float64) * duration
                ts = ts[ts <= t[-1]]
            return cls(events, shape, ts, None, device)
        N = int(events_per_window)
        if N < 1:
            raise ValueError(f'a window holds at least one event, not {events_per_window}')
        begin = np.arange(0, t.size, N, dtype=np.int64)
        return cls(events, shape, t[begin], begin, device)

    @classmethod
    def from_file(cls, path, duration=None, events_per_window=None,
                  boundaries=None, device='cuda'):
        """A recording in ONE file: ``.npz`` with the arrays x, y, t, p
        (one entry per event, sorted by t) and shape = (H, W) of the sensor,
        or ``.hdf5`` / ``.h5`` with datasets of the same names (read through
        ``hdf5io``).  A file that lacks one of them is refused, with the name
        in the message.  The window arguments are ``cut``'s."""
        from pathlib import Path
        path = Path(path)
        suffix = path.suffix.lower()

        def missing(have):
            lacks = [k for k in RECORDING_KEYS if k not in have]
            if lacks:
                raise ValueError(f'{path}: a recording holds the arrays '
                                 f'{", ".join(RECORDING_KEYS)}; missing: {", ".join(lacks)}')
        if suffix == '.npz':
            with np.load(str(path)) as data:
                missing(data.files)
                arrays = {k: np.asarray(data[k]) for k in RECORDING_KEYS}
        elif suffix in ('.hdf5', '.h5'):
            from . import hdf5io
            with hdf5io.File(path, 'r') as f:
                missing(list(f.keys()))
                arrays = {k: np.array(f[k][...]) for k in RECORDING_KEYS}
        else:
            raise ValueError(f'{path}: a recording is a .npz or a .hdf5 file')
        shape = np.asarray(arrays['shape']).reshape(-1)
        if shape.size != 2:
            raise ValueError(f'{path}: shape holds (H, W), not {shape.tolist()}')
        return cls.cut([arrays[k] for k in ('x', 'y', 't', 'p')],
                       (int(shape[0]), int(shape[1])), boundaries=boundaries,
                       duration=duration, events_per_window=events_per_window,
                       device=device)


class EventWindowLoader(SequenceLoader):
    """Frameless training batches in the wire format from a
    ``WindowedEvents``: ``SequenceLoader`` without its images.  The rules are
    that class's own code -- ``draw_k``, the window table of ``plan``, the order
    in which ``draw_params`` consumes the generator, ``state`` / ``restore``,
    the permutation and the dropped incomplete batch of ``__iter__`` -- so a
    recording cut at a ``FrameSequence``'s image timestamps gives that
    loader's events, timestamps and sample_idx.  What is not here: no
    ``image_index`` in the plan, no ``index_select`` of resident images, no
    frames kernel.  A batch carries ``'images': None`` and ``'shape': (h, w)``
    of the crop (docs/FRAMELESS_SPEC.md)."""

    def __init__(self, seq, shape, batch_size, augmentation=False,
                 collapse_length=6, seq_length=1, angle=30, rng=None,
                 steps=None):
        assert isinstance(seq, WindowedEvents)
        assert seq_length >= 1 and collapse_length >= 1 and batch_size >= 1
        self.seq, self.shape = seq, (int(shape[0]), int(shape[1]))
        self.batch_size, self.augmentation = int(batch_size), bool(augmentation)
        self.collapse_length, self.seq_length = int(collapse_length), int(seq_length)
        self.angle, self.steps = angle, steps
        self.rng = np.random.default_rng() if rng is None else rng
        check_box(central_box(seq.shape, self.shape), seq.shape)
        if self.num_samples < self.batch_size:
            raise ValueError(f'{self.num_samples} windows do not fill a batch '
                             f'of {self.batch_size}')

    def plan(self, idx, k):
        """``SequenceLoader.plan`` without ``image_index``: the window table,
        and timestamps float32 and sample_idx int64 of the B * (seq_length + 1)
        boundaries."""
        pl = super().plan(idx, k)
        del pl['image_index']
        return pl

    def batch(self, idx, k, is_flip, angle, box):
        """One frameless batch from explicit per-sample parameters (those of
        ``SequenceLoader.batch``)."""
        from .augment import augment_events_batch
        s = self.seq
        pl = self.plan(idx, k)
        B = np.asarray(idx).size
        cols, _, (ts, sidx), _ = s.windows(
            pl['win_begin'], pl['win_end'], pl['win_origin'], pl['win_sample'],
            pl['win_element'], extra=(pl['timestamps'], pl['sample_idx']))
        raw = {'events': cols, 'timestamps': ts, 'sample_idx': sidx,
               'images': None, 'shape': s.shape,
               'augmentation_params': {
                   'idx': torch.from_numpy(np.asarray(idx, np.int64).reshape(-1).copy()),
                   'sequence_length': torch.full((B,), self.seq_length, dtype=torch.long),
                   'collapse_length': torch.from_numpy(np.asarray(k, np.int64).reshape(-1).copy())},
               'size': B}
        return augment_events_batch(raw, is_flip, angle, box, s.shape, device=s.device)
