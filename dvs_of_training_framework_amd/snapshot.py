"""Device snapshot of a training state (csrc/snapshot.hip,
docs/CHECKPOINT_SPEC.md): every float32 tensor of the model's and the
optimizer's state dicts leaves the device through ONE gather launch into a
device slab and ONE device-to-host copy into a pinned slab.  The training
thread only enqueues; whoever wants the values (serializer.Serializer's writer
thread) waits on the ticket's event and rebuilds the tensors on the host.

PyTorch is plumbing here: memory, streams, events.
"""
import copy

import torch

from . import _lib

HEADER_FLOATS = _lib.CONSTANTS['DVSOF_SNAPSHOT_HEADER_BYTES'] // 4
ALIGN_FLOATS = 4        # destination offsets are multiples of 16 bytes


def _as_int64(x):
    return x - (1 << 64) if x >= (1 << 63) else x


def _dense(t):
    """Dense, non-overlapping storage of exactly numel elements."""
    if t.is_contiguous() or (t.dim() == 4 and
                             t.is_contiguous(memory_format=torch.channels_last)):
        return True
    order = sorted(range(t.dim()), key=lambda d: (t.stride(d), t.size(d)))
    run = 1
    for d in order:
        if t.size(d) == 1:
            continue
        if t.stride(d) != run:
            return False
        run *= t.size(d)
    return True


def packable(t):
    return t.is_cuda and t.dtype == torch.float32 and not t.is_sparse and _dense(t)


class _Ref:
    """Stands for tensor ``index`` in a state structure taken apart."""
    __slots__ = ('index',)

    def __init__(self, index):
        self.index = index


def take_apart(obj, tensors):
    """A deep copy of ``obj`` (dicts, lists, tuples, plain values) with every
    tensor appended to ``tensors`` and replaced by a ``_Ref``: the copy can be
    handed to another thread while training goes on."""
    if torch.is_tensor(obj):
        tensors.append(obj.detach())
        return _Ref(len(tensors) - 1)
    if isinstance(obj, dict):
        return type(obj)((k, take_apart(v, tensors)) for k, v in obj.items())
    if isinstance(obj, (list, tuple)):
        return type(obj)(take_apart(v, tensors) for v in obj)
    return copy.deepcopy(obj)


def put_together(obj, tensors):
    if isinstance(obj, _Ref):
        return tensors[obj.index]
    if isinstance(obj, dict):
        return type(obj)((k, put_together(v, tensors)) for k, v in obj.items())
    if isinstance(obj, (list, tuple)):
        return type(obj)(put_together(v, tensors) for v in obj)
    return obj


def slab_layout(tensors):
    """-> (entries, index, total): the slab entries of ``tensors`` (packable
    ones), de-duplicated by (address, size, strides): ``entries[e]`` =
    (tensor, offset in floats from the slab's start), ``index[i]`` = the entry
    of tensors[i], ``total`` = floats of the slab, header included."""
    entries, index, seen = [], [], {}
    off = HEADER_FLOATS
    for t in tensors:
        key = (t.data_ptr(), tuple(t.shape), t.stride()) if t.numel() else None
        e = seen.get(key) if key is not None else None
        if e is None:
            e = len(entries)
            entries.append((t, off))
            off += -(-t.numel() // ALIGN_FLOATS) * ALIGN_FLOATS
            if key is not None:
                seen[key] = e
        index.append(e)
    return entries, index, off


class PackTables:
    """Device tables of one slab layout (the optimizers' (tensor, chunk) table,
    optim._FusedBase._table, with a destination offset per tensor)."""

    def __init__(self, entries, device):
        chunk = _lib.lib().dvsof_snapshot_chunk_elems()
        srcs, counts, offsets, items = [], [], [], []
        for t, (q, off) in enumerate(entries):
            assert packable(q), 'float32, dense device tensors only'
            assert off % ALIGN_FLOATS == 0 and off >= HEADER_FLOATS
            assert q.numel() == 0 or q.data_ptr() % 4 == 0
            srcs.append(_as_int64(q.data_ptr()))
            counts.append(q.numel())
            offsets.append(off)
            items += [(t, c) for c in range(-(-q.numel() // chunk))]
        self.num_items = len(items)
        self.key = tuple(srcs)
        if self.num_items:
            self.srcs = torch.tensor(srcs, dtype=torch.int64, device=device)
            self.counts = torch.tensor(counts, dtype=torch.int64, device=device)
            self.offsets = torch.tensor(offsets, dtype=torch.int64, device=device)
            self.items = torch.tensor(items, dtype=torch.int32, device=device)

    def launch(self, slab, parity):
        if not self.num_items:
            return 0
        rc = _lib.lib().dvsof_snapshot_pack(
            self.srcs.data_ptr(), self.counts.data_ptr(), self.offsets.data_ptr(),
            self.items.data_ptr(), self.num_items, slab.data_ptr(), parity,
            _lib.stream())
        _lib.check(rc, 'dvsof_snapshot_pack')
        return self.num_items


def pack(tensors, slab, parity=0):
    """Gather ``tensors`` into ``slab`` (float32 or int32 device tensor) on the
    current stream -> (entries, index, total floats).  For tests and tools;
    DeviceSnapshot keeps its tables."""
    entries, index, total = slab_layout(tensors)
    assert total <= slab.numel(), 'slab too small'
    PackTables(entries, slab.device).launch(slab, parity)
    return entries, index, total


class Ticket:
    """One snapshot on its way to the host."""

    def __init__(self, snap, structure, tensors, entries, index, total, parity,
                 others, launched):
        self.snap, self.structure = snap, structure
        self.meta = [(tuple(t.shape), t.stride()) for t in tensors]
        self.entry_of = index           # per tensor: slab entry or ('other', j)
        self.entry_off = [(off, q.numel()) for q, off in entries]
        self.total, self.parity = total, parity
        self.others, self.launched = others, launched
        self.copied = snap.copied

    def collect(self):
        """Wait for the copy (this is the only GPU call of the writer thread)
        -> (state structure of host tensors that own their storage, count of
        non-finite values)."""
        self.copied.synchronize()
        host = self.snap.host[:self.total]
        bad = int(host[:HEADER_FLOATS].view(torch.int32)[self.parity]) & 0xffffffff \
            if self.launched else 0
        built, out = {}, []
        for (size, stride), e in zip(self.meta, self.entry_of):
            if isinstance(e, tuple):
                t = self.others[e[1]]
                if t.is_floating_point():
                    bad += int((~torch.isfinite(t)).sum())
                out.append(t)
                continue
            if e not in built:
                off, n = self.entry_off[e]
                built[e] = host[off:off + n].clone().as_strided(size, stride)
            out.append(built[e])
        return put_together(self.structure, out), bad


class DeviceSnapshot:
    """One device slab, one pinned host slab, two events; regrown only when
    the state grows.  ``take`` must not be called while the host slab of the
    previous ticket is still being read (the serializer waits for its writer
    first: back-pressure)."""

    def __init__(self, device, copy_stream=None):
        from .feed import copy_stream as shared_copy_stream
        self.device = torch.device(device)
        self.stream = copy_stream or shared_copy_stream(self.device)
        self.dev = self.host = None
        self.tables = None
        self.parity = 0
        self.packed = torch.cuda.Event(enable_timing=True)
        self.copied = torch.cuda.Event(enable_timing=True)
        self.copy_start = torch.cuda.Event(enable_timing=True)
        self.pack_start = torch.cuda.Event(enable_timing=True)
        self.launches = 0
        self.table_builds = 0
        self.bytes = 0

    def _grow(self, total):
        if self.dev is not None and self.dev.numel() >= total:
            return
        # zeroed: the first launch adds into a header word nobody zeroed for it
        self.dev = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.host = torch.empty(total, dtype=torch.float32).pin_memory()
        self.parity = 0

    def take(self, state):
        """Enqueue the snapshot of ``state`` (any nesting of dicts / lists of
        tensors and plain values) behind everything the current stream holds
        -> Ticket.  Nothing here waits for the device."""
        tensors = []
        structure = take_apart(state, tensors)
        slab_t, where, others = [], [], []
        for t in tensors:
            if packable(t):
                where.append(len(slab_t))
                slab_t.append(t)
            else:
                where.append(('other', len(others)))
                others.append(t)
        entries, index, total = slab_layout(slab_t)
        self._grow(total)
        key = tuple(_as_int64(q.data_ptr()) for q, _ in entries)
        if self.tables is None or self.tables.key != key or \
                self.tables.total != total:
            self.tables = PackTables(entries, self.device)
            self.tables.total = total
            self.table_builds += 1
        main = torch.cuda.current_stream(self.device)
        # the device slab is reused only after the copy out of it
        if self.launches:
            main.wait_event(self.copied)
        parity = self.parity
        self.pack_start.record(main)
        launched = self.tables.launch(self.dev, parity)
        # what the kernel does not take (no such tensor in this project's models: other
        # dtypes, strided views) is cloned in stream order, the clone copied below
        others = [t.clone() for t in others]
        self.packed.record(main)
        if launched:
            self.parity ^= 1
        st = self.stream
        st.wait_event(self.packed)
        with torch.cuda.stream(st):
            self.copy_start.record(st)
            self.host[:total].copy_(self.dev[:total], non_blocking=True)
            moved = []
            for t in others:
                if t.is_cuda:
                    buf = torch.empty(t.shape, dtype=t.dtype).pin_memory()
                    buf.copy_(t, non_blocking=True)
                    t.record_stream(st)
                    moved.append(buf)
                else:
                    moved.append(t)
            self.copied.record(st)
        self.launches += 1
        self.bytes = 4 * total
        entry_of = [index[w] if not isinstance(w, tuple) else w for w in where]
        return Ticket(self, structure, tensors, entries, entry_of, total, parity,
                      moved, bool(launched))
