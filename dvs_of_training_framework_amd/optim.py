"""Fused optimizers on the HIP path (csrc/optim.hip).

``FusedAdamW`` is what ``construct_optimizer`` builds for ``--optimizer ADAM``
(reference train_flownet.py:57-75: ``torch.optim.AdamW(amsgrad=True)``).  It
keeps torch's state-dict schema (step, exp_avg, exp_avg_sq, max_exp_avg_sq)
so checkpoints interchange with the reference's (utils/serializer.py:60-110).
One kernel launch per parameter group updates every tensor of the group.

``set_guard`` puts a step under the STEP GUARD (docs/STEP_GUARD_SPEC.md): the
global gradient norm and the count of non-finite gradient elements are reduced
on the device at the head of ``step()``, the update kernels read the decision
from a 32-byte device record -- clip by a scale, or write nothing at all --
and the host never waits for it.
"""
import ctypes
import struct

import torch

from . import _lib

GUARD_FIELDS = ('scale', 'skip', 'norm', 'bad', 'skipped', 'clipped', 'consecutive')
_GUARD_STRUCT = '<fIdIIII'      # the record of include/dvsof.h
assert struct.calcsize(_GUARD_STRUCT) == _lib.CONSTANTS['DVSOF_GUARD_RECORD_BYTES']


class _FusedBase(torch.optim.Optimizer):
    """Shared machinery: per-group device tables of {param, grad, state...}
    pointers, element counts and (tensor, chunk) work items; the protocol of
    a step captured in a hipGraph (``begin_capture`` / ``advance`` /
    ``end_capture``: what changes per step travels in a device table)."""
    STATE = ()          # names of the 3 state tensors after param and grad

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._tables = {}
        self._guard = None      # set_guard: (max_norm, skip_nonfinite, record, [partials])
        self._guard_tables = None

    def _init_state(self, p, st):
        for name in self.STATE:
            st[name] = torch.zeros_like(p)

    def _state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st['step'] = 0
            self._init_state(p, st)
        return st

    def load_state_dict(self, state_dict):
        """torch's loader keeps the SAVED strides of state tensors; a state
        dict written by ``torch.optim.AdamW`` (the reference's optimizer, or a
        CPU run) holds contiguous moments while the conv weights here are
        channels_last.  The kernels index parameter, gradient and state with
        one offset, so state is re-laid to its parameter's strides."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for p in group['params']:
                st = self.state.get(p)
                if not st:
                    continue
                shared = {}     # RAdam aliases slow_buffer to exp_avg
                for name in self.STATE:
                    v = st.get(name)
                    if not torch.is_tensor(v):
                        continue
                    if id(v) in shared:
                        st[name] = shared[id(v)]
                        continue
                    if v.stride() != p.stride() or v.dtype != p.dtype or \
                            v.device != p.device:
                        st[name] = torch.empty_like(p).copy_(v)
                    shared[id(v)] = st[name]
                if torch.is_tensor(st.get('step')):
                    st['step'] = int(st['step'])
        self._tables = {}

    def _extra_table(self, group, plist):
        """A class's own device table for these tensors (cached and kept alive
        with the pointer tables); handed to ``_launch`` as ``tables[4]``."""
        return None

    def _table(self, gi, plist, group=None):
        """Device tables for group gi; rebuilt only when a pointer moved."""
        key = tuple((p.data_ptr(), p.grad.data_ptr()) for p in plist)
        cached = self._tables.get(gi)
        if cached is not None and cached[0] == key:
            return cached[1:]
        chunk = _lib.lib().dvsof_adamw_chunk_elems()
        ptrs, sizes, chunks = [], [], []
        for t, p in enumerate(plist):
            st = self._state(p)
            for q in (p, p.grad) + tuple(st[n] for n in self.STATE):
                assert q.dtype == torch.float32 and q.is_cuda
                assert q.stride() == p.stride(), \
                    'parameter, gradient and state must share one layout'
                ptrs.append(q.data_ptr())
            sizes.append(p.numel())
            chunks += [(t, c) for c in range((p.numel() + chunk - 1) // chunk)]
        dev = plist[0].device
        # uint64 pointers travel as int64 bit patterns
        t_ptrs = torch.tensor([_as_int64(x) for x in ptrs], dtype=torch.int64,
                              device=dev)
        t_sizes = torch.tensor(sizes, dtype=torch.int64, device=dev)
        t_chunks = torch.tensor(chunks, dtype=torch.int32, device=dev)
        self._tables[gi] = (key, t_ptrs, t_sizes, t_chunks, len(chunks),
                            self._extra_table(group, plist))
        return self._tables[gi][1:]

    def _launch(self, group, tables, step, plist):
        raise NotImplementedError

    def _step_params(self, key, group, plist, tables=None):
        _lib.require_cuda(*plist)
        for p in plist:
            assert _dense(p) and not p.grad.is_sparse
        steps = set()
        frozen = getattr(self, '_use_dyn', False)   # captured step: advance() counts
        for p in plist:
            st = self._state(p)
            if not frozen:
                st['step'] = int(st['step']) + 1
            steps.add(st['step'])
        assert len(steps) == 1, 'tensors of one group step together'
        if tables is None:
            tables = self._table(key, plist, group)
        self._launch(group, tables, max(steps.pop(), 1), plist)

    # ---- a step captured in a hipGraph (capture.CapturedTrainStep) ---------
    def _dyn_row(self, group, step, out4):
        """Fill the host float[4] of ``group`` at step count ``step``."""
        raise NotImplementedError

    def _dyn_ptr(self, group):
        gi = next(i for i, g in enumerate(self.param_groups) if g is group)
        return self._dyn[gi].data_ptr()

    def begin_capture(self, device):
        """From now on ``step()`` enqueues the dyn-table kernel and leaves the
        step counters alone (capturing enqueues nothing; ``advance`` counts).
        The table is allocated once: a captured graph keeps its address."""
        if getattr(self, '_dyn', None) is None:
            ng = len(self.param_groups)
            self._dyn = torch.zeros(ng, 4, dtype=torch.float32, device=device)
        self._use_dyn = True

    def advance(self):
        """Before every replay: count the step and refresh the row of every
        group (one tiny kernel carrying the values as arguments:
        dvsof_adamw_set_dynamic)."""
        ng = len(self.param_groups)
        buf, rows = (ctypes.c_float * 4)(), (ctypes.c_float * (4 * ng))()
        for gi, group in enumerate(self.param_groups):
            steps = set()
            for p in group['params']:
                st = self._state(p)
                st['step'] = int(st['step']) + 1
                steps.add(st['step'])
            assert len(steps) == 1
            self._dyn_row(group, steps.pop(), buf)
            rows[4 * gi:4 * gi + 4] = buf[:]
        _lib.check(_lib.lib().dvsof_adamw_set_dynamic(
            self._dyn.data_ptr(), rows, 4 * ng, _lib.stream()), 'dvsof_adamw_set_dynamic')

    def end_capture(self):
        """Back to eager steps (the table stays: a graph may still use it)."""
        self._use_dyn = False

    # ---- the step guard (docs/STEP_GUARD_SPEC.md) ---------------------------
    def set_guard(self, max_norm=None, skip_nonfinite=True):
        """Clip the global gradient norm of every step to ``max_norm`` (None:
        no clipping; ``torch.nn.utils.clip_grad_norm_`` semantics over ALL
        parameter groups) and, with ``skip_nonfinite``, write nothing in a
        step whose gradients hold a NaN or an Inf.  Decided on the device:
        ``step()`` enqueues the statistic and updates that obey it, and never
        waits.  Step counters, bias corrections, RAdam's rectification and the
        learning-rate schedule therefore advance on a skipped step like on any
        other; a Lookahead synchronisation that falls on a skipped step is
        missed and happens at the next multiple of ``k``.

        ``set_guard(None, False)`` removes the guard.  The record (and its
        counters) is made once and survives a change of the settings; it is
        not part of ``state_dict()``: counters are per run."""
        if max_norm is None and not skip_nonfinite:
            self._guard = None
            return
        if hasattr(self, 'fused_active'):
            raise ValueError('set_guard cannot be combined with fuse_into_backward: a bucket '
                             'updated during the backward cannot wait for the global gradient '
                             'norm of the step')
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError(f'max_norm must be positive (or None), got {max_norm}')
        max_norm = 0.0 if max_norm is None else float(max_norm)     # 0: the kernels do not clip
        dev = next(p.device for g in self.param_groups for p in g['params'])
        if self._guard is None:
            record = torch.zeros(struct.calcsize(_GUARD_STRUCT) // 8, dtype=torch.int64,
                                 device=dev)
            partials = [torch.zeros(0, dtype=torch.int64, device=dev)]
        else:
            record, partials = self._guard[2:]
        self._guard = (max_norm, bool(skip_nonfinite), record, partials)

    def guard_state(self):
        """The guard record as a dict (GUARD_FIELDS), by ONE 32-byte copy
        from the device (which waits for the work enqueued so far)."""
        assert self._guard is not None, 'no guard is set'
        raw = self._guard[2].cpu().numpy().tobytes()
        out = dict(zip(GUARD_FIELDS, struct.unpack(_GUARD_STRUCT, raw)))
        out['skip'] = bool(out['skip'])
        return out

    def guard_tensors(self):
        """Device tensors the guard's kernels point at (a captured step keeps
        them alive); empty without a guard."""
        if self._guard is None:
            return []
        keep = [self._guard[2], self._guard[3][0]]
        if self._guard_tables is not None:
            keep += list(self._guard_tables[1:4])
        return keep

    def _guard_reserve(self, num_chunks):
        """The partials workspace, grown EAGERLY: a recording takes its
        address, so it must not grow inside one."""
        partials = self._guard[3]
        need = num_chunks * _lib.lib().dvsof_grad_guard_partial_bytes()
        if partials[0].numel() * 8 < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('the step guard\'s workspace would have to grow inside a '
                                   'recording: run one eager step over these parameters first')
            partials[0] = torch.zeros(max(need // 8, 2 * partials[0].numel()),
                                      dtype=torch.int64, device=partials[0].device)
        return partials[0]

    def _enqueue_guard(self, work):
        """The statistic over ALL groups that step now: their tables
        concatenated (tensor ids offset), one norm, one decision.  Reads the
        raw gradients: before any centralisation."""
        tables = [self._table(key, plist, group) for key, group, plist in work]
        key = [t[0] for t in tables]    # (the tensors themselves: an address may be reused)
        cached = self._guard_tables
        if cached is None or len(cached[0]) != len(key) or \
                any(a is not b for a, b in zip(cached[0], key)):
            if len(tables) == 1:
                t_ptrs, t_sizes, t_chunks, n = tables[0][:4]
            elif tables:
                chunks, first = [], 0
                for t in tables:
                    c = t[2].reshape(-1, 2).clone()
                    c[:, 0] += first
                    chunks.append(c)
                    first += t[1].numel()
                t_ptrs = torch.cat([t[0] for t in tables])
                t_sizes = torch.cat([t[1] for t in tables])
                t_chunks = torch.cat(chunks)
                n = sum(t[3] for t in tables)
            else:
                t_ptrs = t_sizes = t_chunks = None
                n = 0
            cached = self._guard_tables = (key, t_ptrs, t_sizes, t_chunks, n)
        _, t_ptrs, t_sizes, t_chunks, n = cached
        max_norm, skip_nonfinite, record, _ = self._guard
        partials = self._guard_reserve(n)
        _lib.check(_lib.lib().dvsof_grad_guard(
            t_ptrs.data_ptr() + 8 if n else None, 5,
            t_sizes.data_ptr() if n else None, t_chunks.data_ptr() if n else None, n,
            partials.data_ptr() if n else None, partials.numel() * 8, max_norm,
            1 if skip_nonfinite else 0, record.data_ptr(), _lib.stream()),
            'dvsof_grad_guard')
        return tables

    def _guard_args(self, name):
        """(entry point, its name, trailing arguments) of an update launch:
        the guarded twin and the record when a guard is set."""
        if self._guard is None:
            return getattr(_lib.lib(), name), name, (_lib.stream(),)
        name += '_guarded'
        return getattr(_lib.lib(), name), name, (self._guard[2].data_ptr(), _lib.stream())

    # ---- update fused into the backward ------------------------------------
    def fuse_into_backward(self, predictor, flush_at=None):
        """Update the gradient buckets of ``predictor`` as soon as their
        gradients are final (after the all-reduce under data parallelism)
        instead of in ``step()``: the HBM-bound update then runs beside the
        MFMA-bound backward kernels.  Same arithmetic, same result; ``step()``
        still has to be called and updates whatever is left.  Set
        ``fused_active = False`` on micro-batches that only accumulate.

        flush_at: bucket indices at which everything collected so far is
        updated in ONE launch (None: one launch per bucket).  ``(5,)`` updates
        the decoder and residual parameters (82 % of the bytes) when the last
        residual weight gradient is done, beside the encoder's backward, and
        leaves the encoder buckets to ``step()``."""
        if self._guard is not None:
            raise ValueError('fuse_into_backward cannot be combined with set_guard: a bucket '
                             'updated during the backward cannot wait for the global gradient '
                             'norm of the step')
        self.fused_active = True
        self._flush_at = None if flush_at is None else set(flush_at)
        self._pending = []
        self._done = set()
        self._group_of = {id(p): (gi, g) for gi, g in enumerate(self.param_groups)
                          for p in g['params']}
        predictor.bucket_hook = self._on_bucket

    @torch.no_grad()
    def _on_bucket(self, b, params):
        if not getattr(self, 'fused_active', False):
            return
        if self._flush_at is not None:      # collect, update at the flush points
            self._pending += params
            if b not in self._flush_at:
                return
            params, self._pending = self._pending, []
        by_group = {}
        for p in params:
            if id(p) in self._group_of and p.grad is not None:
                gi, g = self._group_of[id(p)]
                by_group.setdefault(gi, (g, []))[1].append(p)
        for gi, (g, plist) in by_group.items():
            self._step_params((gi, b), g, plist)
            self._done.update(id(p) for p in plist)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        done = getattr(self, '_done', None)
        if getattr(self, '_pending', None):
            self._pending = []          # never flushed this step: step() takes them
        work = []
        for gi, group in enumerate(self.param_groups):
            plist = [p for p in group['params'] if p.grad is not None and
                     not (done and id(p) in done)]
            if plist:
                work.append((gi if not done else (gi, 'rest'), group, plist))
        tables = [None] * len(work)
        if self._guard is not None:
            tables = self._enqueue_guard(work)  # one decision for all groups; the updates obey it
        for (key, group, plist), t in zip(work, tables):
            self._step_params(key, group, plist, t)
        if done:
            done.clear()
        return loss


class FusedAdamW(_FusedBase):
    STATE = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=1e-2, amsgrad=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps,
                                      weight_decay=weight_decay,
                                      amsgrad=amsgrad))

    def _launch(self, group, tables, step, plist):
        t_ptrs, t_sizes, t_chunks, n = tables[:4]
        b1, b2 = group['betas']
        if getattr(self, '_use_dyn', False):     # captured step: lr and bias corrections from the device table
            fn, name, tail = self._guard_args('dvsof_adamw_step_dyn')
            _lib.check(fn(
                t_ptrs.data_ptr(), t_sizes.data_ptr(), t_chunks.data_ptr(), n,
                self._dyn_ptr(group), float(b1), float(b2),
                float(group['eps']), float(group['weight_decay']),
                1 if group['amsgrad'] else 0, *tail), name)
            return
        fn, name, tail = self._guard_args('dvsof_adamw_step')
        _lib.check(fn(
            t_ptrs.data_ptr(), t_sizes.data_ptr(), t_chunks.data_ptr(), n,
            float(group['lr']), float(b1), float(b2), float(group['eps']),
            float(group['weight_decay']), step,
            1 if group['amsgrad'] else 0, *tail), name)

    def _dyn_row(self, group, step, out4):
        """{lr, lr/bc1, sqrt(bc2), 0}"""
        b1, b2 = group['betas']
        out4[3] = 0.0
        _lib.lib().dvsof_adamw_dynamic(float(group['lr']), float(b1), float(b2),
                                       step, out4)


class _RAdamKind(_FusedBase):
    """RAdam and Ranger share one kernel; a class says what is constant for a
    group: ``_consts`` -> (N_sma threshold, flag word of dvsof_radam_step,
    Lookahead k or 0, Lookahead alpha or 0)."""
    STATE = ('exp_avg', 'exp_avg_sq', 'slow_buffer')

    def _consts(self, group):
        raise NotImplementedError

    def _launch(self, group, tables, step, plist):
        t_ptrs, t_sizes, t_chunks, n = tables[:4]
        b1, b2 = group['betas']
        thr, flags, k, alpha = self._consts(group)
        if getattr(self, '_use_dyn', False):     # captured step: lr, step size and the two decisions from the device table
            fn, name, tail = self._guard_args('dvsof_radam_step_dyn')
            _lib.check(fn(
                t_ptrs.data_ptr(), t_sizes.data_ptr(), t_chunks.data_ptr(), n,
                self._dyn_ptr(group), float(b1), float(b2),
                float(group['eps']), float(group['weight_decay']), alpha,
                *tail), name)
            return
        fn, name, tail = self._guard_args('dvsof_radam_step')
        _lib.check(fn(
            t_ptrs.data_ptr(), t_sizes.data_ptr(), t_chunks.data_ptr(), n,
            float(group['lr']), float(b1), float(b2), float(group['eps']),
            float(group['weight_decay']), step, thr, flags,
            1 if k and step % k == 0 else 0, alpha, *tail), name)

    def _dyn_row(self, group, step, out4):
        """{lr, step size (-1: no update), rectified, Lookahead sync now}"""
        b1, b2 = group['betas']
        thr, flags, k, _ = self._consts(group)
        _lib.lib().dvsof_radam_dynamic(float(group['lr']), float(b1), float(b2),
                                       step, thr, flags, k, out4)


class FusedRAdam(_RAdamKind):
    """Rectified Adam (Liu et al., ICLR 2020) with the defaults of the
    ``RAdam.radam.RAdam`` class the reference builds for ``--optimizer RADAM``
    (train_flownet.py:62-64; upstream submodule absent: parity unpinned,
    oracle/ref_optim.py restates the published algorithm)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0, degenerated_to_sgd=True):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps,
                                      weight_decay=weight_decay,
                                      degenerated_to_sgd=degenerated_to_sgd))

    def _init_state(self, p, st):
        st['exp_avg'] = torch.zeros_like(p)
        st['exp_avg_sq'] = torch.zeros_like(p)
        st['slow_buffer'] = st['exp_avg']      # unused by the kernel

    def _consts(self, group):
        return 5.0, 2 | (1 if group['degenerated_to_sgd'] else 0), 0, 0.0


class FusedRanger(_RAdamKind):
    """Ranger = RAdam + Lookahead (k, alpha) + gradient centralisation, with
    the defaults of lessw2020's ``ranger.Ranger`` which the reference builds
    for its DEFAULT ``--optimizer RANGER`` (train_flownet.py:65-71,
    utils/options.py:254-257; upstream submodule absent: parity unpinned)."""

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5,
                 betas=(.95, 0.999), eps=1e-5, weight_decay=0, use_gc=True,
                 gc_conv_only=False):
        super().__init__(params, dict(
            lr=lr, alpha=alpha, k=k, N_sma_threshhold=N_sma_threshhold,
            betas=betas, eps=eps, weight_decay=weight_decay, use_gc=use_gc,
            gc_conv_only=gc_conv_only))

    def _init_state(self, p, st):
        st['exp_avg'] = torch.zeros_like(p)
        st['exp_avg_sq'] = torch.zeros_like(p)
        st['slow_buffer'] = p.detach().clone()

    def _consts(self, group):
        return float(group['N_sma_threshhold']), 1, int(group['k']), \
            float(group['alpha'])

    def _extra_table(self, group, plist):
        """Row table of the gradient centralisation: {address, length} of
        every row (everything but dim 0) of every eligible gradient."""
        if not group['use_gc']:
            return None, 0
        gc_dim = 3 if group['gc_conv_only'] else 1
        return centralize_rows([p.grad for p in plist if p.dim() > gc_dim])

    def _launch(self, group, tables, step, plist):
        t_rows, n_rows = tables[4]
        if n_rows:      # ONE launch for the group's (bucket's) tensors, a workgroup per row
            _lib.check(_lib.lib().dvsof_grad_centralize_multi(
                t_rows.data_ptr(), n_rows, _lib.stream()),
                'dvsof_grad_centralize_multi')
        super()._launch(group, tables, step, plist)


def centralize_rows(grads):
    """-> (device int64 [rows, 2] of {row address, row length}, rows) for
    dvsof_grad_centralize_multi: the rows of dim 0 of every tensor in
    ``grads`` (float32, dim 0 outermost in memory: contiguous or
    channels_last)."""
    rows = []
    for g in grads:
        assert g.dtype == torch.float32 and g.is_cuda and _dense(g)
        n = g.numel() // g.shape[0]
        assert g.shape[0] == 1 or g.stride(0) == n, 'dim 0 must be outermost'
        rows += [(_as_int64(g.data_ptr() + 4 * r * n), n) for r in range(g.shape[0])]
    if not rows:
        return None, 0
    return torch.tensor(rows, dtype=torch.int64, device=grads[0].device), len(rows)


def _as_int64(x):
    """A uint64 pointer as the int64 of the same bits."""
    return x - (1 << 64) if x >= (1 << 63) else x


def _dense(t):
    """Dense, non-overlapping storage (any permutation of strides)."""
    return t.is_contiguous() or \
        t.is_contiguous(memory_format=torch.channels_last) or \
        t.numel() == t.untyped_storage().nbytes() // t.element_size()
