"""Checkpoints behind the reference's ``Serializer`` surface
(utils/serializer.py:37-148): permanent and temporal checkpoints, pruning of
the temporal ones, resume.  Restated, with this build's additions
(docs/CHECKPOINT_SPEC.md):

  * files appear atomically (``step_N.pt.tmp`` -> ``os.replace``), pruning
    follows the rename;
  * a model on a GPU is snapshotted by one gather launch and one copy
    (snapshot.DeviceSnapshot) and the file is written by a writer thread;
    ``async_snapshot=False`` (and every CPU model) takes the reference's way,
    ``state_dict()`` + ``torch.save`` on the calling thread;
  * a state holding NaN or Inf is not written and prunes nothing;
  * ``wait`` / ``close``; an error of the writer thread is raised by the next
    ``checkpoint_model`` / ``wait`` / ``close``.
"""
import math
import os
import queue
import re
import sys
import threading
import time
from pathlib import Path

import torch


def template_regex(template):
    """'step_{}.pt' -> a compiled expression matching exactly the names the
    template makes from a non-negative integer."""
    try:
        made = template.format(0)
    except (IndexError, KeyError):
        made = template
    if made == template or template.count('{}') != 1:
        raise ValueError('checkpoint name template for the serializer has to use '
                         f'exactly one argument, the checkpoint id: {template!r}')
    head, tail = template.split('{}')
    return re.compile(re.escape(head) + r'(\d+)' + re.escape(tail))


def own_storage(state):
    """``state`` with every tensor owning exactly its bytes: ``torch.save`` of
    a view writes the whole storage underneath.  Tensors that are one tensor
    (optim.FusedRAdam: slow_buffer is exp_avg) stay one."""
    memo = {}

    def visit(obj):
        if torch.is_tensor(obj):
            t = obj.detach()
            if t.untyped_storage().nbytes() == t.numel() * t.element_size():
                return t
            key = (t.data_ptr(), tuple(t.shape), t.stride(), t.dtype)
            if key not in memo:
                memo[key] = t.clone()
            return memo[key]
        if isinstance(obj, dict):
            return type(obj)((k, visit(v)) for k, v in obj.items())
        if isinstance(obj, (list, tuple)):
            return type(obj)(visit(v) for v in obj)
        return obj
    return visit(state)


def count_nonfinite(state):
    """NaN / Inf values in the floating-point tensors of ``state`` (a tensor
    listed twice counts once)."""
    seen, bad = set(), 0
    stack = [state]
    while stack:
        obj = stack.pop()
        if torch.is_tensor(obj):
            key = (obj.data_ptr(), tuple(obj.shape), obj.stride())
            if obj.is_floating_point() and obj.numel() and key not in seen:
                seen.add(key)
                bad += int((~torch.isfinite(obj)).sum())
        elif isinstance(obj, dict):
            stack += list(obj.values())
        elif isinstance(obj, (list, tuple)):
            stack += list(obj)
    return bad


def _aliases(opt_state):
    """{param id: [(name, name of the earlier entry it shares memory with)]}"""
    out = {}
    for pid, st in opt_state.get('state', {}).items():
        first = {}
        for name, v in st.items():
            if not torch.is_tensor(v) or not v.numel():
                continue
            key = (v.data_ptr(), tuple(v.shape), v.stride())
            if key in first:
                out.setdefault(pid, []).append((name, first[key]))
            else:
                first[key] = name
    return out


class Serializer:
    def __init__(self, path, keep_checkpoints_max=math.inf,
                 permanent_checkpoint_interval=1, name_template='step_{}.pt',
                 async_snapshot=True):
        self._path = Path(path)
        self._history_size = keep_checkpoints_max
        self._permanent_interval = permanent_checkpoint_interval
        self._permanent_checkpoints = dict()
        self._temporal_checkpoints = dict()
        self._name_re = template_regex(name_template)
        self._name_template = name_template
        self.async_snapshot = bool(async_snapshot)
        self.refused = []           # (step, non-finite values)
        self.stalls = 0             # snapshots that waited for the one before
        self.timings = []           # per asynchronous checkpoint: writer seconds
        self._replace = os.replace
        self._lock = threading.Lock()
        self._jobs = None
        self._thread = None
        self._idle = threading.Event()
        self._idle.set()
        self._error = None
        self._snap = None
        self._find_checkpoints()

    # ------------------------------------------------------------ the files
    def _is_permanent(self, step):
        return self._permanent_interval > 0 and \
            step % self._permanent_interval == 0

    def _find_checkpoints(self):
        known = {}
        self._path.mkdir(parents=True, exist_ok=True)
        for p in self._path.iterdir():
            if p.name.endswith('.tmp') and \
                    self._name_re.fullmatch(p.name[:-len('.tmp')]):
                p.unlink()          # a write that never reached its rename
                continue
            m = self._name_re.fullmatch(p.name)
            if m:
                known[int(m.group(1))] = p.name
        with self._lock:
            self._permanent_checkpoints = {
                s: n for s, n in known.items() if self._is_permanent(s)}
            self._temporal_checkpoints = {
                s: n for s, n in known.items()
                if s not in self._permanent_checkpoints}

    def _id2path(self, global_step):
        return self._path / self._name_template.format(global_step)

    def _remove_old(self):
        if self._history_size <= 0:
            return
        with self._lock:
            steps = sorted(self._temporal_checkpoints, reverse=True)
            old = [] if math.isinf(self._history_size) else \
                steps[int(self._history_size):]
            names = [self._temporal_checkpoints.pop(s) for s in old]
        for name in names:
            (self._path / name).unlink(missing_ok=True)

    def _commit(self, state, global_step):
        """Write, rename, list, prune -- or refuse."""
        bad = state.pop('__nonfinite__', None)
        if bad is None:
            bad = count_nonfinite([state['model'], state['optimizer']])
        if bad:
            self.refused.append((global_step, bad))
            print(f'checkpoint: step {global_step} NOT written: {bad} non-finite '
                  'values in the parameters / optimizer state; older checkpoints '
                  'are kept', file=sys.stderr)
            return False
        path = self._id2path(global_step)
        tmp = path.with_name(path.name + '.tmp')
        with open(tmp, 'wb') as f:
            torch.save(state, f)
            f.flush()
            os.fsync(f.fileno())
        self._replace(tmp, path)
        with self._lock:
            if self._is_permanent(global_step):
                self._permanent_checkpoints[global_step] = path.name
            else:
                self._temporal_checkpoints[global_step] = path.name
        self._remove_old()
        return True

    # ------------------------------------------------------ the writer thread
    def _writer(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            try:
                job()
            except BaseException as e:      # surfaced by the next call
                self._error = e
            finally:
                self._idle.set()

    def _enqueue(self, job):
        if self._thread is None:
            self._jobs = queue.Queue()
            self._thread = threading.Thread(target=self._writer, daemon=True,
                                            name='checkpoint-writer')
            self._thread.start()
        self._idle.clear()
        self._jobs.put(job)

    def _raise_pending(self):
        e, self._error = self._error, None
        if e is not None:
            raise RuntimeError(f'writing a checkpoint failed: {e!r}') from e

    def wait(self):
        """Block until nothing is in flight; raise what the writer met."""
        self._idle.wait()
        self._raise_pending()

    def close(self):
        try:
            self.wait()
        finally:
            if self._thread is not None:
                self._jobs.put(None)
                self._thread.join()
                self._thread = self._jobs = None

    # ------------------------------------------------------------ checkpoints
    @staticmethod
    def _device_of(model):
        for p in model.parameters():
            return p.device
        return torch.device('cpu')

    def checkpoint_model(self, model, optimizer, global_step, **kwargs):
        """model + optimizer + ``kwargs`` as ``step_<global_step>.pt``.  On a
        GPU (and ``async_snapshot``) this returns once the snapshot is
        enqueued; the file is there after ``wait()``."""
        device = self._device_of(model)
        if not (self.async_snapshot and device.type == 'cuda'):
            self.wait()
            state = {'model': model.state_dict(),
                     'optimizer': optimizer.state_dict(),
                     'global_step': global_step}
            state.update(kwargs)
            return self._commit(own_storage(state), global_step)
        if not self._idle.is_set():     # one device slab, one host slab: back-pressure
            self.stalls += 1
            self._idle.wait()
        self._raise_pending()
        if self._snap is None:
            from .snapshot import DeviceSnapshot
            self._snap = DeviceSnapshot(device)
        state = {'model': model.state_dict(),
                 'optimizer': optimizer.state_dict(),
                 'global_step': global_step}
        state.update(kwargs)
        ticket = self._snap.take(state)

        def job():
            t0 = time.perf_counter()
            host_state, bad = ticket.collect()
            t1 = time.perf_counter()
            host_state['__nonfinite__'] = bad
            self._commit(host_state, global_step)
            del self.timings[:-15]      # the last few are enough for a tool to read
            self.timings.append({'step': global_step, 'wait_s': t1 - t0,
                                 'write_s': time.perf_counter() - t1})
        self._enqueue(job)
        return None

    def has_checkpoints(self):
        with self._lock:
            return (len(self._temporal_checkpoints) +
                    len(self._permanent_checkpoints)) > 0

    def list_known_steps(self):
        with self._lock:
            return sorted(list(self._temporal_checkpoints) +
                          list(self._permanent_checkpoints))

    def read_state_dict(self, global_step, map_location=None):
        return torch.load(self._id2path(global_step), map_location=map_location,
                          weights_only=True)

    def finalize(self, global_step, path, map_location=None):
        """The bare model state dict of a checkpoint, for deployment."""
        torch.save(self.read_state_dict(global_step, map_location)['model'], path)

    def load_checkpoint(self, model, global_step, optimizer=None, device=None):
        """-> (global step of the file, what else the file holds)."""
        self.wait()
        if global_step not in self.list_known_steps():
            raise ValueError(f'Checkpoint for step {global_step} not found')
        state = self.read_state_dict(global_step, device)
        global_step = state.pop('global_step')
        model.load_state_dict(state.pop('model'))
        opt_state = state.pop('optimizer')
        if optimizer:
            shared = _aliases(opt_state)
            optimizer.load_state_dict(opt_state)
            # entries that were one tensor in the file are one tensor again
            params = [p for g in optimizer.param_groups for p in g['params']]
            for pid, pairs in shared.items():
                st = optimizer.state[params[pid]]
                for name, first in pairs:
                    st[name] = st[first]
        return global_step, state
