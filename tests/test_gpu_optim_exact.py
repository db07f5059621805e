"""adamw_kernel, radam_kernel and the gradient centralisation (csrc/optim.hip) against the
float32 oracle of tests/optim_cases.py, BIT FOR BIT (docs/OPTIM_SPEC.md): parameters, both
moments, max_exp_avg_sq / slow_buffer and the gradient left in p.grad, after every one of 13
steps, for every variant of the case table; on the eager entry points, on the table-driven ones
(begin_capture / advance / step without a graph) and under a step guard that clips every step.
The table holds the vector tail, the chunk edges, three misaligned views, a parameter without
a gradient, a zero-element tensor, channels_last weights, and slices of zero, denormal-making
and 1e18 gradients.  tests/test_optim_oracle.py ties the oracle to the published algorithms
and shows that these inputs tell each wrong variant from the right one."""
import functools

import numpy as np
import pytest
import torch

from tests import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F = np.float32
PAD = -7.25         # what surrounds a misaligned view, and the planted max_exp_avg_sq


def lib():
    from dvs_of_training_framework_amd import _lib, optim  # noqa: F401  (registers the entry points)
    return _lib


@functools.lru_cache(maxsize=None)
def world():
    c = lib().lib().dvsof_adamw_chunk_elems()
    sp = oc.specs(c)
    return c, sp, oc.initial(sp)


def to_device(a, s):
    """A float32 array as the device tensor of this Spec -> (tensor, the buffer around a
    misaligned view or None)."""
    t = torch.tensor(a)
    if s.offset:
        buf = torch.full((a.size + 4,), PAD, device=DEV)
        view = buf[s.offset:s.offset + a.size]
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * s.offset
        return view, buf
    t = t.to(DEV)
    return (t.contiguous(memory_format=torch.channels_last) if s.layout == 'cl' else t), None


def mem_bits(t, cl):
    """The int32 bits of a device tensor or an oracle array, in MEMORY order."""
    if torch.is_tensor(t):
        t = t.detach()
        t = t.permute(0, 2, 3, 1) if cl else t
        return t.contiguous().view(-1).cpu().numpy().view(np.int32)
    t = t.transpose(0, 2, 3, 1) if cl else t
    return np.ascontiguousarray(t).reshape(-1).view(np.int32)


def same_bits(got, want, cl, where, offset=0):
    a, b = mem_bits(got, cl), mem_bits(want, cl)
    assert a.shape == b.shape, (where, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    if bad.size:
        i, c = int(bad[0]), world()[0]
        pytest.fail(f'{where}: {bad.size} of {a.size} elements differ; first at element {i} '
                    f'(chunk {i // c}, offset % 4 = {i % 4}, view at +{4 * offset} B): '
                    f'got {int(a[i]) & 0xffffffff:#010x} ({a[i:i + 1].view(F)[0]!r}), '
                    f'want {int(b[i]) & 0xffffffff:#010x} ({b[i:i + 1].view(F)[0]!r})')


def ulps(a, b):
    return abs(int(F(a).view(np.int32)) - int(F(b).view(np.int32)))


class Device:
    """The table on the device; parameter AND gradient of a misaligned Spec are views at the
    same byte offset into larger buffers."""

    def __init__(self, sp, p0):
        self.sp, self.t, self.buf, self.gbuf = sp, {}, {}, {}
        for s in sp:
            q, buf = to_device(p0[s.name], s)
            self.t[s.name] = q.requires_grad_(True)
            assert self.t[s.name].is_leaf
            if buf is not None:
                self.buf[s.name] = buf

    def set_grads(self, grads):
        for s in self.sp:
            g = grads[s.name]
            if g is None:
                self.t[s.name].grad = None
                continue
            self.t[s.name].grad, gbuf = to_device(g, s)
            assert self.t[s.name].grad.stride() == self.t[s.name].stride()
            if gbuf is not None:
                self.gbuf[s.name] = gbuf

    def padding_is_untouched(self, where):
        for bufs in (self.buf, self.gbuf):
            for name, buf in bufs.items():
                o = next(s.offset for s in self.sp if s.name == name)
                pad = torch.cat([buf[:o], buf[o + oc.OFFSET_N:]]).cpu().numpy()
                assert pad.size == 4 and (pad == F(PAD)).all(), (where, name, pad)


def make_optimizer(case, dev):
    from dvs_of_training_framework_amd.optim import FusedAdamW, FusedRAdam, FusedRanger
    cls = {'adamw': FusedAdamW, 'radam': FusedRAdam, 'ranger': FusedRanger}[case.kind]
    return cls(oc.param_groups(case, dev.t, dev.sp), **case.hyper)


def run(case, dyn=False, guarded=False):
    _, sp, p0 = world()
    dev = Device(sp, p0)
    opt = make_optimizer(case, dev)
    orc = oc.Oracle32(case, sp, p0)
    third = type(opt).STATE[2]
    if guarded:
        opt.set_guard(oc.MAX_NORM)
    if dyn:
        opt.begin_capture(DEV)
    for t in range(1, oc.STEPS + 1):
        grads = oc.step_grads(sp, t, huge=not guarded)
        dev.set_grads(grads)
        if dyn:
            opt.advance()
        opt.step()
        scale = None
        if guarded:
            rec = opt.guard_state()
            scale = F(rec['scale'])     # the float32 of the record, as it is
            assert scale < 1 and not rec['skip'] and rec['clipped'] == t and rec['bad'] == 0
            assert ulps(scale, oc.ref_scale(grads, oc.MAX_NORM)) <= 1
        orc.step(grads, scale)
        for s in sp:
            p = dev.t[s.name]
            where = f'{case.name} step {t} {s.name}'
            if not s.grad:
                # (advance() makes the state of every parameter of the group: zero moments)
                assert all(not opt.state[p][n].any() for n in ('exp_avg', 'exp_avg_sq')) \
                    if dyn else len(opt.state[p]) == 0
                same_bits(p, p0[s.name], False, where + '.p (no gradient)')
                continue
            st, cl = opt.state[p], s.layout == 'cl'
            assert st['step'] == t
            want = orc.arrays(s.name)
            same_bits(p, want['p'], cl, where + '.p', s.offset)
            same_bits(st['exp_avg'], want['m'], cl, where + '.exp_avg', s.offset)
            same_bits(st['exp_avg_sq'], want['v'], cl, where + '.exp_avg_sq', s.offset)
            same_bits(p.grad, orc.g[s.name], cl, where + '.grad', s.offset)
            if case.kind == 'radam':
                assert st['slow_buffer'] is st['exp_avg']       # stays the alias
                if not case.hyper['degenerated_to_sgd'] and t <= 5:
                    # un-rectified and no degenerate step: no update and NO DECAY
                    same_bits(p, p0[s.name], cl, where + '.p (untouched)', s.offset)
            elif case.kind == 'adamw' and not case.hyper['amsgrad']:
                # never read, never written: it keeps the bits planted after the first step
                x = st[third]
                if x.numel():
                    assert float(x.min()) == float(x.max()) == (0.0 if t == 1 else PAD), where
                    x.fill_(PAD)
            else:
                same_bits(st[third], want['x'], cl, f'{where}.{third}', s.offset)
        dev.padding_is_untouched(f'{case.name} step {t}')
    if dyn:
        opt.end_capture()
    return opt, dev


@pytest.mark.parametrize('case', oc.CASES, ids=lambda c: c.name)
def test_eager_steps_equal_the_float32_oracle_bit_for_bit(case):
    run(case)


@pytest.mark.parametrize('name', oc.DYN_CASES)
def test_table_driven_steps_equal_the_float32_oracle_bit_for_bit(name):
    """dvsof_adamw_step_dyn / dvsof_radam_step_dyn: lr, step size and the two decisions come
    from the device table that advance() fills, eagerly, with no graph."""
    opt, _ = run(oc.BY_NAME[name], dyn=True)
    assert opt._dyn is not None and opt._dyn.shape == (2, 4)


@pytest.mark.parametrize('name', oc.GUARD_CASES)
def test_clipped_steps_equal_the_float32_oracle_bit_for_bit(name):
    """A guard that binds on every step: g * scale with the record's own float32, AFTER the
    centralisation (which the tolerance of tests/test_gpu_step_guard.py cannot see)."""
    opt, _ = run(oc.BY_NAME[name], guarded=True)
    assert opt.guard_state()['clipped'] == oc.STEPS and opt.guard_state()['skipped'] == 0


@pytest.mark.parametrize('layout', ['contiguous', 'channels_last'])
@pytest.mark.parametrize('kind', ['dyadic', 'normal'])
@pytest.mark.parametrize('entry', ['single', 'multi'])
def test_centralisation_equals_the_oracle_bit_for_bit(entry, kind, layout):
    """Row lengths 1 ... 2304.  'single': dvsof_grad_centralize tensor by tensor.  'multi':
    dvsof_grad_centralize_multi with rows 0 and 2 of every tensor in the table -- row 1 and a
    1-D tensor that is in no table keep every bit."""
    _lib = lib()
    cl = layout == 'channels_last'
    host = oc.gc_grads(kind)
    grads, vector = host[:-1], host[-1]
    spec = oc.Spec('g', None, 1, 'cl' if cl else 'nd', 0, True)
    dev = [to_device(g, spec)[0] for g in grads]
    dvec = torch.tensor(vector).to(DEV)
    lengths = [g[0].numel() for g in dev]
    assert lengths == oc.GC_ROW_LENGTHS and all(g.shape[0] == 1 or g.stride(0) == n
                                                for g, n in zip(dev, lengths))
    if entry == 'single':
        for g, n in zip(dev, lengths):
            _lib.check(_lib.lib().dvsof_grad_centralize(g.data_ptr(), g.shape[0], n, _lib.stream()),
                       'dvsof_grad_centralize')
        want = [oc.centralize(g) for g in grads]
    else:
        rows = [(g.data_ptr() + 4 * r * n, n) for g, n in zip(dev, lengths) for r in (0, 2)]
        table = torch.tensor(rows, dtype=torch.int64, device=DEV)
        _lib.check(_lib.lib().dvsof_grad_centralize_multi(table.data_ptr(), len(rows), _lib.stream()),
                   'dvsof_grad_centralize_multi')
        want = []
        for g in grads:
            w = oc.centralize(g).copy()
            w[1] = g[1]
            want.append(w)
    torch.cuda.synchronize()
    for g, w, n in zip(dev, want, lengths):
        same_bits(g, w, cl, f'{entry} {kind} {layout} row length {n}')
    same_bits(dvec, vector, False, 'the 1-D tensor')
