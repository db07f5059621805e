"""The frame pyramid on the device against its restatement (tests/pyramid_cases.py,
docs/PYRAMID_SPEC.md), byte for byte: dvsof_resize_bilinear_ac, dvsof_loss_pyramid on
either tile size and on the per-level path, and the frames and the loss that
dvsof_loss_fused_pyramid leaves.

Every output is prefilled with a NaN pattern no kernel produces and lies between two guard
bands of it: a pixel nobody stored, and a store outside the level, both show.  NaNs are
compared by position, everything else by bits.  Every call runs twice and has to repeat its
bytes, and the source is read back after it.  Which kernel a case runs is not reported by
any entry point; tests/test_pyramid_oracle.py shows from the restated plan that the table
reaches each of them."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from tests import loss_pixel_cases as lpc
from tests import pyramid_cases as pc

pytestmark = pytest.mark.gpu

GUARD = 1024            # sentinel floats on either side of every output (4 KiB: keeps 16-byte alignment)
SENTINEL = 0x7FC5A5A5   # a NaN no kernel produces


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


class Arena:
    """``numel`` floats of sentinel between two guard bands, ``offset`` floats off the
    allocation's alignment."""

    def __init__(self, numel, offset=0):
        self.numel, self.lo = numel, GUARD + offset
        self.raw = torch.full((2 * GUARD + offset + numel,), SENTINEL, dtype=torch.int32, device='cuda')
        self.ptr = self.raw.data_ptr() + 4 * self.lo

    def tensor(self, *shape):
        return self.raw[self.lo:self.lo + self.numel].view(torch.float32).view(*shape)

    def read(self, shape, what, written=True):
        """-> the body as float32 [shape]; the guards are intact, and the body holds no
        sentinel (``written``) or nothing else."""
        raw = self.raw.cpu().numpy()
        body = raw[self.lo:self.lo + self.numel]
        assert (raw[:self.lo] == SENTINEL).all() and (raw[self.lo + self.numel:] == SENTINEL).all(), \
            f'{what}: a store outside the output'
        left = int((body == SENTINEL).sum())
        if written:
            assert left == 0, f'{what}: {left} of {body.size} elements were never stored'
        else:
            assert left == body.size, f'{what}: {body.size - left} elements were stored'
        return body.view(np.float32).reshape(shape)


def lib():
    from dvs_of_training_framework_amd import _lib
    return _lib.lib(), _lib.stream()


def resize_raw(src, n, hin, win, hout, wout, expect=0, written=True):
    """One call of dvsof_resize_bilinear_ac on a device tensor (or None) -> the output."""
    fn, st = lib()
    out = Arena(max(n, 1) * hout * wout if hout > 0 and wout > 0 else 16)
    rc = fn.dvsof_resize_bilinear_ac(None if src is None else src.data_ptr(), out.ptr, n, hin, win,
                                     hout, wout, st)
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    return out.read((-1,), (n, hin, win, hout, wout), written)


def pyramid_raw(images, D, H, W, shapes, offset=0, expect=0, written=True, nulls=()):
    """One call of dvsof_loss_pyramid -> the levels.  ``nulls``: arguments passed as NULL
    ('images', 'levels', 'hs', 'ws' or the index of a level)."""
    fn, st = lib()
    K = len(shapes)
    arenas = [Arena(max(D, 1) * max(h, 1) * max(w, 1), offset if k == K - 1 else 0)
              for k, (h, w) in enumerate(shapes)]
    ptrs = (ctypes.c_void_p * max(K, 1))(*[None if k in nulls else a.ptr for k, a in enumerate(arenas)])
    hs = (ctypes.c_int * max(K, 1))(*[h for h, _ in shapes])
    ws = (ctypes.c_int * max(K, 1))(*[w for _, w in shapes])
    rc = fn.dvsof_loss_pyramid(None if 'images' in nulls else images.data_ptr(), D, H, W,
                               None if 'levels' in nulls else ptrs, None if 'hs' in nulls else hs,
                               None if 'ws' in nulls else ws, K, st)
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect, shapes)
    return [a.read((-1,), (shapes, k), written) for k, a in enumerate(arenas)]


def assert_levels(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.reshape(w.shape)
        assert pc.same_bits(g, w), f'{what} level {k} {w.shape}: {pc.first_difference(g, w)}'


# ---------------------------------------------------------------------------
# dvsof_resize_bilinear_ac
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('n', pc.RESIZE_N)
@pytest.mark.parametrize('i', range(len(pc.RESIZE_CASES)), ids=lambda i: '%dx%d-%dx%d' % (
    pc.RESIZE_CASES[i][0] + pc.RESIZE_CASES[i][1]))
def test_resize_is_the_restatement(i, n):
    (hin, win), (hout, wout) = pc.RESIZE_CASES[i]
    src, want = pc.resize_case(i, n)
    d = dev(src)
    got = [resize_raw(d, n, hin, win, hout, wout).reshape(want.shape) for _ in range(2)]
    assert pc.same_bits(got[0], want), pc.first_difference(got[0], want)
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    assert np.array_equal(d.cpu().numpy().view(np.uint32), src.view(np.uint32))
    if (hin, win) == (hout, wout):      # the source's bytes
        assert np.array_equal(got[0].view(np.uint32), src.view(np.uint32))


def test_interpolate_takes_leading_dimensions_and_strides():
    """loss.interpolate on a non-contiguous [2,3,7,9] input."""
    from dvs_of_training_framework_amd.loss import interpolate
    src = pc.frames_host('random', 6, 9, 7).reshape(2, 3, 9, 7)
    x = dev(src).transpose(-1, -2)
    assert not x.is_contiguous() and x.shape == (2, 3, 7, 9)
    want = pc.resize_host(np.ascontiguousarray(src.transpose(0, 1, 3, 2)).reshape(6, 7, 9), 17, 65)
    got = interpolate(x, (17, 65))
    assert got.shape == (2, 3, 17, 65) and got.is_contiguous()
    assert pc.same_bits(got.cpu().numpy().reshape(6, 17, 65), want)
    assert np.array_equal(x.cpu().numpy(), src.transpose(0, 1, 3, 2))


def test_resize_argument_rules():
    src = dev(pc.frames_host('random', 1, 5, 7))
    for args in ((1, 0, 7, 3, 3), (1, 5, 0, 3, 3), (1, 5, 7, 0, 3), (1, 5, 7, 3, 0), (-1, 5, 7, 3, 3)):
        resize_raw(src, *args, expect=pc.EINVAL, written=False)
    resize_raw(None, 1, 5, 7, 3, 3, expect=pc.EINVAL, written=False)
    fn, st = lib()
    assert fn.dvsof_resize_bilinear_ac(src.data_ptr(), None, 1, 5, 7, 3, 3, st) == pc.EINVAL
    resize_raw(src, 0, 5, 7, 3, 3, written=False)           # n = 0: nothing to do
    many = dev(pc.frames_host('random', pc.MAX_FRAMES + 1, 1, 1))
    got = resize_raw(many, pc.MAX_FRAMES, 1, 1, 1, 1)
    assert np.array_equal(got.view(np.uint32), many.cpu().numpy().reshape(-1)[:pc.MAX_FRAMES].view(np.uint32))
    resize_raw(many, pc.MAX_FRAMES + 1, 1, 1, 1, 1, expect=pc.EINVAL, written=False)


# ---------------------------------------------------------------------------
# dvsof_loss_pyramid
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(pc.PYRAMID_CASES))
def test_pyramid_is_the_restatement(name):
    c = pc.case(name)
    D, (H, W), shapes = c['D'], c['src'], c['shapes']
    img = dev(c['images'])
    got = [pyramid_raw(img, D, H, W, shapes, c['offset']) for _ in range(2)]
    assert_levels(got[0], c['levels'], f'{name} {c["plan"]}')
    for a, b in zip(*got):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert np.array_equal(img.cpu().numpy().view(np.uint32), c['images'].view(np.uint32))
    if name == 'copy':
        assert np.array_equal(got[0][0].view(np.uint32), c['images'].reshape(-1).view(np.uint32))


def test_pyramid_argument_rules():
    shapes = ((5, 7), (9, 12))
    img = dev(pc.frames_host('random', 3, 20, 40))
    bad = dict(expect=pc.EINVAL, written=False)
    for null in ('images', 'levels', 'hs', 'ws', 0, 1):
        pyramid_raw(img, 3, 20, 40, shapes, nulls=(null,), **bad)
    pyramid_raw(img, 3, 20, 40, ((5, 7), (0, 12)), **bad)
    pyramid_raw(img, 3, 20, 40, ((5, 7), (9, 0)), **bad)
    pyramid_raw(img, 3, 20, 40, (), **bad)                 # K = 0
    pyramid_raw(img, 3, 0, 40, shapes, **bad)              # H = 0
    pyramid_raw(img, 3, 20, 0, shapes, **bad)
    pyramid_raw(img, -1, 20, 40, shapes, **bad)
    nine = pc.PYRAMID_CASES['k8']['shapes'] + ((18, 66),)
    pyramid_raw(img, 3, 20, 40, nine, **bad)               # K = 9
    pyramid_raw(img, 0, 20, 40, shapes, written=False)     # D = 0: DVSOF_OK, nothing written
    pyramid_raw(img, 0, 20, 40, ((9, 12), (5, 7)), written=False)


# ---------------------------------------------------------------------------
# dvsof_loss_fused_pyramid
# ---------------------------------------------------------------------------
def _fused_case(name):
    """-> dict(K, N, D, shapes, start, stop, flows, images [D,H,W])."""
    if name == 'scales5':       # sizes that go up and down: the per-level path
        c = lpc.case(name)
        return dict(c, images=c['frames'][-1])
    N, shapes = 3, pc.FUSED_SHAPES
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    flows = [np.stack([lpc.make_flow(rng, h, w, lpc.STATES[(n + k) % 4]) for n in range(N)])
             for k, (h, w) in enumerate(shapes)]
    return dict(K=len(shapes), N=N, D=2 * N, shapes=shapes, flows=flows,
                start=np.arange(N, dtype=np.int32), stop=np.arange(N, 2 * N, dtype=np.int32),
                images=pc.frames_host('random', 2 * N, *pc.FUSED_SRC))


WEIGHTS = (0.3, 2.0, 1.5)


def _apply(c, frames, images):
    from dvs_of_training_framework_amd.loss import _FusedLoss
    flows = [dev(f).requires_grad_(True) for f in c['flows']]
    loss, terms = _FusedLoss.apply(frames, images, dev(c['start']), dev(c['stop']), WEIGHTS, 1.0, *flows)
    grads = torch.autograd.grad(loss, flows)
    return dict(loss=loss.detach().cpu().numpy(), terms=terms.detach().cpu().numpy(),
                grads=[g.cpu().numpy() for g in grads])


def _same(a, b, what):
    for key in ('loss', 'terms'):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), (what, key, a[key], b[key])
    for k, (x, y) in enumerate(zip(a['grads'], b['grads'])):
        assert pc.same_bits(x, y), f'{what}: gradient of scale {k}: {pc.first_difference(x, y)}'


@pytest.mark.parametrize('name', ['fused_chain', 'scales5'])
def test_fused_pyramid_frames_and_loss_through_them(name):
    """The levels dvsof_loss_fused_pyramid leaves in ``frames`` are the restatement's bytes,
    and loss, terms, out-of-border counts and every flow gradient are the bytes of the
    ``images is None`` path on the restated levels -- the path tests/test_gpu_loss_pixels.py
    pins per pixel against float64 for given frames.  Together: the photometric term and
    its gradient through the pyramid at more than one scale."""
    from tests.test_gpu_loss_pixels import fused_raw
    c = _fused_case(name)
    D, shapes = c['D'], c['shapes']
    H, W = c['images'].shape[1:]
    plan = pc.plan_host(D, H, W, shapes)
    assert plan == ('per_level' if name == 'scales5' else ('fused', False))
    want = pc.pyramid_host(c['images'], shapes)
    restated = tuple(dev(w) for w in want)

    # the path without images repeats its own bytes: a mismatch below then means what it says
    base = _apply(c, restated, None)
    _same(base, _apply(c, restated, None), f'{name}: given frames, two calls')
    t0, l0, oob0, g0 = fused_raw(c, restated, None, WEIGHTS, [dev(f) for f in c['flows']])
    assert np.isfinite(base['terms']).all() and (base['terms'][1] > 0).all()

    images = dev(c['images'])
    for run in range(2):
        arenas = [Arena(D * h * w) for h, w in shapes]
        frames = tuple(a.tensor(D, h, w) for a, (h, w) in zip(arenas, shapes))
        got = _apply(c, frames, images)
        levels = [a.read((D, h, w), (name, k)) for k, (a, (h, w)) in enumerate(zip(arenas, shapes))]
        assert_levels(levels, want, f'{name} {plan} run {run}')
        _same(got, base, f'{name}: through the pyramid, run {run}')
    assert np.array_equal(images.cpu().numpy().view(np.uint32), c['images'].view(np.uint32))

    # the counts (and everything again) through the C ABI
    arenas = [Arena(D * h * w) for h, w in shapes]
    frames = tuple(a.tensor(D, h, w) for a, (h, w) in zip(arenas, shapes))
    t1, l1, oob1, g1 = fused_raw(c, frames, images, WEIGHTS, [dev(f) for f in c['flows']])
    assert np.array_equal(oob0, oob1) and np.array_equal(t0.view(np.uint32), t1.view(np.uint32)) and l0 == l1
    for k, (x, y) in enumerate(zip(g0, g1)):
        assert pc.same_bits(x, y), (name, k)
    assert_levels([a.read((D, h, w), (name, k)) for k, (a, (h, w)) in enumerate(zip(arenas, shapes))],
                  want, f'{name} C ABI')
    assert (oob0 > 0).any()
