"""Voxeliser on the GPU against the fixed-point restatement of VOXEL_SPEC
(tests/voxel_cases.py), every kernel path and edge of the matrix.

Tiled path (wire and encoded entry): the grid is BITWISE equal to
``voxel_exact`` -- the exact sum of the 2^-32 fixed-point weights, rounded once
-- on random float timestamps as well as dyadic ones; bin0 / lin0 bitwise; the
control words are zero after the call; a second call on the same workspace is
bitwise equal to the first.
Thread-per-event path: bitwise on dyadic input (every float32 partial sum is
exact there, ``Exact.order_free``); on random input each voxel is within
``vc.v1_bound`` (k additions rounding a partial sum of at most sum |w|, the
rounding of 1 - f, the truncation of F, half an ulp) -- derived, not measured.
Every case asserts the kernel it means to reach through ``vc.plan`` and the
library's control_bytes.
"""
import numpy as np
import pytest
import torch

from oracle import cpu_oracle as orc
from tests import voxel_cases as vc

pytestmark = pytest.mark.gpu


def dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def control_words(voxel, n, c):
    """The (only) cached workspace's control region; () on the thread-per-event path."""
    control = voxel._lib.lib().dvsof_voxelize_control_bytes(n, c.B, c.C, c.H, c.W)
    if control == 0:
        return control, None
    assert len(voxel._WORKSPACES) == 1
    return control, next(iter(voxel._WORKSPACES.values()))[:control]


def check_grid(c, ex, got, what):
    got = got.cpu().numpy()
    assert got.shape == (c.B, c.C, c.H, c.W) and got.dtype == np.float32
    if c.kernel == 'tiled' or c.dyadic:
        if c.dyadic:
            assert ex.order_free
        bad = bits(got) != bits(ex.grid)
        diff = np.abs(got.astype(np.float64) - ex.grid)
        print(f'{what}: {int(bad.sum())} of {bad.size} voxels differ, max |diff| {diff.max():.3e}')
        assert not bad.any(), (what, int(bad.sum()), float(diff.max()),
                               np.argwhere(bad)[:4].tolist())
    else:
        err = np.abs(got.ravel().astype(np.float64) - ex.acc.astype(np.float64) * 2.0 ** -32)
        bound = vc.v1_bound(ex, got)
        print(f'{what}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}')
        assert (err <= bound).all(), (what, int((err > bound).sum()), float((err / bound).max()))


def run_entry(c, ex, entry):
    from dvs_of_training_framework_amd import voxel
    n = c.ev['x'].size
    t0, t1 = torch.from_numpy(c.t0).cuda(), torch.from_numpy(c.t1).cuda()
    if entry == 'wire':
        d = dev({k: c.ev[k] for k in vc.KEYS})
        call = lambda: voxel.voxelize(d, t0, t1, c.B, c.C, c.H, c.W, debug=True)   # noqa: E731
    else:
        d = dev(vc.compact(c.ev, c.B))
        call = lambda: voxel.voxelize_compact(d, t0, t1, c.B, c.C, c.H, c.W, debug=True)  # noqa: E731
    voxel._WORKSPACES.clear()
    got, gbin, glin = call()
    torch.cuda.synchronize()
    control, words = control_words(voxel, n, c)
    assert (control > 0) == (c.kernel == 'tiled')
    assert np.array_equal(gbin.cpu().numpy(), ex.bin0), entry
    assert np.array_equal(glin.cpu().numpy(), ex.lin0), entry
    check_grid(c, ex, got, f'{entry} first call')
    if words is not None:
        assert int(words.view(torch.int32).ne(0).sum()) == 0, 'control words not cleaned'
        again, _, _ = call()                    # same workspace, no memset
        assert len(voxel._WORKSPACES) == 1
        assert torch.equal(again, got), f'{entry}: second call on the same workspace differs'
        assert int(words.view(torch.int32).ne(0).sum()) == 0
    voxel._WORKSPACES.clear()
    return got


def test_plan_matches_the_library():
    """Every case reaches the kernel it names (first: the rest relies on it)."""
    from dvs_of_training_framework_amd import _lib
    lib = _lib.lib()
    for name, build in vc.CASES.items():
        if name in ('ept8', 'ept16'):
            continue                             # (built once, in their own test)
        c = build()
        n = c.ev['x'].size
        pl = vc.plan(n, c.B, c.C, c.H, c.W)
        assert (pl.kernel, pl.ept) == (c.kernel, c.ept), name
        assert lib.dvsof_voxelize_control_bytes(n, c.B, c.C, c.H, c.W) == pl.control, name
        assert lib.dvsof_voxelize_workspace_bytes(n, c.B, c.C, c.H, c.W) == pl.workspace, name


@pytest.mark.parametrize('name', list(vc.CASES))
def test_case(name):
    c = vc.CASES[name]()
    n = c.ev['x'].size
    pl = vc.plan(n, c.B, c.C, c.H, c.W)
    assert (pl.kernel, pl.ept) == (c.kernel, c.ept)
    ex = vc.voxel_exact(c.ev, c.t0, c.t1, c.B, c.C, c.H, c.W)
    if c.dyadic:        # ... and then the double oracle gives the same bits
        want, _, _ = orc.voxelize(c.ev, c.t0, c.t1, c.B, c.C, c.H, c.W)
        assert np.array_equal(bits(want), bits(ex.grid))
    wire = run_entry(c, ex, 'wire')
    if name in vc.ENCODED_FAMILY or (vc.compactable(c.ev, c.B) and n <= 100_000):
        enc = run_entry(c, ex, 'encoded')
        if c.kernel == 'tiled' or c.dyadic:
            assert torch.equal(enc, wire)
    else:
        assert name not in vc.ENCODED_FAMILY


def test_one_workspace_through_overflowing_and_well_spread_calls():
    """One workspace, zero-filled once: well-spread, three buckets overflowing,
    everything on one pixel, a bucket filled to exactly cap + 1, well-spread
    again -- every result bitwise exact, control words zero after every call."""
    from dvs_of_training_framework_amd import voxel
    B, C, H, W = vc.FILL_SHAPE
    n = B * vc.FILL_N
    voxel._WORKSPACES.clear()
    order = ('fill1023', 'fill_three_overflows', 'one_pixel', f'fill{vc.FILL_CAP + 1}',
             'fill1023', 'one_pixel_dyadic', 'fill1024_dyadic')
    for name in order:
        c = vc.CASES[name]()
        assert (c.B, c.C, c.H, c.W, c.ev['x'].size) == (B, C, H, W, n) and c.kernel == 'tiled'
        ex = vc.voxel_exact(c.ev, c.t0, c.t1, B, C, H, W)
        got, gbin, glin = voxel.voxelize(dev({k: c.ev[k] for k in vc.KEYS}),
                                         torch.from_numpy(c.t0).cuda(),
                                         torch.from_numpy(c.t1).cuda(), B, C, H, W, debug=True)
        check_grid(c, ex, got, name)
        assert np.array_equal(glin.cpu().numpy(), ex.lin0)
        control, words = control_words(voxel, n, c)
        assert control > 0 and int(words.view(torch.int32).ne(0).sum()) == 0, name
    voxel._WORKSPACES.clear()
