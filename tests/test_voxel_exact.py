"""CPU self-tests of the voxeliser test matrix (tests/voxel_cases.py): the
fixed-point restatement against the double-precision oracle on every case, the
restated launch plan against the library's own sizes, and the premises the GPU
assertions rest on (no GPU needed: the two size entry points are host code)."""
import numpy as np
import pytest

from oracle import cpu_oracle as orc
from tests import voxel_cases as vc


@pytest.fixture(scope='module')
def hip_lib():
    from dvs_of_training_framework_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize('name', list(vc.CASES))
def test_case_against_the_double_oracle_and_the_plan(name, hip_lib):
    c = vc.CASES[name]()
    n = c.ev['x'].size
    ex = vc.voxel_exact(c.ev, c.t0, c.t1, c.B, c.C, c.H, c.W)
    want, bin0, lin0 = orc.voxelize(c.ev, c.t0, c.t1, c.B, c.C, c.H, c.W)
    assert np.array_equal(ex.bin0, bin0)
    assert np.array_equal(ex.lin0, lin0)
    # |acc| < 2^53 and fewer than 2^21 addends: asserted inside voxel_exact
    err = np.abs(ex.grid.ravel().astype(np.float64) - want.ravel())
    bound = vc.oracle_bound(ex, want)
    assert (err <= bound).all(), (err.max(), int((err > bound).sum()))
    if c.dyadic:
        assert ex.quantum >= 1 << 24 and ex.order_free     # weights are multiples of 2^-8
        assert np.array_equal(ex.grid.view(np.uint32), want.view(np.uint32))
    # the kernel this case means to reach, and the sizes that follow from the plan
    pl = vc.plan(n, c.B, c.C, c.H, c.W)
    assert (pl.kernel, pl.ept) == (c.kernel, c.ept)
    assert hip_lib.dvsof_voxelize_control_bytes(n, c.B, c.C, c.H, c.W) == pl.control
    assert hip_lib.dvsof_voxelize_workspace_bytes(n, c.B, c.C, c.H, c.W) == pl.workspace


def test_plan_thresholds():
    """The shapes the matrix relies on, read off v2_plan."""
    p = vc.plan
    assert [p(12000, 2, C, 70, 90).lp for C in (1, 6, 7, 37)] == [10, 10, 9, 9]
    assert p(12000, 2, 16, 70, 90).tile_lds == 64 * 1024          # exactly 64 KiB
    assert p(12000, 2, 17, 70, 90).tile_lds > 64 * 1024 and p(12000, 2, 17, 70, 90).tiled
    assert p(12000, 2, 37, 70, 90).tiled and not p(12000, 2, 38, 70, 90).tiled
    assert not p(4095, 2, 5, 70, 90).tiled and p(4096, 2, 5, 70, 90).tiled
    assert [p(65536, B, 1, H, 512).ntile for B, H in ((32, 510), (32, 512), (33, 512))] \
        == [8160, 8192, 8448]
    assert [p(n, 2, 5, 256, 256).ept for n in ((1 << 21) - 1, 1 << 21, (3 << 20) - 1, 3 << 20)] \
        == [4, 8, 8, 16]
    assert [p(12000, 2, 5, 70, W).lx for W in (1, 16, 90, 346, 512, 640)] == [6, 6, 6, 7, 9, 7]
    assert vc.CASES['v1_grid_stride']().ev['x'].size > vc.V1_GRID


def test_fill_cases_put_the_exact_number_of_events_in_the_tile():
    B, C, H, W = vc.FILL_SHAPE
    pl = vc.plan(B * vc.FILL_N, B, C, H, W)
    assert (pl.ntile, pl.cap, pl.lp, pl.lx) == (16, vc.FILL_CAP, 10, 6) and pl.cap > 1025
    for name in [n for n in vc.CASES if n.startswith('fill')]:
        c = vc.CASES[name]()
        ex = vc.voxel_exact(c.ev, c.t0, c.t1, B, C, H, W)
        hist = np.bincount(vc.tile_ids(c.ev, ex, pl), minlength=pl.ntile)
        assert hist.sum() == B * vc.FILL_N
        if name.startswith('fill_three'):
            assert all(hist[t] == k for t, k in vc.MULTI_FILLS.items())
            assert (hist > pl.cap).sum() == 3 and (np.delete(hist, list(vc.MULTI_FILLS)) > 0).all()
        else:
            want = int(name[4:].split('_')[0])
            assert hist[vc.FILL_TILE] == want and (np.delete(hist, vc.FILL_TILE) < 1023).all()
    c = vc.CASES['one_pixel']()
    ex = vc.voxel_exact(c.ev, c.t0, c.t1, B, C, H, W)
    assert set(vc.tile_ids(c.ev, ex, pl)) == {13} and ex.k.max() > 1 << 10
    c = vc.CASES['shuffled_across_samples']()
    pl = vc.plan(c.ev['x'].size, c.B, c.C, c.H, c.W)
    ex = vc.voxel_exact(c.ev, c.t0, c.t1, c.B, c.C, c.H, c.W)
    t = vc.tile_ids(c.ev, ex, pl)[:1024]        # the first workgroup's events
    assert t.min() < pl.ntile // 8 and t.max() >= pl.ntile - pl.ntile // 8


def test_window_edges_are_what_they_claim():
    c = vc.CASES['window_edges']()
    ex = vc.voxel_exact(c.ev, c.t0, c.t1, c.B, c.C, c.H, c.W)
    s, t = c.ev['sample_index'], c.ev['timestamp']
    kept = ex.bin0 >= 0
    assert c.t0[2] == c.t1[2] and c.t1[3] < c.t0[3] and c.t0.max() > 2.0
    assert len(set(np.round(c.t1[:2] - c.t0[:2], 4))) == 2      # windows of different length
    assert not kept[s == 3].any()
    assert kept[(s == 2) & (t == c.t0[2])].all() and not kept[(s == 2) & (t != c.t0[2])].any()
    assert (ex.bin0[(s == 2) & kept] == 0).all()
    for b in (0, 1):
        lo, hi = c.t0[b], c.t1[b]
        m = s == b
        assert (ex.bin0[m & (t == lo)] == 0).all() and (ex.bin0[m & (t == hi)] == c.C - 1).all()
        assert (m & (t == lo)).sum() > 100 and (m & (t == hi)).sum() > 100
        for out in (np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))):
            assert (m & (t == out)).sum() > 100 and not kept[m & (t == out)].any()
        assert (ex.bin0[m & (t == np.nextafter(lo, np.float32(np.inf)))] == 0).all()
    assert np.isnan(t).sum() > 200 and not kept[np.isnan(t)].any()      # NaN: dropped
    assert np.isinf(t).sum() > 400 and not kept[np.isinf(t)].any()
    # a fraction below 2^-32 truncates to F = 0: rounding instead would show
    c = vc.CASES['window_open_end']()
    ex = vc.voxel_exact(c.ev, c.t0, c.t1, c.B, c.C, c.H, c.W)
    assert np.isinf(c.t1[0]) and (ex.bin0[c.ev['sample_index'] == 0] == 0).all()


def test_nan_timestamp_is_dropped_by_the_oracle():
    """VOXEL_SPEC: dropped unless t0 <= t <= t1 -- a NaN timestamp compares false."""
    ev = {'x': np.array([1, 2]), 'y': np.array([1, 1]), 'polarity': np.array([1, -1]),
          'sample_index': np.array([0, 0]), 'timestamp': np.array([np.nan, 0.01], np.float32)}
    z, w = np.zeros(1, np.float32), np.full(1, 0.04, np.float32)
    grid, bin0, lin0 = orc.voxelize(ev, z, w, 1, 3, 4, 4)
    ex = vc.voxel_exact(ev, z, w, 1, 3, 4, 4)
    assert list(bin0) == [-1, 0] == list(ex.bin0) and list(lin0) == [-1, 6] == list(ex.lin0)
    assert grid[0, :, 1, 1].tolist() == [0, 0, 0] and np.array_equal(grid, ex.grid)


def test_compact_columns_carry_empty_samples():
    c = vc.CASES['encoded_gaps']()
    assert vc.compactable(c.ev, c.B)
    off = vc.compact(c.ev, c.B)['sample_event_offsets']
    assert off.tolist() == [0, 0, 4000, 4000, 4000, 8000, 8000]
    assert (c.ev['x'] < 0).any() and (c.ev['y'] == -32768).any()
    assert not vc.compactable(vc.CASES['drops']().ev, 3)
    assert not vc.compactable(vc.CASES['shuffled_across_samples']().ev, 6)
