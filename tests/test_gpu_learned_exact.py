"""Order-independent forward of the learnable representation on the GPU
(dvsof_learned_voxelize_tiled; docs/LEARNED_VOXEL_SPEC.md, "Order-independent
forward") against the integer restatement of tests/learned_exact_cases.py.

The grid is BITWISE equal to the restatement on every input of the voxeliser's
test matrix (tests/voxel_cases.py: the smallest shapes that reach each edge of
the bucket and tile passes), on the tiled and on the three-kernel path, from wire
and from encoded columns, in any event order and for every events-per-thread
instantiation of the bucket pass; the control words are zero after every call;
every voxel is within k * 2^-32 + ulp/2 of the float64 restatement (truncation
per addend plus the one final rounding: derived, not measured); on dyadic input
with the initial table the grid is the fixed voxeliser's, bit for bit.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import learned_exact_cases as le
from tests import learned_voxel_cases as lc
from tests import voxel_cases as vc

pytestmark = pytest.mark.gpu

WS_CLEAN, LV_GLOBAL, LV_EPT8, LV_EPT16 = 1, 2, 4, 8
EINVAL, ENOSPACE = -1, -2
RS = ((2, 8), (3, 16), (1, 1))
# case -> what it reaches; (R, S) is spread over the cases in this order
MATRIX = ('ept4',                                                           # the plain tiled path
          'depth1', 'depth6', 'depth7', 'depth16', 'depth17', 'depth37',    # tile size, LDS limits
          'frame70x16', 'frame300x1', 'frame1x640', 'frame260x346',         # ragged tiles
          'tiles8192',                                                      # tile count at the limit
          'fill1279', 'fill1280', 'fill1281', 'fill_three_overflows', 'one_pixel',
          'window_edges', 'window_open_end', 'drops',
          'all_dropped', 'all_polarity_zero',
          'encoded_gaps',
          'v1_small', 'depth38_fallback', 'tiles8448_fallback')             # the three-kernel path
ENCODED_LIMIT = 100_000


def dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@lru_cache(maxsize=None)
def ref(name):
    """-> (case, R, S, theta, restatement): computed once, shared, left unchanged."""
    c = vc.CASES[name]()
    i = MATRIX.index(name)
    R, S = RS[i % 3]
    theta = le.random_theta(900 + i, R, S)
    return c, R, S, theta, le.learned_exact(c.ev, c.t0, c.t1, theta, R, S, c.B, c.C, c.H, c.W)


def columns(c, entry):
    if entry == 'wire':
        return dev({k: c.ev[k] for k in vc.KEYS})
    return dev(vc.compact(c.ev, c.B))


def assert_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    bad = bits(got) != bits(want)
    diff = np.abs(got.astype(np.float64) - want)
    print(f'{what}: {int(bad.sum())} of {bad.size} voxels differ, max |diff| {diff.max():.3e}')
    assert not bad.any(), (what, int(bad.sum()), float(diff.max()), np.argwhere(bad)[:4].tolist())


def control_words(lv, n, c):
    """The (only) cached workspace's control region; None on the three-kernel path."""
    control = lv._lib.lib().dvsof_learned_voxelize_tiled_control_bytes(n, c.B, c.C, c.H, c.W, 0)
    if control == 0:
        return control, None
    assert len(lv._WORKSPACES) == 1
    return control, next(iter(lv._WORKSPACES.values()))[:control]


def call_abi(c, cols, theta, R, S, flags, ws=None, out=None, n=None):
    """dvsof_learned_voxelize_tiled as the C ABI takes it -> (rc, out, workspace)."""
    from dvs_of_training_framework_amd import _lib
    lib = _lib.lib()
    encoded = 'sample_event_offsets' in cols
    n = cols['x'].numel() if n is None else n
    if ws is None:
        nbytes = lib.dvsof_learned_voxelize_tiled_workspace_bytes(n, c.B, c.C, c.H, c.W, flags)
        ws = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device='cuda')
    if out is None:
        out = torch.full((c.B, c.C, c.H, c.W), float('nan'), device='cuda')
    t0, t1 = torch.from_numpy(c.t0).cuda(), torch.from_numpy(c.t1).cuda()
    th = torch.from_numpy(theta).cuda()
    smp = cols['sample_event_offsets' if encoded else 'sample_index']
    rc = lib.dvsof_learned_voxelize_tiled(
        cols['x'].data_ptr(), cols['y'].data_ptr(), cols['timestamp'].data_ptr(),
        cols['polarity'].data_ptr(), smp.data_ptr(), int(encoded), n, t0.data_ptr(), t1.data_ptr(),
        th.data_ptr(), R, S, c.B, c.C, c.H, c.W, out.data_ptr(), ws.data_ptr(), ws.numel(), flags,
        _lib.stream())
    torch.cuda.synchronize()
    return rc, out, ws


def run_entry(name, entry):
    from dvs_of_training_framework_amd import learned_voxel as lv
    c, R, S, theta, ex = ref(name)
    n = c.ev['x'].size
    t0, t1 = torch.from_numpy(c.t0).cuda(), torch.from_numpy(c.t1).cuda()
    th = torch.from_numpy(theta).cuda()
    cols = columns(c, entry)
    call = lambda: lv.voxelize(cols, t0, t1, th, R, S, c.B, c.C, c.H, c.W,      # noqa: E731
                               deterministic=True)
    lv._WORKSPACES.clear()
    got = call()
    torch.cuda.synchronize()
    control, words = control_words(lv, n, c)
    assert (control > 0) == (c.kernel == 'tiled'), 'the case reaches the other path'
    assert_bits(got, ex.grid, f'{name} {entry} R={R} S={S}')
    if words is not None:
        assert int(words.view(torch.int32).ne(0).sum()) == 0, 'control words not cleaned'
    again = call()                      # same workspace, no fill of the control words
    assert len(lv._WORKSPACES) == 1
    assert torch.equal(again, got), f'{entry}: second call on the same workspace differs'
    if words is not None:
        assert int(words.view(torch.int32).ne(0).sum()) == 0
    lv._WORKSPACES.clear()
    return got


def test_sizes_follow_the_fixed_voxelisers_plan():
    """Every case reaches the path it names; the tiled workspace is the fixed
    voxeliser's, the three-kernel one the int64 scratch grid; DVSOF_LV_GLOBAL
    forces the latter."""
    from dvs_of_training_framework_amd import _lib
    lib = _lib.lib()
    for name in MATRIX:
        c = vc.CASES[name]()
        n = c.ev['x'].size
        pl = vc.plan(n, c.B, c.C, c.H, c.W)
        assert pl.kernel == c.kernel, name
        grid8 = c.B * c.C * c.H * c.W * 8
        assert lib.dvsof_learned_voxelize_tiled_control_bytes(n, c.B, c.C, c.H, c.W, 0) == pl.control, name
        assert lib.dvsof_learned_voxelize_tiled_workspace_bytes(n, c.B, c.C, c.H, c.W, 0) == \
            (pl.workspace if pl.tiled else grid8), name
        assert lib.dvsof_learned_voxelize_tiled_control_bytes(n, c.B, c.C, c.H, c.W, LV_GLOBAL) == 0
        assert lib.dvsof_learned_voxelize_tiled_workspace_bytes(n, c.B, c.C, c.H, c.W, LV_GLOBAL) == grid8
    # 480 x 640 x 9 at batch 16: 9600 tiles
    assert lib.dvsof_learned_voxelize_tiled_control_bytes(1 << 20, 16, 9, 480, 640, 0) == 0


@pytest.mark.parametrize('name', MATRIX)
def test_case(name):
    """Bitwise against the restatement (wire columns; encoded ones too where the
    events can be encoded), control words clean, a second call equal; every voxel
    within k * 2^-32 + ulp/2 of the float64 restatement."""
    c, R, S, theta, ex = ref(name)
    wire = run_entry(name, 'wire')
    if vc.compactable(c.ev, c.B) and c.ev['x'].size <= ENCODED_LIMIT:
        assert torch.equal(run_entry(name, 'encoded'), wire)
    else:
        assert name not in vc.ENCODED_FAMILY
    fw = lc.learned_forward(c.ev, c.t0, c.t1, theta, R, S, c.B, c.C, c.H, c.W)
    got = wire.cpu().numpy()
    err = np.abs(got.ravel().astype(np.float64) - fw.acc)
    bound = le.exact_bound(fw, got)
    print(f'{name}: max k {int(fw.k.max(initial=0))}, max err {err.max():.3e}, '
          f'max err / bound {(err / bound).max():.3f}')
    assert (err <= bound).all(), (name, int((err > bound).sum()), float((err / bound).max()))


@pytest.mark.parametrize('name,flags', [('ept4', LV_EPT8), ('ept4', LV_EPT16), ('ept4', LV_GLOBAL),
                                        ('fill_three_overflows', LV_GLOBAL),
                                        ('fill_three_overflows', LV_EPT16)])
def test_path_and_instantiation_variants_give_the_bits_of_the_plain_call(name, flags):
    c, R, S, theta, ex = ref(name)
    for entry in ('wire', 'encoded'):
        cols = columns(c, entry)
        rc, plain, _ = call_abi(c, cols, theta, R, S, 0)
        assert rc == 0
        rc, got, ws = call_abi(c, cols, theta, R, S, flags)
        assert rc == 0
        assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), (name, flags, entry)
        assert_bits(got, ex.grid, f'{name} flags={flags} {entry}')
        if not flags & LV_GLOBAL:
            control = vc.plan(c.ev['x'].size, c.B, c.C, c.H, c.W).control
            assert int(ws[:control].view(torch.int32).ne(0).sum()) == 0


@pytest.mark.parametrize('name', ['ept4', 'one_pixel'])
def test_the_order_of_the_events_changes_no_bit(name):
    c, R, S, theta, ex = ref(name)
    wire = {k: c.ev[k] for k in vc.KEYS}
    rc, a, _ = call_abi(c, dev(wire), theta, R, S, 0)
    rc2, b, _ = call_abi(c, dev(vc.shuffled(wire)), theta, R, S, 0)
    rc3, a2, _ = call_abi(c, dev(wire), theta, R, S, 0)
    assert rc == rc2 == rc3 == 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a.view(torch.int32), a2.view(torch.int32))
    assert_bits(a, ex.grid, name)
    assert int(ex.k.max()) >= (2000 if name == 'one_pixel' else 2)


def test_one_workspace_through_overflowing_and_well_spread_calls():
    """One workspace, zero-filled once, DVSOF_VOX_WS_CLEAN throughout: three
    buckets overflowing, well-spread, everything on one pixel, overflowing again
    -- every result bitwise exact, control words zero after every call."""
    B, C, H, W = vc.FILL_SHAPE
    n = B * vc.FILL_N
    ws = None
    for name in ('fill_three_overflows', 'fill1279', 'one_pixel', 'fill_three_overflows'):
        c, R, S, theta, ex = ref(name)
        assert (c.B, c.C, c.H, c.W, c.ev['x'].size) == (B, C, H, W, n) and c.kernel == 'tiled'
        rc, got, ws = call_abi(c, columns(c, 'wire'), theta, R, S, WS_CLEAN, ws=ws)
        assert rc == 0
        assert_bits(got, ex.grid, name)
        control = vc.plan(n, B, C, H, W).control
        assert control > 0 and int(ws[:control].view(torch.int32).ne(0).sum()) == 0, name


def test_no_events_give_zeros():
    from dvs_of_training_framework_amd import learned_voxel as lv
    c, R, S, theta, _ = ref('ept4')
    empty = {k: v[:0] for k, v in c.ev.items() if k in vc.KEYS}
    t0, t1 = torch.from_numpy(c.t0).cuda(), torch.from_numpy(c.t1).cuda()
    got = lv.voxelize(dev(empty), t0, t1, torch.from_numpy(theta).cuda(), R, S, c.B, c.C, c.H, c.W,
                      deterministic=True)
    assert got.shape == (c.B, c.C, c.H, c.W) and not got.view(torch.int32).any()
    # ... through the ABI with no workspace at all, and the control words of one that is passed stay zero
    from dvs_of_training_framework_amd import _lib
    out = torch.full((c.B, c.C, c.H, c.W), float('nan'), device='cuda')
    rc = _lib.lib().dvsof_learned_voxelize_tiled(
        None, None, None, None, None, 0, 0, t0.data_ptr(), t1.data_ptr(),
        torch.from_numpy(theta).cuda().data_ptr(), R, S, c.B, c.C, c.H, c.W, out.data_ptr(), None, 0,
        0, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0 and not out.view(torch.int32).any()


@pytest.mark.parametrize('name', ['ept4', 'v1_small'])
def test_a_workspace_that_is_too_small_is_refused_and_nothing_is_written(name):
    from dvs_of_training_framework_amd import _lib
    c, R, S, theta, _ = ref(name)
    n = c.ev['x'].size
    need = _lib.lib().dvsof_learned_voxelize_tiled_workspace_bytes(n, c.B, c.C, c.H, c.W, 0)
    small = torch.zeros(need - 1, dtype=torch.uint8, device='cuda')
    rc, out, _ = call_abi(c, columns(c, 'wire'), theta, R, S, 0, ws=small)
    assert rc == ENOSPACE
    assert bool(torch.isnan(out).all()) and not small.any()
    rc, out, _ = call_abi(c, columns(c, 'wire'), theta, R, S, 0,
                          ws=torch.zeros(need, dtype=torch.uint8, device='cuda'))
    assert rc == 0 and bool(torch.isfinite(out).all())


def test_bad_arguments_are_refused():
    from dvs_of_training_framework_amd import _lib
    c, R, S, theta, _ = ref('ept4')
    cols = columns(c, 'wire')
    for flags in (16, 1 << 30, LV_EPT8 | LV_EPT16):
        rc, out, _ = call_abi(c, cols, theta, R, S, flags,
                              ws=torch.zeros(1 << 24, dtype=torch.uint8, device='cuda'))
        assert rc == EINVAL and bool(torch.isnan(out).all()), flags
    for r, s in ((0, 8), (4, 8), (2, 0), (2, 17)):
        rc, out, _ = call_abi(c, cols, theta, r, s, 0,
                              ws=torch.zeros(1 << 24, dtype=torch.uint8, device='cuda'))
        assert rc == EINVAL and bool(torch.isnan(out).all()), (r, s)
    rc, out, _ = call_abi(c, cols, theta, R, S, 0, n=-1,
                          ws=torch.zeros(1 << 24, dtype=torch.uint8, device='cuda'))
    assert rc == EINVAL
    with pytest.raises(RuntimeError, match='dvsof_learned_voxelize_tiled'):
        _lib.check(rc, 'dvsof_learned_voxelize_tiled')


def test_dyadic_input_with_the_initial_table_is_the_fixed_grid():
    """... and the grid of the float-atomics forward, which is exact there."""
    from dvs_of_training_framework_amd import learned_voxel as lv, voxel
    c = lc.dyadic_case()
    d = dev({k: c.ev[k] for k in vc.KEYS})
    t0, t1 = torch.from_numpy(c.t0).cuda(), torch.from_numpy(c.t1).cuda()
    th = lv.initial_kernel(c.R, c.S).cuda()
    assert np.array_equal(th.cpu().numpy(), c.theta)
    got = lv.voxelize(d, t0, t1, th, c.R, c.S, c.B, c.C, c.H, c.W, deterministic=True)
    fixed = voxel.voxelize(d, t0, t1, c.B, c.C, c.H, c.W)
    atomics = lv.voxelize(d, t0, t1, th, c.R, c.S, c.B, c.C, c.H, c.W)
    assert torch.equal(got.view(torch.int32), fixed.view(torch.int32))
    assert torch.equal(got.view(torch.int32), atomics.view(torch.int32))
    assert int(got.count_nonzero()) > 1000
    # the same through the tiled path: the dyadic twin of the plain tiled case
    c4 = vc.CASES['ept4_dyadic']()
    d4 = dev({k: c4.ev[k] for k in vc.KEYS})
    t0, t1 = torch.from_numpy(c4.t0).cuda(), torch.from_numpy(c4.t1).cuda()
    got = lv.voxelize(d4, t0, t1, th, c.R, c.S, c4.B, c4.C, c4.H, c4.W, deterministic=True)
    fixed = voxel.voxelize(d4, t0, t1, c4.B, c4.C, c4.H, c4.W)
    assert torch.equal(got.view(torch.int32), fixed.view(torch.int32))


def test_a_captured_call_replays_bit_for_bit_on_new_events():
    """torch.cuda.graph on one stream, warmed workspace: the replay on new event
    contents copied into the static inputs equals the eager call on them."""
    from dvs_of_training_framework_amd import learned_voxel as lv
    c, R, S, theta, ex = ref('ept4')
    n = c.ev['x'].size
    other, _, _ = vc.spread(991, c.B, c.H, c.W, n // c.B)
    other['timestamp'] = vc.stamps(np.random.default_rng(992), c.t0, c.t1, other['sample_index'], False)
    t0, t1 = torch.from_numpy(c.t0).cuda(), torch.from_numpy(c.t1).cuda()
    th = torch.from_numpy(theta).cuda()
    static = dev({k: c.ev[k] for k in vc.KEYS})
    lv._WORKSPACES.clear()
    call = lambda cols: lv.voxelize(cols, t0, t1, th, R, S, c.B, c.C, c.H, c.W,     # noqa: E731
                                    deterministic=True)
    warm = call(static)
    assert_bits(warm, ex.grid, 'eager, first events')
    want = call(dev(other)).clone()
    torch.cuda.synchronize()
    assert not torch.equal(want, warm) and len(lv._WORKSPACES) == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(static)
    assert len(lv._WORKSPACES) == 1          # the capture took the warmed workspace
    for k, v in dev(other).items():
        static[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    for k, v in dev({k: c.ev[k] for k in vc.KEYS}).items():
        static[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    assert_bits(out, ex.grid, 'replay, first events again')
    words = next(iter(lv._WORKSPACES.values()))[:vc.plan(n, c.B, c.C, c.H, c.W).control]
    assert int(words.view(torch.int32).ne(0).sum()) == 0
    del graph
    lv._WORKSPACES.clear()
