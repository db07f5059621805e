"""CPU checks of the extension header include/dvsof_avg_timestamp_pyramid.h:
the library exports what it declares, the derived binding equals a recorded
table (tests/golden/abi_signatures_avg_timestamp_pyramid.json) and signatures
written out by hand, a C compiler accepts the header (twice, and beside the
older ones), the older tables and structs are left as they were, the workspace
is laid out as the header says, and every refusal comes before any launch."""
import ctypes
import json
import os
import pathlib
import subprocess

from dvs_of_training_framework_amd import _abi, _lib, loss as L
from tests import avg_timestamp_pyramid_cases as apc

NAMES = ['dvsof_avg_timestamp_pyramid_bwd', 'dvsof_avg_timestamp_pyramid_fwd',
         'dvsof_avg_timestamp_pyramid_workspace_bytes']
GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'abi_signatures_avg_timestamp_pyramid.json'
SIGNATURES = _lib._AVG_TIMESTAMP_PYRAMID_SIGNATURES


def _category(t):
    if t is _lib.ContrastLevels:
        return 'levels'
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_library_exports_every_symbol_the_header_declares():
    assert _lib.declared_avg_timestamp_pyramid_symbols() == NAMES == sorted(SIGNATURES)
    assert SIGNATURES is _abi.AVG_TIMESTAMP_PYRAMID_FUNCTIONS
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert hasattr(lib, name), f'{name} declared in dvsof_avg_timestamp_pyramid.h, not exported'
    bound = _lib.lib()
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_signatures_are_the_recorded_ones():
    golden = json.loads(GOLDEN.read_text())
    assert set(golden) == set(NAMES)
    for name, (res, args) in SIGNATURES.items():
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name


def test_signatures_written_out_by_hand():
    vp, i, sz, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int64
    lv = _lib.ContrastLevels            # the very class of dvsof_contrast_pyramid.h: no second struct
    head = [vp, vp, vp, vp, vp, i64, vp, vp, i, i, i, i, i, lv]
    assert SIGNATURES['dvsof_avg_timestamp_pyramid_fwd'] == (i, head + [vp, vp, vp, sz, vp])
    assert SIGNATURES['dvsof_avg_timestamp_pyramid_bwd'] == (i, head + [vp, sz, vp, vp])
    assert SIGNATURES['dvsof_avg_timestamp_pyramid_workspace_bytes'] == (sz, [i, i, i, i, i, lv])
    assert L.AVG_TIMESTAMP_SCALES == ('finest', 'all')


def test_the_older_tables_and_structs_are_left_alone():
    assert _lib.declared_avg_timestamp_symbols() == ['dvsof_avg_timestamp_bwd', 'dvsof_avg_timestamp_fwd',
                                                     'dvsof_avg_timestamp_workspace_bytes']
    assert _lib.declared_contrast_pyramid_symbols() == ['dvsof_contrast_pyramid_bwd', 'dvsof_contrast_pyramid_fwd',
                                                        'dvsof_contrast_pyramid_workspace_bytes']
    older = set(_lib._SIGNATURES) | set(_lib._EXTENSION_SIGNATURES) | set(_lib._CONTRAST_MULTI_SIGNATURES) \
        | set(_lib._IWE_MULTI_SIGNATURES) | set(_lib._LOSS_FRAMELESS_SIGNATURES) \
        | set(_lib._CONTRAST_PYRAMID_SIGNATURES) | set(_lib._AVG_TIMESTAMP_SIGNATURES)
    assert not set(NAMES) & older
    assert sorted(_abi.CONTRAST_PYRAMID_STRUCTS) == ['dvsof_contrast_level_t', 'dvsof_contrast_levels_t']
    assert ctypes.sizeof(_lib.ContrastLevels) == 456 and ctypes.sizeof(_lib.ContrastLevel) == 56
    assert _lib.STRUCTS is _abi.STRUCTS and not any('level' in n for n in _abi.STRUCTS)
    golden = pathlib.Path(__file__).parent / 'golden'
    for stem, table in (('avg_timestamp', _lib._AVG_TIMESTAMP_SIGNATURES),
                        ('contrast_pyramid', _lib._CONTRAST_PYRAMID_SIGNATURES)):
        recorded = json.loads((golden / f'abi_signatures_{stem}.json').read_text())
        assert set(table) <= set(recorded) and not set(NAMES) & set(recorded)
    assert not any('avg_timestamp' in n for n in _lib.declared_symbols())


def test_a_c_compiler_takes_the_header(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include <stddef.h>\n#include "dvsof_avg_timestamp_pyramid.h"\n#include "dvsof_avg_timestamp.h"\n'
                   '#include "dvsof_contrast_multi.h"\n#include "dvsof_contrast_pyramid.h"\n'
                   '#include "dvsof_avg_timestamp_pyramid.h"\n'
                   'size_t (*const probe)(int, int, int, int, int, dvsof_contrast_levels_t) = '
                   'dvsof_avg_timestamp_pyramid_workspace_bytes;\n'
                   f'_Static_assert(sizeof(dvsof_contrast_levels_t) == {ctypes.sizeof(_lib.ContrastLevels)}, "t");\n'
                   'int main(void) { return 0; }\n')
    subprocess.run([os.environ.get('CC', 'cc'), '-std=c11', '-Wall', '-Werror', '-c', '-I',
                    str(_abi.HEADER_PATH.parent), str(src), '-o', str(tmp_path / 'use.o')], check=True)


def _table(shape, shapes, F=3, M=18, **change):
    tb = L.contrast_level_table(shape, shapes, F, M, [0.25] * len(shapes))
    for k, v in change.items():
        name, level = k.rsplit('_', 1)
        setattr(tb.level[int(level)], name, v)
    return tb


def test_the_workspace_is_laid_out_as_the_header_says():
    """Host code only: q, s, base, sums and count of all levels, padding to 8,
    K M records of 64 bytes, K F units of 8, K M rows of 32 and the partials for
    M images of the largest level; 0 for what the calls refuse."""
    lib = _lib.lib()
    for F, mask, pol, shape, shapes in ((3, 7, 1, (24, 40), ((24, 40), (12, 20), (6, 10))),
                                        (3, 1, 0, (21, 37), ((3, 5), (6, 10), (11, 19), (21, 37))),
                                        (1, 5, 1, (21, 37), ((11, 19),)), (2, 2, 0, (1, 1), ((1, 1), (1, 1))),
                                        (1, 1, 0, (5, 7), ((5, 7), (3, 4), (2, 2), (1, 1)))):
        M = F * bin(mask).count('1') * (1 + pol)
        K = len(shapes)
        tb = L.contrast_level_table(shape, shapes, F, M, [1.0] * K)
        pixels = sum(h * w for h, w in shapes)
        head = (3 * 8 * M * pixels + 16 * F * pixels + 4 * M * pixels + 7) // 8 * 8
        nb = max(min(max(-(-h * w // 1024), 1), 128) for h, w in shapes)
        want = head + 64 * K * M + 8 * K * F + 32 * K * M + 32 * M * nb
        assert lib.dvsof_avg_timestamp_pyramid_workspace_bytes(F, mask, pol, *shape, tb) == want, (shape, shapes)
        assert want == apc.layout(F, M, shapes)['bytes'] == L.avg_timestamp_pyramid_layout(F, M, shapes)['bytes']
        for key in ('s', 'base', 'sums', 'count', 'rec', 'unit', 'rows', 'part'):
            assert apc.layout(F, M, shapes)[key] == L.avg_timestamp_pyramid_layout(F, M, shapes)[key], key
    # a frame above 1024 pixels per block of the reduction: nb of the largest level, not of the frame
    big = ((400, 400), ((400, 400), (200, 200)))
    tb = L.contrast_level_table(*big, 1, 2, [1.0, 1.0])
    assert lib.dvsof_avg_timestamp_pyramid_workspace_bytes(1, 5, 0, 400, 400, tb) == apc.layout(1, 2, big[1])['bytes']
    # one level of shift 0: the one-level workspace
    tb = L.contrast_level_table((21, 37), ((21, 37),), 3, 18, [1.0])
    assert lib.dvsof_avg_timestamp_pyramid_workspace_bytes(3, 7, 1, 21, 37, tb) == \
        lib.dvsof_avg_timestamp_workspace_bytes(3, 7, 1, 21, 37) == L.avg_timestamp_layout(3, 18, 21, 37)['bytes']
    good = ((24, 40), ((24, 40), (12, 20), (6, 10)))
    assert lib.dvsof_avg_timestamp_pyramid_workspace_bytes(3, 7, 1, 24, 40, _table(*good)) > 0
    # the offsets are not read here; the shapes, the shifts and K are
    assert lib.dvsof_avg_timestamp_pyramid_workspace_bytes(3, 7, 1, 24, 40, _table(*good, image_offset_1=5)) > 0
    for args, tb in (((0, 7, 1, 24, 40), _table(*good)), ((-1, 7, 1, 24, 40), _table(*good)),
                     ((3, 0, 1, 24, 40), _table(*good)), ((3, 8, 1, 24, 40), _table(*good)),
                     ((3, 7, 2, 24, 40), _table(*good)), ((10923, 7, 1, 24, 40), _table(*good)),
                     ((3, 7, 1, 24, 41), _table(*good)), ((3, 7, 1, 0, 40), _table(*good)),
                     ((3, 7, 1, 24, 40), _table(*good, w_1=21)), ((3, 7, 1, 24, 40), _table(*good, shift_1=2)),
                     ((3, 7, 1, 24, 40), _table(*good, shift_2=16)), ((3, 7, 1, 24, 40), _table(*good, shift_0=-1)),
                     ((3, 7, 1, 24, 40), _table(*good, h_2=0))):
        assert lib.dvsof_avg_timestamp_pyramid_workspace_bytes(*args, tb) == 0, args
    for K in (0, 9, -1):
        tb = _table(*good)
        tb.K = K
        assert lib.dvsof_avg_timestamp_pyramid_workspace_bytes(3, 7, 1, 24, 40, tb) == 0, K


def test_refusals_need_no_device():
    """Every refusal comes before any launch, so the calls can be made on a
    machine without a GPU: the order of the header, K and the shift rule among
    them, K before F == 0."""
    lib = _lib.lib()
    good = ((24, 40), ((24, 40), (12, 20), (6, 10)))
    from tests import contrast_cases as cc
    EINVAL, ENOSPACE = cc.EINVAL, cc.ENOSPACE
    one = ctypes.c_int64(1)                 # a non-null address nothing reads
    a = ctypes.addressof(one)

    def fwd(tb, F=3, h=24, w=40, n=5, mask=7, pol=1, ws=a, nbytes=1 << 40, out=a, p=a, x=a):
        return lib.dvsof_avg_timestamp_pyramid_fwd(x, a, a, p, a, n, a, a, F, h, w, mask, pol, tb, out, out, ws,
                                                   nbytes, None)

    def bwd(tb, F=3, h=24, w=40, n=5, mask=7, pol=1, ws=a, nbytes=1 << 40, out=a, p=a, x=a):
        return lib.dvsof_avg_timestamp_pyramid_bwd(x, a, a, p, a, n, a, a, F, h, w, mask, pol, tb, ws, nbytes, out,
                                                   None)
    flows = [a, a, a]

    def table(**change):
        tb = L.contrast_level_table(*good, 3, 18, [0.25] * 3, flows, flows)
        for k, v in change.items():
            name, level = k.rsplit('_', 1)
            setattr(tb.level[int(level)], name, v)
        return tb
    for call in (fwd, bwd):
        for kw in (dict(F=-1), dict(n=-1), dict(mask=0), dict(mask=8), dict(pol=2), dict(F=65536), dict(F=10923),
                   dict(h=25), dict(w=0), dict(h=32768)):
            assert call(table(), **kw) == EINVAL, kw
        for change in (dict(shift_1=2), dict(shift_1=16), dict(shift_0=-1), dict(w_1=21), dict(h_2=7), dict(h_0=0),
                       dict(image_offset_2=1), dict(row_offset_1=0), dict(sums_offset_1=1), dict(flow_0=None)):
            assert call(table(**change)) == EINVAL, change
        for K in (0, 9, -1):
            tb = table()
            tb.K = K
            assert call(tb) == EINVAL, K
        assert call(table(), out=None) == EINVAL
        assert call(table(), x=None) == EINVAL and call(table(), p=None) == EINVAL
        # the order: a bad option before a bad K, a bad K before a bad shape, a bad table before a
        # missing workspace, null pointers before it too
        tb = table()
        tb.K = 0
        assert call(tb, mask=0, ws=None) == EINVAL and call(tb, h=0, ws=None) == EINVAL
        assert call(table(shift_1=2), ws=None) == EINVAL and call(table(), out=None, ws=None) == EINVAL
        assert call(table(), ws=None) == ENOSPACE and call(table(), nbytes=100) == ENOSPACE
        need = lib.dvsof_avg_timestamp_pyramid_workspace_bytes(3, 7, 1, 24, 40, table())
        assert call(table(), nbytes=need - 1) == ENOSPACE
        # K is looked at before F == 0 says there is nothing to do
        assert call(tb, F=0) == EINVAL and call(table(), F=0) == 0
        assert call(table(), F=0, ws=None, out=None, x=None) == 0
    assert bwd(table(grad_flow_2=None)) == EINVAL
    assert fwd(table(grad_flow_2=None), ws=None) == ENOSPACE        # the forward does not look at grad_flow
