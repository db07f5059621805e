"""CPU checks of the extension header include/dvsof_contrast.h: the library
exports what it declares, the derived binding equals a recorded table
(tests/golden/abi_signatures_contrast.json) and signatures written out by
hand, a C compiler accepts the header, the table of include/dvsof.h is left as it
was, and the workspace is that of the general entry points at their defaults."""
import ctypes
import json
import os
import pathlib
import subprocess

import pytest

from dvs_of_training_framework_amd import _abi, _lib

NAMES = ['dvsof_contrast_bwd', 'dvsof_contrast_fwd', 'dvsof_contrast_workspace_bytes']


def _category(t):
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_library_exports_every_symbol_the_extension_declares():
    assert _lib.declared_extension_symbols() == NAMES == sorted(_lib._EXTENSION_SIGNATURES)
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert hasattr(lib, name), f'{name} declared in dvsof_contrast.h, not exported'
    bound = _lib.lib()
    for name, (res, args) in _lib._EXTENSION_SIGNATURES.items():
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_signatures_are_the_recorded_ones():
    golden = json.loads((pathlib.Path(__file__).parent / 'golden' / 'abi_signatures_contrast.json').read_text())
    assert set(golden) == set(_lib._EXTENSION_SIGNATURES) and len(golden) == 3
    for name, (res, args) in _lib._EXTENSION_SIGNATURES.items():
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name


def test_signatures_written_out_by_hand():
    vp, i, f, sz, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_int64
    row = _abi.STRUCTS['dvsof_iwe_result_t']
    res, args = _lib._EXTENSION_SIGNATURES['dvsof_contrast_fwd']
    assert res is i and args[:14] == [vp, vp, vp, vp, i64, vp, vp, vp, i, i, i, vp, vp, args[13]]
    assert issubclass(args[13], ctypes.POINTER(row)) and args[14:] == [vp, vp, sz, vp]
    assert _lib._EXTENSION_SIGNATURES['dvsof_contrast_bwd'] == \
        (i, [vp, vp, vp, vp, i64, vp, vp, vp, i, i, i, vp, vp, sz, vp, f, vp, vp])
    assert _lib._EXTENSION_SIGNATURES['dvsof_contrast_workspace_bytes'] == (sz, [i, i, i])


def test_the_table_of_dvsof_h_is_left_alone():
    assert not set(_lib._EXTENSION_SIGNATURES) & set(_lib._SIGNATURES)
    assert not any(n.startswith('dvsof_contrast') for n in _lib.declared_symbols())


def test_a_c_compiler_takes_the_header(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "dvsof_contrast.h"\n#include "dvsof_contrast.h"\n'
                   'size_t (*const probe)(int, int, int) = dvsof_contrast_workspace_bytes;\n'
                   'int main(void) { return sizeof(dvsof_iwe_result_t) == 48 ? 0 : 1; }\n')
    subprocess.run([os.environ.get('CC', 'cc'), '-std=c11', '-Wall', '-Werror', '-c', '-I',
                    str(_abi.HEADER_PATH.parent), str(src), '-o', str(tmp_path / 'use.o')], check=True)


def test_an_extension_header_may_only_add_functions():
    base = _abi.Abi(_abi.HEADER_PATH.read_text())
    ext = _abi.Abi('int dvsof_x(const dvsof_iwe_result_t *r, void *stream);', base=base, name='x.h')
    assert list(ext.functions) == ['dvsof_x'] and ext.structs.keys() == base.structs.keys()
    with pytest.raises(_abi.AbiError, match=r'x\.h line 2:'):
        _abi.Abi('\nint dvsof_x(widget_t *w);', base=base, name='x.h')


def test_the_workspace_is_that_of_the_general_entry_points_at_the_start_without_polarity():
    """Host code only.  The refused sizes are those tests/test_gpu_contrast.py lists."""
    lib = _lib.lib()
    for F, h, w in ((1, 5, 7), (3, 33, 31), (3, 2, 3), (65535, 1, 1)):
        need = lib.dvsof_contrast_workspace_bytes(F, h, w)
        assert need == lib.dvsof_contrast_multi_workspace_bytes(F, 1, 0, h, w)
        assert need == 16 * F * h * w + 32 * F + 8 * F + lib.dvsof_iwe_stats_workspace_bytes(F, h, w) > 0
    for F, h, w in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 32768)):
        assert lib.dvsof_contrast_workspace_bytes(F, h, w) == 0, (F, h, w)
        assert lib.dvsof_contrast_multi_workspace_bytes(F, 1, 0, h, w) == 0, (F, h, w)
