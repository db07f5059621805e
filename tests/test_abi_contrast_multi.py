"""CPU checks of the extension header include/dvsof_contrast_multi.h: the
library exports what it declares, the derived binding equals a recorded table
(tests/golden/abi_signatures_contrast_multi.json) and signatures written out
by hand, a C compiler accepts the header, and the tables of include/dvsof.h
and include/dvsof_contrast.h are left as they were."""
import ctypes
import json
import os
import pathlib
import subprocess

from dvs_of_training_framework_amd import _abi, _lib

NAMES = ['dvsof_contrast_multi_bwd', 'dvsof_contrast_multi_fwd', 'dvsof_contrast_multi_workspace_bytes']
OLD_NAMES = ['dvsof_contrast_bwd', 'dvsof_contrast_fwd', 'dvsof_contrast_workspace_bytes']


def _category(t):
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_library_exports_every_symbol_the_header_declares():
    assert _lib.declared_contrast_multi_symbols() == NAMES == sorted(_lib._CONTRAST_MULTI_SIGNATURES)
    assert _lib._CONTRAST_MULTI_SIGNATURES is _abi.CONTRAST_MULTI_FUNCTIONS
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert hasattr(lib, name), f'{name} declared in dvsof_contrast_multi.h, not exported'
    bound = _lib.lib()
    for name, (res, args) in _lib._CONTRAST_MULTI_SIGNATURES.items():
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_signatures_are_the_recorded_ones():
    golden = json.loads((pathlib.Path(__file__).parent / 'golden' /
                         'abi_signatures_contrast_multi.json').read_text())
    assert set(golden) == set(_lib._CONTRAST_MULTI_SIGNATURES) and len(golden) == 3
    for name, (res, args) in _lib._CONTRAST_MULTI_SIGNATURES.items():
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name


def test_signatures_written_out_by_hand():
    vp, i, f, sz, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_int64
    row = _abi.STRUCTS['dvsof_iwe_result_t']
    res, args = _lib._CONTRAST_MULTI_SIGNATURES['dvsof_contrast_multi_fwd']
    assert res is i and args[:16] == [vp, vp, vp, vp, vp, i64, vp, vp, vp, i, i, i, i, i, vp, vp]
    assert issubclass(args[16], ctypes.POINTER(row)) and args[17:] == [vp, vp, sz, vp]
    assert _lib._CONTRAST_MULTI_SIGNATURES['dvsof_contrast_multi_bwd'] == \
        (i, [vp, vp, vp, vp, vp, i64, vp, vp, vp, i, i, i, i, i, vp, vp, sz, vp, f, vp, vp])
    assert _lib._CONTRAST_MULTI_SIGNATURES['dvsof_contrast_multi_workspace_bytes'] == (sz, [i, i, i, i, i])


def test_the_older_tables_are_left_alone():
    assert _abi.EXTENSION_PATHS == (_abi.HEADER_PATH.with_name('dvsof_contrast.h'),)
    assert sorted(_abi.EXTENSION_FUNCTIONS) == OLD_NAMES == sorted(_lib._EXTENSION_SIGNATURES)
    assert _lib.declared_extension_symbols() == OLD_NAMES
    assert not set(_lib._CONTRAST_MULTI_SIGNATURES) & (set(_lib._SIGNATURES) | set(_lib._EXTENSION_SIGNATURES))
    assert not any(n.startswith('dvsof_contrast') for n in _lib.declared_symbols())


def test_a_c_compiler_takes_the_header(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "dvsof_contrast_multi.h"\n#include "dvsof_contrast.h"\n'
                   '#include "dvsof_contrast_multi.h"\n'
                   'size_t (*const probe)(int, int, int, int, int) = dvsof_contrast_multi_workspace_bytes;\n'
                   'int main(void) { return sizeof(dvsof_iwe_result_t) == 48 ? 0 : 1; }\n')
    subprocess.run([os.environ.get('CC', 'cc'), '-std=c11', '-Wall', '-Werror', '-c', '-I',
                    str(_abi.HEADER_PATH.parent), str(src), '-o', str(tmp_path / 'use.o')], check=True)


def test_the_workspace_is_laid_out_as_the_header_says():
    """Host code only: the sums, M records of 32 bytes, F units of 8, the
    statistics' partials for M frames; 0 for what the calls refuse."""
    lib = _lib.lib()
    for F, mask, pol, h, w in ((1, 1, 0, 5, 7), (3, 7, 1, 40, 40), (2, 5, 0, 33, 31), (4, 2, 1, 1, 1)):
        M = F * bin(mask).count('1') * (1 + pol)
        assert lib.dvsof_contrast_multi_workspace_bytes(F, mask, pol, h, w) == \
            16 * F * h * w + 32 * M + 8 * F + lib.dvsof_iwe_stats_workspace_bytes(M, h, w)
    for bad in ((0, 7, 1, 4, 4), (-1, 7, 1, 4, 4), (65536, 1, 0, 4, 4), (1, 0, 0, 4, 4), (1, 8, 0, 4, 4),
                (1, 7, 2, 4, 4), (1, 7, -1, 4, 4), (1, 7, 1, 0, 4), (1, 7, 1, 4, 32768), (10923, 7, 1, 4, 4)):
        assert lib.dvsof_contrast_multi_workspace_bytes(*bad) == 0, bad
    assert lib.dvsof_contrast_multi_workspace_bytes(10922, 7, 1, 1, 1) > 0      # M = 65532
