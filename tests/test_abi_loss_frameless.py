"""CPU checks of the extension header include/dvsof_loss_frameless.h: the
library exports what it declares, the derived binding equals a recorded table
(tests/golden/abi_signatures_loss_frameless.json) and signatures written out by
hand, a C compiler accepts the header, the four older tables are left as they
were, and the host side of the two entry points (the workspace size and every
refusal, which come before any launch and need no device)."""
import ctypes
import json
import os
import pathlib
import subprocess

from dvs_of_training_framework_amd import _abi, _lib

NAMES = ['dvsof_loss_frameless', 'dvsof_loss_frameless_workspace_bytes']
OLD = {'abi_signatures_contrast.json': '_EXTENSION_SIGNATURES',
       'abi_signatures_contrast_multi.json': '_CONTRAST_MULTI_SIGNATURES',
       'abi_signatures_iwe_multi.json': '_IWE_MULTI_SIGNATURES',
       'abi_signatures.json': '_SIGNATURES'}
GOLDEN = pathlib.Path(__file__).parent / 'golden'
EINVAL, ENOSPACE = -1, -2       # include/dvsof.h


def _category(t):
    if t is None:
        return 'void'
    if t is ctypes.c_char_p:
        return 'cstr'
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_uint64: 'u64',
            ctypes.c_ulonglong: 'u64', ctypes.c_float: 'f32', ctypes.c_double: 'f64'}[t]


def test_library_exports_every_symbol_the_header_declares():
    assert _lib.declared_loss_frameless_symbols() == NAMES == sorted(_lib._LOSS_FRAMELESS_SIGNATURES)
    assert _lib._LOSS_FRAMELESS_SIGNATURES is _abi.LOSS_FRAMELESS_FUNCTIONS
    assert _abi.LOSS_FRAMELESS_PATH == _abi.HEADER_PATH.with_name('dvsof_loss_frameless.h')
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert hasattr(lib, name), f'{name} declared in dvsof_loss_frameless.h, not exported'
    bound = _lib.lib()
    for name, (res, args) in _lib._LOSS_FRAMELESS_SIGNATURES.items():
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_signatures_are_the_recorded_ones():
    golden = json.loads((GOLDEN / 'abi_signatures_loss_frameless.json').read_text())
    assert set(golden) == set(_lib._LOSS_FRAMELESS_SIGNATURES) and len(golden) == 2
    for name, (res, args) in _lib._LOSS_FRAMELESS_SIGNATURES.items():
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name


def test_signatures_written_out_by_hand():
    vp, i, f, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    scale = ctypes.POINTER(_abi.STRUCTS['dvsof_loss_scale_t'])
    res, args = _lib._LOSS_FRAMELESS_SIGNATURES['dvsof_loss_frameless']
    assert res is i and issubclass(args[0], scale)
    assert args[1:] == [i, i, vp, f, vp, vp, vp, vp, sz, vp]
    res, args = _lib._LOSS_FRAMELESS_SIGNATURES['dvsof_loss_frameless_workspace_bytes']
    assert res is sz and issubclass(args[0], scale) and args[1:] == [i, i]


def test_the_older_tables_are_left_alone():
    taken = set()
    for file, table in OLD.items():
        golden = json.loads((GOLDEN / file).read_text())
        signatures = getattr(_lib, table)
        assert set(golden) == set(signatures), file
        for name, (res, args) in signatures.items():
            assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name
        assert not set(signatures) & set(NAMES), file
        taken |= set(signatures)
    assert not any('frameless' in n for n in taken)
    assert not any('frameless' in n for n in _lib.declared_symbols() + _lib.declared_extension_symbols()
                   + _lib.declared_contrast_multi_symbols() + _lib.declared_iwe_multi_symbols())


def test_a_c_compiler_takes_the_header(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "dvsof_loss_frameless.h"\n#include "dvsof_iwe_multi.h"\n'
                   '#include "dvsof_loss_frameless.h"\n'
                   'size_t (*const probe)(const dvsof_loss_scale_t *, int, int) = '
                   'dvsof_loss_frameless_workspace_bytes;\n'
                   'int main(void) { return sizeof(dvsof_loss_scale_t) == 32 ? 0 : 1; }\n')
    subprocess.run([os.environ.get('CC', 'cc'), '-std=c11', '-Wall', '-Werror', '-c', '-I',
                    str(_abi.HEADER_PATH.parent), str(src), '-o', str(tmp_path / 'use.o')], check=True)


def _scales(shapes, flow=8, grad=8):
    arr = (_lib.LossScale * len(shapes))()
    for k, (h, w) in enumerate(shapes):
        arr[k].frames, arr[k].flow, arr[k].grad_flow = None, flow, grad     # addresses never followed
        arr[k].h, arr[k].w = h, w
    return arr


def test_the_workspace_is_laid_out_as_the_kernels_use_it():
    """Host code only: 8 accumulators of 8 bytes per (scale, sample), one
    int32 per 64 x 16 tile, rounded up to 16 bytes plus 16; .frames is NULL
    throughout; 0 for what the call refuses."""
    lib = _lib.lib()
    for shapes, N in ((((5, 7),), 1), (((16, 64), (17, 65)), 3), (((2, 2),) * 8, 2), (((2, 257 * 64),), 2)):
        tiles = sum(N * -(-h // 16) * -(-w // 64) for h, w in shapes)
        raw = 64 * len(shapes) * N + 4 * tiles
        assert lib.dvsof_loss_frameless_workspace_bytes(_scales(shapes), len(shapes), N) == \
            (raw + 15) // 16 * 16 + 16
    one = ((4, 4),)
    assert lib.dvsof_loss_frameless_workspace_bytes(_scales(one * 9), 9, 1) == 0
    assert lib.dvsof_loss_frameless_workspace_bytes(_scales(one), 0, 1) == 0
    assert lib.dvsof_loss_frameless_workspace_bytes(_scales(one), 1, 0) == 0
    assert lib.dvsof_loss_frameless_workspace_bytes(_scales(((0, 4),)), 1, 1) == 0
    assert lib.dvsof_loss_frameless_workspace_bytes(_scales(((4, 0),)), 1, 1) == 0
    assert lib.dvsof_loss_frameless_workspace_bytes(_scales(one, flow=None), 1, 1) == 0
    assert lib.dvsof_loss_frameless_workspace_bytes(_scales(one, grad=None), 1, 1) == 0
    assert lib.dvsof_loss_frameless_workspace_bytes(None, 1, 1) == 0


def test_every_refusal_comes_before_a_launch():
    """The error returns need no device: with addresses that are never
    followed, every refused call returns its code (a launch would need a GPU,
    and this test runs without one)."""
    lib = _lib.lib()
    one = ((4, 4),)
    w = (ctypes.c_float * 2)(0.5, 1)
    need = lib.dvsof_loss_frameless_workspace_bytes(_scales(one), 1, 2)

    def call(arr, K, N, weights=w, terms=8, loss=8, oob=8, ws=8, nbytes=need):
        return lib.dvsof_loss_frameless(arr, K, N, weights, 1.0, terms, loss, oob, ws, nbytes, None)
    assert call(_scales(one * 9), 9, 2) == EINVAL
    assert call(_scales(one), 0, 2) == EINVAL
    assert call(_scales(one), 1, 0) == EINVAL
    assert call(None, 1, 2) == EINVAL
    assert call(_scales(one, flow=None), 1, 2) == EINVAL
    assert call(_scales(one, grad=None), 1, 2) == EINVAL
    assert call(_scales(((0, 4),)), 1, 2) == EINVAL
    assert call(_scales(one), 1, 2, weights=None) == EINVAL
    assert call(_scales(one), 1, 2, terms=None) == EINVAL
    assert call(_scales(one), 1, 2, loss=None) == EINVAL
    assert call(_scales(one), 1, 2, oob=None) == EINVAL
    assert call(_scales(one), 1, 2, ws=None) == ENOSPACE
    assert call(_scales(one), 1, 2, nbytes=need - 1) == ENOSPACE
    assert call(_scales(one), 1, 2, nbytes=0) == ENOSPACE
