"""CPU checks of the extension header include/dvsof_iwe_avg_timestamp.h: the
library exports what it declares, the derived binding equals a recorded table
(tests/golden/abi_signatures_iwe_avg_timestamp.json) and signatures written out
by hand, a C compiler accepts the header, the older tables are left as they
were, and the two size functions give what the header states."""
import ctypes
import json
import os
import pathlib
import subprocess

from dvs_of_training_framework_amd import _abi, _lib

NAMES = ['dvsof_iwe_avg_timestamp', 'dvsof_iwe_avg_timestamp_image_bytes', 'dvsof_iwe_avg_timestamp_render',
         'dvsof_iwe_avg_timestamp_workspace_bytes']
IWE_MULTI_NAMES = ['dvsof_iwe_multi_images', 'dvsof_iwe_splat_multi']
AVG_TIMESTAMP_NAMES = ['dvsof_avg_timestamp_bwd', 'dvsof_avg_timestamp_fwd', 'dvsof_avg_timestamp_workspace_bytes']
OLDER = {'abi_signatures.json': '_SIGNATURES', 'abi_signatures_contrast.json': '_EXTENSION_SIGNATURES',
         'abi_signatures_contrast_multi.json': '_CONTRAST_MULTI_SIGNATURES',
         'abi_signatures_iwe_multi.json': '_IWE_MULTI_SIGNATURES',
         'abi_signatures_loss_frameless.json': '_LOSS_FRAMELESS_SIGNATURES',
         'abi_signatures_contrast_pyramid.json': '_CONTRAST_PYRAMID_SIGNATURES',
         'abi_signatures_avg_timestamp.json': '_AVG_TIMESTAMP_SIGNATURES',
         'abi_signatures_avg_timestamp_pyramid.json': '_AVG_TIMESTAMP_PYRAMID_SIGNATURES',
         'abi_signatures_event_terms_encoded.json': '_EVENT_TERMS_ENCODED_SIGNATURES'}
GOLDEN = pathlib.Path(__file__).parent / 'golden'


def _category(t):
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_library_exports_every_symbol_the_header_declares():
    assert _lib.declared_iwe_avg_timestamp_symbols() == NAMES == sorted(_lib._IWE_AVG_TIMESTAMP_SIGNATURES)
    assert _lib._IWE_AVG_TIMESTAMP_SIGNATURES is _abi.IWE_AVG_TIMESTAMP_FUNCTIONS
    assert _abi.IWE_AVG_TIMESTAMP_PATH == _abi.HEADER_PATH.with_name('dvsof_iwe_avg_timestamp.h')
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert hasattr(lib, name), f'{name} declared in dvsof_iwe_avg_timestamp.h, not exported'
    bound = _lib.lib()
    for name, (res, args) in _lib._IWE_AVG_TIMESTAMP_SIGNATURES.items():
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_signatures_are_the_recorded_ones():
    golden = json.loads((GOLDEN / 'abi_signatures_iwe_avg_timestamp.json').read_text())
    assert set(golden) == set(_lib._IWE_AVG_TIMESTAMP_SIGNATURES) and len(golden) == 4
    for name, (res, args) in _lib._IWE_AVG_TIMESTAMP_SIGNATURES.items():
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name


def test_signatures_written_out_by_hand():
    vp, i, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    sig = _lib._IWE_AVG_TIMESTAMP_SIGNATURES
    assert sig['dvsof_iwe_avg_timestamp_image_bytes'] == (sz, [i, i, i, i, i])
    assert sig['dvsof_iwe_avg_timestamp_workspace_bytes'] == (sz, [i, i, i, i, i])
    assert sig['dvsof_iwe_avg_timestamp'] == \
        (i, [vp, vp, vp, vp, i64, vp, vp, vp, i, i, i, i, i, vp, sz, vp, vp, sz, vp])
    assert sig['dvsof_iwe_avg_timestamp_render'] == (i, [vp, i, i, i, i, i, vp, vp])


def test_the_older_tables_are_left_alone():
    assert _abi.EXTENSION_PATHS == (_abi.HEADER_PATH.with_name('dvsof_contrast.h'),)
    assert sorted(_abi.IWE_MULTI_FUNCTIONS) == IWE_MULTI_NAMES == _lib.declared_iwe_multi_symbols()
    assert sorted(_abi.AVG_TIMESTAMP_FUNCTIONS) == AVG_TIMESTAMP_NAMES == _lib.declared_avg_timestamp_symbols()
    older = set()
    for file, table in OLDER.items():
        names = set(getattr(_lib, table))
        recorded = {k for k in json.loads((GOLDEN / file).read_text()) if not k.endswith('_t')}    # functions
        assert recorded == names, file
        assert not names & older and not names & set(NAMES), file
        older |= names
    assert not any(n in NAMES for n in _lib.declared_symbols())
    # functions only: no struct and no constant of its own
    assert set(_abi.STRUCTS) == set(_abi.Abi(_abi.IWE_AVG_TIMESTAMP_PATH.read_text(), base=_abi._header,
                                             name='dvsof_iwe_avg_timestamp.h').structs)


def test_a_c_compiler_takes_the_header(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "dvsof_iwe_avg_timestamp.h"\n#include "dvsof_iwe_multi.h"\n'
                   '#include "dvsof_avg_timestamp.h"\n#include "dvsof_iwe_avg_timestamp.h"\n'
                   'size_t (*const probe)(int, int, int, int, int) = dvsof_iwe_avg_timestamp_image_bytes;\n'
                   'int (*const draw)(const void *, int, int, int, int, int, uint8_t *, void *) =\n'
                   '    dvsof_iwe_avg_timestamp_render;\n'
                   'int main(void) { return sizeof(dvsof_iwe_result_t) == 48 ? 0 : 1; }\n')
    subprocess.run([os.environ.get('CC', 'cc'), '-std=c11', '-Wall', '-Werror', '-c', '-I',
                    str(_abi.HEADER_PATH.parent), str(src), '-o', str(tmp_path / 'use.o')], check=True)


def test_the_sizes_are_what_the_header_says():
    """Host code only.  The region: 28 bytes per pixel of the M images, padded to 8; the
    workspace: 32 bytes per image and partial block; 0 for what the call refuses."""
    lib = _lib.lib()

    def nb(h, w):
        return min(max((h * w + 1023) // 1024, 1), 128)
    for F, h, w, mask, pol in ((1, 1, 1, 1, 0), (3, 5, 7, 7, 1), (2, 33, 37, 5, 0), (4, 3, 129, 2, 1),
                               (1, 400, 400, 4, 0), (65535, 1, 1, 4, 0), (10922, 1, 3, 7, 1), (1, 32767, 2, 1, 0),
                               (2, 32, 32, 1, 0), (2, 32, 33, 1, 0)):
        M = F * bin(mask).count('1') * (1 + pol)
        P = M * h * w
        assert lib.dvsof_iwe_avg_timestamp_image_bytes(F, h, w, mask, pol) == (28 * P + 7) // 8 * 8, (F, h, w)
        assert lib.dvsof_iwe_avg_timestamp_workspace_bytes(F, h, w, mask, pol) == 32 * M * nb(h, w), (F, h, w)
        assert lib.dvsof_iwe_stats_workspace_bytes(M, h, w) == 48 * M * nb(h, w)       # the same partial blocks
    assert lib.dvsof_iwe_avg_timestamp_image_bytes(1, 1, 1, 1, 0) == 32          # 28 bytes, padded
    for bad in ((0, 4, 4, 7, 1), (-1, 4, 4, 7, 1), (65536, 4, 4, 1, 0), (1, 0, 4, 1, 0), (1, 4, 0, 1, 0),
                (1, -3, 4, 1, 0), (1, 32768, 4, 1, 0), (1, 4, 32768, 1, 0), (1, 4, 4, 0, 0), (1, 4, 4, 8, 0),
                (1, 4, 4, -1, 0), (1, 4, 4, 7, 2), (1, 4, 4, 7, -1), (10923, 4, 4, 7, 1), (32768, 4, 4, 1, 1),
                (32768, 4, 4, 3, 0)):
        assert lib.dvsof_iwe_avg_timestamp_image_bytes(*bad) == 0, bad
        assert lib.dvsof_iwe_avg_timestamp_workspace_bytes(*bad) == 0, bad
