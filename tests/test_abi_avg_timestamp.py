"""CPU checks of the extension header include/dvsof_avg_timestamp.h: the
library exports what it declares, the derived binding equals a recorded table
(tests/golden/abi_signatures_avg_timestamp.json) and signatures written out by
hand, a C compiler accepts the header, the workspace is laid out as the header
says, every refusal comes without a device, and the older tables are left as
they were."""
import ctypes
import json
import os
import pathlib
import subprocess

import numpy as np

from dvs_of_training_framework_amd import _abi, _lib, loss as L
from tests import avg_timestamp_cases as ac

NAMES = ['dvsof_avg_timestamp_bwd', 'dvsof_avg_timestamp_fwd', 'dvsof_avg_timestamp_workspace_bytes']


def _category(t):
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_library_exports_every_symbol_the_header_declares():
    assert _lib.declared_avg_timestamp_symbols() == NAMES == sorted(_lib._AVG_TIMESTAMP_SIGNATURES)
    assert _lib._AVG_TIMESTAMP_SIGNATURES is _abi.AVG_TIMESTAMP_FUNCTIONS
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert hasattr(lib, name), f'{name} declared in dvsof_avg_timestamp.h, not exported'
    bound = _lib.lib()
    for name, (res, args) in _lib._AVG_TIMESTAMP_SIGNATURES.items():
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_signatures_are_the_recorded_ones():
    golden = json.loads((pathlib.Path(__file__).parent / 'golden' / 'abi_signatures_avg_timestamp.json').read_text())
    assert set(golden) == set(_lib._AVG_TIMESTAMP_SIGNATURES) and len(golden) == 3
    for name, (res, args) in _lib._AVG_TIMESTAMP_SIGNATURES.items():
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name


def test_signatures_written_out_by_hand():
    vp, i, f, sz, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_int64
    head = [vp, vp, vp, vp, vp, i64, vp, vp, vp, i, i, i, i, i]
    assert _lib._AVG_TIMESTAMP_SIGNATURES['dvsof_avg_timestamp_fwd'] == (i, head + [vp, vp, sz, vp])
    assert _lib._AVG_TIMESTAMP_SIGNATURES['dvsof_avg_timestamp_bwd'] == (i, head + [vp, sz, vp, f, vp, vp])
    assert _lib._AVG_TIMESTAMP_SIGNATURES['dvsof_avg_timestamp_workspace_bytes'] == (sz, [i, i, i, i, i])
    # the head is that of the contrast calls: the same columns, tables and options in the same order
    assert _lib._CONTRAST_MULTI_SIGNATURES['dvsof_contrast_multi_fwd'][1][:14] == head


def test_the_older_tables_are_left_alone():
    assert _abi.EXTENSION_PATHS == (_abi.HEADER_PATH.with_name('dvsof_contrast.h'),)
    assert sorted(_abi.EXTENSION_FUNCTIONS) == ['dvsof_contrast_bwd', 'dvsof_contrast_fwd',
                                                'dvsof_contrast_workspace_bytes']
    older = (_lib._SIGNATURES, _lib._EXTENSION_SIGNATURES, _lib._CONTRAST_MULTI_SIGNATURES,
             _lib._IWE_MULTI_SIGNATURES, _lib._LOSS_FRAMELESS_SIGNATURES, _lib._CONTRAST_PYRAMID_SIGNATURES)
    assert [len(t) for t in older[1:]] == [3, 3, 2, 2, 3]
    for table in older:
        assert not set(table) & set(NAMES)
    assert not any(n.startswith('dvsof_avg_timestamp') for n in _lib.declared_symbols())
    assert set(_abi.CONTRAST_PYRAMID_STRUCTS) == {'dvsof_contrast_level_t', 'dvsof_contrast_levels_t'}


def test_a_c_compiler_takes_the_header(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "dvsof_avg_timestamp.h"\n#include "dvsof_contrast_multi.h"\n'
                   '#include "dvsof_avg_timestamp.h"\n'
                   'size_t (*const probe)(int, int, int, int, int) = dvsof_avg_timestamp_workspace_bytes;\n'
                   'int main(void) { return 0; }\n')
    subprocess.run([os.environ.get('CC', 'cc'), '-std=c11', '-Wall', '-Werror', '-c', '-I',
                    str(_abi.HEADER_PATH.parent), str(src), '-o', str(tmp_path / 'use.o')], check=True)


def test_the_workspace_is_laid_out_as_the_header_says():
    """Host code only: q, s, base, the sums and count as one region, padded to 8 bytes; M records
    of 64 bytes, F units of 8, M rows of 32 and nb partials of 32 per image; 0 for what the calls
    refuse.  loss.avg_timestamp_layout, which the device tests read the workspace by, says the same."""
    lib = _lib.lib()
    for F, mask, pol, h, w in ((1, 1, 0, 5, 7), (3, 7, 1, 40, 40), (2, 5, 0, 33, 31), (4, 2, 1, 1, 1),
                               (1, 1, 0, 400, 400)):
        M = F * bin(mask).count('1') * (1 + pol)
        P, S = M * h * w, 2 * F * h * w
        nb = min(max((h * w + 1023) // 1024, 1), 128)
        zeroed = 8 * P + 8 * P + 8 * P + 8 * S + 4 * P
        want = (zeroed + 7) // 8 * 8 + 64 * M + 8 * F + 32 * M + 32 * M * nb
        assert lib.dvsof_avg_timestamp_workspace_bytes(F, mask, pol, h, w) == want
        lay = L.avg_timestamp_layout(F, M, h, w)
        assert lay['bytes'] == want and lay['zeroed_bytes'] == zeroed and lay['nb'] == nb
        assert (lay['q'], lay['s'], lay['base'], lay['sums'], lay['count']) == (0, 8 * P, 16 * P, 24 * P,
                                                                                24 * P + 8 * S)
        assert lay['rec'] % 8 == 0 and lay['unit'] == lay['rec'] + 64 * M and lay['rows'] == lay['unit'] + 8 * F
    assert L.AVG_TIMESTAMP_REC_DTYPE.itemsize == 64 and L.AVG_TIMESTAMP_ROW_DTYPE.itemsize == 32
    for bad in ((0, 7, 1, 4, 4), (-1, 7, 1, 4, 4), (65536, 1, 0, 4, 4), (1, 0, 0, 4, 4), (1, 8, 0, 4, 4),
                (1, 7, 2, 4, 4), (1, 7, -1, 4, 4), (1, 7, 1, 0, 4), (1, 7, 1, 4, 32768), (10923, 7, 1, 4, 4)):
        assert lib.dvsof_avg_timestamp_workspace_bytes(*bad) == 0, bad
    assert lib.dvsof_avg_timestamp_workspace_bytes(10922, 7, 1, 1, 1) > 0       # M = 65532


def test_every_refusal_comes_before_any_launch_and_needs_no_device():
    """The addresses are host arrays nothing reads: a call that got as far as a launch would
    fail on a machine without a device, a refused one returns its code."""
    lib = _lib.lib()
    F, h, w, n = 2, 5, 7, 11
    need = lib.dvsof_avg_timestamp_workspace_bytes(F, 7, 1, h, w)
    held = {k: np.full(64, 7, np.uint8) for k in ('x', 'y', 't', 'p', 's', 'ts', 'fs', 'flow', 'term', 'seed',
                                                   'grad')}
    held['ws'] = np.full(need, 7, np.uint8)
    a = {k: v.ctypes.data for k, v in held.items()}
    a['n'] = n
    seen = 0
    for what, call, expect in ac.bad_calls(lib, a, F, h, w):
        assert call() == expect, what
        seen += 1
    assert seen >= 55
    assert all(bool((v == 7).all()) for v in held.values())
    assert all(rc == 0 for rc in ac.empty_calls(lib))
    # a null p is refused only where it would be read: with polarity and events
    assert lib.dvsof_avg_timestamp_fwd(a['x'], a['y'], a['t'], None, a['s'], n, a['ts'], a['fs'], a['flow'], F, h, w,
                                       7, 1, a['term'], a['ws'], need, None) == ac.EINVAL
    # the order of the refusals: the options before the sizes, the pointers before the workspace
    assert lib.dvsof_avg_timestamp_fwd(None, None, None, None, None, n, None, None, None, F, 0, w, 9, 1, None, None,
                                       0, None) == ac.EINVAL
    assert lib.dvsof_avg_timestamp_fwd(a['x'], a['y'], a['t'], a['p'], a['s'], n, a['ts'], a['fs'], a['flow'], F, h,
                                       w, 7, 1, None, None, 0, None) == ac.EINVAL
    assert lib.dvsof_avg_timestamp_bwd(a['x'], a['y'], a['t'], a['p'], a['s'], n, a['ts'], a['fs'], a['flow'], F, h,
                                       w, 7, 1, None, 0, a['seed'], 1.0, a['grad'], None) == ac.ENOSPACE
