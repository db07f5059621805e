"""CPU checks of the extension header include/dvsof_event_terms_encoded.h: the
library exports what it declares, the derived binding equals a recorded table
(tests/golden/abi_signatures_event_terms_encoded.json) and signatures written
out by hand, each from its wire twin's, a C compiler accepts the header (twice,
and beside the older ones), the older tables and structs are left as they were,
and every refusal comes before any launch, the twin's in the twin's order."""
import ctypes
import json
import os
import pathlib
import subprocess

from dvs_of_training_framework_amd import _abi, _lib, loss as L
from tests import contrast_cases as cc

TWINS = {'dvsof_contrast_multi_fwd': _lib._CONTRAST_MULTI_SIGNATURES,
         'dvsof_contrast_multi_bwd': _lib._CONTRAST_MULTI_SIGNATURES,
         'dvsof_contrast_pyramid_fwd': _lib._CONTRAST_PYRAMID_SIGNATURES,
         'dvsof_contrast_pyramid_bwd': _lib._CONTRAST_PYRAMID_SIGNATURES,
         'dvsof_avg_timestamp_fwd': _lib._AVG_TIMESTAMP_SIGNATURES,
         'dvsof_avg_timestamp_bwd': _lib._AVG_TIMESTAMP_SIGNATURES,
         'dvsof_avg_timestamp_pyramid_fwd': _lib._AVG_TIMESTAMP_PYRAMID_SIGNATURES,
         'dvsof_avg_timestamp_pyramid_bwd': _lib._AVG_TIMESTAMP_PYRAMID_SIGNATURES}
NAMES = sorted(f'{n}_encoded' for n in TWINS)
GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'abi_signatures_event_terms_encoded.json'
SIGNATURES = _lib._EVENT_TERMS_ENCODED_SIGNATURES
EINVAL, ENOSPACE = cc.EINVAL, cc.ENOSPACE


def _category(t):
    if t is _lib.ContrastLevels:
        return 'levels'
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_library_exports_every_symbol_the_header_declares():
    assert _lib.declared_event_terms_encoded_symbols() == NAMES == sorted(SIGNATURES)
    assert SIGNATURES is _abi.EVENT_TERMS_ENCODED_FUNCTIONS
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert hasattr(lib, name), f'{name} declared in dvsof_event_terms_encoded.h, not exported'
    bound = _lib.lib()
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_signatures_are_the_recorded_ones():
    golden = json.loads(GOLDEN.read_text())
    assert set(golden) == set(NAMES)
    for name, (res, args) in SIGNATURES.items():
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name


def test_every_signature_is_its_twins_with_the_columns_replaced():
    """The five column pointers of the twin become five pointers and an int
    (x, y, t, polarity, sample_event_offsets, B); everything behind is the twin's."""
    vp, i = ctypes.c_void_p, ctypes.c_int
    for twin, table in TWINS.items():
        res, args = table[twin]
        assert args[:5] == [vp] * 5 and args[5] is ctypes.c_int64, twin
        assert SIGNATURES[twin + '_encoded'] == (res, [vp] * 5 + [i] + args[5:]), twin
    assert not any(n.endswith('workspace_bytes') for n in SIGNATURES)      # the workspace is the twin's


def test_the_older_tables_and_structs_are_left_alone():
    older = set(_lib._SIGNATURES) | set(_lib._EXTENSION_SIGNATURES) | set(_lib._CONTRAST_MULTI_SIGNATURES) \
        | set(_lib._IWE_MULTI_SIGNATURES) | set(_lib._LOSS_FRAMELESS_SIGNATURES) \
        | set(_lib._CONTRAST_PYRAMID_SIGNATURES) | set(_lib._AVG_TIMESTAMP_SIGNATURES) \
        | set(_lib._AVG_TIMESTAMP_PYRAMID_SIGNATURES)
    assert not set(NAMES) & older
    assert sorted(_abi.CONTRAST_PYRAMID_STRUCTS) == ['dvsof_contrast_level_t', 'dvsof_contrast_levels_t']
    assert ctypes.sizeof(_lib.ContrastLevels) == 456 and ctypes.sizeof(_lib.ContrastLevel) == 56
    assert _lib.STRUCTS is _abi.STRUCTS and not any('level' in n for n in _abi.STRUCTS)
    golden = pathlib.Path(__file__).parent / 'golden'
    for stem, table in (('contrast_multi', _lib._CONTRAST_MULTI_SIGNATURES),
                        ('contrast_pyramid', _lib._CONTRAST_PYRAMID_SIGNATURES),
                        ('avg_timestamp', _lib._AVG_TIMESTAMP_SIGNATURES),
                        ('avg_timestamp_pyramid', _lib._AVG_TIMESTAMP_PYRAMID_SIGNATURES)):
        recorded = json.loads((golden / f'abi_signatures_{stem}.json').read_text())
        assert set(table) <= set(recorded) and not set(NAMES) & set(recorded), stem
    assert not any('encoded' in n and ('contrast' in n or 'avg_timestamp' in n) for n in _lib.declared_symbols())


def test_a_c_compiler_takes_the_header(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include <stddef.h>\n#include "dvsof_event_terms_encoded.h"\n#include "dvsof_avg_timestamp.h"\n'
                   '#include "dvsof_contrast_multi.h"\n#include "dvsof_avg_timestamp_pyramid.h"\n'
                   '#include "dvsof_event_terms_encoded.h"\n'
                   'int (*const probe)(const int16_t *, const int16_t *, const float *, const uint8_t *, '
                   'const int64_t *, int, int64_t, const float *, const int64_t *, const float *, int, int, int, '
                   'int, int, float *, void *, size_t, void *) = dvsof_avg_timestamp_fwd_encoded;\n'
                   'int main(void) { return 0; }\n')
    subprocess.run([os.environ.get('CC', 'cc'), '-std=c11', '-Wall', '-Werror', '-c', '-I',
                    str(_abi.HEADER_PATH.parent), str(src), '-o', str(tmp_path / 'use.o')], check=True)


def test_refusals_need_no_device():
    """Every refusal comes before any launch, so the calls can be made on a
    machine without a GPU: the twin's codes in the twin's order, a null
    sample_event_offsets and B < 1 where the twin refuses a null column, a null
    polarity only with polarity channels, nothing of it at n_events = 0."""
    lib = _lib.lib()
    one = ctypes.c_int64(1)                 # a non-null address nothing reads
    a = ctypes.addressof(one)
    good = ((24, 40), ((24, 40), (12, 20), (6, 10)))

    def table(M=18, **change):
        tb = L.contrast_level_table(*good, 3, M, [0.25] * 3, [a] * 3, [a] * 3)
        for k, v in change.items():
            name, level = k.rsplit('_', 1)
            setattr(tb.level[int(level)], name, v)
        return tb

    def call(name, x=a, t=a, p=a, off=a, B=2, n=5, F=3, h=24, w=40, mask=7, pol=1, ws=a, nbytes=1 << 40, out=a,
             tb=None):
        head = [x, a, t, p, off, B, n, a, a]
        tail = {'dvsof_contrast_multi_fwd': [a, F, h, w, mask, pol, out, a, a, a, ws, nbytes, None],
                'dvsof_contrast_multi_bwd': [a, F, h, w, mask, pol, a, ws, nbytes, out, 1.0, a, None],
                'dvsof_contrast_pyramid_fwd': [F, h, w, mask, pol, tb or table(), out, a, a, ws, nbytes, None],
                'dvsof_contrast_pyramid_bwd': [F, h, w, mask, pol, tb or table(), ws, nbytes, out, None],
                'dvsof_avg_timestamp_fwd': [a, F, h, w, mask, pol, out, ws, nbytes, None],
                'dvsof_avg_timestamp_bwd': [a, F, h, w, mask, pol, ws, nbytes, out, 1.0, a, None],
                'dvsof_avg_timestamp_pyramid_fwd': [F, h, w, mask, pol, tb or table(), out, a, ws, nbytes, None],
                'dvsof_avg_timestamp_pyramid_bwd': [F, h, w, mask, pol, tb or table(), ws, nbytes, out, None]}[name]
        return getattr(lib, name + '_encoded')(*head, *tail)

    for name in TWINS:
        # the twin's refusals
        for kw in (dict(F=-1), dict(n=-1), dict(mask=0), dict(mask=8), dict(pol=2), dict(F=65536), dict(F=10923),
                   dict(w=0), dict(h=32768), dict(out=None)):
            assert call(name, **kw) == EINVAL, (name, kw)
        # the columns, where the twin looks at its own
        for kw in (dict(x=None), dict(t=None), dict(p=None), dict(off=None), dict(B=0), dict(B=-3)):
            assert call(name, **kw) == EINVAL, (name, kw)
            assert call(name, ws=None, **kw) == EINVAL, (name, kw)     # before the workspace
            assert call(name, mask=0, **kw) == EINVAL, (name, kw)
        assert call(name, ws=None) == ENOSPACE and call(name, nbytes=100) == ENOSPACE, name
        # polarity may be null without polarity channels (M = 9 images then)
        assert call(name, p=None, pol=0, ws=None, tb=table(M=9)) == ENOSPACE, name
        # n_events = 0: the columns, the offsets and B are not looked at
        assert call(name, n=0, x=None, t=None, p=None, off=None, B=0, ws=None) == ENOSPACE, name
        # F = 0: nothing to do, with no pointer at all
        assert call(name, F=0, x=None, t=None, p=None, off=None, B=0, ws=None, out=None) == 0, name
    for name in ('dvsof_contrast_pyramid_fwd', 'dvsof_contrast_pyramid_bwd', 'dvsof_avg_timestamp_pyramid_fwd',
                 'dvsof_avg_timestamp_pyramid_bwd'):
        # a bad table before a bad column, as in the twin
        assert call(name, tb=table(shift_1=2), off=None) == EINVAL
        tb = table()
        tb.K = 0
        assert call(name, tb=tb, F=0) == EINVAL
