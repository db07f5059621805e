"""CPU checks of the drop-in boundary: the C-ABI library loads without a GPU
and exports every symbol include/dvsof.h declares; the Python side refuses to
run without device tensors (no CPU fallback).  The binding is derived from the
header (_abi.py), so it is pinned against authorities other than the header:
the C compiler's layouts, signatures written out by hand, the recorded table
tests/golden/abi_signatures.json, literal constants, and constructs the reader
must refuse."""
import ctypes
import json
import os
import pathlib
import subprocess

import pytest
import torch

from dvs_of_training_framework_amd import _abi, _lib


def test_library_loads_and_exports_every_declared_symbol():
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    declared = _lib.declared_symbols()
    assert 'dvsof_loss_fwd' in declared and len(declared) >= 9
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in dvsof.h, not exported'


def test_every_declared_symbol_has_a_python_signature():
    for name in _lib.declared_symbols():
        assert name in _lib._SIGNATURES, name


def test_version_and_error_strings():
    lib = _lib.lib()
    assert lib.dvsof_version() == 100
    assert b'workspace' in lib.dvsof_error_string(-2)
    assert b'invalid' in lib.dvsof_error_string(-1)


def test_no_cpu_fallback():
    from dvs_of_training_framework_amd.loss import Losses
    ev = Losses([(4, 4)], 1, 'cpu')
    z = torch.zeros
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ev([z(1, 2, 4, 4)], z(1, 2), z(1, dtype=torch.long), z(2, 1, 4, 4),
           z(2), z(2, dtype=torch.long))


def test_product_package_never_imports_the_oracle():
    import pathlib
    pkg = pathlib.Path(_lib.__file__).parent
    for py in pkg.rglob('*.py'):
        text = py.read_text()
        assert 'import oracle' not in text and 'from oracle' not in text, py


def _desc(B, H, W, cin, cout, layout=0, stride=1, up=False, mfma=0, nsrc=1):
    """Descriptor with dummy (never dereferenced) source pointers: the
    planning entry points below only read the shape fields."""
    from dvs_of_training_framework_amd import conv as C
    d = C.ConvDesc()
    d.nsrc = nsrc
    for i in range(nsrc):
        d.src[i].p, d.src[i].C, d.src[i].layout = 4096, cin, layout
    d.B, d.H, d.W = B, H, W
    d.upsample, d.ksize, d.stride, d.pad = int(up), 3, stride, 1
    d.Cout, d.act, d.mfma = cout, C.ACT_RELU, mfma
    return d


def test_winograd_planning_is_a_pure_function_of_the_shape():
    """Host-side dispatch of the wide 3x3 layers (no GPU needed): F(4x4,3x3)
    from 64 tiles on 4-aligned images, F(2x2,3x3) from 128 tiles, the direct
    kernel below (batch-1 inference), for narrow / strided / up-sampling /
    multi-source layers and for bf16-rounded operands; prepared-weight and
    scratch sizes follow the form."""
    from dvs_of_training_framework_amd import conv as C
    lib = C._lib.lib()
    ref = ctypes.byref

    def plan(d):
        return (lib.dvsof_conv2d_winograd_tile(ref(d), 0),
                lib.dvsof_conv2d_winograd_tile(ref(d), 2),
                lib.dvsof_conv2d_scratch_bytes(ref(d)),
                lib.dvsof_conv2d_fwd_weight_elems(ref(d)),
                lib.dvsof_conv2d_dgrad_weight_elems(ref(d)))
    raw = 512 * 512 * 9
    # the headline residual layer: batch 8, 16x16, 512 -> 512: 128 tiles of 4x4
    f, w, scratch, nf, ndg = plan(_desc(8, 16, 16, 512, 512))
    assert (f, w) == (4, 4) and nf == ndg == 36 * 512 * 512
    assert scratch == 36 * 128 * (512 + 512) * 4
    # batch 4: 64 4x4 tiles forward, weight gradient falls back to the 2x2 form (< 128 tiles)
    assert plan(_desc(4, 16, 16, 512, 512))[:2] == (4, 2)
    # batch 2: 32 4x4 tiles -> 2x2 form (128 tiles); batch 1: direct
    assert plan(_desc(2, 16, 16, 512, 512))[:2] == (2, 2)
    assert plan(_desc(1, 16, 16, 512, 512)) == (0, 0, 0, raw, raw)
    # W not a multiple of 4 -> 2x2 form; odd sizes -> direct
    assert plan(_desc(8, 16, 18, 256, 256))[0] == 2
    assert plan(_desc(8, 15, 16, 256, 256))[0] == 0
    # bf16x3 operands keep the 2x2 form, bf16-rounded operands the direct kernel
    assert plan(_desc(8, 16, 16, 512, 512, mfma=2))[:2] == (2, 2)
    assert plan(_desc(8, 16, 16, 512, 512, mfma=1))[0] == 0
    # not a wide 3x3 stride-1 single-source NHWC layer -> direct
    for d in (_desc(8, 16, 16, 128, 512), _desc(8, 16, 16, 512, 128),
              _desc(8, 32, 32, 512, 512, stride=2), _desc(8, 16, 16, 512, 512, up=True),
              _desc(8, 16, 16, 512, 512, layout=1), _desc(8, 16, 16, 256, 256, nsrc=2)):
        assert lib.dvsof_conv2d_winograd_tile(ref(d), 0) == 0
        assert lib.dvsof_conv2d_scratch_bytes(ref(d)) == 0


def test_tile_ids_follow_the_measured_rule():
    """64x64 for every forward / data-gradient problem with more than 32
    output channels, 128x32 for the 32-channel stage (profiles/round1/i_tile_sweep.txt)."""
    from dvs_of_training_framework_amd import conv as C
    lib = C._lib.lib()
    assert lib.dvsof_conv2d_tile_id(ctypes.byref(_desc(8, 64, 64, 64, 128, stride=2)), 0) == 3
    assert lib.dvsof_conv2d_tile_id(ctypes.byref(_desc(8, 128, 128, 64, 32, up=True)), 0) == 5
    assert lib.dvsof_conv2d_tile_id(ctypes.byref(_desc(1, 16, 16, 512, 512)), 0) == 3


# ------------------------------------------------ the reader of include/dvsof.h
_STRUCTS = ('dvsof_eval_result_t', 'dvsof_render_item_t', 'dvsof_render_stats_t',
            'dvsof_eval_panel_stats_t', 'dvsof_iwe_result_t', 'dvsof_loss_scale_t', 'dvsof_src_t',
            'dvsof_conv_desc_t', 'dvsof_grad_dst_t')


def test_struct_layouts_are_the_c_compilers(tmp_path):
    """sizeof of every struct and offsetof of every field, printed by a C
    program that includes dvsof.h, against the derived Structures and the numpy
    dtypes made from them."""
    from dvs_of_training_framework_amd import conv, eval as ev, visualization as vis
    assert tuple(_abi.STRUCTS) == _STRUCTS
    lines = []
    for name, cls in _abi.STRUCTS.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dvsof.h"\n'
                   'int main(void) {\n' + '\n'.join(lines) + '\nreturn 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run([os.environ.get('CC', 'cc'), '-std=c11', '-I', str(_abi.HEADER_PATH.parent),
                    str(src), '-o', str(exe)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                     text=True).stdout.splitlines())
    dtypes = {'dvsof_eval_result_t': ev.RESULT_DTYPE, 'dvsof_iwe_result_t': ev.IWE_RESULT_DTYPE,
              'dvsof_render_item_t': vis.ITEM_DTYPE, 'dvsof_render_stats_t': vis.STATS_DTYPE,
              'dvsof_eval_panel_stats_t': vis.PANEL_STATS_DTYPE,
              'dvsof_loss_scale_t': _abi.dtype_of(_lib.LossScale), 'dvsof_src_t': _abi.dtype_of(conv.Src),
              'dvsof_grad_dst_t': _abi.dtype_of(conv.GradDst)}
    with pytest.raises(TypeError):      # an array of nested structs is no record
        _abi.dtype_of(conv.ConvDesc)
    checked = 0
    for name, cls in _abi.STRUCTS.items():
        assert ctypes.sizeof(cls) == int(c[name]), name
        dt = dtypes.get(name)
        assert dt is None or dt.itemsize == int(c[name]), name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == int(c[f'{name}.{f}']), (name, f)
            assert dt is None or dt.fields[f][1] == int(c[f'{name}.{f}']), (name, f)
            checked += 1
        assert dt is None or dt.names == tuple(f for f, _ in cls._fields_)
    assert checked == len(c) - len(_STRUCTS) and len(conv.ConvDesc._fields_) == 24
    assert conv.ConvDesc is _abi.STRUCTS['dvsof_conv_desc_t'] and _lib.LossScale is _abi.STRUCTS['dvsof_loss_scale_t']
    assert conv.ConvDesc.src.size == 3 * ctypes.sizeof(conv.Src)


def test_signatures_written_out_by_hand():
    """One function per mapping rule of the reader."""
    from dvs_of_training_framework_amd import conv
    vp, i, f, sz, P = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.POINTER
    want = {
        'dvsof_error_string': (ctypes.c_char_p, [i]),
        'dvsof_loss_workspace_bytes': (sz, [P(_lib.LossScale), i, i]),
        'dvsof_conv2d_dgrad': (i, [P(conv.ConvDesc), vp, vp, P(conv.GradDst), i, vp]),
        'dvsof_to_bf16_many': (i, [vp, vp, vp, i, vp]),
        'dvsof_grad_guard': (i, [vp, i, vp, vp, i, vp, sz, ctypes.c_double, i, vp, vp]),
        'dvsof_adamw_dynamic': (None, [f, f, f, i, vp]),
    }
    for name, (res, args) in want.items():
        got_res, got_args = _lib._SIGNATURES[name]
        assert got_res is res and len(got_args) == len(args), name
        for k, (g, w) in enumerate(zip(got_args, args)):
            # a struct pointer is POINTER(Structure) that converts an address too
            assert g is w or (hasattr(w, '_type_') and issubclass(g, w) and g._type_ is w._type_), (name, k)
    desc = conv.ConvDesc()
    p = _lib._SIGNATURES['dvsof_conv2d_dgrad'][1][0]
    assert p.from_param(ctypes.addressof(desc)).value == ctypes.addressof(desc)
    p.from_param(ctypes.byref(desc)), p.from_param(None)
    for wrong in (conv.GradDst(), 1.5, 'desc'):
        with pytest.raises(TypeError):
            p.from_param(wrong)


def _category(t):
    if t is None:
        return 'void'
    if t is ctypes.c_char_p:
        return 'cstr'
    if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_uint64: 'u64',
            ctypes.c_ulonglong: 'u64', ctypes.c_float: 'f32', ctypes.c_double: 'f64'}[t]


def test_signatures_are_the_recorded_ones():
    """tests/golden/abi_signatures.json: {name: [arity, [category of the return
    value, category of every argument]]}, recorded from the hand-kept tables
    this binding replaced.  A pull request that changes the ABI changes that
    file in the same diff."""
    golden = json.loads((pathlib.Path(__file__).parent / 'golden' / 'abi_signatures.json').read_text())
    assert len(golden) == 114
    assert set(golden) == set(_lib._SIGNATURES) == set(_lib.declared_symbols())
    for name, (res, args) in _lib._SIGNATURES.items():
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name


def test_constants_by_literal():
    from dvs_of_training_framework_amd import conv, visualization
    assert _abi.CONSTANTS['DVSOF_VERSION'] == 100
    assert conv.K_WGRAD_MIN == 14 and len(conv.KERNEL_NAMES) == 17 and conv.KERNEL_NAMES[1] == 'general_v1'
    assert _lib.MAX_SCALES == 8 and visualization.MAX_CHUNKS == 64
    assert (conv.ACT_NONE, conv.ACT_RELU, conv.ACT_MISH, conv.NHWC, conv.NCHW, conv.WGRAD_SKIP_FLAT) == (0, 1, 2, 0, 1, 1)
    assert (visualization.FLOW, visualization.FRAME, visualization.FILL) == (0, 1, 2)
    assert _abi.CONSTANTS['DVSOF_ECOMM'] == -3


@pytest.mark.parametrize('line,header', [
    (1, 'int dvsof_x(widget_t *w);'),                           # an unknown type
    (2, '\nint dvsof_x(int (*callback)(int), void *stream);'),  # a function pointer parameter
    (3, 'typedef struct {\n  int a;\n  int b : 3;\n} dvsof_x_t;'),   # a bit field
    (2, '\ntypedef union { int a; float b; } dvsof_x_t;'),      # a union
    (3, '/* two lines\n */\nenum { DVSOF_A = 1, DVSOF_B };'),   # an enum member without =
    (4, 'int dvsof_ok(void);\n\n\nint dvsof_x(int a)'),         # no terminating ;
])
def test_reader_refuses_what_it_does_not_know(line, header):
    with pytest.raises(_abi.AbiError, match=rf'line {line}:'):
        _abi.Abi(header)


def test_reader_accepts_the_grammar_of_the_header():
    """Every construct the header uses, in four lines."""
    a = _abi.Abi('#define DVSOF_N 0x10 /* hex */\nenum { DVSOF_A = -1, };\n'
                 'typedef struct { const float *p; int a, b; uint8_t c[3]; } dvsof_s_t;\n'
                 'typedef struct { dvsof_s_t s[2]; size_t n; } dvsof_t_t;\n'
                 'const char *dvsof_f(const dvsof_s_t *s, float *const *pp, const int hs[],\n'
                 '                    unsigned long long n /* count */, char *name, void *stream);\n'
                 'void dvsof_g(void);')
    assert a.constants == {'DVSOF_N': 16, 'DVSOF_A': -1}
    s, t = a.structs['dvsof_s_t'], a.structs['dvsof_t_t']
    assert [n for n, _ in s._fields_] == ['p', 'a', 'b', 'c'] and ctypes.sizeof(s) == 24
    assert t.n.offset == 48 and t.s.size == 48
    res, args = a.functions['dvsof_f']
    assert res is ctypes.c_char_p and args[0]._type_ is s
    assert args[1:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_char_p, ctypes.c_void_p]
    assert a.functions['dvsof_g'] == (None, [])
