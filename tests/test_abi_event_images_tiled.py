"""CPU checks of the tiled schedule of the images of warped events: the library
exports what include/dvsof_event_images_tiled.h declares, the derived binding
equals the recorded table (tests/golden/abi_signatures_event_images_tiled.json)
and every twin's signature plus the three tile arguments; and train_flownet.py
refuses --event-images-tiled where no tiled form exists, naming the option."""
import ctypes
import json
import pathlib

import pytest

import train_flownet as tf
from dvs_of_training_framework_amd import _abi, _lib

NAMES = ['dvsof_contrast_multi_fwd_encoded_tiled', 'dvsof_contrast_multi_fwd_tiled', 'dvsof_event_images_tiled_plan',
         'dvsof_event_images_tiled_workspace_bytes', 'dvsof_iwe_splat_multi_tiled']
TWINS = {'dvsof_iwe_splat_multi': _lib._IWE_MULTI_SIGNATURES,
         'dvsof_contrast_multi_fwd': _lib._CONTRAST_MULTI_SIGNATURES,
         'dvsof_contrast_multi_fwd_encoded': _lib._EVENT_TERMS_ENCODED_SIGNATURES}


def _category(t):
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_the_headers_names_are_exported_bound_and_recorded():
    sig = _lib._EVENT_IMAGES_TILED_SIGNATURES
    assert _lib.declared_event_images_tiled_symbols() == NAMES == sorted(sig)
    assert sig is _abi.EVENT_IMAGES_TILED_FUNCTIONS
    assert _abi.EVENT_IMAGES_TILED_PATH == _abi.HEADER_PATH.with_name('dvsof_event_images_tiled.h')
    raw, bound = ctypes.CDLL(str(_lib.LIB_PATH)), _lib.lib()
    golden = json.loads((pathlib.Path(__file__).parent / 'golden' / 'abi_signatures_event_images_tiled.json')
                        .read_text())
    assert set(golden) == set(sig)
    for name, (res, args) in sig.items():
        assert hasattr(raw, name), f'{name} declared in dvsof_event_images_tiled.h, not exported'
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name
    tail = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    for twin, table in TWINS.items():
        res, args = table[twin]
        assert sig[twin + '_tiled'] == (res, args + tail), twin
    i, i64 = ctypes.c_int, ctypes.c_int64
    assert sig['dvsof_event_images_tiled_plan'] == (i, [i, i, i, i, i, i64, ctypes.c_void_p])
    assert sig['dvsof_event_images_tiled_workspace_bytes'] == (ctypes.c_size_t, [i, i, i, i, i, i64])
    older = [getattr(_lib, k) for k in dir(_lib) if k.endswith('_SIGNATURES') and getattr(_lib, k) is not sig]
    assert len(older) == 10 and not any(set(t) & set(NAMES) for t in older)


@pytest.mark.parametrize('extra,named', [
    (['--contrast-weight', '0.25', '--contrast-scales', 'all'], '--contrast-scales all'),
    (['--sharpness-period', '5', '--sharpness-rsat'], '--sharpness-rsat'),
    (['--contrast-weight', '0.25', '--capture', '--capture-event-terms'], '--capture-event-terms'),
    ([], 'needs a positive --contrast-weight or --sharpness-period')])
def test_the_parser_refuses_the_flag_where_no_tiled_form_exists(extra, named, tmp_path):
    model = ['-m', str(tmp_path / 'm'), '--synthetic']
    with pytest.raises(SystemExit, match='--event-images-tiled.*' + named):
        tf.parse_args(model + ['--event-images-tiled'] + extra)
    assert tf.parse_args(model + ['--event-images-tiled', '--contrast-weight', '0.25']).event_images_tiled is True
    assert tf.parse_args(model + ['--event-images-tiled', '--sharpness-period', '5']).event_images_tiled is True
    assert not hasattr(tf.parse_args(model + extra[:4]), 'event_images_tiled')      # the run without the flag
