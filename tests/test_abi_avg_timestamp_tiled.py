"""CPU checks of the tiled schedule of the average-timestamp images: the library
exports what include/dvsof_avg_timestamp_tiled.h declares, the derived binding
equals the recorded table (tests/golden/abi_signatures_avg_timestamp_tiled.json)
and every twin's signature plus the three tile arguments; train_flownet.py takes
--avg-timestamp-tiled where a tiled form exists and refuses it, naming the
option, where none does; and Losses.avg_timestamp_tiled extends avg_timestamp."""
import ctypes
import inspect
import json
import pathlib

import pytest

import train_flownet as tf
from dvs_of_training_framework_amd import _abi, _lib, loss as L

NAMES = ['dvsof_avg_timestamp_fwd_encoded_tiled', 'dvsof_avg_timestamp_fwd_tiled',
         'dvsof_avg_timestamp_tiled_workspace_bytes', 'dvsof_iwe_avg_timestamp_tiled']
TWINS = {'dvsof_avg_timestamp_fwd': _abi.AVG_TIMESTAMP_FUNCTIONS,
         'dvsof_avg_timestamp_fwd_encoded': _abi.EVENT_TERMS_ENCODED_FUNCTIONS,
         'dvsof_iwe_avg_timestamp': _abi.IWE_AVG_TIMESTAMP_FUNCTIONS}


def _category(t):
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_the_headers_names_are_exported_bound_and_recorded():
    sig = _abi.AVG_TIMESTAMP_TILED_FUNCTIONS
    assert _lib.declared_avg_timestamp_tiled_symbols() == NAMES == sorted(sig)
    assert _abi.AVG_TIMESTAMP_TILED_PATH == _abi.HEADER_PATH.with_name('dvsof_avg_timestamp_tiled.h')
    raw, bound = ctypes.CDLL(str(_lib.LIB_PATH)), _lib.lib()
    golden = json.loads((pathlib.Path(__file__).parent / 'golden' / 'abi_signatures_avg_timestamp_tiled.json')
                        .read_text())
    assert set(golden) == set(sig)
    for name, (res, args) in sig.items():
        assert hasattr(raw, name), f'{name} declared in dvsof_avg_timestamp_tiled.h, not exported'
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name
    tail = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    for twin, table in TWINS.items():
        res, args = table[twin]
        assert sig[twin + '_tiled'] == (res, args + tail), twin
    i = ctypes.c_int
    assert sig['dvsof_avg_timestamp_tiled_workspace_bytes'] == (ctypes.c_size_t, [i, i, i, i, i, ctypes.c_int64])


@pytest.mark.parametrize('extra,refusal', [
    (['--avg-timestamp-weight', '0.5'], None),
    (['--sharpness-period', '5', '--sharpness-rsat'], None),
    (['--avg-timestamp-weight', '0.5', '--avg-timestamp-scales', 'all'], '--avg-timestamp-scales all'),
    (['--avg-timestamp-weight', '0.5', '--capture', '--capture-event-terms'], '--capture-event-terms'),
    ([], 'needs a positive --avg-timestamp-weight, or --sharpness-rsat with --sharpness-period')])
def test_the_parser_takes_the_flag_where_a_tiled_form_exists(extra, refusal, tmp_path):
    model = ['-m', str(tmp_path / 'm'), '--synthetic']
    if refusal is None:
        assert tf.parse_args(model + ['--avg-timestamp-tiled'] + extra).avg_timestamp_tiled is True
    else:
        with pytest.raises(SystemExit, match='--avg-timestamp-tiled.*' + refusal):
            tf.parse_args(model + ['--avg-timestamp-tiled'] + extra)
    assert not hasattr(tf.parse_args(model + extra), 'avg_timestamp_tiled')     # the run without the flag


def test_losses_avg_timestamp_tiled_takes_the_arguments_of_avg_timestamp():
    tiled = inspect.signature(L.Losses.avg_timestamp_tiled).parameters
    assert list(tiled)[:8] == list(inspect.signature(L.Losses.avg_timestamp).parameters)
    assert list(tiled)[8:] == ['tiled'] and tiled['tiled'].default is True
