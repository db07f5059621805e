"""CPU checks of the tiled schedule of the events-only terms on every flow scale:
the library exports what include/dvsof_event_pyramids_tiled.h declares, the
derived binding equals the recorded table
(tests/golden/abi_signatures_event_pyramids_tiled.json) and every twin's
signature plus the three tile arguments; and train_flownet.py takes
--event-pyramids-tiled with either ``... all`` option and refuses it, naming
the option, where no term runs on every scale."""
import ctypes
import json
import pathlib

import pytest

import train_flownet as tf
from dvs_of_training_framework_amd import _abi, _lib

NAMES = ['dvsof_avg_timestamp_pyramid_fwd_encoded_tiled', 'dvsof_avg_timestamp_pyramid_fwd_tiled',
         'dvsof_avg_timestamp_pyramid_tiled_workspace_bytes', 'dvsof_contrast_pyramid_fwd_encoded_tiled',
         'dvsof_contrast_pyramid_fwd_tiled', 'dvsof_contrast_pyramid_tiled_workspace_bytes',
         'dvsof_event_pyramids_tiled_plan']
TWINS = {'dvsof_contrast_pyramid_fwd': _abi.CONTRAST_PYRAMID_FUNCTIONS,
         'dvsof_contrast_pyramid_fwd_encoded': _abi.EVENT_TERMS_ENCODED_FUNCTIONS,
         'dvsof_avg_timestamp_pyramid_fwd': _abi.AVG_TIMESTAMP_PYRAMID_FUNCTIONS,
         'dvsof_avg_timestamp_pyramid_fwd_encoded': _abi.EVENT_TERMS_ENCODED_FUNCTIONS}


def _category(t):
    if t is _lib.ContrastLevels:
        return 'levels'
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_the_headers_names_are_exported_bound_and_recorded():
    sig = _abi.EVENT_PYRAMIDS_TILED_FUNCTIONS
    assert _lib.declared_event_pyramids_tiled_symbols() == NAMES == sorted(sig)
    assert _abi.EVENT_PYRAMIDS_TILED_PATH == _abi.HEADER_PATH.with_name('dvsof_event_pyramids_tiled.h')
    raw, bound = ctypes.CDLL(str(_lib.LIB_PATH)), _lib.lib()
    golden = json.loads((pathlib.Path(__file__).parent / 'golden' / 'abi_signatures_event_pyramids_tiled.json')
                        .read_text())
    assert set(golden) == set(sig)
    for name, (res, args) in sig.items():
        assert hasattr(raw, name), f'{name} declared in dvsof_event_pyramids_tiled.h, not exported'
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name
    tail = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    for twin, table in TWINS.items():
        res, args = table[twin]
        assert sig[twin + '_tiled'] == (res, args + tail), twin
    i, i64, lv = ctypes.c_int, ctypes.c_int64, _lib.ContrastLevels
    assert sig['dvsof_event_pyramids_tiled_plan'] == (i, [i, i, i, i, i, lv, i64, ctypes.c_void_p])
    for family in ('contrast', 'avg_timestamp'):
        assert sig[f'dvsof_{family}_pyramid_tiled_workspace_bytes'] == (ctypes.c_size_t, [i, i, i, i, i, lv, i64])


@pytest.mark.parametrize('extra,refusal', [
    (['--contrast-weight', '0.25', '--contrast-scales', 'all'], None),
    (['--avg-timestamp-weight', '0.5', '--avg-timestamp-scales', 'all'], None),
    (['--contrast-weight', '0.25', '--contrast-scales', 'all', '--capture', '--capture-event-terms'],
     '--capture-event-terms'),
    (['--contrast-weight', '0.25', '--avg-timestamp-weight', '0.5'],
     'needs --contrast-weight with --contrast-scales all'),
    ([], 'needs --contrast-weight with --contrast-scales all')])
def test_the_parser_takes_the_flag_where_a_term_runs_on_every_scale(extra, refusal, tmp_path):
    model = ['-m', str(tmp_path / 'm'), '--synthetic']
    if refusal is None:
        assert tf.parse_args(model + ['--event-pyramids-tiled'] + extra).event_pyramids_tiled is True
    else:
        with pytest.raises(SystemExit, match='--event-pyramids-tiled.*' + refusal):
            tf.parse_args(model + ['--event-pyramids-tiled'] + extra)
    assert not hasattr(tf.parse_args(model + extra), 'event_pyramids_tiled')        # the run without the flag
