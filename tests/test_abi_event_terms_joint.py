"""CPU checks of the joint calls of the two events-only terms: the library
exports what include/dvsof_event_terms_joint.h declares, the derived binding
equals the recorded table (tests/golden/abi_signatures_event_terms_joint.json);
and train_flownet.py takes --event-terms-joint where both terms can share one
splat and refuses it, naming the condition, everywhere else."""
import ctypes
import json
import pathlib

import pytest
import torch

import train_flownet as tf
from dvs_of_training_framework_amd import _abi, _lib, training

NAMES = ['dvsof_event_terms_joint_bwd', 'dvsof_event_terms_joint_bwd_encoded', 'dvsof_event_terms_joint_fwd',
         'dvsof_event_terms_joint_fwd_encoded', 'dvsof_event_terms_joint_workspace_bytes']
BOTH = ['--contrast-weight', '0.25', '--avg-timestamp-weight', '0.5']
ALL = ['--contrast-scales', 'all', '--avg-timestamp-scales', 'all']


def _category(t):
    if t is _lib.ContrastLevels:
        return 'levels'
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'ptr'
    return {ctypes.c_int: 'int', ctypes.c_int64: 'i64', ctypes.c_size_t: 'u64', ctypes.c_float: 'f32'}[t]


def test_the_headers_names_are_exported_bound_and_recorded():
    sig = _abi.EVENT_TERMS_JOINT_FUNCTIONS
    assert _lib.declared_event_terms_joint_symbols() == NAMES == sorted(sig)
    assert _abi.EVENT_TERMS_JOINT_PATH == _abi.HEADER_PATH.with_name('dvsof_event_terms_joint.h')
    raw, bound = ctypes.CDLL(str(_lib.LIB_PATH)), _lib.lib()
    golden = json.loads((pathlib.Path(__file__).parent / 'golden' / 'abi_signatures_event_terms_joint.json')
                        .read_text())
    assert set(golden) == set(sig)
    for name, (res, args) in sig.items():
        assert hasattr(raw, name), f'{name} declared in dvsof_event_terms_joint.h, not exported'
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert [len(args), [_category(res)] + [_category(a) for a in args]] == golden[name], name
    # the twins' event columns and frame tables in front, the three tile arguments behind the forward
    for form, table in (('', _abi.AVG_TIMESTAMP_PYRAMID_FUNCTIONS), ('_encoded', _abi.EVENT_TERMS_ENCODED_FUNCTIONS)):
        head = table['dvsof_avg_timestamp_pyramid_fwd' + form][1]
        head = head[:head.index(_lib.ContrastLevels) - 2]           # up to (F, h, w)
        for which in ('fwd', 'bwd'):
            assert sig[f'dvsof_event_terms_joint_{which}{form}'][1][:len(head)] == head
        assert sig['dvsof_event_terms_joint_fwd' + form][1][-3:] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]


@pytest.mark.parametrize('extra,refusal', [
    (BOTH, None),
    (BOTH + ALL + ['--event-pyramids-tiled'], None),
    (BOTH + ['--event-pyramids-tiled', '--avg-timestamp-references', 'start,middle,end', '--contrast-references',
             'middle'], None),
    (['--contrast-weight', '0.25'], 'needs both terms'),
    (['--avg-timestamp-weight', '0.5'], 'needs both terms'),
    (BOTH + ['--contrast-references', 'middle'], 'subset of the --avg-timestamp-references'),
    (BOTH + ['--contrast-polarity'], 'same polarity'),
    (BOTH + ['--contrast-scales', 'all'], 'same scales'),
    (BOTH + ALL + ['--capture', '--capture-event-terms'], '--capture-event-terms'),
    (BOTH + ['--event-images-tiled'], '--event-images-tiled'),
    (BOTH + ['--avg-timestamp-tiled'], '--avg-timestamp-tiled')])
def test_the_parser_takes_the_flag_where_both_terms_share_a_splat(extra, refusal, tmp_path):
    model = ['-m', str(tmp_path / 'm'), '--synthetic']
    if refusal is None:
        assert tf.parse_args(model + ['--event-terms-joint'] + extra).event_terms_joint is True
    else:
        with pytest.raises(SystemExit, match='--event-terms-joint.*' + refusal):
            tf.parse_args(model + ['--event-terms-joint'] + extra)
    assert not hasattr(tf.parse_args(model + [a for a in extra if a != '--event-pyramids-tiled' or 'all' in extra]),
                       'event_terms_joint')                         # the run without the flag


@pytest.mark.parametrize('change,refusal', [
    (dict(avg_timestamp_weight=0.0), 'needs both terms'), (dict(contrast_weight=0.0), 'needs both terms'),
    (dict(contrast_references=('middle',)), 'subset of the avg-timestamp references'),
    (dict(avg_timestamp_polarity=True), 'same polarity'), (dict(contrast_scales='all'), 'same scales'),
    (dict(capture_event_terms=True), 'capture_event_terms'), (dict(contrast_tiled=True), 'contrast_tiled'),
    (dict(avg_timestamp_tiled=True), 'avg_timestamp_tiled'), ({}, None)])
def test_the_training_loop_names_the_condition_it_refuses(change, refusal):
    options = dict(dict(contrast_weight=0.25, avg_timestamp_weight=0.5, contrast_references=('start',),
                        avg_timestamp_references=('start', 'end'), contrast_polarity=False,
                        avg_timestamp_polarity=False, contrast_scales='finest', avg_timestamp_scales='finest'),
                   **change)
    got = training.event_terms_joint_refusal(**options)
    assert got is None if refusal is None else refusal in got


def test_combined_loss_refuses_the_flag_with_one_term_only():
    flows = [torch.zeros(1, 2, 4, 4)]
    with pytest.raises(ValueError, match='event_terms_joint needs both terms'):
        training.combined_loss(lambda *a, **k: ((flows[0].sum(),),) * 3, flows, None, None, None, None, None, None,
                               contrast_weight=0.25, events={}, event_terms_joint=True)
