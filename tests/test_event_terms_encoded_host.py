"""The events-only terms on the encoded event columns, without a GPU: the
transform that makes the device matrix of tests/contrast_multi_cases.py
expressible in those columns and the conditions under which it still tests
something, ``loss.wire_event_columns`` against ``encoding.decode_batch`` and
against hand-made offsets, and the flag ``--compact-event-terms``."""
from pathlib import Path

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import encoding, loss as L, options
from tests import contrast_multi_cases as mc, event_terms_encoded_cases as ec

GOLD = torch.load(Path(__file__).parent / 'golden' / 'encoding.pt', weights_only=True)


# ------------------------------------------------------------- the transform
def test_every_case_of_the_device_matrix_is_encodable_and_still_a_test():
    """No case is left out, the coordinates fit int16 (asserted inside
    ``encodable``), and in every case of at least 255 events at most 25 % are -1
    slots and at least 70 % lie inside the frame with a valid sample."""
    matrix = mc.device_matrix()
    assert len(matrix) == 95
    worst_slots, worst_inside = 0.0, 1.0
    for name, (c, mask, pol) in matrix.items():
        compact, d, B = ec.encodable(c)
        assert B == int(c['fs'].max()) + 1 and compact['sample_event_offsets'].shape == (B + 1,), name
        assert compact['x'].dtype == compact['y'].dtype == np.int16 and compact['polarity'].dtype == bool, name
        assert compact['timestamp'].dtype == np.float32 and compact['x'].size == c['x'].size, name
        assert d['s'].size == 0 or (d['s'].min() >= 0 and d['s'].max() < B and (np.diff(d['s']) >= 0).all()), name
        assert set(np.unique(d['p'])) <= {-1, 1}, name
        if c['x'].size >= 255:
            slots, inside = ec.census(c, d)
            assert slots <= 0.25 and inside >= 0.70, (name, slots, inside)
            worst_slots, worst_inside = max(worst_slots, slots), min(worst_inside, inside)
    assert 0.20 < worst_slots and worst_inside < 0.75       # the transform does make slots: 20.8 % and 74.9 % at worst


def test_the_transform_keeps_the_events_it_can_and_is_deterministic():
    c = mc.device_matrix()['33x31_F3_n4097_m7_p1'][0]
    compact, d, B = ec.encodable(c)
    again = ec.encodable(c)[0]
    assert all(np.array_equal(compact[k], again[k], equal_nan=(k == 'timestamp')) for k in compact)
    keep = (c['s'] >= 0) & (c['s'] < B) & (c['p'] != 0)
    live = ~((d['x'] == -1) & (d['y'] == -1))
    # the events that were expressible are all there, as a multiset of (sample, x, y, p) and in their order per sample
    was = np.stack([c[k][keep] for k in ('s', 'x', 'y', 'p')], 1)
    was = was[~((was[:, 1] == -1) & (was[:, 2] == -1))]
    now = np.stack([d[k][live] for k in ('s', 'x', 'y', 'p')], 1)
    assert np.array_equal(was[np.argsort(was[:, 0], kind='stable')], now)


def test_the_degenerate_case_keeps_its_empty_samples():
    c = mc.device_matrix()['degenerate_windows_m7_p1'][0]
    compact, d, B = ec.encodable(c)
    assert B == 8 and 7 in c['fs']
    off = compact['sample_event_offsets']
    assert (np.diff(off) == 0).sum() >= 6 and off[7] == off[8]       # repeated offsets; sample 7 has no events


# ----------------------------------------------------- wire_event_columns
def test_wire_event_columns_on_the_golden_batch_is_decode_batch():
    encoded = GOLD['encoding']['encoded']
    want = encoding.decode_batch(encoded)['events']
    got = L.wire_event_columns(encoding.compact_events(encoded))
    assert sorted(got) == ['polarity', 'sample_index', 'timestamp', 'x', 'y']
    for k in got:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert want['x'].numel() > 0 and want['sample_index'].max() > 0


@pytest.mark.parametrize('offsets', [[0, 0, 3, 3, 7, 7], [0, 0, 0, 7, 7, 7], [0, 7], [0, 2, 2, 2, 5, 7, 7],
                                     [0, 3, 5]])      # the last one: a padded tail of two slots
def test_wire_event_columns_on_hand_made_offsets(offsets):
    """Empty first, middle and last samples; an event past the last offset falls to sample B - 1."""
    n, B = 7, len(offsets) - 1
    rng = np.random.default_rng(len(offsets))
    compact = {'x': rng.integers(-1, 300, n).astype(np.int16), 'y': rng.integers(-1, 300, n).astype(np.int16),
               'timestamp': rng.random(n).astype(np.float32), 'polarity': rng.random(n) < 0.5,
               'sample_event_offsets': np.array(offsets, np.int64)}
    want = ec.decode(compact, B)
    got = L.wire_event_columns({k: torch.from_numpy(v) for k, v in compact.items()})
    for key, name in (('x', 'x'), ('y', 'y'), ('timestamp', 't'), ('polarity', 'p'), ('sample_index', 's')):
        assert np.array_equal(got[key].numpy(), want[name]), (key, offsets)
    assert got['x'].dtype == got['polarity'].dtype == got['sample_index'].dtype == torch.long
    by_hand = [max(b for b in range(B) if offsets[b] <= i) for i in range(n)]
    assert got['sample_index'].tolist() == by_hand


def test_wire_event_columns_leaves_a_wire_dict_alone_and_takes_an_empty_one():
    wire = {'x': torch.zeros(3, dtype=torch.long), 'sample_index': torch.zeros(3, dtype=torch.long)}
    assert L.wire_event_columns(wire) is wire
    empty = {'x': torch.zeros(0, dtype=torch.short), 'y': torch.zeros(0, dtype=torch.short),
             'timestamp': torch.zeros(0), 'polarity': torch.zeros(0, dtype=torch.bool),
             'sample_event_offsets': torch.zeros(3, dtype=torch.long)}
    assert all(v.numel() == 0 for v in L.wire_event_columns(empty).values())


# ---------------------------------------------------------------- the flag
def _parser():
    from argparse import ArgumentParser
    return options.add_preprocessed_dataset_arguments(options.add_train_arguments(ArgumentParser()))


def _parse(*extra):
    return options.validate_train_args(_parser().parse_args(['-m', 'm'] + list(extra)))


def test_the_flag_is_absent_from_the_namespace_unless_given():
    for extra in ((), ('--compact-events',), ('--contrast-weight', '0.25'), ('--avg-timestamp-weight', '0.5')):
        assert 'compact_event_terms' not in vars(_parse(*extra)), extra
    args = _parse('--compact-events', '--contrast-weight', '0.25', '--compact-event-terms')
    assert args.compact_event_terms is True and args.compact_events is True


@pytest.mark.parametrize('extra,what', [
    (['--compact-event-terms'], '--compact-event-terms needs --compact-events'),
    (['--compact-event-terms', '--contrast-weight', '0.25'], '--compact-event-terms needs --compact-events'),
    (['--compact-event-terms', '--compact-events'], 'needs a positive --contrast-weight or'),
    (['--compact-event-terms', '--compact-events', '--contrast-weight', '0'], '--avg-timestamp-weight'),
    (['--compact-event-terms', '--compact-events', '--avg-timestamp-weight', '0'], '--compact-event-terms needs'),
])
def test_the_flag_is_refused_without_what_it_needs(extra, what):
    with pytest.raises(SystemExit) as e:
        _parse(*extra)
    assert what in str(e.value), e.value


def test_with_the_flag_both_terms_pass_and_every_option_travels():
    args = _parse('--compact-events', '--compact-event-terms', '--contrast-weight', '0.25', '--contrast-references',
                  'start,middle,end', '--contrast-polarity', '--contrast-scales', 'all', '--avg-timestamp-weight',
                  '0.5', '--avg-timestamp-scales', 'all')
    assert args.contrast_weight == 0.25 and args.avg_timestamp_weight == 0.5 and args.compact_events
    assert args.contrast_references == ('start', 'middle', 'end') and args.contrast_scales == 'all'
    assert _parse('--compact-events', '--compact-event-terms', '--avg-timestamp-weight', '0.5').compact_event_terms
    # ... with the captured step and the device feeder too
    args = _parse('--compact-events', '--compact-event-terms', '--contrast-weight', '0.25', '--capture',
                  '--capture-event-terms', '--device-feeder')
    assert args.capture_event_terms and args.compact_event_terms


def test_without_the_flag_the_two_refusals_are_the_parents():
    for run, what in ((['--contrast-weight', '0.25'],
                       '--contrast-weight cannot be combined with --compact-events: the term '
                       'reads the int64 / float32 wire columns, not the 9 B/event encoded ones'),
                      (['--avg-timestamp-weight', '0.5'],
                       '--avg-timestamp-weight cannot be combined with --compact-events: the term '
                       'reads the int64 / float32 wire columns, not the 9 B/event encoded ones')):
        with pytest.raises(SystemExit) as e:
            _parse(*run, '--compact-events')
        assert str(e.value) == what


def test_the_other_refusals_stay_with_the_flag():
    run = ['--compact-events', '--compact-event-terms', '--contrast-weight', '0.25']
    with pytest.raises(SystemExit) as e:
        _parse(*run, '--recording', 'r.npz', '--window-duration', '0.05')
    assert '--recording' in str(e.value) and '--compact-events' in str(e.value)
    with pytest.raises(SystemExit) as e:
        _parse(*run, '--ev_images')
    assert '--contrast-weight cannot be combined with --ev_images' in str(e.value)
    with pytest.raises(SystemExit) as e:
        _parse('--compact-events', '--compact-event-terms', '--avg-timestamp-weight', '0.5', '--ev_images')
    assert '--avg-timestamp-weight cannot be combined with --ev_images' in str(e.value)
