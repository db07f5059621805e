"""Host side of the device-resident sequences (docs/SEQUENCE_SPEC.md), no GPU:
``frame_ranges`` against a plain restatement of ``frame_generator``
(utils/data.py:139-152), the loader's sample plan against a numpy restatement
of ``DatasetImpl.__getitem__`` (utils/dataset.py:647-751, is_raw, static
sequence length, aligned) on the ten consecutive reference samples of
tests/golden/fixtures.npz, and what the wrapper and the constructor refuse.

``fixture_samples`` and ``restated_sample`` are shared with
tests/test_gpu_sequence.py."""
import shutil
from pathlib import Path

import numpy as np
import pytest

from dvs_of_training_framework_amd import hdf5io
from dvs_of_training_framework_amd.sequence import (
    EventSequence, FrameSequence, SequenceLoader, central_box)

GOLDEN = Path(__file__).parent / 'golden'
N_FIXTURES = 10


def fixture_samples(fixtures):
    """The ten per-frame files as the dicts a reader of them would hold."""
    return [dict(events=fixtures[f'events_{i}'].copy(),
                 image1=fixtures['frames'][i], image2=fixtures['frames'][i + 1],
                 start=fixtures['start'][i], stop=fixtures['stop'][i])
            for i in range(N_FIXTURES)]


def restated_sample(samples, idx, k, seq_length):
    """One sample of the per-frame dataset before its augmentation, in this
    project's words: ``seq_length`` elements of ``k`` consecutive files each.
    -> events float32 [m,5] (x, y, t, p, element), image timestamps float32
    [seq_length+1], image numbers [seq_length+1]; times relative to the start
    of file ``idx``, subtracted in float64 and then narrowed."""
    assert idx + k * seq_length <= len(samples)
    rows, stamps, numbers = [], [], []
    for element in range(seq_length):
        files = samples[idx + element * k: idx + (element + 1) * k]
        for a, b in zip(files[:-1], files[1:]):
            assert a['stop'] == b['start']
        ev = np.vstack([f['events'] for f in files]).astype(np.float64)
        rows.append(np.hstack([ev, np.full((len(ev), 1), float(element))]))
        if element == 0:
            stamps.append(float(files[0]['start']))
            numbers.append(idx)
        stamps.append(float(files[-1]['stop']))
        numbers.append(idx + (element + 1) * k)
    rows = np.vstack(rows)
    stamps = np.array(stamps, np.float64)
    rows[:, 2] -= stamps[0]
    stamps = stamps - stamps[0]
    return rows.astype(np.float32), stamps.astype(np.float32), np.array(numbers)


def synthetic_events(seed=5, n=3000, shape=(40, 56), t0=1.5e9):
    rng = np.random.default_rng(seed)
    t = t0 + np.sort(rng.integers(0, 4000, n)) * 1e-6      # ties included
    return [rng.integers(0, shape[1], n).astype(np.float64),
            rng.integers(0, shape[0], n).astype(np.float64), t,
            rng.choice([-1.0, 1.0], n)]


# ------------------------------------------------------------ frame_ranges
def test_frame_ranges_follow_frame_generator():
    ev = synthetic_events()
    t = ev[2]
    seq = EventSequence(ev, (40, 56), device='cpu')
    first, last = t[0], t[-1]
    between = 0.5 * (t[1000] + t[1001]) if t[1000] != t[1001] else t[1000] + 2.5e-7
    frames = [
        (first - 1.0, first - 0.5),             # wholly before the first event
        (first - 1.0, t[10]),                   # begins before it, ends on an event
        (t[10], t[500]),                        # both bounds exactly on events
        (t[500], t[500]),                       # empty, on an event
        (between, between),                     # empty, between two events
        (t[2000], last + 1.0),                  # ends after the last event
        (last, last + 1.0),                     # nothing left: the last event is excluded
        (last + 1.0, last + 2.0),               # wholly after
        (first - 1.0, last + 1.0),              # everything
    ]
    got = seq.frame_ranges(frames)
    assert got.dtype == np.int64 and got.shape == (len(frames), 2)
    for (start, stop), (lo, hi) in zip(frames, got):
        # a frame holds the events with start < t <= stop; t is sorted
        assert lo == np.count_nonzero(t <= start)
        assert hi == np.count_nonzero(t <= stop)
        inside = (t > start) & (t <= stop)
        assert np.array_equal(np.flatnonzero(inside), np.arange(lo, hi))
    assert tuple(got[0]) == (0, 0) and tuple(got[-1]) == (0, t.size)
    assert got[3][0] == got[3][1] and tuple(got[7]) == (t.size, t.size)


# ------------------------------------------------------------- sample plan
@pytest.fixture(scope='module')
def frame_sequence(fixtures):
    return FrameSequence.from_samples(fixture_samples(fixtures), device='cpu')


def test_from_samples_lays_the_files_end_to_end(fixtures, frame_sequence):
    s = frame_sequence
    counts = [len(fixtures[f'events_{i}']) for i in range(N_FIXTURES)]
    assert s.n_samples == N_FIXTURES and s.shape == (260, 346)
    assert np.array_equal(s.frame_event_begin, np.concatenate([[0], np.cumsum(counts)]))
    assert np.array_equal(s.image_ts, np.concatenate([fixtures['start'][:1], fixtures['stop']]))
    assert np.array_equal(s.images.numpy(), fixtures['frames'])
    # the default boundaries (searchsorted 'right' on the image timestamps) agree here
    ev = np.concatenate([fixtures[f'events_{i}'] for i in range(N_FIXTURES)])
    again = FrameSequence([ev[:, c] for c in range(4)], fixtures['frames'], s.image_ts,
                          device='cpu')
    assert np.array_equal(again.frame_event_begin, s.frame_event_begin)
    broken = fixture_samples(fixtures)
    broken[4]['start'] = broken[4]['start'] + 1e-6
    with pytest.raises(AssertionError):
        FrameSequence.from_samples(broken, device='cpu')


@pytest.mark.parametrize('seq_length', [1, 2])
@pytest.mark.parametrize('k', [1, 2, 3])
def test_sample_plan_matches_the_restated_getitem(fixtures, frame_sequence, k, seq_length):
    samples = fixture_samples(fixtures)
    s = frame_sequence
    loader = SequenceLoader(s, (256, 256), batch_size=2, seq_length=seq_length)
    last = N_FIXTURES - k * seq_length          # idx at both ends of the recording
    idx = [0, last]
    plan = loader.plan(idx, [k, k])
    B, L = 2, seq_length
    assert plan['win_begin'].shape == (B * L,)
    all_t = s.t
    all_ev = np.concatenate([f['events'] for f in samples])
    for b, i0 in enumerate(idx):
        want_ev, want_ts, want_img = restated_sample(samples, i0, k, L)
        sl = slice(b * L, (b + 1) * L)
        assert np.array_equal(plan['win_sample'][sl], np.full(L, b))
        assert np.array_equal(plan['win_element'][sl], np.arange(L))
        assert np.array_equal(plan['win_origin'][sl], np.full(L, samples[i0]['start']))
        assert np.array_equal(plan['image_index'][b * (L + 1):(b + 1) * (L + 1)], want_img)
        assert np.array_equal(plan['sample_idx'][b * (L + 1):(b + 1) * (L + 1)],
                              np.full(L + 1, b))
        got_ts = plan['timestamps'][b * (L + 1):(b + 1) * (L + 1)]
        assert got_ts.dtype == np.float32 and np.array_equal(got_ts, want_ts)
        # the windows, read back through the arithmetic of the spec, are the sample's events
        rows = []
        for w in range(b * L, (b + 1) * L):
            lo, hi = plan['win_begin'][w], plan['win_end'][w]
            file0 = i0 + plan['win_element'][w] * k
            assert lo == s.frame_event_begin[file0] and hi == s.frame_event_begin[file0 + k]
            e = all_ev[lo:hi]
            rows.append(np.column_stack([
                e[:, 0], e[:, 1], (all_t[lo:hi] - plan['win_origin'][w]).astype(np.float32),
                e[:, 3], np.full(hi - lo, plan['win_element'][w])]).astype(np.float32))
        assert np.array_equal(np.vstack(rows), want_ev)
    # one step further does not fit
    with pytest.raises(AssertionError):
        loader.plan([last + 1], [k])
    with pytest.raises(AssertionError):
        restated_sample(samples, last + 1, k, L)


def test_loader_draws_follow_the_dataset_rules(frame_sequence):
    s = frame_sequence
    plain = SequenceLoader(s, (256, 256), batch_size=3, seq_length=2)
    assert plain.num_samples == N_FIXTURES - 2 + 1 and len(plain) == 3
    assert all(plain.draw_k(i) == 1 for i in range(plain.num_samples))
    assert central_box(s.shape, (256, 256)) == [2, 45, 256, 256]
    aug = SequenceLoader(s, (256, 256), batch_size=3, seq_length=2, augmentation=True,
                         collapse_length=3, rng=np.random.default_rng(0))
    for idx in range(aug.num_samples):
        ks = {aug.draw_k(idx) for _ in range(60)}
        top = min(3, (N_FIXTURES - idx) // 2)
        assert ks == set(range(1, top + 1)), (idx, ks)
    with pytest.raises(ValueError):
        SequenceLoader(s, (256, 256), batch_size=N_FIXTURES + 1)
    with pytest.raises(ValueError):
        SequenceLoader(s, (261, 256), batch_size=1)


@pytest.mark.skipif(not hdf5io.available(), reason='libhdf5 not found')
def test_from_directory_reads_the_per_frame_files(fixtures, tmp_path):
    shutil.copy(GOLDEN / 'h5py_seq_000001.hdf5', tmp_path / '000001.hdf5')
    s = FrameSequence.from_directory(tmp_path, device='cpu')
    assert s.n_samples == 1
    assert np.array_equal(s.image_ts, [fixtures['start'][1], fixtures['stop'][1]])
    assert np.array_equal(s.images.numpy(), fixtures['frames'][1:3])
    ev = fixtures['events_1']
    assert np.array_equal(s.t, ev[:, 2])
    assert np.array_equal(s.x.numpy(), ev[:, 0].astype(np.int16))
    assert np.array_equal(s.p.numpy(), ev[:, 3].astype(np.int8))


# ---------------------------------------------------------------- refusals
def test_wrapper_refuses_a_bad_window_table():
    seq = EventSequence(synthetic_events(n=100), (40, 56), device='cpu')

    def call(begin, end, win_out=None, box=None):
        W = len(begin)
        return seq.windows(begin, end, np.zeros(W), np.zeros(W), np.zeros(W),
                           win_out=win_out, box=box, capacity=0 if win_out is None else None)
    with pytest.raises(ValueError, match='begin <= end'):
        call([5, 20], [10, 19])
    with pytest.raises(ValueError, match='begin <= end'):
        call([5, 90], [10, 101])                    # end > N
    with pytest.raises(ValueError, match='begin <= end'):
        call([-1], [3])
    with pytest.raises(ValueError, match='prefix sum'):
        call([5, 20], [10, 30], win_out=[0, 5, 14])
    with pytest.raises(ValueError, match='prefix sum'):
        call([5, 20], [10, 30], win_out=[0, 5])
    for box in ((0, 0, 41, 56), (0, 1, 40, 56), (-1, 0, 10, 10), (0, 0, 0, 10)):
        with pytest.raises(ValueError, match='outside the frame'):
            call([0], [0], box=box)
    with pytest.raises(ValueError, match='capacity'):
        seq.windows([0], [10], [0.0], [0], [0], capacity=9)
    # a valid table with nothing to write needs no device
    cols, win_out, _, _ = seq.windows([3, 3], [3, 3], [0.0, 0.0], [0, 1], [0, 0],
                                   win_out=[0, 0, 0], box=(0, 0, 40, 56))
    assert cols['x'].numel() == 0 and win_out.tolist() == [0, 0, 0]


def test_constructor_refuses_bad_events():
    x, y, t, p = synthetic_events(n=50)
    EventSequence([x, y, t, p], (40, 56), device='cpu')
    unsorted = t.copy()
    unsorted[[10, 30]] = unsorted[[30, 10]]
    assert (np.diff(unsorted) < 0).any()
    with pytest.raises(ValueError, match='not sorted'):
        EventSequence([x, y, unsorted, p], (40, 56), device='cpu')
    for col, value in ((0, 56.0), (0, -1.0), (1, 40.0), (1, -1.0)):
        cols = [x.copy(), y.copy()]
        cols[col][7] = value
        with pytest.raises(ValueError, match='invalid entry in coordinates array'):
            EventSequence([cols[0], cols[1], t, p], (40, 56), device='cpu')
    bad_p = p.copy()
    bad_p[3] = 2
    with pytest.raises(ValueError, match='polarit'):
        EventSequence([x, y, t, bad_p], (40, 56), device='cpu')
    zero_p = p.copy()
    zero_p[3] = 0
    assert EventSequence([x, y, t, zero_p], (40, 56), device='cpu').p[3] == 0
