"""Host side of a resumed run: the loaders' position in the data stream
(``state`` / ``restore``), the position arithmetic of the preprocessed loader,
and the schedulers after ``construct_train_tools(passed_steps=k)``."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import train_flownet as tf
from dvs_of_training_framework_amd.sequence import FrameSequence, SequenceLoader
from .test_sequence_plan import fixture_samples

STEPS = 8       # 3 batches per permutation (10 samples, batch 3): three permutations


@pytest.fixture(scope='module')
def frame_sequence(fixtures):
    return FrameSequence.from_samples(fixture_samples(fixtures), device='cpu')


def recording_loader(seq, augmentation, steps, seed):
    loader = SequenceLoader(seq, (256, 256), batch_size=3, seq_length=1, collapse_length=3,
                            augmentation=augmentation, rng=np.random.default_rng(seed),
                            steps=steps)
    loader.batch = lambda idx, k, is_flip, angle, box: (        # nothing is launched
        np.asarray(idx).tolist(), np.asarray(k).tolist(), np.asarray(is_flip).tolist(),
        np.asarray(angle).tolist(), np.asarray(box).tolist())
    return loader


@pytest.fixture(scope='module')
def stream(frame_sequence):
    """The uninterrupted argument stream of ``batch``, computed once."""
    return {aug: list(recording_loader(frame_sequence, aug, STEPS, 7)) for aug in (False, True)}


def test_the_stream_is_worth_comparing(stream):
    assert len(stream[True]) == STEPS
    assert len({tuple(b[0]) for b in stream[True]}) > 1         # batches differ
    assert any(any(b[2]) for b in stream[True]) and any(max(b[1]) > 1 for b in stream[True])
    assert all(max(b[1]) == 1 and not any(b[2]) for b in stream[False])


@pytest.mark.parametrize('augmentation', [False, True])
@pytest.mark.parametrize('j', [0, 1, 3, 4, 6])     # 0, inside a permutation, its boundary
def test_sequence_loader_resumes_its_stream(frame_sequence, stream, augmentation, j):
    first = recording_loader(frame_sequence, augmentation, STEPS, 7)
    it = iter(first)
    head = [next(it) for _ in range(j)]
    state = first.state()
    assert head == stream[augmentation][:j]
    # the state is what a checkpoint holds: it survives torch.save / weights_only load
    import io
    buf = io.BytesIO()
    torch.save({'loader_state': [state]}, buf)
    buf.seek(0)
    state = torch.load(buf, weights_only=True)['loader_state'][0]
    assert state['drawn'] == (j % 3 or (3 if j else 0))
    resumed = recording_loader(frame_sequence, augmentation, STEPS - j, 99)   # another seed
    resumed.restore(state)
    assert list(resumed) == stream[augmentation][j:]


def test_the_default_draw_sequence_is_unchanged(frame_sequence):
    """state() reads the generator, it never draws: the batches of a loader
    whose state is taken after every batch are those of one left alone."""
    watched = recording_loader(frame_sequence, True, STEPS, 3)
    got = []
    for b in watched:
        got.append(b)
        watched.state()
    assert got == list(recording_loader(frame_sequence, True, STEPS, 3))
    # and what the generator gives is what it gave before this feature: the
    # permutation first, then per batch k per sample and the augmentation draws
    rng = np.random.default_rng(3)
    order = rng.permutation(10)
    assert got[0][0] == order[:3].tolist()


class _Stream:
    def wait_event(self, event):
        pass


class _Event:
    def record(self, stream):
        pass


def cpu_feeder(loader, monkeypatch):
    """feed.DeviceFeeder's own one-ahead iteration with the device parts
    (slots, copies, events) replaced by stand-ins."""
    from dvs_of_training_framework_amd.feed import DeviceFeeder
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda device=None: _Stream())
    feeder = DeviceFeeder.__new__(DeviceFeeder)
    feeder.loader, feeder.device = loader, 'cpu'
    feeder.slots = [SimpleNamespace(ready=_Event(), free=_Event()) for _ in range(2)]
    feeder._stage = lambda batch, slot: (batch, slot)
    return feeder


@pytest.mark.parametrize('j', [0, 2, 3, 5])
def test_a_feeder_one_batch_ahead_reports_the_batch_it_handed_out(frame_sequence, stream, j,
                                                                  monkeypatch):
    first = recording_loader(frame_sequence, True, STEPS, 7)
    feeder = cpu_feeder(first, monkeypatch)
    it = iter(feeder)
    head = [next(it) for _ in range(j)]
    assert head == stream[True][:j]
    state = feeder.state()
    if j:
        assert first.state() != state       # the loader itself is one batch further
    resumed = cpu_feeder(recording_loader(frame_sequence, True, STEPS - j, 99), monkeypatch)
    resumed.restore(state)
    assert list(resumed) == stream[True][j:]


# ------------------------------------------------------- the other loaders
def synthetic_args(tmp_path, *more):
    return tf.parse_args(['-m', str(tmp_path / 'm'), '--optimizer', 'ADAM', '-bs', '4', '-mbs',
                          '2', '--height', '16', '--width', '16', '--synthetic',
                          '--synthetic-events', '50', '-ne', '10', '-d', 'cpu',
                          '--event-representation-depth', '3', *more])


def same_batch(a, b):
    return all(torch.equal(a['events'][k], b['events'][k]) for k in ('x', 'y', 'timestamp')) \
        and torch.equal(a['images'], b['images'])


def test_synthetic_loader_start(tmp_path):
    args = synthetic_args(tmp_path)
    full = list(tf.SyntheticLoader(args, 1, 6))
    part = tf.SyntheticLoader(args, 1, 4)
    it = iter(part)
    assert part.state() == {'next': 0}
    next(it), next(it)
    assert part.state() == {'next': 2}
    for start in (0, 2, 5):
        tail = list(tf.SyntheticLoader(args, 1, 6 - start, start=start))
        assert len(tail) == 6 - start
        assert all(same_batch(a, b) for a, b in zip(tail, full[start:]))
    resumed = tf.SyntheticLoader(args, 1, 4)
    resumed.restore(part.state())
    assert all(same_batch(a, b) for a, b in zip(resumed, full[2:]))
    assert not same_batch(full[0], full[1])
    # validation batches come from other seeds than any rank's training batches
    train_seeds = {1234 + r + 1000 * i for r in range(8) for i in range(100)}
    assert not train_seeds & {tf.VALIDATION_SEED + 1000 * i for i in range(100)}
    assert len(tf._FixedBatches(args, 3, tf.VALIDATION_SEED)) == 3
    a, b = (list(tf._FixedBatches(args, 3, tf.VALIDATION_SEED)) for _ in range(2))
    assert all(same_batch(x, y) for x, y in zip(a, b))      # the same at every pass


def test_preprocessed_position():
    """One process: the reference's ``sample_idx=samples_passed``.  World 2,
    micro-batch 4, 3 batches passed per rank: the loader has served 24 samples;
    rank 0 continues at 24, rank 1 one micro-batch further, and ``_Strided``
    skips the other rank's batch from there."""
    assert tf.preprocessed_position(0, 1, 0, 4) == 0
    assert tf.preprocessed_position(40, 1, 0, 4) == 40
    assert tf.preprocessed_position(0, 2, 1, 4) == 4            # today's start of rank 1
    assert tf.preprocessed_position(12, 2, 0, 4) == 24
    assert tf.preprocessed_position(12, 2, 1, 4) == 28

    class Counter:      # a sequential loader of batches of 4 samples
        def __init__(self, at):
            self.at = at

        def __next__(self):
            self.at += 4
            return self.at - 4
    for rank in range(2):
        straight = tf._Strided(Counter(tf.preprocessed_position(0, 2, rank, 4)), 2)
        seen = [next(straight) for _ in range(5)]
        resumed = tf._Strided(Counter(tf.preprocessed_position(12, 2, rank, 4)), 2)
        assert [next(resumed) for _ in range(2)] == seen[3:]


def test_restore_loader_takes_its_ranks_entry(tmp_path):
    args = synthetic_args(tmp_path)
    loader = tf.SyntheticLoader(args, 1, 4)
    tf.restore_loader(loader, {'loader_state': [{'next': 3}, {'next': 5}]}, 1, 2, 2, args)
    assert loader.state() == {'next': 5}
    tf.restore_loader(loader, {}, 1, 2, 3, args)        # a checkpoint without loader states
    assert loader.state() == {'next': 3 * args.accum_step}


# ------------------------------------------------------------- schedulers
class _Split(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.quantization_layer = torch.nn.Linear(2, 2)
        self.predictor = torch.nn.Linear(2, 2)


@pytest.mark.parametrize('k', [0, 3, 5, 6, 9])      # --representation-start 0.5 of 10 steps = 5
def test_schedulers_continue(tmp_path, k):
    args = synthetic_args(tmp_path, '--representation-start', '0.5', '-lr', '0.25',
                          '--num-warmup-steps', '4', '--half_life', '3')
    opt, sch = tf.construct_train_tools(args, _Split())
    for _ in range(k):
        opt.step()
        sch.step()
    straight = [g['lr'] for g in opt.param_groups]
    resumed_opt, resumed_sch = tf.construct_train_tools(args, _Split(), passed_steps=k)
    assert [g['lr'] for g in resumed_opt.param_groups] == straight
    assert resumed_sch.last_epoch == sch.last_epoch == k
    pred, rep = tf.make_schedulers(args)
    assert straight == [0.25 * rep(k), 0.25 * pred(k)]
    assert (straight[0] > 0) == (k > 5)         # the knots train after the start only
    # one more step on both: still together
    opt.step(), sch.step(), resumed_opt.step(), resumed_sch.step()
    assert [g['lr'] for g in resumed_opt.param_groups] == [g['lr'] for g in opt.param_groups]
