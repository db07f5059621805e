"""Device-resident event sequences against docs/SEQUENCE_SPEC.md.  The spec is
exact, so every comparison is ``torch.equal`` / ``np.array_equal``: the window
kernel against a numpy oracle of the spec's arithmetic, ``seq.collate``
against ``OpticalFlow._collate`` on host-sliced events, ``flow_sequence``
against ``flow_device``, ``evaluate_frames`` on an ``EventSequence`` against
the numpy-events path, and ``SequenceLoader.batch`` against the restated
``__getitem__`` of tests/test_sequence_plan.py followed by the augmentation
oracle."""
import numpy as np
import pytest
import torch

from oracle import cpu_oracle as orc

from . import eval_cases as ec
from .test_sequence_plan import N_FIXTURES, fixture_samples, restated_sample

pytestmark = pytest.mark.gpu

SHAPE = (40, 56)
KEYS = ('x', 'y', 'timestamp', 'polarity', 'sample_index', 'element_index')
SENTINEL = 77
TILED_MIN = 4096        # events from which the voxeliser is the tiled, order-independent kernel


# ---------------------------------------------------------------------------
# the oracle: docs/SEQUENCE_SPEC.md in numpy
# ---------------------------------------------------------------------------
def oracle_windows(cols, begin, end, origin, sample, element, box, capacity,
                   f32_first=False):
    """cols: x int16, y int16, t float64, p int8.  -> the six output columns
    with ``capacity`` slots.  f32_first: the WRONG timestamp arithmetic
    (narrow, then subtract), to show that the data tells the two apart."""
    x, y, t, p = cols
    out = dict(x=np.full(capacity, -1, np.int64), y=np.full(capacity, -1, np.int64),
               timestamp=np.zeros(capacity, np.float32), polarity=np.zeros(capacity, np.int64),
               sample_index=np.zeros(capacity, np.int64),
               element_index=np.zeros(capacity, np.int64))
    slot = 0
    for k in range(len(begin)):
        i = np.arange(begin[k], end[k])
        s = slice(slot, slot + i.size)
        xi, yi = x[i].astype(np.int64), y[i].astype(np.int64)
        if box is not None:
            y0, x0, h, w = box
            keep = (xi >= x0) & (xi < x0 + w) & (yi >= y0) & (yi < y0 + h)
            xi, yi = np.where(keep, xi - x0, -1), np.where(keep, yi - y0, -1)
        out['x'][s], out['y'][s] = xi, yi
        if f32_first:
            out['timestamp'][s] = t[i].astype(np.float32) - np.float32(origin[k])
        else:
            out['timestamp'][s] = (t[i] - np.float64(origin[k])).astype(np.float32)
        out['polarity'][s] = p[i]
        out['sample_index'][s] = sample[k]
        out['element_index'][s] = element[k]
        slot += i.size
    assert slot <= capacity
    return out


def make_events(n=6000, shape=SHAPE, seed=3, t0=1.5e9, spacing=1e-6):
    """MVSEC-sized timestamps on a 1 us grid (ties included), polarities
    -1 / 0 / +1, coordinates that include 0 and shape - 1."""
    rng = np.random.default_rng(seed)
    t = t0 + np.sort(rng.integers(0, 2 * n, n)) * spacing
    x = rng.integers(0, shape[1], n)
    y = rng.integers(0, shape[0], n)
    x[:4], y[:4] = [0, shape[1] - 1, 0, shape[1] - 1], [0, 0, shape[0] - 1, shape[0] - 1]
    p = rng.choice([-1, 0, 1], n)
    return [x.astype(np.float64), y.astype(np.float64), t, p.astype(np.float64)]


def device_cols(seq):
    return (seq.x.cpu().numpy(), seq.y.cpu().numpy(), seq.t_dev.cpu().numpy(), seq.p.cpu().numpy())


def sentinel_out(size):
    return {k: torch.full((size,), SENTINEL, device='cuda',
                          dtype=torch.float32 if k == 'timestamp' else torch.long) for k in KEYS}


def assert_same(got, want, upto=None):
    for k in KEYS:
        g = got[k].cpu().numpy()[:upto]
        assert g.dtype == want[k].dtype, k
        assert np.array_equal(g, want[k]), (k, np.flatnonzero(g != want[k])[:8])


@pytest.fixture(scope='module')
def seq():
    from dvs_of_training_framework_amd.sequence import EventSequence
    s = EventSequence(make_events(), SHAPE)
    cols = device_cols(s)
    assert cols[0].dtype == np.int16 and cols[2].dtype == np.float64 and cols[3].dtype == np.int8
    assert set(np.unique(cols[3])) == {-1, 0, 1}
    assert cols[0].min() == 0 and cols[0].max() == SHAPE[1] - 1
    assert cols[1].min() == 0 and cols[1].max() == SHAPE[0] - 1
    return s


def window_table(N):
    """Every length around the wave (64) and the block (256 threads x 2 slots =
    512, and 1024), empty windows at the front, in the middle and at the end,
    overlapping, repeated and descending windows, one that ends at N."""
    lengths = [0, 1, 63, 64, 65, 0, 0, 1023, 1024, 1025, 511, 512, 513, 0]
    begin = [0, 5, 5, 30, 30, 100, 7, 2000, 1500, 1000, 4000, 300, 300, N]     # overlaps, descending
    begin += [N - 129, N - 129, 0]                                             # ends at N, repeated
    lengths += [129, 129, 0]
    begin, end = np.array(begin), np.array(begin) + np.array(lengths)
    assert end.max() == N
    rng = np.random.default_rng(9)
    sample = rng.integers(0, 1000, begin.size)
    element = rng.integers(0, 7, begin.size)
    return begin, end, sample, element


# ---------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('slack', [0, 1, 37, 700])
def test_window_kernel_matches_the_spec(seq, slack):
    cols = device_cols(seq)
    t = cols[2]
    begin, end, sample, element = window_table(seq.n_events)
    # origins inside, before and behind each window: negative and positive relative times
    origin = np.array([t[min((b + e) // 2, seq.n_events - 1)] for b, e in zip(begin, end)])
    origin[3], origin[8] = t[0] - 0.25, t[-1] + 0.25
    n_out = int((end - begin).sum())
    capacity = n_out + slack
    want = oracle_windows(cols, begin, end, origin, sample, element, None, capacity)
    wrong = oracle_windows(cols, begin, end, origin, sample, element, None, capacity, f32_first=True)
    assert (want['timestamp'][:n_out] < 0).any() and (want['timestamp'][:n_out] > 0).any()
    assert not np.array_equal(want['timestamp'], wrong['timestamp'])    # the data tells them apart
    out = sentinel_out(capacity + 5)
    got, win_out, _, _ = seq.windows(begin, end, origin, sample, element, capacity=capacity, out=out)
    assert win_out.cpu().tolist() == np.concatenate([[0], np.cumsum(end - begin)]).tolist()
    assert_same(got, want, capacity)
    for k in KEYS:          # nothing behind the capacity is touched
        assert (out[k][capacity:] == SENTINEL).all(), k
    if slack:
        assert (got['x'][n_out:capacity] == -1).all() and (got['timestamp'][n_out:capacity] == 0).all()
    # the same call again: the same bytes; fresh outputs too
    again, _, _, _ = seq.windows(begin, end, origin, sample, element, capacity=capacity)
    for k in KEYS:
        assert torch.equal(again[k], got[k][:capacity]), k


def test_window_kernel_unaligned_outputs(seq):
    """Output columns that do not start on 16 bytes take the one-slot path."""
    cols = device_cols(seq)
    begin, end, sample, element = window_table(seq.n_events)
    origin = cols[2][begin.clip(max=seq.n_events - 1)]
    n_out = int((end - begin).sum())
    base = sentinel_out(n_out + 4)
    out = {k: v[1:] for k, v in base.items()}
    assert out['x'].data_ptr() % 16 == 8
    got, _, _, _ = seq.windows(begin, end, origin, sample, element, capacity=n_out + 2, out=out)
    assert_same(got, oracle_windows(cols, begin, end, origin, sample, element, None, n_out + 2),
                n_out + 2)
    for k in KEYS:
        assert base[k][0] == SENTINEL and base[k][-1] == SENTINEL, k


def test_no_windows_and_no_events(seq):
    none = np.zeros(0, np.int64)
    out = sentinel_out(40)
    got, win_out, _, _ = seq.windows(none, none, none, none, none, capacity=33, out=out)   # W = 0
    assert_same(got, oracle_windows(device_cols(seq), none, none, none, none, none, None, 33), 33)
    assert win_out.tolist() == [0]
    assert (out['x'][33:] == SENTINEL).all()
    out = sentinel_out(8)
    got, _, _, _ = seq.windows([5, 9], [5, 9], [0.0, 0.0], [1, 2], [3, 4], capacity=7, out=out)  # n_out = 0
    assert_same(got, oracle_windows(device_cols(seq), [5, 9], [5, 9], [0.0, 0.0], [1, 2], [3, 4],
                                    None, 7), 7)
    assert (out['polarity'][7:] == SENTINEL).all()
    got, _, _, _ = seq.windows([5], [5], [0.0], [1], [3])          # capacity 0: nothing to do
    assert got['x'].numel() == 0


def test_box_edges(seq):
    from dvs_of_training_framework_amd.sequence import EventSequence
    y0, x0, h, w = box = (3, 5, 32, 48)
    xs = [0, x0 - 1, x0, x0 + 1, x0 + w - 1, x0 + w, SHAPE[1] - 1]
    ys = [0, y0 - 1, y0, y0 + 1, y0 + h - 1, y0 + h, SHAPE[0] - 1]
    grid = np.array([(a, b, p) for a in xs for b in ys for p in (-1, 0, 1)], np.float64)
    t = 1.5e9 + np.arange(len(grid)) * 1e-6
    s = EventSequence([grid[:, 0], grid[:, 1], t, grid[:, 2]], SHAPE)
    cols = device_cols(s)
    n = len(grid)
    begin, end = np.array([0, n // 3, 0]), np.array([n, n, 0])
    origin = np.array([t[0], t[5], 0.0])
    want = oracle_windows(cols, begin, end, origin, [0, 1, 2], [0, 0, 0], box, end.sum() - begin.sum())
    kept = want['x'] >= 0
    assert set(want['x'][kept]) == {0, 1, w - 1} and set(want['y'][kept]) == {0, 1, h - 1}
    assert np.array_equal(want['x'] < 0, want['y'] < 0)
    got, _, _, _ = s.windows(begin, end, origin, [0, 1, 2], [0, 0, 0], box=box)
    assert_same(got, want)
    # the right and bottom edges are open: a box shifted by one loses x0 + w - 1 ... and so on
    for other in ((0, 0, 40, 56), (0, 0, 1, 1), (39, 55, 1, 1), (y0, x0, h + 1, w + 1)):
        got, _, _, _ = s.windows(begin, end, origin, [0, 1, 2], [0, 0, 0], box=other)
        assert_same(got, oracle_windows(cols, begin, end, origin, [0, 1, 2], [0, 0, 0], other,
                                        end.sum() - begin.sum()))


def test_call_is_capturable_and_replays_to_the_same_bytes(seq):
    """A stream capture of the C ABI call (thread_local mode, as of.py uses it)
    holds the kernel alone and rewrites the outputs on replay."""
    cols = device_cols(seq)
    begin, end, sample, element = window_table(seq.n_events)
    origin = cols[2][begin.clip(max=seq.n_events - 1)]
    n_out = int((end - begin).sum())
    capacity = n_out + 100
    eager, _, _, table = seq.windows(begin, end, origin, sample, element, capacity=capacity)
    want = {k: v.clone() for k, v in eager.items()}
    static = sentinel_out(capacity)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        seq.launch(table, (0, 0, 0, 0), static, n_out, capacity)
    for _ in range(2):
        for v in static.values():
            v.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(static[k], want[k]), k


# ---------------------------------------------------------------------------
# collate == OpticalFlow._collate on host-sliced events
# ---------------------------------------------------------------------------
def frames_of(t, n_frames, per_frame, first=50):
    """Consecutive frames of ``per_frame`` events each, bounds on event times."""
    cuts = t[first + per_frame * np.arange(n_frames + 1)]
    return list(cuts[:-1]), list(cuts[1:])


def host_frames(events, starts, stops, box):
    evs = []
    for e, _, _ in ec.frame_generator(events, list(zip(starts, stops))):
        e = np.array(e)
        evs.append(e if box is None else ec.EventCrop(box)(e.T.copy()).T)
    return evs


@pytest.fixture(scope='module')
def flow_nets():
    from dvs_of_training_framework_amd.of import OpticalFlow
    torch.manual_seed(0)
    eager = OpticalFlow((32, 48), model=None, event_representation_depth=5)
    graphed = OpticalFlow((32, 48), model=None, event_representation_depth=5, graph=True)
    graphed.load_state_dict(eager._net.state_dict())
    return eager, graphed


@pytest.mark.parametrize('box', [None, (3, 5, 32, 48)])
def test_collate_matches_the_host_collation(seq, flow_nets, box):
    events = make_events()
    t = events[2]
    starts = [t[0] - 1.0, t[700], t[700], t[2000], t[5000], t[-1]]
    stops = [t[10], t[1900], t[700], t[2001], t[-1] + 1.0, t[-1] + 2.0]     # empty frames among them
    want_ev, want_ts, want_sidx = flow_nets[0]._collate(host_frames(events, starts, stops, box),
                                                       starts, stops)
    got_ev, got_ts, got_sidx = seq.collate(starts, stops, box=box)
    assert torch.equal(got_ts, want_ts) and got_ts.dtype == torch.float32
    assert torch.equal(got_sidx, want_sidx) and got_sidx.dtype == torch.long
    keep = got_ev['x'] != -1
    assert (box is None) == bool(keep.all())
    assert list(got_ev) == list(want_ev)
    for k in want_ev:
        assert got_ev[k].dtype == want_ev[k].dtype, k
        assert torch.equal(got_ev[k][keep], want_ev[k]), k
    # padded into caller-owned columns
    out = sentinel_out(got_ev['x'].numel() + 9)
    pad_ev, _, _ = seq.collate(starts, stops, box=box, out=out)
    n = got_ev['x'].numel()
    for k in want_ev:
        assert pad_ev[k] is out[k] and torch.equal(pad_ev[k][:n], got_ev[k]), k
    assert (out['x'][n:] == -1).all() and (out['sample_index'][n:] == 0).all()


# ---------------------------------------------------------------------------
# flow_sequence == flow_device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('box', [None, (3, 5, 32, 48)])
def test_flow_sequence_matches_flow_device(flow_nets, box):
    from dvs_of_training_framework_amd.sequence import EventSequence
    shape = (32, 48) if box is None else SHAPE
    events = make_events(n=30000, shape=shape, seed=11)
    s = EventSequence(events, shape)
    eager, graphed = flow_nets
    for first in (50, 3000):        # the second round replays the captured graph
        starts, stops = frames_of(events[2], 8, 1600, first)
        evs = host_frames(events, starts, stops, box)
        # both sides on the tiled voxeliser: bitwise independent of order and of dropped slots
        assert all(e.shape[1] >= 1500 for e in host_frames(events, starts, stops, None))
        assert sum(e.shape[1] for e in evs) >= TILED_MIN
        want = eager.flow_device(evs, starts, stops)
        got = eager.flow_sequence(s, starts, stops, box=box)
        assert got.shape == (8, 2, 32, 48) and torch.equal(got, want)
        assert torch.equal(graphed.flow_sequence(s, starts, stops, box=box), want)
    assert graphed._graphs[8]['graph'] is not None


# ---------------------------------------------------------------------------
# evaluate_frames: EventSequence == numpy events
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def eval_case():
    # the synthetic sequence at the smallest event count that keeps every batch
    # of four frames at TILED_MIN events after the central crop
    return ec.make_eval_case(per_frame=3000)


@pytest.mark.parametrize('boxed', [False, True])
def test_evaluate_frames_matches_the_numpy_events_path(eval_case, boxed):
    from dvs_of_training_framework_amd import testing
    from dvs_of_training_framework_amd.of import OpticalFlow
    from dvs_of_training_framework_amd.sequence import EventSequence
    c = eval_case
    y0, x0, h, w = ec.EVAL_BOX
    assert (y0, x0) == ((ec.EVAL_SHAPE[0] - h) // 2, (ec.EVAL_SHAPE[1] - w) // 2)     # central
    if boxed:
        events, shape = [col for col in c['events']], ec.EVAL_SHAPE
        xm, ym = c['x_maps'], c['y_maps']
        crops = dict(event_preproc_fun=ec.EventCrop(ec.EVAL_BOX), gt_proc_fun=ec.ImageCrop(ec.EVAL_BOX))
    else:       # the same recording seen by a 32 x 64 sensor: nothing left to crop
        events, shape = [col for col in ec.EventCrop(ec.EVAL_BOX)(c['events'].T.copy()).T], (h, w)
        xm, ym = c['x_maps'][:, y0:y0 + h, x0:x0 + w], c['y_maps'][:, y0:y0 + h, x0:x0 + w]
        crops = {}
    gt = dict(timestamps=c['ts'], x_flow_dist=xm, y_flow_dist=ym)
    frames = c['frames']
    for b0 in range(0, len(frames), 4):
        kept = sum(e.shape[1] for e in host_frames(events, frames[b0:b0 + 4, 0], frames[b0:b0 + 4, 1],
                                                   ec.EVAL_BOX if boxed else None))
        assert kept >= TILED_MIN, (b0, kept)
    torch.manual_seed(1)
    of = OpticalFlow((h, w), model=None, event_representation_depth=5)
    want = testing.evaluate_frames(of, events, frames, gt, batch_size=4, **crops)
    s = EventSequence(events, shape)
    got = testing.evaluate_frames(of, s, frames, gt, batch_size=4, **crops)
    assert got.dtype == want.dtype and len(got) == len(frames)
    for name in want.dtype.names:
        assert ec.same_bits(got[name], want[name]), (name, got[name], want[name])
    assert (want['n_points'] > 0).all()
    assert testing.evaluate(of, s, frames, gt, batch_size=4, **crops) == \
        testing.evaluate(of, events, frames, gt, batch_size=4, **crops)
    with pytest.raises(TypeError, match='numpy-events path'):
        testing.evaluate_frames(of, s, frames, gt, batch_size=4,
                                event_preproc_fun=ec.Opaque(ec.EventCrop(ec.EVAL_BOX)))


# ---------------------------------------------------------------------------
# SequenceLoader
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def frame_sequence(fixtures):
    from dvs_of_training_framework_amd.sequence import FrameSequence
    return FrameSequence.from_samples(fixture_samples(fixtures))


@pytest.mark.parametrize('k,seq_length', [(1, 1), (2, 2), (3, 1)])
def test_loader_batch_matches_the_restated_dataset(fixtures, frame_sequence, k, seq_length):
    from dvs_of_training_framework_amd.sequence import SequenceLoader, central_box
    samples = fixture_samples(fixtures)
    L = seq_length
    loader = SequenceLoader(frame_sequence, (256, 256), batch_size=4, seq_length=L)
    central, off = central_box((260, 346), (256, 256)), [1, 7, 256, 256]
    assert central == [2, 45, 256, 256]
    idx = [0, N_FIXTURES - k * L, 1, 2]
    is_flip, angle = [True, False, True, False], [0.0, 17.5, 17.5, 0.0]
    box = [central, off, off, central]
    batch = loader.batch(idx, [k] * 4, is_flip, angle, box)
    assert batch['size'] == 4 and batch['images'].shape == (4 * (L + 1), 1, 256, 256)
    ev = {name: col.cpu().numpy() for name, col in batch['events'].items()}
    assert all(col.is_cuda for col in batch['events'].values()) and batch['images'].is_cuda
    slot = 0
    for b, i0 in enumerate(idx):
        rows, stamps, numbers = restated_sample(samples, i0, k, L)
        images, nx, ny = orc.augment_sample(fixtures['frames'][numbers], rows[:, 0].astype(np.int64),
                                            rows[:, 1].astype(np.int64), is_flip[b], angle[b], box[b])
        s = slice(slot, slot + len(rows))
        assert np.array_equal(ev['x'][s], nx) and np.array_equal(ev['y'][s], ny)
        assert ev['timestamp'].dtype == np.float32 and np.array_equal(ev['timestamp'][s], rows[:, 2])
        assert np.array_equal(ev['polarity'][s], rows[:, 3].astype(np.int64))
        assert np.array_equal(ev['element_index'][s], rows[:, 4].astype(np.int64))
        assert np.array_equal(ev['sample_index'][s], np.full(len(rows), b))
        f = slice(b * (L + 1), (b + 1) * (L + 1))
        assert np.array_equal(batch['images'][f, 0].cpu().numpy(), images)
        assert np.array_equal(batch['timestamps'][f].cpu().numpy(), stamps)
        assert np.array_equal(batch['sample_idx'][f].cpu().numpy(), np.full(L + 1, b))
        slot += len(rows)
    assert slot == ev['x'].size
    assert batch['timestamps'].dtype == torch.float32 and batch['sample_idx'].dtype == torch.long
    aug = batch['augmentation_params']
    assert aug['idx'].tolist() == idx and aug['sequence_length'].tolist() == [L] * 4
    assert aug['collapse_length'].tolist() == [k] * 4 and aug['box'].tolist() == box
    assert aug['angle'].tolist() == angle and aug['is_flip'].tolist() == is_flip


def test_two_training_steps_from_the_loader(frame_sequence):
    """Smoke: training.train fed by a SequenceLoader on a 32 x 48 crop."""
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.optim import FusedAdamW
    from dvs_of_training_framework_amd.sequence import SequenceLoader
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import train
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = Model(dev, event_representation_depth=3)
    opt = FusedAdamW(model.predictor.parameters(), lr=1e-3, amsgrad=True)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
    losses = init_losses((32, 48), 2, model, dev, sequence_length=1)
    loader = SequenceLoader(frame_sequence, (32, 48), batch_size=2, augmentation=True,
                            collapse_length=3, rng=np.random.default_rng(4), steps=2)
    before = [p.detach().clone() for p in model.predictor.parameters()]
    seen = []

    class Log:
        def add_scalar(self, tag, value, x):
            if tag == 'General/Train loss':
                seen.append((x, value))
    train(model, dev, loader, opt, 2, sch, Log(), losses, timers=FakeTimer())
    torch.cuda.synchronize()
    assert [x for x, _ in seen] == [2, 4] and all(np.isfinite(v) for _, v in seen)
    assert any(not torch.equal(a, b) for a, b in zip(before, model.predictor.parameters()))
