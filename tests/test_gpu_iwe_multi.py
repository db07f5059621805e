"""csrc/iwe.hip with its options on the device against the numpy float32
restatement (eval.iwe_splat_multi_host, docs/IWE_SPEC.md sections 8-13), byte for byte: on
every case of tests/iwe_cases.py with a polarity column, at five masks and both
polarity settings, in any order of the events, in a batch or frame by frame,
from filled buffers, beyond one pass of the capped grid; against the entry
points of section 2 at the default options; the statistics and the panels on M
images; the argument rules; and testing.flow_warp_loss with the options."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import eval as dev_eval, testing
from dvs_of_training_framework_amd.loss import contrast_reference_mask
from tests import eval_cases as ec, iwe_cases as ic, iwe_multi_cases as mc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
INTEGERS = ('sum_q', 'max_q', 'count_sum', 'count_sq', 'count_max')
MULTI = [n for n in ic.CASE_IDS if '_F3_' in n]


def on_device(c):
    return {k: torch.from_numpy(np.array(c[k])).to(DEV)         # a copy: the shared case is read-only
            for k in ('x', 'y', 't', 'p', 'begin', 'ts', 'flow')}


def splat(c, mask=1, polarity=False, d=None):
    d = on_device(c) if d is None else d
    return dev_eval.iwe_splat_multi({'x': d['x'], 'y': d['y'], 'timestamp': d['t'], 'polarity': d['p']},
                                    d['begin'], d['ts'], d['flow'], mask, polarity)


_want = {}


def want(name, mask, polarity):
    """The restatement's answer, computed once: (q int64, count uint32)."""
    key = (name, mask, polarity)
    if key not in _want:
        _want[key] = dev_eval.iwe_splat_multi_host(*mc.args_of(mc.case(name)), mask, polarity)
    return _want[key]


def same(got, expected):
    q, count = got
    assert q.dtype == torch.long and count.dtype == torch.int32 and q.is_cuda and count.is_cuda
    assert q.shape == count.shape == expected[0].shape
    return np.array_equal(q.cpu().numpy(), expected[0]) and \
        np.array_equal(count.cpu().numpy().view(np.uint32), expected[1])


# ------------------------------------------------------------------ splat
@pytest.mark.parametrize('name', ic.CASE_IDS)
def test_splat_equals_the_restatement_byte_for_byte(name):
    c = mc.case(name)
    d = on_device(c)
    for mask, polarity in mc.OPTIONS:
        assert same(splat(c, mask, polarity, d), want(name, mask, polarity)), (mask, polarity)


@pytest.mark.parametrize('name', ic.CASE_IDS)
def test_start_without_polarity_is_the_splat_and_the_count_image_of_section_2(name):
    c = mc.case(name)
    d = on_device(c)
    q, count = splat(c, 1, False, d)
    old = dev_eval.iwe_splat({'x': d['x'], 'y': d['y'], 'timestamp': d['t']}, d['begin'], d['ts'], d['flow'])
    h, w = c['shape']
    assert torch.equal(q, old)
    assert torch.equal(count, dev_eval.count_image_batched(d['x'], d['y'], d['begin'], (h, w), (0, 0, h, w)))
    # p is not read: a column of zeros, or none at all
    bare = {'x': d['x'], 'y': d['y'], 'timestamp': d['t']}
    q2, count2 = dev_eval.iwe_splat_multi(bare, d['begin'], d['ts'], d['flow'])
    assert torch.equal(q2, q) and torch.equal(count2, count)


@pytest.mark.parametrize('name', ic.CASE_IDS)
def test_splat_does_not_depend_on_the_order_of_the_events(name):
    c = mc.case(name)
    for mask, polarity in ((7, True), (5, False), (2, True)):
        assert same(splat(mc.permuted(c), mask, polarity), want(name, mask, polarity)), (mask, polarity)


@pytest.mark.parametrize('name', MULTI)
def test_a_batch_equals_its_frames_alone(name):
    c = mc.case(name)
    for mask, polarity in ((7, True), (5, False)):
        per = mc.images_of(1, mask, polarity)
        q, count = splat(c, mask, polarity)
        rows = dev_eval.iwe_stats(q, count)
        for f in range(3):
            q1, count1 = splat(mc.single_frame(c, f), mask, polarity)
            assert torch.equal(q1, q[f * per:(f + 1) * per]) and torch.equal(count1, count[f * per:(f + 1) * per])
            assert torch.equal(dev_eval.iwe_stats(q1, count1), rows[f * per:(f + 1) * per])


@pytest.mark.parametrize('name', ['5x7_F3_empty_middle', '33x31_F3_recorded', '400x400_F1'])
def test_every_output_byte_is_written(name):
    c = mc.case(name)
    d = on_device(c)
    lib = dev_eval._lib.lib()
    F, (h, w) = len(c['begin']) - 1, c['shape']
    for mask, polarity in ((7, True), (1, False), (6, True)):
        expected = want(name, mask, polarity)
        M = lib.dvsof_iwe_multi_images(F, mask, int(polarity))
        assert M == len(expected[0])
        for fill in (0xAA, 0x55):
            q = torch.full((M, h, w, 8), fill, dtype=torch.uint8, device=DEV)
            count = torch.full((M, h, w, 4), fill, dtype=torch.uint8, device=DEV)
            assert lib.dvsof_iwe_splat_multi(d['x'].data_ptr(), d['y'].data_ptr(), d['t'].data_ptr(),
                                             d['p'].data_ptr(), d['x'].numel(), d['begin'].data_ptr(),
                                             d['ts'].data_ptr(), d['flow'].data_ptr(), F, h, w, mask, int(polarity),
                                             q.data_ptr(), count.data_ptr(), dev_eval._lib.stream()) == 0
            assert q.cpu().numpy().tobytes() == expected[0].tobytes(), (mask, polarity, hex(fill))
            assert count.cpu().numpy().tobytes() == expected[1].tobytes(), (mask, polarity, hex(fill))


def test_more_events_than_one_pass_of_the_capped_grid():
    """2048 blocks of 256 threads cover 524288 events: the last 1000 are a thread's second."""
    h, w, n = 16, 16, 2048 * 256 + 1000
    rng = np.random.default_rng(12)
    c = dict(x=rng.integers(-1, w, n), y=rng.integers(0, h, n), t=(rng.integers(0, 257, n) / 512).astype(np.float32),
             p=rng.integers(-1, 2, n), begin=np.array([3, n - 5], np.int64), ts=np.array([0, 0.5], np.float32),
             flow=rng.normal(0, 3, (1, 2, h, w)).astype(np.float32), shape=(h, w))
    expected = dev_eval.iwe_splat_multi_host(*mc.args_of(c), 7, True)
    assert same(splat(c, 7, True), expected)
    assert int(expected[1].max()) > 200 and expected[1][0::2].sum() + expected[1][1::2].sum() > 3 * n // 2
    tail = dict(c, begin=np.array([2048 * 256, n], np.int64))       # the second pass alone
    expected = dev_eval.iwe_splat_multi_host(*mc.args_of(tail), 7, True)
    assert same(splat(tail, 7, True), expected) and 0 < int(expected[1][0].sum()) < 1000


# ------------------------------------------------- statistics and panels
@pytest.mark.parametrize('name', ['5x7_F3_degenerate', '33x31_F3_recorded', '400x400_F3_empty_middle', '1x1_F1'])
def test_statistics_and_panels_on_all_images(name):
    q, count = want(name, 7, True)
    M, h, w = q.shape
    qd, cd = torch.from_numpy(q).to(DEV), torch.from_numpy(count.view(np.int32)).to(DEV)
    rows = dev_eval.iwe_stats(qd, cd)
    assert tuple(rows.shape) == (M, 48)
    res, host = dev_eval.read_iwe_results(rows), dev_eval.iwe_stats_host(q, count)
    for k in INTEGERS:
        assert np.array_equal(res[k], host[k]), k
    assert res['sum_sq'].tobytes() == dev_eval.iwe_sum_sq_kernel_order(q).tobytes()     # the kernels' order
    expected = dev_eval.iwe_render_host(q, count, res)
    canvas = dev_eval.iwe_render(qd, cd, rows)
    assert tuple(canvas.shape) == (M, h, 2 * w, 3) and np.array_equal(canvas.cpu().numpy(), expected)
    # the six images of a frame below one another are a view of the same bytes
    assert canvas.is_contiguous() and np.array_equal(canvas.view(M // 6, 6 * h, 2 * w, 3)[0].cpu().numpy(),
                                                     expected[:6].reshape(6 * h, 2 * w, 3))


# --------------------------------------------------------- argument rules
def test_argument_rules_on_the_device_build():
    lib = dev_eval._lib.lib()
    F, h, w, n = 2, 5, 7, 11
    M = 6 * F
    t = dict(x=torch.zeros(n, dtype=torch.long), y=torch.zeros(n, dtype=torch.long), t=torch.zeros(n),
             p=torch.ones(n, dtype=torch.long), begin=torch.tensor([0, 5, 11]), ts=torch.zeros(2 * F),
             flow=torch.zeros(F, 2, h, w), q=torch.full((M, h, w, 8), 0xAA, dtype=torch.uint8),
             count=torch.full((M, h, w, 4), 0xAA, dtype=torch.uint8))
    t = {k: v.to(DEV) for k, v in t.items()}
    a = {k: v.data_ptr() for k, v in t.items()}
    a['n'] = n
    seen = 0
    for what, call in mc.bad_calls(lib, a, F, h, w):
        assert call() == mc.EINVAL, what
        seen += 1
    torch.cuda.synchronize()
    assert seen == 25
    for k in ('q', 'count'):
        assert bool((t[k] == 0xAA).all()), k
    assert all(rc == 0 for rc in mc.empty_calls(lib))
    # without polarity p may be null; without events every column may
    args = (a['begin'], a['ts'], a['flow'], F, h, w)
    assert lib.dvsof_iwe_splat_multi(a['x'], a['y'], a['t'], None, n, *args, 7, 0, a['q'], a['count'], None) == 0
    torch.cuda.synchronize()
    assert int(t['count'].view(torch.int32)[:3 * F].sum()) == 3 * n      # C = 1: the first half of the buffers
    t['q'].fill_(0xAA), t['count'].fill_(0xAA)
    assert lib.dvsof_iwe_splat_multi(None, None, None, None, 0, *args, 7, 1, a['q'], a['count'], None) == 0
    torch.cuda.synchronize()
    assert not t['q'].any() and not t['count'].any()        # n_events = 0 zeroes the outputs


# --------------------------------------------------------- flow_warp_loss
SHAPE = ec.EVAL_BOX[2:]


class PrescribedFlow:
    """A predictor with ``flow_sequence`` that answers with prescribed flows,
    looked up by the window's start (tests/test_gpu_iwe.py)."""

    def __init__(self, frames, flows):
        self._index = {float(f[0]): i for i, f in enumerate(frames)}
        self._flows = flows

    def flow_sequence(self, seq, starts, stops, box=None, return_events=False):
        c = seq.collate_frames(starts, stops, box)
        flow = torch.stack([self._flows[self._index[float(s)]] for s in starts])
        return (flow, c) if return_events else flow


@pytest.fixture(scope='module')
def exact_sequence():
    """The recording of tests/eval_cases.py with its event times on a grid of 2^-16 s: every
    relative time of a collated batch is exact, whatever the batch (tests/test_gpu_iwe.py)."""
    from dvs_of_training_framework_amd.sequence import FrameSequence
    c = ec.make_eval_case(per_frame=3000)
    x, y, t, p = c['events']
    t = np.round(t * 65536.0) / 65536.0
    image_ts = np.append(c['frames'][:, 0], c['frames'][-1, 1])
    images = np.zeros((len(image_ts),) + ec.EVAL_SHAPE, np.uint8)
    return FrameSequence([x, y, t, p], images, image_ts, device=DEV)


@pytest.fixture(scope='module')
def prescribed():
    frames = ec.EVAL_FRAMES
    rng = np.random.default_rng(3)
    flows = torch.from_numpy(rng.normal(0, 2.5, (len(frames), 2) + SHAPE).astype(np.float32)).to(DEV)
    return frames, PrescribedFlow(frames, flows)


def by_hand(of, seq, frames, mask, polarity):
    """The images and rows from the pieces: flow_sequence, the restatement."""
    starts, stops = [a for a, _ in frames], [b for _, b in frames]
    pred, c = of.flow_sequence(seq, starts, stops, box=ec.EVAL_BOX, return_events=True)
    ev = {k: c.events[k].cpu().numpy() for k in ('x', 'y', 'timestamp', 'polarity')}
    q, count = dev_eval.iwe_splat_multi_host(ev['x'], ev['y'], ev['timestamp'], ev['polarity'],
                                             c.win_out.cpu().numpy(), c.timestamps.cpu().numpy(),
                                             pred.cpu().numpy(), mask, polarity)
    rows = dev_eval.iwe_stats_host(q, count)
    rows['sum_sq'] = dev_eval.iwe_sum_sq_kernel_order(q)
    return q, count, rows


@pytest.mark.parametrize('references,polarity', [(('start', 'middle', 'end'), True), (('end',), False),
                                                 (('start',), True)])
def test_flow_warp_loss_with_options_is_the_sum_of_its_parts(exact_sequence, prescribed, references, polarity):
    frames, of = prescribed
    mask = contrast_reference_mask(references)
    per = mc.images_of(1, mask, polarity)
    seen = []
    eight = testing.flow_warp_loss(of, exact_sequence, frames, ec.EVAL_BOX, batch_size=8, references=references,
                                   polarity=polarity, observer=lambda *a: seen.append(a))
    one = testing.flow_warp_loss(of, exact_sequence, frames, ec.EVAL_BOX, batch_size=1, references=mask,
                                 polarity=polarity)
    assert eight.dtype == dev_eval.IWE_RESULT_DTYPE and eight.shape == (len(frames) * per,)
    assert one.tobytes() == eight.tobytes()
    q, count, rows = by_hand(of, exact_sequence, frames, mask, polarity)
    (first, qd, cd, res), = seen
    assert first == 0 and tuple(qd.shape) == tuple(cd.shape) == (len(frames) * per,) + SHAPE
    assert np.array_equal(qd.cpu().numpy(), q) and np.array_equal(cd.cpu().numpy().view(np.uint32), count)
    assert dev_eval.read_iwe_results(res).tobytes() == eight.tobytes() == rows.tobytes()
    assert (eight['count_sum'] > 100).all() and (eight['sum_q'] > 0).all()


def test_flow_warp_loss_with_the_defaults_makes_the_calls_it_made(exact_sequence, prescribed, monkeypatch):
    frames, of = prescribed
    calls = []
    for name in ('count_image_batched', 'iwe_splat', 'iwe_splat_multi'):
        def spy(*a, _name=name, _f=getattr(dev_eval, name), **k):
            calls.append(_name)
            return _f(*a, **k)
        monkeypatch.setattr(dev_eval, name, spy)
    seen = []
    rows = testing.flow_warp_loss(of, exact_sequence, frames, ec.EVAL_BOX, batch_size=4,
                                  observer=lambda *a: seen.append(a))
    assert calls == ['count_image_batched', 'iwe_splat'] * 2
    named = testing.flow_warp_loss(of, exact_sequence, frames, ec.EVAL_BOX, batch_size=4, references=('start',),
                                   polarity=False)
    assert calls == ['count_image_batched', 'iwe_splat'] * 4 and named.tobytes() == rows.tobytes()
    # today's rows: F of them, the bytes of the pieces of section 2
    starts, stops = [a for a, _ in frames], [b for _, b in frames]
    pred, c = of.flow_sequence(exact_sequence, starts, stops, box=ec.EVAL_BOX, return_events=True)
    count = dev_eval.count_image_batched(c.events['x'], c.events['y'], c.win_out, SHAPE, (0, 0) + SHAPE)
    q = dev_eval.iwe_splat(c.events, c.win_out, c.timestamps, pred)
    assert rows.shape == (len(frames),)
    assert rows.tobytes() == dev_eval.read_iwe_results(dev_eval.iwe_stats(q, count)).tobytes()
    assert [tuple(s[1].shape) for s in seen] == [(4,) + SHAPE, (3,) + SHAPE]
    # and the new call at the same options gives the same rows
    calls.clear()
    multi = dev_eval.iwe_splat_multi(c.events, c.win_out, c.timestamps, pred)
    assert dev_eval.read_iwe_results(dev_eval.iwe_stats(*multi)).tobytes() == rows.tobytes()
