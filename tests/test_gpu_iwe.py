"""csrc/iwe.hip on the device against the numpy float32 restatement of
docs/IWE_SPEC.md (eval.iwe_*_host), byte for byte where the spec pins bytes:
the splat on every case of tests/iwe_cases.py, in any order of the events, in
a batch or frame by frame; the statistics; the rendered panels;
the argument rules; and testing.flow_warp_loss on a synthetic sequence."""
import math

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import eval as dev_eval, testing
from tests import eval_cases as ec, iwe_cases as ic

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def on_device(c):
    return {k: torch.from_numpy(np.array(c[k])).to(DEV)         # a copy: the shared case is read-only
            for k in ('x', 'y', 't', 'begin', 'ts', 'flow')}


def splat(c):
    d = on_device(c)
    return dev_eval.iwe_splat({'x': d['x'], 'y': d['y'], 'timestamp': d['t']}, d['begin'], d['ts'],
                              d['flow'])


def count_of(c):
    d = on_device(c)
    return dev_eval.count_image_batched(d['x'], d['y'], d['begin'], c['shape'])


_want = {}


def want(name):
    """The restatement's answer for a case, computed once: (q, count, rows)."""
    if name not in _want:
        c = ic.case(name)
        q = dev_eval.iwe_splat_host(c['x'], c['y'], c['t'], c['begin'], c['ts'], c['flow'])
        count = ic.count_image(c)
        _want[name] = (q, count, dev_eval.iwe_stats_host(q, count))
    return _want[name]


INTEGERS = ('sum_q', 'max_q', 'count_sum', 'count_sq', 'count_max')
MULTI = [n for n in ic.CASE_IDS if '_F3_' in n]


# ------------------------------------------------------------------ splat
@pytest.mark.parametrize('name', ic.CASE_IDS)
def test_splat_equals_the_restatement_byte_for_byte(name):
    q = splat(ic.case(name))
    assert q.dtype == torch.long and q.is_cuda
    assert np.array_equal(q.cpu().numpy(), want(name)[0])
    assert np.array_equal(count_of(ic.case(name)).cpu().numpy().view(np.uint32), want(name)[1])


@pytest.mark.parametrize('name', ic.CASE_IDS)
def test_splat_does_not_depend_on_the_order_of_the_events(name):
    c = ic.case(name)
    assert torch.equal(splat(ic.permuted(c)), splat(c))


@pytest.mark.parametrize('name', MULTI)
def test_a_batch_equals_its_frames_alone(name):
    c = ic.case(name)
    q, count = splat(c), count_of(c)
    rows = dev_eval.iwe_stats(q, count)
    for f in range(3):
        one = ic.single_frame(c, f)
        q1, count1 = splat(one), count_of(one)
        assert torch.equal(q1[0], q[f]) and torch.equal(count1[0], count[f])
        assert torch.equal(dev_eval.iwe_stats(q1, count1)[0], rows[f])       # sum_sq too: its bits


# ------------------------------------------------------------- statistics
@pytest.mark.parametrize('name', ic.CASE_IDS)
def test_statistics(name):
    q, count, host = want(name)
    qd, cd = torch.from_numpy(q).to(DEV), torch.from_numpy(count.view(np.int32)).to(DEV)
    rows = dev_eval.iwe_stats(qd, cd)
    assert rows.dtype == torch.uint8 and tuple(rows.shape) == (len(q), 48) and rows.is_cuda
    res = dev_eval.read_iwe_results(rows)
    for k in INTEGERS:
        assert np.array_equal(res[k], host[k]), k
    n = q.shape[1] * q.shape[2]
    for f in range(len(q)):
        exact = math.fsum((int(v) * 2.0 ** -32) ** 2 for v in q[f].ravel())
        print(name, f, 'sum_sq', res['sum_sq'][f], 'error', abs(res['sum_sq'][f] - exact),
              'bound', n * 2.0 ** -53 * exact)
        assert abs(res['sum_sq'][f] - exact) <= n * 2.0 ** -53 * exact
    assert res['sum_sq'].tobytes() == dev_eval.iwe_sum_sq_kernel_order(q).tobytes()     # the kernels' order
    assert torch.equal(dev_eval.iwe_stats(qd, cd), rows)        # a second run: the same bits


# ----------------------------------------------------------------- render
@pytest.mark.parametrize('name', ic.CASE_IDS)
def test_render_equals_the_restatement_and_writes_every_byte(name):
    q, count, host = want(name)
    F, h, w = q.shape
    qd, cd = torch.from_numpy(q).to(DEV), torch.from_numpy(count.view(np.int32)).to(DEV)
    rows = dev_eval.iwe_stats(qd, cd)
    expected = dev_eval.iwe_render_host(q, count, dev_eval.read_iwe_results(rows))
    assert np.array_equal(dev_eval.iwe_render(qd, cd, rows).cpu().numpy(), expected)
    lib = dev_eval._lib.lib()
    for fill in (0xAA, 0x55):
        canvas = torch.full((F, h, 2 * w, 3), fill, dtype=torch.uint8, device=DEV)
        assert lib.dvsof_iwe_render(qd.data_ptr(), cd.data_ptr(), rows.data_ptr(), F, h, w,
                                    canvas.data_ptr(), dev_eval._lib.stream()) == 0
        assert np.array_equal(canvas.cpu().numpy(), expected), hex(fill)


# --------------------------------------------------------- argument rules
def test_argument_rules_on_the_device_build():
    lib = dev_eval._lib.lib()
    F, h, w, n = 2, 5, 7, 11
    t = dict(x=torch.zeros(n, dtype=torch.long), y=torch.zeros(n, dtype=torch.long), t=torch.zeros(n),
             begin=torch.tensor([0, 5, 11]), ts=torch.zeros(2 * F), flow=torch.zeros(F, 2, h, w),
             q=torch.full((F, h, w), 7, dtype=torch.long), count=torch.zeros(F, h, w, dtype=torch.int32),
             result=torch.full((F, 48), 7, dtype=torch.uint8),
             ws=torch.zeros(lib.dvsof_iwe_stats_workspace_bytes(F, h, w), dtype=torch.uint8),
             canvas=torch.full((F, h, 2 * w, 3), 7, dtype=torch.uint8))
    t = {k: v.to(DEV) for k, v in t.items()}
    a = {k: v.data_ptr() for k, v in t.items()}
    a['n'] = n
    seen = 0
    for what, call, expect in ic.bad_calls(lib, a, F, h, w):
        assert call() == expect, what
        seen += 1
    torch.cuda.synchronize()
    assert seen >= 35
    for k in ('q', 'result', 'canvas'):
        assert bool((t[k] == 7).all()), k
    assert all(rc == 0 for rc in ic.empty_calls(lib))


# --------------------------------------------------------- flow_warp_loss
SHAPE = ec.EVAL_BOX[2:]
FRAMES = ec.EVAL_FRAMES[:6]     # a batch the network repeats its own bits at (test_gpu_evaluation_hook.py)


@pytest.fixture(scope='module')
def sequence():
    from dvs_of_training_framework_amd.sequence import FrameSequence
    c = ec.make_eval_case(per_frame=3000)
    image_ts = np.append(c['frames'][:, 0], c['frames'][-1, 1])
    images = np.zeros((len(image_ts),) + ec.EVAL_SHAPE, np.uint8)
    return FrameSequence([col for col in c['events']], images, image_ts, device=DEV)


def by_hand(of, seq, frames):
    """The rows from the pieces: flow_sequence, count_image_batched, the restatement."""
    starts, stops = [a for a, _ in frames], [b for _, b in frames]
    pred, c = of.flow_sequence(seq, starts, stops, box=ec.EVAL_BOX, return_events=True)
    count = dev_eval.count_image_batched(c.events['x'], c.events['y'], c.win_out, SHAPE, (0, 0) + SHAPE)
    ev = {k: c.events[k].cpu().numpy() for k in ('x', 'y', 'timestamp')}
    q = dev_eval.iwe_splat_host(ev['x'], ev['y'], ev['timestamp'], c.win_out.cpu().numpy(),
                                c.timestamps.cpu().numpy(), pred.cpu().numpy())
    return q, dev_eval.iwe_stats_host(q, count.cpu().numpy())


def same_rows(rows, host, n):
    for k in INTEGERS:
        assert np.array_equal(rows[k], host[k]), k
    assert np.all(np.abs(rows['sum_sq'] - host['sum_sq']) <= 2 * n * 2.0 ** -53 * host['sum_sq'])


def test_flow_warp_loss_is_the_sum_of_its_parts(sequence):
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.of import OpticalFlow
    torch.manual_seed(0)
    model = Model(DEV, event_representation_depth=5).eval()
    of = OpticalFlow.from_model(model, SHAPE)
    seen = []
    rows = testing.flow_warp_loss(of, sequence, FRAMES, ec.EVAL_BOX,
                                  observer=lambda first, q, count, res: seen.append((first, q, count, res)))
    assert rows.dtype == dev_eval.IWE_RESULT_DTYPE and rows.shape == (6,) and [s[0] for s in seen] == [0]
    q, host = by_hand(of, sequence, FRAMES)
    assert np.array_equal(seen[0][1].cpu().numpy(), q)
    # two float64 sums of the same terms in two orders: each within N 2^-53 of the exact sum
    same_rows(rows, host, SHAPE[0] * SHAPE[1])
    assert dev_eval.read_iwe_results(seen[0][3]).tobytes() == rows.tobytes()
    assert (rows['count_sum'] > 500).all() and (rows['sum_q'] > 0).all()
    fwl, kept = dev_eval.derive_fwl(rows, SHAPE[0] * SHAPE[1])
    assert np.isfinite(fwl).all() and ((0 < kept) & (kept <= 1)).all()
    # without an observer nothing changes
    assert testing.flow_warp_loss(of, sequence, FRAMES, ec.EVAL_BOX).tobytes() == rows.tobytes()
    # host columns are refused: the events stay on the device
    with pytest.raises(TypeError, match='EventSequence'):
        testing.flow_warp_loss(of, [np.zeros(3)] * 4, FRAMES, ec.EVAL_BOX)
    with pytest.raises(ValueError, match='outside the frame'):
        testing.flow_warp_loss(of, sequence, FRAMES, (10, 10, 32, 64))
    assert len(testing.flow_warp_loss(of, sequence, [], ec.EVAL_BOX)) == 0


class PrescribedFlow:
    """A predictor with ``flow_sequence`` that answers with prescribed flows,
    looked up by the window's start: what it says about a frame does not depend
    on the batch the frame comes in (a network's last bits do)."""

    def __init__(self, frames, flows):
        self._index = {float(f[0]): i for i, f in enumerate(frames)}
        self._flows = flows

    def flow_sequence(self, seq, starts, stops, box=None, return_events=False):
        c = seq.collate_frames(starts, stops, box)
        flow = torch.stack([self._flows[self._index[float(s)]] for s in starts])
        return (flow, c) if return_events else flow


@pytest.fixture(scope='module')
def exact_sequence():
    """The same recording with its event times on a grid of 2^-16 s.  A collated batch carries
    float32 times relative to ITS earliest start, so an arbitrary float64 time is rounded
    differently in another batch and tau moves in its last bit; on this grid (and with the
    dyadic frame bounds of eval_cases) every relative time is exact, whatever the batch."""
    from dvs_of_training_framework_amd.sequence import FrameSequence
    c = ec.make_eval_case(per_frame=3000)
    x, y, t, p = c['events']
    t = np.round(t * 65536.0) / 65536.0
    image_ts = np.append(c['frames'][:, 0], c['frames'][-1, 1])
    images = np.zeros((len(image_ts),) + ec.EVAL_SHAPE, np.uint8)
    return FrameSequence([x, y, t, p], images, image_ts, device=DEV)


def test_flow_warp_loss_in_batches_of_one_and_of_eight(exact_sequence):
    """With the network itself the rows of two batch sizes differ: its last bits depend on the
    batch it runs in (measured on the MI355X with the model of the test above, all 7 frames
    differ in sum_q between batches of one and of eight).  At batch 1 most frames do not even
    repeat their own bits, and that is the voxeliser, not the network: five of the seven frames
    hold fewer than 4096 events (3503, 856, 4048, 4539, 877, 2703, 4176), so their calls run the
    thread-per-event kernel with float atomics, the documented order-dependent path
    (docs/VOXEL_SPEC.md; tests/test_gpu_network_repeat.py pins that every call of 4096 events
    or more repeats).  What flow_warp_loss adds to that must not depend on the batch: a
    predictor that answers per frame, exact times."""
    sequence = exact_sequence
    frames = ec.EVAL_FRAMES
    rng = np.random.default_rng(3)
    flows = torch.from_numpy(rng.normal(0, 2.5, (len(frames), 2) + SHAPE).astype(np.float32)).to(DEV)
    of = PrescribedFlow(frames, flows)
    firsts = []
    one = testing.flow_warp_loss(of, sequence, frames, ec.EVAL_BOX, batch_size=1,
                                 observer=lambda first, *a: firsts.append(first))
    eight = testing.flow_warp_loss(of, sequence, frames, ec.EVAL_BOX, batch_size=8)
    three = testing.flow_warp_loss(of, sequence, frames, ec.EVAL_BOX, batch_size=3)
    assert firsts == list(range(7)) and len(one) == 7
    assert one.tobytes() == eight.tobytes() == three.tobytes()
    q, host = by_hand(of, sequence, frames)
    same_rows(eight, host, SHAPE[0] * SHAPE[1])
