"""The average-timestamp images of the validation metric on the device
(csrc/iwe.hip, include/dvsof_iwe_avg_timestamp.h, docs/IWE_SPEC.md sections
14-21) against the numpy restatement (eval.iwe_avg_timestamp_host,
iwe_avg_timestamp_rows_host, iwe_avg_timestamp_render_host), byte for byte: the
four images, the statistics rows and the canvas at five masks and both polarity
settings on every case of tests/iwe_avg_timestamp_cases.py (one partial block
and two, 1x1, an odd thin frame, 128 partials); q and count against
dvsof_iwe_splat_multi; everything against the workspace of
dvsof_avg_timestamp_fwd where the two frame rules pick the same events; any
order of the events; events of no frame and -1 slots; flows that splat nothing;
no events and no frames; more events than one pass of the grid; filled buffers;
and the argument rules with guard bytes around every output."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L
from tests import iwe_avg_timestamp_cases as rc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GUARD = 64


def on_device(c):
    return {k: torch.from_numpy(np.array(c[k])).to(DEV)         # a copy: the shared case is read-only
            for k in ('x', 'y', 't', 'p', 'begin', 'ts', 'flow')}


def run(c, mask=1, polarity=False, d=None):
    d = on_device(c) if d is None else d
    return dev_eval.iwe_avg_timestamp({'x': d['x'], 'y': d['y'], 'timestamp': d['t'], 'polarity': d['p']},
                                      d['begin'], d['ts'], d['flow'], mask, polarity)


_want = {}


def want(name, mask, polarity):
    """The restatement's answer, computed once: ((q, s, base, count), rows, canvas)."""
    key = (name, mask, polarity)
    if key not in _want:
        images = dev_eval.iwe_avg_timestamp_host(*rc.args_of(rc.case(name)), mask, polarity)
        _want[key] = (images, dev_eval.iwe_avg_timestamp_rows_host(*images),
                      dev_eval.iwe_avg_timestamp_render_host(*images))
    return _want[key]


def host(images):
    q, s, base, count = (a.cpu().numpy() for a in images)
    return q, s, base, count.view(np.uint32)


def same(got, expected):
    """The device's images and rows against the restatement's."""
    images, rows = got
    assert all(a.is_cuda and a.dtype == torch.long for a in images[:3]) and images[3].dtype == torch.int32
    assert rows.is_cuda and rows.dtype == torch.uint8 and tuple(rows.shape) == (len(expected[1]), 32)
    for k, a, b in zip(rc.IMAGES, host(images), expected[0]):
        assert a.shape == b.shape and np.array_equal(a, b), k
    assert rows.cpu().numpy().tobytes() == expected[1].tobytes()
    return True


# ------------------------------------------------------------ restatement
@pytest.mark.parametrize('name', rc.CASE_IDS)
def test_device_equals_the_restatement_byte_for_byte(name):
    c = rc.case(name)
    d = on_device(c)
    for mask, polarity in rc.OPTIONS:
        expected = want(name, mask, polarity)
        images, rows = run(c, mask, polarity, d)
        assert same((images, rows), expected), (mask, polarity)
        canvas = dev_eval.iwe_avg_timestamp_render(*images)
        assert canvas.dtype == torch.uint8 and tuple(canvas.shape) == expected[2].shape
        assert np.array_equal(canvas.cpu().numpy(), expected[2]), (mask, polarity)
        # the four images are views of one region
        P = images[0].numel()
        assert [a.data_ptr() - images[0].data_ptr() for a in images] == [0, 8 * P, 16 * P, 24 * P]


@pytest.mark.parametrize('name', rc.CASE_IDS)
def test_q_and_count_are_those_of_the_splat_of_the_flow_warp_loss(name):
    c = rc.case(name)
    d = on_device(c)
    events = {'x': d['x'], 'y': d['y'], 'timestamp': d['t'], 'polarity': d['p']}
    for mask, polarity in ((7, True), (1, False), (5, False), (2, True)):
        images, _ = run(c, mask, polarity, d)
        q, count = dev_eval.iwe_splat_multi(events, d['begin'], d['ts'], d['flow'], mask, polarity)
        assert torch.equal(images[0], q) and torch.equal(images[3], count), (mask, polarity)
        # and so are the rows of the flow warp loss, from either
        assert torch.equal(dev_eval.iwe_stats(images[0], images[3]), dev_eval.iwe_stats(q, count))


def term_workspace(c, mask, polarity):
    """dvsof_avg_timestamp_fwd on the case with one frame per sample -> the regions of its workspace."""
    lib = _lib.lib()
    x, y, t, p, sample, ts, fs, flow = (torch.from_numpy(np.array(a)).to(DEV) for a in rc.one_frame_per_sample(c))
    F, (h, w) = len(fs), c['shape']
    M = rc.images_of(F, mask, polarity)
    P = M * h * w
    lay = L.avg_timestamp_layout(F, M, h, w)
    nbytes = lib.dvsof_avg_timestamp_workspace_bytes(F, mask, int(polarity), h, w)
    assert nbytes == lay['bytes']
    ws = torch.full((nbytes // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=DEV)
    term = torch.zeros((), device=DEV)
    assert lib.dvsof_avg_timestamp_fwd(x.data_ptr(), y.data_ptr(), t.data_ptr(), p.data_ptr(), sample.data_ptr(),
                                       x.numel(), ts.data_ptr(), fs.data_ptr(), flow.data_ptr(), F, h, w, mask,
                                       int(polarity), term.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()) == 0
    raw = ws.cpu().numpy().view(np.uint8)

    def part(key, dtype, count):
        return raw[lay[key]:lay[key] + count * np.dtype(dtype).itemsize].view(dtype)
    return ([part(k, np.int64, P).reshape(M, h, w) for k in ('q', 's', 'base')]
            + [part('count', np.uint32, P).reshape(M, h, w)], part('rows', L.AVG_TIMESTAMP_ROW_DTYPE, M),
            term.cpu().numpy())


@pytest.mark.parametrize('name', rc.ONE_PER_SAMPLE_IDS)
def test_with_one_frame_per_sample_the_bytes_are_the_training_terms(name):
    c = rc.case(name)
    d = on_device(c)
    for mask, polarity in ((5, False), (7, True), (1, False), (2, True)):
        images, rows = run(c, mask, polarity, d)
        term_images, term_rows, term = term_workspace(c, mask, polarity)
        for k, a, b in zip(rc.IMAGES, host(images), term_images):
            assert np.array_equal(a, b), (k, mask, polarity)
        assert rows.cpu().numpy().tobytes() == term_rows.tobytes(), (mask, polarity)
        rsat = dev_eval.derive_rsat(rows)
        total = np.float64(0)
        for v in np.where(np.isnan(rsat), 0.0, rsat):       # the term counts an image without a baseline as 0
            total = total + v
        assert np.float32(total / np.float64(len(rsat))).tobytes() == term.tobytes(), (mask, polarity)


@pytest.mark.parametrize('name', rc.CASE_IDS)
def test_the_order_of_the_events_does_not_matter(name):
    c = rc.case(name)
    for mask, polarity in ((7, True), (5, False), (2, True)):
        assert same(run(rc.permuted(c), mask, polarity), want(name, mask, polarity)), (mask, polarity)


@pytest.mark.parametrize('name', [n for n in rc.CASE_IDS if '_F3' in n])
def test_a_batch_equals_its_frames_alone(name):
    c = rc.case(name)
    for mask, polarity in ((7, True), (5, False)):
        per = rc.images_of(1, mask, polarity)
        images, rows = run(c, mask, polarity)
        for f in range(3):
            alone, rows1 = run(rc.single_frame(c, f), mask, polarity)
            for a, b in zip(alone, images):
                assert torch.equal(a, b[f * per:(f + 1) * per]), (f, mask, polarity)
            assert torch.equal(rows1, rows[f * per:(f + 1) * per])


# ------------------------------------------------------------ frame rule
def small_case(n=600, shape=(5, 7), F=3, seed=3):
    h, w = shape
    rng = np.random.default_rng(seed)
    begin = np.array([40, 40 + (n - 90) // 2, 40 + (n - 90) // 2, n - 50], np.int64)    # an empty middle frame
    c = dict(x=rng.integers(0, w, n), y=rng.integers(0, h, n), t=(rng.integers(0, 257, n) / 512).astype(np.float32),
             p=rng.choice(np.array([-1, 1], np.int64), n), begin=begin, ts=np.tile(np.array([0, 0.5], np.float32), F),
             flow=rng.normal(0, 2, (F, 2, h, w)).astype(np.float32), shape=shape)
    return c


def test_events_of_no_frame_and_cropped_slots_take_no_part():
    c = small_case()
    n, begin = c['x'].size, c['begin']
    expected = dev_eval.iwe_avg_timestamp_host(*rc.args_of(c), 7, True)
    rows = dev_eval.iwe_avg_timestamp_rows_host(*expected)
    assert same(run(c, 7, True), (expected, rows))
    per = rc.images_of(1, 7, True)
    assert not any(a[per:2 * per].any() for a in expected), 'the middle frame is empty'
    assert np.isnan(dev_eval.derive_rsat(rows)[per:2 * per]).all()
    # what lies before begin[0] and from begin[F] on changes nothing, whatever it holds
    other = {k: c[k].copy() for k in ('x', 'y', 't', 'p')}
    for k in ('x', 'y'):
        other[k][:begin[0]] = 0
        other[k][begin[-1]:] = 0
    other['t'][:begin[0]] = 0.25
    assert same(run(dict(c, **other), 7, True), (expected, rows))
    # events of the frames alone: the same images
    inside = dict(c, begin=begin - begin[0], **{k: c[k][begin[0]:begin[-1]] for k in ('x', 'y', 't', 'p')})
    assert same(run(inside, 7, True), (expected, rows))
    # -1 slots (either coordinate, or one past the frame) are in no count: the events that are left
    slots = {k: c[k].copy() for k in ('x', 'y')}
    slots['x'][45:60], slots['y'][60:75] = -1, -1
    slots['x'][75:80], slots['y'][80:85] = c['shape'][1], c['shape'][0]
    cut = dict(c, **slots)
    expected_cut = dev_eval.iwe_avg_timestamp_host(*rc.args_of(cut), 7, True)
    assert int(expected[3][0::2].sum() + expected[3][1::2].sum()) - \
        int(expected_cut[3][0::2].sum() + expected_cut[3][1::2].sum()) == 3 * 40
    assert same(run(cut, 7, True), (expected_cut, dev_eval.iwe_avg_timestamp_rows_host(*expected_cut)))
    # tau is clamped, not tested: an event outside its window's times counts, at tau = 0 or 1
    late = c['t'].copy()
    late[begin[0]:begin[0] + 20], late[begin[0] + 20:begin[0] + 40] = 3.0, -1.0
    moved = dict(c, t=late)
    expected_late = dev_eval.iwe_avg_timestamp_host(*rc.args_of(moved), 7, True)
    assert np.array_equal(expected_late[3], expected[3]) and not np.array_equal(expected_late[2], expected[2])
    assert same(run(moved, 7, True), (expected_late, dev_eval.iwe_avg_timestamp_rows_host(*expected_late)))


def test_a_flow_of_nan_or_1e30_is_counted_and_splats_nothing():
    h, w = 5, 7
    flow = np.zeros((1, 2, h, w), np.float32)
    flow[0, 0, 1, 2], flow[0, 1, 3, 4] = np.nan, 1e30
    x, y = np.array([2, 2, 4, 4, 0], np.int64), np.array([1, 1, 3, 3, 0], np.int64)
    c = dict(x=x, y=y, t=np.array([0.25, 0.5, 0.25, 0.125, 0.25], np.float32), p=np.ones(5, np.int64),
             begin=np.array([0, 5], np.int64), ts=np.array([0, 0.5], np.float32), flow=flow, shape=(h, w))
    (q, s, base, count), rows = run(c, 4, False)      # warped to the end of the window: a = 1 - tau
    q, s, base, count = host((q, s, base, count))
    one = 1 << 32
    assert count[0, 1, 2] == 2 and count[0, 3, 4] == 2 and count[0, 0, 0] == 1 and count.sum() == 5
    assert base[0, 1, 2] == one // 2 and base[0, 3, 4] == one // 2 + one * 3 // 4 and base[0, 0, 0] == one // 2
    assert q.sum() == one and q[0, 0, 0] == one and s.sum() == one // 2 and s[0, 0, 0] == one // 2
    expected = dev_eval.iwe_avg_timestamp_host(*rc.args_of(c), 4, False)
    for a, b in zip((q, s, base, count), expected):
        assert np.array_equal(a, b)
    assert rows.cpu().numpy().tobytes() == dev_eval.iwe_avg_timestamp_rows_host(*expected).tobytes()
    res = dev_eval.read_avg_timestamp_rows(rows)
    assert res['n'][0] == 1 and res['n0'][0] == 3


def test_no_events_and_no_frames():
    lib = _lib.lib()
    F, h, w, mask, pol = 2, 5, 7, 7, 1
    M = rc.images_of(F, mask, pol)
    nbytes = lib.dvsof_iwe_avg_timestamp_image_bytes(F, h, w, mask, pol)
    need = lib.dvsof_iwe_avg_timestamp_workspace_bytes(F, h, w, mask, pol)
    begin = torch.zeros(F + 1, dtype=torch.long, device=DEV)
    ts, flow = torch.zeros(2 * F, device=DEV), torch.ones(F, 2, h, w, device=DEV)
    images = torch.full((nbytes,), 0xAA, dtype=torch.uint8, device=DEV)
    rows = torch.full((M, 32), 0xAA, dtype=torch.uint8, device=DEV)
    ws = torch.full((need,), 0xAA, dtype=torch.uint8, device=DEV)
    # n_events = 0, with no column at all: the images are zeroed, the rows are those of empty images
    assert lib.dvsof_iwe_avg_timestamp(None, None, None, None, 0, begin.data_ptr(), ts.data_ptr(), flow.data_ptr(),
                                       F, h, w, mask, pol, images.data_ptr(), nbytes, rows.data_ptr(), ws.data_ptr(),
                                       need, _lib.stream()) == 0
    torch.cuda.synchronize()
    assert not images.any() and not rows.any()
    assert np.isnan(dev_eval.derive_rsat(rows)).all()
    # F = 0: nothing is touched, no pointer is needed
    images.fill_(0x55), rows.fill_(0x55)
    assert all(rc_ == 0 for rc_ in rc.empty_calls(lib))
    assert lib.dvsof_iwe_avg_timestamp(None, None, None, None, 0, None, None, None, 0, h, w, mask, pol,
                                       images.data_ptr(), nbytes, rows.data_ptr(), ws.data_ptr(), need,
                                       _lib.stream()) == 0
    torch.cuda.synchronize()
    assert bool((images == 0x55).all()) and bool((rows == 0x55).all())
    # the front end
    empty = {'x': torch.zeros(0, dtype=torch.long, device=DEV), 'y': torch.zeros(0, dtype=torch.long, device=DEV),
             'timestamp': torch.zeros(0, device=DEV), 'polarity': torch.zeros(0, dtype=torch.long, device=DEV)}
    got, r = dev_eval.iwe_avg_timestamp(empty, begin, ts, flow, mask, True)
    assert all(tuple(a.shape) == (M, h, w) and not a.any() for a in got) and not r.any()
    got, r = dev_eval.iwe_avg_timestamp(empty, begin[:1], ts[:0], flow[:0], mask, True)
    assert all(tuple(a.shape) == (0, h, w) for a in got) and tuple(r.shape) == (0, 32)


def test_more_events_than_one_pass_of_the_capped_grid():
    """2048 blocks of 256 threads cover 524288 events: the last 300 are a thread's second."""
    h, w, n = 16, 16, 2048 * 256 + 300
    rng = np.random.default_rng(12)
    c = dict(x=rng.integers(-1, w, n), y=rng.integers(0, h, n), t=(rng.integers(0, 257, n) / 512).astype(np.float32),
             p=rng.integers(-1, 2, n), begin=np.array([3, n - 5], np.int64), ts=np.array([0, 0.5], np.float32),
             flow=rng.normal(0, 3, (1, 2, h, w)).astype(np.float32), shape=(h, w))
    expected = dev_eval.iwe_avg_timestamp_host(*rc.args_of(c), 5, True)
    assert same(run(c, 5, True), (expected, dev_eval.iwe_avg_timestamp_rows_host(*expected)))
    assert int(expected[3].max()) > 200
    tail = dict(c, begin=np.array([2048 * 256, n], np.int64))       # the second pass alone
    expected = dev_eval.iwe_avg_timestamp_host(*rc.args_of(tail), 5, True)
    assert same(run(tail, 5, True), (expected, dev_eval.iwe_avg_timestamp_rows_host(*expected)))
    assert 0 < int(expected[3][0].sum()) < 300


# ----------------------------------------------------------- every byte
@pytest.mark.parametrize('name', ['5x7_F3_empty_middle', '33x37_F3', '3x129_F3_empty_middle', '1x1_F1'])
def test_every_output_byte_is_written_from_either_fill(name):
    c = rc.case(name)
    d = on_device(c)
    lib = _lib.lib()
    F, (h, w) = len(c['begin']) - 1, c['shape']
    for mask, polarity in ((7, True), (1, False), (6, True)):
        (q, s, base, count), rows_want, canvas_want = want(name, mask, polarity)
        M = len(q)
        region_want = b''.join(a.tobytes() for a in (q, s, base, count))
        nbytes = lib.dvsof_iwe_avg_timestamp_image_bytes(F, h, w, mask, int(polarity))
        need = lib.dvsof_iwe_avg_timestamp_workspace_bytes(F, h, w, mask, int(polarity))
        assert len(region_want) == 28 * M * h * w <= nbytes < len(region_want) + 8
        for fill in (0xAA, 0x55):
            region = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
            rows = torch.full((M, 32), fill, dtype=torch.uint8, device=DEV)
            ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
            canvas = torch.full((M, h, 2 * w, 3), fill, dtype=torch.uint8, device=DEV)
            assert lib.dvsof_iwe_avg_timestamp(
                d['x'].data_ptr(), d['y'].data_ptr(), d['t'].data_ptr(), d['p'].data_ptr(), d['x'].numel(),
                d['begin'].data_ptr(), d['ts'].data_ptr(), d['flow'].data_ptr(), F, h, w, mask, int(polarity),
                region.data_ptr(), nbytes, rows.data_ptr(), ws.data_ptr(), need, _lib.stream()) == 0
            assert lib.dvsof_iwe_avg_timestamp_render(region.data_ptr(), F, h, w, mask, int(polarity),
                                                      canvas.data_ptr(), _lib.stream()) == 0
            got = region.cpu().numpy().tobytes()
            assert got[:len(region_want)] == region_want, (mask, polarity, hex(fill))
            assert got[len(region_want):] == bytes([fill]) * (nbytes - len(region_want)), 'the padding is left alone'
            assert rows.cpu().numpy().tobytes() == rows_want.tobytes(), (mask, polarity, hex(fill))
            assert np.array_equal(canvas.cpu().numpy(), canvas_want), (mask, polarity, hex(fill))


def test_the_render_of_a_selection_of_images():
    """The hook draws some frames of a batch: their images, gathered."""
    name = '33x37_F3'
    images, _ = run(rc.case(name), 5, True)
    canvas_want = want(name, 5, True)[2]
    pick = torch.tensor([8, 9, 10, 11, 0, 1, 2, 3], device=DEV)
    canvas = dev_eval.iwe_avg_timestamp_render(*(a[pick] for a in images))
    assert np.array_equal(canvas.cpu().numpy(), canvas_want[pick.cpu().numpy()])


# --------------------------------------------------------- argument rules
def test_argument_rules_with_guard_bytes_around_every_output():
    lib = _lib.lib()
    F, h, w, n = 2, 5, 7, 11
    mask, pol = 7, 1
    M = 6 * F
    nbytes = lib.dvsof_iwe_avg_timestamp_image_bytes(F, h, w, mask, pol)
    need = lib.dvsof_iwe_avg_timestamp_workspace_bytes(F, h, w, mask, pol)
    assert nbytes == 28 * M * h * w and need == 32 * M
    t = dict(x=torch.zeros(n, dtype=torch.long), y=torch.zeros(n, dtype=torch.long), t=torch.zeros(n),
             p=torch.ones(n, dtype=torch.long), begin=torch.tensor([0, 5, 11]), ts=torch.zeros(2 * F),
             flow=torch.zeros(F, 2, h, w))
    t = {k: v.to(DEV) for k, v in t.items()}
    # the outputs with guard bytes in front and behind
    sizes = dict(images=nbytes, rows=32 * M, ws=need, canvas=M * h * 2 * w * 3)
    out = {k: torch.full((GUARD + v + GUARD,), 0xAA, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
    a = {k: v.data_ptr() for k, v in t.items()}
    a.update({k: v.data_ptr() + GUARD for k, v in out.items()})
    a['n'] = n
    seen = {rc.EINVAL: 0, rc.ENOSPACE: 0}
    for what, call, code in rc.bad_calls(lib, a, F, h, w, mask, pol):
        assert call() == code, what
        seen[code] += 1
    torch.cuda.synchronize()
    assert seen == {rc.EINVAL: 43, rc.ENOSPACE: 5}
    for k, v in out.items():
        assert bool((v == 0xAA).all()), f'{k}: a refused call wrote'
    assert all(code == 0 for code in rc.empty_calls(lib))
    # a good call writes inside the guards only; without polarity p may be null
    args = (a['begin'], a['ts'], a['flow'], F, h, w)
    assert lib.dvsof_iwe_avg_timestamp(a['x'], a['y'], a['t'], None, n, *args, mask, 0, a['images'], nbytes,
                                       a['rows'], a['ws'], need, None) == 0
    assert lib.dvsof_iwe_avg_timestamp_render(a['images'], F, h, w, mask, 0, a['canvas'], None) == 0
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v[:GUARD] == 0xAA).all()) and bool((v[-GUARD:] == 0xAA).all()), k
    half = 28 * (M // 2) * h * w                 # C = 1: half the images
    region = out['images'][GUARD:GUARD + half].cpu().numpy()
    count = region[24 * (M // 2) * h * w:].view(np.uint32)
    assert int(count.sum()) == 3 * n and bool((out['images'][GUARD + half:-GUARD] == 0xAA).all())
    # the Python front end refuses what it can name
    ev = {'x': t['x'], 'y': t['y'], 'timestamp': t['t']}
    with pytest.raises(ValueError, match='polarity column'):
        dev_eval.iwe_avg_timestamp(ev, t['begin'], t['ts'], t['flow'], 7, True)
    with pytest.raises(ValueError, match='outside'):
        dev_eval.iwe_avg_timestamp(ev, t['begin'], t['ts'], t['flow'], 8, False)
