"""The tiled schedule of the splat into the images of warped events
(csrc/tiled_splat.hip, include/dvsof_event_images_tiled.h) against the
numpy restatements the per-event kernels are pinned to
(eval.iwe_splat_multi_host, loss.contrast_multi_fwd_host), byte for byte, at
mode 1: tile seams and ragged edges, a bucket past its capacity, a refused
plan, empty calls, both frame rules and both column forms, the backward on the
tiled forward's workspace, and the keyword through the public interface.  Tile
size and capacity are read from dvsof_event_images_tiled_plan."""
import ctypes

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L, testing
from tests import contrast_multi_cases as cm, eval_cases as ec, iwe_multi_cases as im

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32 = np.float32
OPTIONS = [(1, False), (1, True), (7, False), (7, True)]
TERM_KEYS = ('x', 'y', 't', 'p', 's')


def plan(F, mask, pol, h, w, n):
    """-> (tile width, tile height, tiles, capacity), or None where the plan is refused."""
    out = (ctypes.c_int32 * 4)()
    return tuple(out) if _lib.lib().dvsof_event_images_tiled_plan(F, mask, int(pol), h, w, n, out) else None


def seam_case():
    """Three frames of (2 TH + 8) x (2 TW + 8): eight events on every crossing of the first and
    last column and row of every tile, 300 anywhere, under a flow of up to three pixels (so
    footprints straddle every seam, reach corner -1 and leave the image) with one NaN under an
    event.  For the metric the middle frame is empty and five events at either end belong to
    no frame; for the term two windows of sample 0 overlap."""
    tw, th = plan(1, 1, 0, 64, 64, 0)[:2]
    h, w = 2 * th + 8, 2 * tw + 8
    rng = np.random.default_rng(11)
    xs, ys = [0, tw - 1, tw, 2 * tw - 1, 2 * tw, w - 1], [0, th - 1, th, 2 * th - 1, 2 * th, h - 1]
    x = np.concatenate([np.repeat(np.tile(xs, len(ys)), 8), rng.integers(0, w, 300)]).astype(np.int64)
    y = np.concatenate([np.repeat(np.repeat(ys, len(xs)), 8), rng.integers(0, h, 300)]).astype(np.int64)
    order = rng.permutation(x.size)
    x, y, n = x[order], y[order], x.size
    flow = rng.uniform(-3, 3, (3, 2, h, w)).astype(F32)
    flow[0, 0, y[7], x[7]] = np.nan
    p = rng.choice(np.array([-1, 1], np.int64), n)
    s = (np.arange(n) >= n // 2).astype(np.int64)
    return dict(x=x, y=y, t=rng.random(n).astype(F32) * F32(1.5), p=p, s=s, shape=(h, w), flow=flow,
                ts=np.array([0, 1, 0.5, 1.5, 0, 1.5], F32), fs=np.array([0, 0, 1], np.int64),
                begin=np.array([5, n // 2, n // 2, n - 5], np.int64))


def metric(c, mask, pol, mode=1):
    """dvsof_iwe_splat_multi_tiled (or the twin) from filled buffers -> (rc, q, count uint32)."""
    lib = _lib.lib()
    h, w = c['shape']
    F = len(c['begin']) - 1
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in ('x', 'y', 't', 'p', 'begin', 'ts', 'flow')}
    M = im.images_of(F, mask, pol)
    q = torch.full((M, h, w), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=DEV)
    count = torch.full((M, h, w), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    args = [d[k].data_ptr() for k in ('x', 'y', 't', 'p')] + [d['x'].numel()] + \
        [d[k].data_ptr() for k in ('begin', 'ts', 'flow')] + [F, h, w, mask, int(pol), q.data_ptr(), count.data_ptr(),
                                                              _lib.stream()]
    if mode is None:
        rc = lib.dvsof_iwe_splat_multi(*args)
    else:
        ws, nbytes = dev_eval.event_images_tiled_workspace(F, mask, pol, h, w, d['x'].numel(), DEV)
        if ws is not None:
            ws.fill_(0x5A5A5A5A5A5A5A5A)
        rc = lib.dvsof_iwe_splat_multi_tiled(*args, _lib.ptr(ws), nbytes, mode)
    return rc, q.cpu().numpy(), count.cpu().numpy().view(np.uint32)


def term(c, mask, pol, tiled, encoded=False):
    """The term's forward (tiled at mode 1, or the twin) and backward -> dict of numpy."""
    lib = _lib.lib()
    h, w = c['shape']
    F, n = len(c['fs']), c['x'].size
    M = F * len(cm.rhos(mask)) * (2 if pol else 1)
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in TERM_KEYS + ('ts', 'fs', 'flow')}
    if encoded:     # the events are in sample order
        off = torch.from_numpy(np.searchsorted(c['s'], np.arange(int(c['s'].max()) + 2))).to(DEV)
        cols = [d['x'].short(), d['y'].short(), d['t'], (d['p'] > 0).to(torch.uint8), off]
        head, form = [k.data_ptr() for k in cols] + [off.numel() - 1, n], '_encoded'
    else:
        head, form = [d[k].data_ptr() for k in TERM_KEYS] + [n], ''
    head += [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, h, w, mask, int(pol)]
    q = torch.full((M, h, w), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=DEV)
    count = torch.full((M, h, w), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rows = torch.full((M, 48), 0x5A, dtype=torch.uint8, device=DEV)
    value = torch.full((), float('nan'), device=DEV)
    nbytes = lib.dvsof_contrast_multi_workspace_bytes(F, mask, int(pol), h, w)
    ws = torch.full((nbytes // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=DEV)
    out = [q.data_ptr(), count.data_ptr(), rows.data_ptr(), value.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()]
    if tiled:
        tiles, tile_bytes = dev_eval.event_images_tiled_workspace(F, mask, pol, h, w, n, DEV)
        assert tiles is not None
        tiles.fill_(0x5A5A5A5A5A5A5A5A)
        out += [tiles.data_ptr(), tile_bytes, 1]
    assert getattr(lib, 'dvsof_contrast_multi_fwd' + form + ('_tiled' if tiled else ''))(*head, *out) == 0
    seed = torch.ones((), device=DEV)
    grad = torch.full((F, 2, h, w), float('nan'), device=DEV)
    assert getattr(lib, 'dvsof_contrast_multi_bwd' + form)(*head, q.data_ptr(), ws.data_ptr(), nbytes,
                                                          seed.data_ptr(), 0.75, grad.data_ptr(), _lib.stream()) == 0
    return dict(q=q.cpu().numpy(), count=count.cpu().numpy().view(np.uint32), rows=rows.cpu().numpy(),
                term=value.cpu().numpy(), grad=grad.cpu().numpy())


@pytest.fixture(scope='module')
def seams():
    return seam_case()


@pytest.mark.parametrize('mask,pol', OPTIONS)
def test_seams_and_ragged_edges_by_the_metrics_frame_rule(seams, mask, pol):
    h, w = seams['shape']
    tw, th, tiles, _ = plan(3, mask, pol, h, w, seams['x'].size)
    assert tiles == im.images_of(3, mask, pol) * 3 * 3 and (h, w) == (2 * th + 8, 2 * tw + 8)
    want_q, want_count = dev_eval.iwe_splat_multi_host(*im.args_of(seams), mask, pol)
    rc, q, count = metric(seams, mask, pol)
    assert rc == 0 and np.array_equal(q, want_q) and np.array_equal(count, want_count)
    f = im.images_of(1, mask, pol)      # the middle frame is empty, its neighbours are not
    assert not want_q[f:2 * f].any() and want_q[:f].any() and want_q[2 * f:].any()


@pytest.mark.parametrize('encoded', [False, True], ids=['wire', 'encoded'])
@pytest.mark.parametrize('mask,pol', OPTIONS)
def test_the_term_and_its_backward_on_both_column_forms(seams, mask, pol, encoded):
    c = seams
    in_two = (c['s'] == 0) & (c['t'] >= 0.5) & (c['t'] <= 1)
    assert in_two.sum() > 50                                    # events in both windows of sample 0
    want = L.contrast_multi_fwd_host(*cm.args_of(c), mask, pol)
    got, twin = term(c, mask, pol, True, encoded), term(c, mask, pol, False, encoded)
    assert np.array_equal(got['q'], want['q']) and np.array_equal(got['count'], want['count'])
    assert got['term'].tobytes() == want['term'].tobytes()
    for k in ('q', 'count', 'rows', 'term', 'grad'):
        assert got[k].tobytes() == twin[k].tobytes(), k
    assert np.abs(got['grad']).max() > 0 and not np.isnan(got['grad']).any()


def test_a_bucket_past_its_capacity_loses_nothing():
    tw, th = plan(1, 1, 0, 64, 64, 0)[:2]
    c = cm.sink_case(shape=(5 * th, 5 * tw), n=6000)     # the centre lies inside the middle tile
    h, w = c['shape']
    _, _, tiles, cap = plan(1, 1, False, h, w, 6000)
    assert tiles == 25
    # the records of the centre's tile, from the float64 warp: far more than a bucket holds
    t = c['t'].astype(np.float64)
    xw, yw = c['x'] - t * (c['x'] - w / 2), c['y'] - t * (c['y'] - h / 2)
    per_tile = np.bincount((np.floor(yw) // th * 5 + np.floor(xw) // tw).astype(np.int64), minlength=25)
    assert per_tile.max() > 1.25 * cap, (per_tile, cap)
    want = L.contrast_multi_fwd_host(*cm.args_of(c), 1, False)
    got = term(c, 1, False, True)
    assert np.array_equal(got['q'], want['q']) and np.array_equal(got['count'], want['count'])
    assert got['term'].tobytes() == want['term'].tobytes()


def test_a_refused_plan_runs_the_per_event_kernel():
    F, n = 1400, 2800                    # 8400 tiles of 2 x 2 pixels at six images a frame
    rng = np.random.default_rng(5)
    c = dict(x=rng.integers(0, 2, n), y=rng.integers(0, 2, n), t=rng.random(n).astype(F32),
             p=rng.choice(np.array([-1, 1], np.int64), n), begin=np.arange(F + 1, dtype=np.int64) * 2,
             ts=np.tile(np.array([0, 1], F32), F), flow=rng.uniform(-1, 1, (F, 2, 2, 2)).astype(F32), shape=(2, 2))
    assert plan(F, 7, True, 2, 2, n) is None and plan(F // 2, 7, True, 2, 2, n) is not None
    assert _lib.lib().dvsof_event_images_tiled_workspace_bytes(F, 7, 1, 2, 2, n) == 0
    rc, q, count = metric(c, 7, True)
    twin = metric(c, 7, True, mode=None)
    assert rc == twin[0] == 0 and np.array_equal(q, twin[1]) and np.array_equal(count, twin[2]) and q.any()


def test_empty_calls_are_the_twins(seams):
    lib = _lib.lib()
    none = dict(seams, **{k: seams[k][:0] for k in ('x', 'y', 't', 'p')})
    for c in (none, dict(seams, begin=np.zeros(4, np.int64))):          # no events; events of no frame
        got, twin = metric(c, 7, True), metric(c, 7, True, mode=None)
        assert got[0] == twin[0] == 0 and not got[1].any() and not got[2].any()
    nothing = (None,) * 4 + (0,) + (None,) * 3 + (0, 4, 4, 7, 1, None, None, None)
    assert lib.dvsof_iwe_splat_multi_tiled(*nothing, None, 0, 1) == lib.dvsof_iwe_splat_multi(*nothing) == 0
    term_nothing = (None,) * 5 + (0,) + (None,) * 3 + (0, 4, 4, 7, 1) + (None,) * 5 + (0, None)
    assert lib.dvsof_contrast_multi_fwd_tiled(*term_nothing, None, 0, 1) == \
        lib.dvsof_contrast_multi_fwd(*term_nothing) == 0
    assert lib.dvsof_iwe_splat_multi_tiled(*nothing, None, 0, 2) != 0          # no such mode


def test_losses_contrast_with_the_keyword_returns_the_same_bits(seams):
    c = seams
    h, w = c['shape']
    events = {k: torch.from_numpy(np.array(c[v])).to(DEV)
              for k, v in (('x', 'x'), ('y', 'y'), ('timestamp', 't'), ('polarity', 'p'), ('sample_index', 's'))}
    ts, fs = torch.from_numpy(c['ts']).to(DEV), torch.from_numpy(c['fs']).to(DEV)
    losses = L.Losses([(h, w)], 2, DEV)
    runs = []
    for options in ({}, {'tiled': 'force'}, {'tiled': 'force'}, {'tiled': True}):
        flow = torch.from_numpy(np.nan_to_num(c['flow'])).to(DEV).requires_grad_(True)
        value, logged = losses.contrast([flow], ts, fs, events, weight=0.5, references=('start', 'end'),
                                        polarity=True, **options)
        value.backward()
        runs.append((value.detach().cpu().numpy().tobytes(), logged.cpu().numpy().tobytes(),
                     flow.grad.cpu().numpy().tobytes()))
    assert runs[0] == runs[1] == runs[2] == runs[3]
    with pytest.raises(ValueError, match='tiled'):
        losses.contrast([flow], ts, fs, events, tiled='always')


def test_flow_warp_loss_with_the_keyword_returns_the_same_bits():
    from dvs_of_training_framework_amd.sequence import FrameSequence
    case = ec.make_eval_case(per_frame=3000)
    x, y, t, p = case['events']
    image_ts = np.append(case['frames'][:, 0], case['frames'][-1, 1])
    seq = FrameSequence([x, y, np.round(t * 65536.0) / 65536.0, p],
                        np.zeros((len(image_ts),) + ec.EVAL_SHAPE, np.uint8), image_ts, device=DEV)
    frames = ec.EVAL_FRAMES
    shape = ec.EVAL_BOX[2:]
    flows = torch.from_numpy(np.random.default_rng(3).normal(0, 2.5, (len(frames), 2) + tuple(shape))
                             .astype(F32)).to(DEV)

    class Prescribed:
        def flow_sequence(self, seq, starts, stops, box=None, return_events=False):
            index = {float(f[0]): i for i, f in enumerate(frames)}
            return torch.stack([flows[index[float(s)]] for s in starts]), seq.collate_frames(starts, stops, box)
    for options in ({}, {'references': ('start', 'middle', 'end'), 'polarity': True}):
        plain = testing.flow_warp_loss(Prescribed(), seq, frames, ec.EVAL_BOX, **options)
        for _ in range(2):
            tiled = testing.flow_warp_loss(Prescribed(), seq, frames, ec.EVAL_BOX, tiled='force', **options)
            assert tiled.tobytes() == plain.tobytes() and (plain['sum_q'] > 0).all()
