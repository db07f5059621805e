"""The tiled schedule of the splat into the average-timestamp images
(csrc/tiled_splat.hip, include/dvsof_avg_timestamp_tiled.h) against the
numpy restatements the per-event kernels are pinned to
(loss.avg_timestamp_fwd_host, eval.iwe_avg_timestamp_host), byte for byte, at
mode 1 and from buffers of 0x5A: tile seams and ragged edges, a bucket past its
capacity, a refused plan, empty calls, both frame rules and both column forms,
the backward on the tiled forward's workspace, and the keyword through the
public interface."""
import ctypes

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L, testing
from tests import avg_timestamp_cases as ac, eval_cases as ec, iwe_avg_timestamp_cases as rc
from tests.test_gpu_event_images_tiled import seam_case

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32 = np.float32
FILL = 0x5A5A5A5A5A5A5A5A
OPTIONS = [(1, False), (1, True), (7, False), (7, True)]


def plan(F, mask, pol, h, w, n):
    """-> (tile width, tile height, tiles, capacity), or None where the plan is refused."""
    out = (ctypes.c_int32 * 4)()
    return tuple(out) if _lib.lib().dvsof_event_images_tiled_plan(F, mask, int(pol), h, w, n, out) else None


def tile_tail(F, mask, pol, h, w, n, mode):
    """The three arguments behind the twin's, the tile workspace filled."""
    tiles, nbytes = dev_eval.avg_timestamp_tiled_workspace(F, mask, pol, h, w, n, DEV)
    if tiles is not None:
        tiles.fill_(FILL)
    return tiles, [_lib.ptr(tiles), nbytes, mode]


def metric(c, mask, pol, mode=1):
    """dvsof_iwe_avg_timestamp_tiled (mode None: the twin) -> (rc, (q, s, base, count), rows bytes)."""
    lib = _lib.lib()
    h, w = c['shape']
    F = len(c['begin']) - 1
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in ('x', 'y', 't', 'p', 'begin', 'ts', 'flow')}
    n, M = d['x'].numel(), rc.images_of(F, mask, pol)
    nbytes = lib.dvsof_iwe_avg_timestamp_image_bytes(F, h, w, mask, int(pol))
    images = torch.full((nbytes // 8,), FILL, dtype=torch.long, device=DEV)
    rows = torch.full((M, 32), 0x5A, dtype=torch.uint8, device=DEV)
    ws_bytes = lib.dvsof_iwe_avg_timestamp_workspace_bytes(F, h, w, mask, int(pol))
    ws = torch.full((ws_bytes // 8,), FILL, dtype=torch.long, device=DEV)
    args = [d[k].data_ptr() for k in ('x', 'y', 't', 'p')] + [n] + [d[k].data_ptr() for k in ('begin', 'ts', 'flow')] \
        + [F, h, w, mask, int(pol), images.data_ptr(), nbytes, rows.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream()]
    if mode is None:
        code = lib.dvsof_iwe_avg_timestamp(*args)
    else:
        keep, tail = tile_tail(F, mask, pol, h, w, n, mode)
        code = lib.dvsof_iwe_avg_timestamp_tiled(*args, *tail)
    views = dev_eval._avg_timestamp_views(images.view(torch.uint8), M, h, w)
    q, s, base, count = (v.cpu().numpy() for v in views)
    return code, (q, s, base, count.view(np.uint32)), rows.cpu().numpy().tobytes()


def term(c, mask, pol, tiled, encoded=False):
    """The term's forward (tiled at mode 1, or the twin) and backward -> the workspace after the
    forward as bytes, its images and rows, the term and the gradient."""
    lib = _lib.lib()
    h, w = c['shape']
    F, n = len(c['fs']), c['x'].size
    M = F * len(ac.rhos(mask)) * (2 if pol else 1)
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in ac.KEYS}
    if encoded:     # the events are in sample order
        off = torch.from_numpy(np.searchsorted(c['s'], np.arange(int(c['s'].max()) + 2))).to(DEV)
        cols = [d['x'].short(), d['y'].short(), d['t'], (d['p'] > 0).to(torch.uint8), off]
        head, form = [k.data_ptr() for k in cols] + [off.numel() - 1, n], '_encoded'
    else:
        head, form = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n], ''
    head += [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, h, w, mask, int(pol)]
    value = torch.full((), float('nan'), device=DEV)
    nbytes = lib.dvsof_avg_timestamp_workspace_bytes(F, mask, int(pol), h, w)
    ws = torch.full((nbytes // 8,), FILL, dtype=torch.long, device=DEV)
    out = [value.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()]
    if tiled:
        keep, tail = tile_tail(F, mask, pol, h, w, n, 1)
        assert keep is not None
        out += tail
    assert getattr(lib, 'dvsof_avg_timestamp_fwd' + form + ('_tiled' if tiled else ''))(*head, *out) == 0
    after = ws.cpu().numpy().view(np.uint8)
    seed = torch.ones((), device=DEV)
    grad = torch.full((F, 2, h, w), float('nan'), device=DEV)
    assert getattr(lib, 'dvsof_avg_timestamp_bwd' + form)(*head, ws.data_ptr(), nbytes, seed.data_ptr(), 0.75,
                                                         grad.data_ptr(), _lib.stream()) == 0
    lay, P = L.avg_timestamp_layout(F, M, h, w), M * h * w
    got = {k: after[lay[k]:lay[k] + P * 8].view(np.int64).reshape(M, h, w) for k in ('q', 's', 'base')}
    got['count'] = after[lay['count']:lay['count'] + P * 4].view(np.uint32).reshape(M, h, w)
    got['rows'] = after[lay['rows']:lay['rows'] + M * 32].view(L.AVG_TIMESTAMP_ROW_DTYPE)
    return dict(got, ws=after.tobytes(), term=value.cpu().numpy(), grad=grad.cpu().numpy())


def same_as_host(got, want):
    for k in ('q', 's', 'base', 'count'):
        assert np.array_equal(got[k], want[k]), k
    assert got['rows'].tobytes() == want['rows'].tobytes() and got['term'].tobytes() == want['term'].tobytes()


@pytest.fixture(scope='module')
def seams():
    return seam_case()


@pytest.mark.parametrize('encoded', [False, True], ids=['wire', 'encoded'])
@pytest.mark.parametrize('mask,pol', OPTIONS)
def test_the_term_and_its_backward_on_both_column_forms(seams, mask, pol, encoded):
    c = seams
    h, w = c['shape']
    tw, th, tiles, _ = plan(3, mask, pol, h, w, c['x'].size)
    assert tiles == rc.images_of(3, mask, pol) * 3 * 3 and (h, w) == (2 * th + 8, 2 * tw + 8)
    got, twin = term(c, mask, pol, True, encoded), term(c, mask, pol, False, encoded)
    same_as_host(got, L.avg_timestamp_fwd_host(*ac.args_of(c), mask, pol))
    assert got['ws'] == twin['ws'], 'a region of the workspace differs from the twin\'s'
    assert got['term'].tobytes() == twin['term'].tobytes() and got['grad'].tobytes() == twin['grad'].tobytes()
    assert got['s'].any() and np.abs(got['grad']).max() > 0 and not np.isnan(got['grad']).any()


@pytest.mark.parametrize('mask,pol', OPTIONS)
def test_seams_and_ragged_edges_by_the_metrics_frame_rule(seams, mask, pol):
    want = dev_eval.iwe_avg_timestamp_host(*rc.args_of(seams), mask, pol)
    code, images, rows = metric(seams, mask, pol)
    assert code == 0 and all(np.array_equal(a, b) for a, b in zip(images, want))
    assert rows == dev_eval.iwe_avg_timestamp_rows_host(*want).tobytes()
    f = rc.images_of(1, mask, pol)      # the middle frame is empty, its neighbours are not
    assert not want[0][f:2 * f].any() and want[1][:f].any() and want[1][2 * f:].any()


def test_a_bucket_past_its_capacity_loses_nothing():
    tw, th = plan(1, 1, 0, 64, 64, 0)[:2]
    c = ac.sink_case(shape=(5 * th, 5 * tw), n=6000)     # the centre lies inside the middle tile
    h, w = c['shape']
    _, _, tiles, cap = plan(1, 1, False, h, w, 6000)
    assert tiles == 25
    # the records of the centre's tile, from the float64 warp: far more than a bucket holds
    t = c['t'].astype(np.float64)
    xw, yw = c['x'] - t * (c['x'] - w / 2), c['y'] - t * (c['y'] - h / 2)
    per_tile = np.bincount((np.floor(yw) // th * 5 + np.floor(xw) // tw).astype(np.int64), minlength=25)
    assert per_tile.max() > 1.25 * cap, (per_tile, cap)
    got = term(c, 1, False, True)
    same_as_host(got, L.avg_timestamp_fwd_host(*ac.args_of(c), 1, False))
    assert got['s'].any()


def test_a_refused_plan_runs_the_per_event_kernel():
    F, n = 1400, 2800                    # 8400 tiles of 2 x 2 pixels at six images a frame
    rng = np.random.default_rng(5)
    c = dict(x=rng.integers(0, 2, n), y=rng.integers(0, 2, n), t=rng.random(n).astype(F32),
             p=rng.choice(np.array([-1, 1], np.int64), n), begin=np.arange(F + 1, dtype=np.int64) * 2,
             ts=np.tile(np.array([0, 1], F32), F), flow=rng.uniform(-1, 1, (F, 2, 2, 2)).astype(F32), shape=(2, 2))
    assert plan(F, 7, True, 2, 2, n) is None and plan(F // 2, 7, True, 2, 2, n) is not None
    assert _lib.lib().dvsof_avg_timestamp_tiled_workspace_bytes(F, 7, 1, 2, 2, n) == 0
    got, twin = metric(c, 7, True), metric(c, 7, True, mode=None)
    assert got[0] == twin[0] == 0 and got[2] == twin[2] and got[1][1].any()
    assert all(np.array_equal(a, b) for a, b in zip(got[1], twin[1]))


def test_empty_calls_are_the_twins(seams):
    lib = _lib.lib()
    none = dict(seams, **{k: seams[k][:0] for k in ('x', 'y', 't', 'p')})
    for c in (none, dict(seams, begin=np.zeros(4, np.int64))):          # no events; events of no frame
        got, twin = metric(c, 7, True), metric(c, 7, True, mode=None)
        assert got[0] == twin[0] == 0 and got[2] == twin[2] and not any(a.any() for a in got[1])
    nothing = (None,) * 4 + (0,) + (None,) * 3 + (0, 4, 4, 7, 1, None, 0, None, None, 0, None)
    assert lib.dvsof_iwe_avg_timestamp_tiled(*nothing, None, 0, 1) == lib.dvsof_iwe_avg_timestamp(*nothing) == 0
    term_nothing = (None,) * 5 + (0,) + (None,) * 3 + (0, 4, 4, 7, 1, None, None, 0, None)
    assert lib.dvsof_avg_timestamp_fwd_tiled(*term_nothing, None, 0, 1) == \
        lib.dvsof_avg_timestamp_fwd(*term_nothing) == 0
    assert lib.dvsof_iwe_avg_timestamp_tiled(*nothing, None, 0, 2) != 0         # no such mode
    assert lib.dvsof_avg_timestamp_fwd_tiled(*term_nothing, None, 0, -1) != 0


def test_losses_avg_timestamp_tiled_returns_the_same_bits(seams):
    c = seams
    h, w = c['shape']
    events = {k: torch.from_numpy(np.array(c[v])).to(DEV)
              for k, v in (('x', 'x'), ('y', 'y'), ('timestamp', 't'), ('polarity', 'p'), ('sample_index', 's'))}
    ts, fs = torch.from_numpy(c['ts']).to(DEV), torch.from_numpy(c['fs']).to(DEV)
    losses = L.Losses([(h, w)], 2, DEV)
    runs = []
    for options in (None, {'tiled': 'force'}, {'tiled': 'force'}, {'tiled': True}, {'tiled': False}):
        flow = torch.from_numpy(np.nan_to_num(c['flow'])).to(DEV).requires_grad_(True)
        method = losses.avg_timestamp if options is None else losses.avg_timestamp_tiled
        value, logged = method([flow], ts, fs, events, weight=0.5, polarity=True, **(options or {}))
        value.backward()
        runs.append((value.detach().cpu().numpy().tobytes(), logged.cpu().numpy().tobytes(),
                     flow.grad.cpu().numpy().tobytes()))
        assert flow.grad.abs().max() > 0
    assert all(r == runs[0] for r in runs)
    with pytest.raises(ValueError, match='tiled'):
        losses.avg_timestamp_tiled([flow], ts, fs, events, tiled='always')


def test_event_alignment_with_the_keyword_returns_the_same_bits():
    from dvs_of_training_framework_amd.sequence import FrameSequence
    case = ec.make_eval_case(per_frame=3000)
    x, y, t, p = case['events']
    image_ts = np.append(case['frames'][:, 0], case['frames'][-1, 1])
    seq = FrameSequence([x, y, np.round(t * 65536.0) / 65536.0, p],
                        np.zeros((len(image_ts),) + ec.EVAL_SHAPE, np.uint8), image_ts, device=DEV)
    frames, shape = ec.EVAL_FRAMES, ec.EVAL_BOX[2:]
    flows = torch.from_numpy(np.random.default_rng(3).normal(0, 2.5, (len(frames), 2) + tuple(shape))
                             .astype(F32)).to(DEV)

    class Prescribed:
        def flow_sequence(self, seq, starts, stops, box=None, return_events=False):
            index = {float(f[0]): i for i, f in enumerate(frames)}
            return torch.stack([flows[index[float(s)]] for s in starts]), seq.collate_frames(starts, stops, box)
    for options in ({}, {'references': ('start', 'middle', 'end'), 'polarity': True}):
        plain = testing.event_alignment(Prescribed(), seq, frames, ec.EVAL_BOX, **options)
        tiled = testing.event_alignment(Prescribed(), seq, frames, ec.EVAL_BOX, tiled='force', **options)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(tiled, plain)) and (plain[1]['S'] > 0).all()
