"""The tiled schedule of the forward splat of the two events-only terms on every
flow scale (csrc/tiled_splat.hip, include/dvsof_event_pyramids_tiled.h) against
the numpy restatements the per-event kernels are pinned to
(loss.contrast_pyramid_fwd_host, loss.avg_timestamp_pyramid_fwd_host), byte for
byte, at mode 1 and from buffers of 0x5A, with the per-event twin called on the
same inputs beside them: tile seams of two levels at once, level tables without
a shift-0 level and out of order, a tile summed in several slices with a bucket
past its capacity, a refused plan and empty calls, and the keyword through the
public interface.  Tile size, slices and capacities are read from
dvsof_event_pyramids_tiled_plan."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L
from tests import contrast_multi_cases as cm
from tests.test_gpu_avg_timestamp_tiled import term as avg_one_level
from tests.test_gpu_event_images_tiled import plan as one_level_plan, term as contrast_one_level

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32 = np.float32
FILL = 0x5A5A5A5A5A5A5A5A
OPTIONS = [(1, False), (1, True), (7, False), (7, True)]
FAMILIES = {'contrast': (L.contrast_pyramid_fwd_host, ('q', 'count'), contrast_one_level),
            'avg_timestamp': (L.avg_timestamp_pyramid_fwd_host, ('q', 's', 'base', 'count'), avg_one_level)}
TW, TH = 64, 16


def level_shapes(shape, shifts):
    return tuple((-(-shape[0] // 2 ** s), -(-shape[1] // 2 ** s)) for s in shifts)


def table_of(c, F, M, flows=None):
    K = len(c['level_shapes'])
    return L.contrast_level_table(c['shape'], c['level_shapes'], F, M, [F32(0.25) / F32(K)] * K, flows)


def plan(c, mask, pol, n):
    """-> (the six constants, [(tiles_k, cap_k, slices_k)]), or None where the plan is refused."""
    F, K = len(c['fs']), len(c['level_shapes'])
    out = (ctypes.c_int32 * (6 + 3 * K))()
    table = table_of(c, F, F * len(cm.rhos(mask)) * (2 if pol else 1))
    if not _lib.lib().dvsof_event_pyramids_tiled_plan(F, mask, int(pol), *c['shape'], table, n, out):
        return None
    return tuple(out[:6]), [tuple(out[6 + 3 * k:9 + 3 * k]) for k in range(K)]


def run(family, c, mask, pol, mode=1, encoded=False):
    """The forward (mode None: the per-event twin) and the twin's backward -> dict: rc, the
    workspace after the forward as bytes, per level the images, rows (contrast), terms, value,
    grads."""
    lib = _lib.lib()
    h, w = c['shape']
    shapes, F, n = c['level_shapes'], len(c['fs']), c['x'].size
    M = F * len(cm.rhos(mask)) * (2 if pol else 1)
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in ('x', 'y', 't', 'p', 's', 'ts', 'fs')}
    flows = [torch.from_numpy(np.array(f)).to(DEV) for f in c['flows']]
    table = table_of(c, F, M, [f.data_ptr() for f in flows])
    if encoded:     # the events are in sample order
        off = torch.from_numpy(np.searchsorted(c['s'], np.arange(int(c['s'].max()) + 2))).to(DEV)
        cols = [d['x'].short(), d['y'].short(), d['t'], (d['p'] > 0).to(torch.uint8), off]
        head, form = [k.data_ptr() for k in cols] + [off.numel() - 1, n], '_encoded'
    else:
        head, form = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n], ''
    head += [d['ts'].data_ptr(), d['fs'].data_ptr(), F, h, w, mask, int(pol)]
    name = f'dvsof_{family}_pyramid'
    nbytes = getattr(lib, name + '_workspace_bytes')(F, mask, int(pol), h, w, table)
    ws = torch.full((nbytes // 8,), FILL, dtype=torch.long, device=DEV)
    rows = torch.full((len(shapes) * M, 48), 0x5A, dtype=torch.uint8, device=DEV)
    out = torch.full((len(shapes) + 1,), float('nan'), device=DEV)
    tail = [table] + ([rows.data_ptr()] if family == 'contrast' else []) + \
        [out.data_ptr(), out[-1:].data_ptr(), ws.data_ptr(), nbytes, _lib.stream()]
    if mode is not None:
        tiles, tile_bytes = dev_eval.event_pyramids_tiled_workspace(family, F, mask, pol, h, w, table, n, DEV)
        if tiles is not None:
            tiles.fill_(FILL)
        tail += [_lib.ptr(tiles), tile_bytes, mode]
    rc = getattr(lib, name + '_fwd' + form + ('' if mode is None else '_tiled'))(*head, *tail)
    after = ws.cpu().numpy().view(np.uint8)
    got = dict(rc=rc, ws=after.tobytes(), rows=rows.cpu().numpy().tobytes(), out=out.cpu().numpy(), levels=[])
    if rc != 0:
        return got
    grads = [torch.full(f.shape, float('nan'), device=DEV) for f in flows]
    for k, g in enumerate(grads):
        table.level[k].grad_flow = g.data_ptr()
    seed = torch.ones((), device=DEV)
    assert getattr(lib, name + '_bwd' + form)(*head, table, ws.data_ptr(), nbytes, seed.data_ptr(), _lib.stream()) == 0
    got['grads'] = [g.cpu().numpy() for g in grads]
    P = M * sum(hk * wk for hk, wk in shapes)
    lay = L.avg_timestamp_pyramid_layout(F, M, shapes) if family == 'avg_timestamp' else \
        dict(q=0, count=8 * P + 16 * F * (P // M))
    pixels = 0
    for hk, wk in shapes:
        lev, e = {}, M * hk * wk
        for key in FAMILIES[family][1]:
            size, dtype = (4, np.uint32) if key == 'count' else (8, np.int64)
            at = lay[key] + size * M * pixels
            lev[key] = after[at:at + size * e].view(dtype).reshape(M, hk, wk)
        got['levels'].append(lev)
        pixels += hk * wk
    return got


@functools.lru_cache(maxsize=None)
def restatement(family, name, mask, pol):
    c = CASES[name]()
    return FAMILIES[family][0](c['x'], c['y'], c['t'], c['p'], c['s'], c['ts'], c['fs'], c['flows'], c['shape'],
                               [F32(0.25) / F32(len(c['flows']))] * len(c['flows']), mask, pol)


def same_as_restatement(family, got, want):
    assert got['rc'] == 0
    for k, (dev, host) in enumerate(zip(got['levels'], want['levels'])):
        for key in FAMILIES[family][1]:
            assert np.array_equal(dev[key], host[key]), (k, key)
    assert got['out'][:-1].tobytes() == want['terms'].tobytes() and got['out'][-1:].tobytes() == want['value'].tobytes()


def same_as_twin(got, twin):
    assert got['rc'] == twin['rc'] and got['ws'] == twin['ws'], 'a region of the workspace differs from the twin\'s'
    assert got['rows'] == twin['rows'] and got['out'].tobytes() == twin['out'].tobytes()
    for a, b in zip(got.get('grads', ()), twin.get('grads', ())):
        assert a.tobytes() == b.tobytes() and not np.isnan(a).any()


@functools.lru_cache(maxsize=None)
def seam_case(shifts=(0, 1, 2, 3)):
    """Three frames of (2 TH + 7) x (2 TW + 7), every halving rounds up: eight events on every
    crossing of the first and last column and row of every level-0 and every level-1 tile (level
    1 is 68 wide: a ragged tile of four pixels), 300 anywhere, flows of up to three pixels with
    one NaN under an event; two windows of sample 0 overlap, the last 20 events are of no frame."""
    h, w = 2 * TH + 7, 2 * TW + 7
    rng = np.random.default_rng(17)
    xs = sorted({0, TW - 1, TW, 2 * TW - 1, 2 * TW, w - 1, 2 * (TW - 1), 2 * TW, 2 * ((w + 1) // 2 - 1)})
    ys = sorted({0, TH - 1, TH, 2 * TH - 1, 2 * TH, h - 1, 2 * (TH - 1), 2 * TH, 2 * ((h + 1) // 2 - 1)})
    x = np.concatenate([np.repeat(np.tile(xs, len(ys)), 8), rng.integers(0, w, 300)]).astype(np.int64)
    y = np.concatenate([np.repeat(np.repeat(ys, len(xs)), 8), rng.integers(0, h, 300)]).astype(np.int64)
    order = rng.permutation(x.size)
    x, y, n = x[order], y[order], x.size
    shapes = level_shapes((h, w), shifts)
    flows = [rng.uniform(-3, 3, (3, 2) + s).astype(F32) for s in shapes]
    flows[0][0, 0, y[7] >> shifts[0], x[7] >> shifts[0]] = np.nan
    s = np.where(np.arange(n) >= n - 20, 2, np.arange(n) >= n // 2).astype(np.int64)
    return dict(x=x, y=y, t=rng.random(n).astype(F32) * F32(1.5), p=rng.choice(np.array([-1, 1], np.int64), n), s=s,
                shape=(h, w), level_shapes=shapes, flows=flows, ts=np.array([0, 1, 0.5, 1.5, 0, 1.5], F32),
                fs=np.array([0, 0, 1], np.int64))


@functools.lru_cache(maxsize=None)
def sink_case():
    """cm.sink_case on one 64 x 64 frame, every event ON, a sink flow on every level."""
    c = cm.sink_case(shape=(64, 64), n=20000)
    shapes = level_shapes((64, 64), (0, 1, 2, 3))
    return dict(c, p=np.ones_like(c['p']), level_shapes=shapes,
                flows=[cm.sink_case(shape=s, n=1)['flow'] for s in shapes])


CASES = {'seams': seam_case, 'no_shift_0': lambda: seam_case((1, 3)), 'unordered': lambda: seam_case((2, 0, 0)),
         'sink': sink_case}


@pytest.mark.parametrize('encoded', [False, True], ids=['wire', 'encoded'])
@pytest.mark.parametrize('mask,pol', OPTIONS)
@pytest.mark.parametrize('family', list(FAMILIES))
def test_seams_on_two_levels_at_once(family, mask, pol, encoded):
    c = seam_case()
    assert one_level_plan(1, 1, 0, 64, 64, 0)[:2] == (TW, TH) and c['level_shapes'][1] == (TH + 4, TW + 4)
    in_two = (c['s'] == 0) & (c['t'] >= 0.5) & (c['t'] <= 1)
    assert in_two.sum() > 50 and (c['s'] == 2).sum() == 20      # lanes diverge inside the agreement
    (tw, th, tiles, _, aggregate, source), levels = plan(c, mask, pol, c['x'].size)
    M = 3 * len(cm.rhos(mask)) * (2 if pol else 1)
    assert [k[0] for k in levels] == [9 * M, 4 * M, M, M] and tiles == 15 * M and source == 0 and aggregate == 4
    got, twin = run(family, c, mask, pol, 1, encoded), run(family, c, mask, pol, None, encoded)
    same_as_restatement(family, got, restatement(family, 'seams', mask, pol))
    same_as_twin(got, twin)
    assert all(np.abs(g).max() > 0 for g in got['grads'])


@pytest.mark.parametrize('name', ['no_shift_0', 'unordered'])
@pytest.mark.parametrize('family', list(FAMILIES))
def test_level_tables_without_a_shift_0_level_and_out_of_order(family, name):
    c = CASES[name]()
    assert plan(c, 7, True, c['x'].size)[0][5] == (0 if name == 'no_shift_0' else 1)    # the first smallest shift
    got = run(family, c, 7, True)
    same_as_restatement(family, got, restatement(family, name, 7, True))
    same_as_twin(got, run(family, c, 7, True, None))


@pytest.mark.parametrize('family', list(FAMILIES))
def test_one_level_at_shift_0_gives_the_bytes_of_the_one_level_tiled_call(family):
    full = seam_case()
    c = dict(full, level_shapes=full['level_shapes'][:1], flows=full['flows'][:1])
    got, one = run(family, c, 7, True), FAMILIES[family][2](dict(c, flow=c['flows'][0]), 7, True, True)
    for key in FAMILIES[family][1]:
        assert np.array_equal(got['levels'][0][key], one[key]) and one[key].any(), key


@pytest.mark.parametrize('family', list(FAMILIES))
def test_a_tile_in_slices_and_a_bucket_past_its_capacity_lose_nothing(family):
    c = sink_case()
    (tw, th, _, kslice, _, _), levels = plan(c, 1, True, 20000)
    assert levels[3][2] >= 2 and levels[3][1] > kslice, levels        # the coarsest level: one tile an image
    # the records of the centre's tile of level 0, from the float64 warp: far more than a bucket holds
    t = c['t'].astype(np.float64)
    yw = c['y'] - t * (c['y'] - 32)
    per_tile = np.bincount((np.floor(yw) // th).astype(np.int64), minlength=4)
    assert per_tile.max() > 1.25 * levels[0][1], (per_tile, levels)
    got = run(family, c, 1, True)
    same_as_restatement(family, got, restatement(family, 'sink', 1, True))
    assert all(lev['q'].any() for lev in got['levels'])


@pytest.mark.parametrize('family', list(FAMILIES))
def test_a_refused_plan_and_empty_calls_are_the_twins(family):
    F, n = 700, 1400                    # 4200 tiles at either level of 2 x 2 and 1 x 1 pixels at six images a frame
    rng = np.random.default_rng(5)
    shapes = ((2, 2), (1, 1))
    c = dict(x=rng.integers(0, 2, n), y=rng.integers(0, 2, n), t=rng.random(n).astype(F32),
             p=rng.choice(np.array([-1, 1], np.int64), n), s=np.arange(n, dtype=np.int64) // 2,
             ts=np.tile(np.array([0, 1], F32), F), fs=np.arange(F, dtype=np.int64), shape=(2, 2), level_shapes=shapes,
             flows=[rng.uniform(-1, 1, (F, 2) + s).astype(F32) for s in shapes])
    assert plan(c, 7, True, n) is None and plan(dict(c, level_shapes=shapes[:1]), 7, True, n) is not None
    table = table_of(c, F, 6 * F)
    assert getattr(_lib.lib(), f'dvsof_{family}_pyramid_tiled_workspace_bytes')(F, 7, 1, 2, 2, table, n) == 0
    got = run(family, c, 7, True)
    same_as_twin(got, run(family, c, 7, True, None))
    assert got['rc'] == 0 and got['levels'][1]['q'].any()
    seams = seam_case()
    none = dict(seams, **{k: seams[k][:0] for k in ('x', 'y', 't', 'p', 's')})
    for c in (none, dict(seams, s=np.full_like(seams['s'], 2))):        # no events; events of no frame
        got = run(family, c, 7, True)
        same_as_twin(got, run(family, c, 7, True, None))
        assert got['rc'] == 0 and not any(lev['count'].any() for lev in got['levels'])
    assert run(family, seams, 7, True, mode=2)['rc'] != 0               # no such mode


def test_the_losses_with_the_keyword_return_the_same_bits():
    c = seam_case()
    events = {k: torch.from_numpy(np.array(c[v])).to(DEV)
              for k, v in (('x', 'x'), ('y', 'y'), ('timestamp', 't'), ('polarity', 'p'), ('sample_index', 's'))}
    ts, fs = torch.from_numpy(c['ts']).to(DEV), torch.from_numpy(c['fs']).to(DEV)
    losses = L.Losses(c['level_shapes'][::-1], 3, DEV)
    for plain, method in ((losses.contrast,) * 2, (losses.avg_timestamp_scales, losses.avg_timestamp_scales_tiled)):
        runs = []
        for options in (None, {'tiled': 'force'}, {'tiled': 'force'}, {'tiled': True}):
            flows = [torch.from_numpy(np.nan_to_num(f)).to(DEV).requires_grad_(True) for f in c['flows'][::-1]]
            value, logged = (plain if options is None else method)(
                flows, ts, fs, events, weight=0.5, references=('start', 'end'), polarity=True, scales='all',
                **(options or {}))
            value.backward()
            assert all(f.grad.abs().max() > 0 for f in flows)
            runs.append((value.detach().cpu().numpy().tobytes(), logged.cpu().numpy().tobytes()) +
                        tuple(f.grad.cpu().numpy().tobytes() for f in flows))
        assert runs[0] == runs[1] == runs[2] == runs[3]
        with pytest.raises(ValueError, match='tiled'):
            method(flows, ts, fs, events, scales='all', tiled='always')
