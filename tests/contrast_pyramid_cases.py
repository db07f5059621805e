"""Shared pieces of the tests of the contrast term on every flow scale
(docs/CONTRAST_SPEC.md sections 19-23): cases made of the generators of
tests/contrast_cases.py and tests/contrast_multi_cases.py with one flow per
level, the column transform written out independently of the package, and the
device calls.  Nothing here but ``device_run`` touches the package under test."""
import numpy as np

from tests import contrast_cases as cc, contrast_multi_cases as mc

F32 = np.float32
# frame -> the levels, finest first here (the network's flows come coarsest first; the order is free)
LEVELS = {(24, 40): ((24, 40), (12, 20), (6, 10)),
          (21, 37): ((21, 37), (11, 19), (6, 10), (3, 5))}
MASKS = (1, 5, 7)
OPTIONS = tuple((mask, pol) for mask in MASKS for pol in (False, True))
N_EVENTS = 3000


def shift_of(shape, level_shape):
    """Independent of loss.contrast_level_shift: by halving, rounding up."""
    h, w = shape
    for s in range(16):
        if (h, w) == tuple(level_shape):
            return s
        h, w = (h + 1) // 2, (w + 1) // 2
    raise AssertionError((shape, level_shape))


def level_columns(c, s):
    """x >> s, y >> s for the events inside the full-resolution frame, -1 for the others."""
    h, w = c['shape']
    inside = (c['x'] >= 0) & (c['x'] < w) & (c['y'] >= 0) & (c['y'] < h)
    return np.where(inside, c['x'] >> s, -1), np.where(inside, c['y'] >> s, -1)


def level_case(c, k):
    """Level k of a pyramid case as a case of tests/contrast_multi_cases.py: the
    transformed columns, the level's flow and shape."""
    s = shift_of(c['shape'], c['level_shapes'][k])
    x, y = level_columns(c, s)
    return dict(c, x=x, y=y, flow=c['flows'][k], shape=c['level_shapes'][k])


_cache = {}


def device_case(shape, n_events=N_EVENTS):
    """F = 3 over two samples (frames 0 and 1 share the window edge 0.5),
    n_events events of contrast_cases.device_case at the full shape -- -1 slots,
    x = w, y = -1, foreign samples, times on and next to the window ends -- plus
    events at y = h and at x = -1 alone, a polarity column with zeros, and one
    flow per level with the special values and border flows of that generator."""
    key = (shape, n_events)
    if key not in _cache:
        h, w = shape
        base = cc.device_case(shape, 3, n_events)
        x, y = base['x'].copy(), base['y'].copy()
        k = np.arange(n_events)
        y[k % 47 == 10] = h
        x[k % 53 == 12] = -1
        x[k % 59 == 14], y[k % 59 == 14] = w, h
        shapes = LEVELS[shape]
        flows = [cc.device_case(s, 3, 1, seed=7 + i)['flow'] for i, s in enumerate(shapes)]
        c = mc.with_polarity(dict(base, x=x, y=y))
        for a in (x, y):
            a.setflags(write=False)
        _cache[key] = dict(c, level_shapes=tuple(shapes), flows=flows)
    return _cache[key]


def halvings(shape, levels):
    shapes = [tuple(shape)]
    for _ in range(levels - 1):
        shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2))
    return tuple(shapes)


def make_oracle_case(name, levels=3, max_rounds=64):
    """The random case of that name of contrast_cases.ORACLE_CASES with
    ``levels`` halvings (finest first), a random flow per level (the finest
    keeps the case's) and a polarity column, its times resampled until every
    event that takes part has its float64 xw, yw of EVERY level and reference
    at least KINK from an integer: the float64 definition and the float32
    restatement then take the same floor and the same inside test at every
    level (CONTRAST_SPEC section 15).  -> (case, rounds it took)."""
    base = cc.case(name)
    shapes = halvings(base['shape'], levels)
    F = len(base['fs'])
    rng = np.random.default_rng([23, len(name), levels])
    flows = [base['flow']] + [rng.normal(0, 2.0 / 2 ** s, (F, 2) + shapes[s]).astype(F32) for s in range(1, levels)]
    c = mc.with_polarity(dict(base, t=base['t'].copy()))
    c = dict(c, level_shapes=shapes, flows=flows)
    for rounds in range(max_rounds):
        bad = np.zeros(c['x'].size, bool)
        for k in range(levels):
            lc = level_case(c, k)
            for rho in mc.RHO:
                for p in mc.pairs64(lc, rho):
                    for a in (p['xw'], p['yw']):
                        bad[p['e'][np.abs(a - np.round(a)) < mc.KINK]] = True
        if not bad.any():
            c['t'].setflags(write=False)
            return c, rounds
        c['t'][bad] = rng.random(int(bad.sum())).astype(F32)
    raise AssertionError(f'{name}: still {int(bad.sum())} events on a kink after {max_rounds} rounds')


def oracle_case(name):
    key = ('oracle', name)
    if key not in _cache:
        _cache[key] = make_oracle_case(name)[0]
    return _cache[key]


def host_args(c):
    """The positional arguments of loss.contrast_pyramid_fwd_host / _bwd_host up to the flows."""
    return c['x'], c['y'], c['t'], c['p'], c['s'], c['ts'], c['fs'], c['flows']


def permuted(c, seed=5):
    return dict(mc.permuted(c, seed), level_shapes=c['level_shapes'], flows=c['flows'])


def translating_case(shape=(96, 96), flow=(12.0, -8.0), levels=3):
    """contrast_cases.translating_pattern, its forty points, on a frame four
    times the side with four times the flow: the coarsest of the three levels
    is then the 24 x 24 grid with the flow (3, -2) of the one-level test
    (tests/test_contrast_multi_oracle.py), so every level still resolves the
    motion and the points stay sparse on its grid.  Level shapes finest first."""
    p = mc.with_polarity(cc.translating_pattern(shape=shape, flow=flow))
    return dict(p, level_shapes=halvings(shape, levels))


# ---------------------------------------------------------------------------
# The device
# ---------------------------------------------------------------------------
def layout(F, M, shapes):
    """Element offsets of the workspace of include/dvsof_contrast_pyramid.h, written out again:
    q int64[P] | sums int64[S] | count uint32[P] | pad to 8 | K M records | K F units."""
    pixels = sum(h * w for h, w in shapes)
    P, S, K = M * pixels, 2 * F * pixels, len(shapes)
    rec = (8 * P + 8 * S + 4 * P + 7) // 8 * 8
    return dict(P=P, S=S, sums=8 * P, count=8 * P + 8 * S, rec=rec, unit=rec + 32 * K * M,
                stats=rec + 32 * K * M + 8 * K * F)


def device_run(c, mask, pol, weights, seed=1.0, fills=(0xAA, 0x55)):
    """dvsof_contrast_pyramid_fwd, then dvsof_contrast_pyramid_bwd once per fill
    pattern of the gradient buffers -> dict of numpy: per level q, count, rows,
    rec [M,4], unit [F], grads (one list per fill); terms, value; sums_after_fwd
    and sums (after the last backward)."""
    import torch
    from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    h, w = c['shape']
    shapes, K, F = c['level_shapes'], len(c['level_shapes']), len(c['fs'])
    M = F * len(mc.rhos(mask)) * (2 if pol else 1)
    d = {k: torch.from_numpy(np.array(c[k])).to(dev) for k in ('x', 'y', 't', 'p', 's', 'ts', 'fs')}
    flows = [torch.from_numpy(np.array(f)).to(dev) for f in c['flows']]
    table = L.contrast_level_table((h, w), shapes, F, M, weights, [f.data_ptr() for f in flows])
    lay = layout(F, M, shapes)
    nbytes = lib.dvsof_contrast_pyramid_workspace_bytes(F, mask, int(pol), h, w, table)
    assert nbytes == lay['stats'] + max(lib.dvsof_iwe_stats_workspace_bytes(M, *s) for s in shapes)
    ws = torch.full((nbytes // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=dev)
    rows = torch.full((K * M, 48), 0x5A, dtype=torch.uint8, device=dev)
    terms = torch.full((K,), float('nan'), device=dev)
    value = torch.full((), float('nan'), device=dev)
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [d['x'].numel()] + \
        [d['ts'].data_ptr(), d['fs'].data_ptr(), F, h, w, mask, int(pol)]
    assert lib.dvsof_contrast_pyramid_fwd(*head, table, rows.data_ptr(), terms.data_ptr(), value.data_ptr(),
                                          ws.data_ptr(), nbytes, _lib.stream()) == 0
    after = ws.cpu().numpy().view(np.uint8)
    seed_t = torch.tensor(seed, dtype=torch.float32, device=dev)
    grads = []
    for fill in fills:
        bufs = [torch.full(f.shape, fill, dtype=torch.uint8, device=dev).repeat_interleave(4, -1).view(torch.float32)
                for f in flows]
        for k, b in enumerate(bufs):
            assert b.shape == flows[k].shape and b.is_contiguous()
            table.level[k].grad_flow = b.data_ptr()
        assert lib.dvsof_contrast_pyramid_bwd(*head, table, ws.data_ptr(), nbytes, seed_t.data_ptr(),
                                              _lib.stream()) == 0
        grads.append([b.cpu().numpy() for b in bufs])
    torch.cuda.synchronize()
    final = ws.cpu().numpy().view(np.uint8)
    all_rows = dev_eval.read_iwe_results(rows)
    out = dict(terms=terms.cpu().numpy(), value=value.cpu().numpy(), grads=grads, levels=[],
               sums_after_fwd=after[lay['sums']:lay['count']].view(np.int64),
               sums=final[lay['sums']:lay['count']].view(np.int64))
    pixels = 0
    for k, (hk, wk) in enumerate(shapes):
        n = M * hk * wk
        q = after[8 * M * pixels:8 * M * pixels + 8 * n].view(np.int64).reshape(M, hk, wk)
        cnt = after[lay['count'] + 4 * M * pixels:lay['count'] + 4 * M * pixels + 4 * n].view(np.uint32)
        rec = after[lay['rec'] + 32 * k * M:lay['rec'] + 32 * (k + 1) * M].view(np.float64).reshape(M, 4)
        unit = after[lay['unit'] + 8 * k * F:lay['unit'] + 8 * (k + 1) * F].view(np.float64)
        out['levels'].append(dict(q=q, count=cnt.reshape(M, hk, wk), rows=all_rows[k * M:(k + 1) * M], rec=rec,
                                  unit=unit))
        pixels += hk * wk
    return out


def multi_device_run(c, mask, pol, weight, seed=1.0):
    """dvsof_contrast_multi_fwd / _bwd on a case of tests/contrast_multi_cases.py -> dict of numpy."""
    import torch
    from dvs_of_training_framework_amd import _lib
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    h, w = c['shape']
    F = len(c['fs'])
    M = F * len(mc.rhos(mask)) * (2 if pol else 1)
    d = {k: torch.from_numpy(np.array(c[k])).to(dev) for k in mc.KEYS}
    q = torch.empty((M, h, w), dtype=torch.long, device=dev)
    count = torch.empty((M, h, w), dtype=torch.int32, device=dev)
    rows = torch.empty((M, 48), dtype=torch.uint8, device=dev)
    term = torch.full((), float('nan'), device=dev)
    nbytes = lib.dvsof_contrast_multi_workspace_bytes(F, mask, int(pol), h, w)
    ws = torch.empty((nbytes // 8,), dtype=torch.long, device=dev)
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [d['x'].numel()] + \
        [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, h, w, mask, int(pol)]
    assert lib.dvsof_contrast_multi_fwd(*head, q.data_ptr(), count.data_ptr(), rows.data_ptr(), term.data_ptr(),
                                        ws.data_ptr(), nbytes, _lib.stream()) == 0
    grad = torch.empty((F, 2, h, w), device=dev)
    seed_t = torch.tensor(seed, dtype=torch.float32, device=dev)
    assert lib.dvsof_contrast_multi_bwd(*head, q.data_ptr(), ws.data_ptr(), nbytes, seed_t.data_ptr(), float(weight),
                                        grad.data_ptr(), _lib.stream()) == 0
    torch.cuda.synchronize()
    return dict(q=q.cpu().numpy(), count=count.cpu().numpy().view(np.uint32), rows=rows.cpu().numpy(),
                term=term.cpu().numpy(), grad=grad.cpu().numpy())
