"""Shared pieces of the tests of the events-only terms on the encoded event
columns (include/dvsof_event_terms_encoded.h): the transform of a case of
tests/contrast_multi_cases.py into one the encoded columns can express, the
decoding written out independently of the package, and one device runner for
the eight entry points and their wire twins.  Nothing here but ``run`` touches
the package under test."""
import numpy as np

from tests import avg_timestamp_pyramid_cases as apc, contrast_multi_cases as mc, contrast_pyramid_cases as cpc

EVENT_KEYS = ('x', 'y', 't', 'p', 's')
FILLS = {'wire': 0xAA, 'encoded': 0x55}     # what each form's buffers and workspace hold before the calls


def decode(compact, n_samples):
    """The wire columns of compact columns, by the definition of the header:
    x, y widened, p = polarity ? +1 : -1, the sample of event i the largest b
    in [0, B) with offsets[b] <= i (a plain loop, no search)."""
    off = np.asarray(compact['sample_event_offsets'], np.int64)
    assert off.shape == (n_samples + 1,)
    n = compact['x'].size
    s = np.zeros(n, np.int64)
    for b in range(n_samples):
        s[off[b]:] = b          # later samples overwrite: the largest b wins; repeated offsets are empty samples
    return dict(x=compact['x'].astype(np.int64), y=compact['y'].astype(np.int64), t=compact['timestamp'].copy(),
                p=np.where(compact['polarity'], 1, -1).astype(np.int64), s=s)


def encodable(c):
    """A case of tests/contrast_multi_cases.py -> (compact columns, the case on
    their decoding, B).  Deterministic: with B = max(frame_sample) + 1 an event
    whose sample is outside [0, B) becomes a -1 slot of sample 0, an event with
    p == 0 a -1 slot with p = -1; then a stable sort by sample."""
    B = int(np.max(c['fs'])) + 1
    x, y, t, p, s = (np.array(c[k]) for k in EVENT_KEYS)
    foreign = (s < 0) | (s >= B)
    x[foreign], y[foreign], s[foreign] = -1, -1, 0
    zero = p == 0
    x[zero], y[zero], p[zero] = -1, -1, -1
    order = np.argsort(s, kind='stable')
    x, y, t, p, s = (a[order] for a in (x, y, t, p, s))
    for a in (x, y):
        assert a.size == 0 or (a.min() >= -2 ** 15 and a.max() < 2 ** 15), 'the coordinates fit int16'
    compact = {'x': x.astype(np.int16), 'y': y.astype(np.int16), 'timestamp': t.astype(np.float32),
               'polarity': p > 0, 'sample_event_offsets': np.searchsorted(s, np.arange(B + 1)).astype(np.int64)}
    d = decode(compact, B)
    assert all(np.array_equal(d[k], a) for k, a in zip(EVENT_KEYS, (x, y, t, p, s)))
    for a in list(compact.values()) + list(d.values()):
        a.setflags(write=False)
    return compact, dict(c, **d), B


def census(c, decoded):
    """-> (share of -1 slots, share of events inside the frame; their samples are valid by construction)."""
    h, w = c['shape']
    x, y = decoded['x'], decoded['y']
    n = max(x.size, 1)
    return float(((x == -1) & (y == -1)).sum()) / n, float(((x >= 0) & (x < w) & (y >= 0) & (y < h)).sum()) / n


def permuted_within_samples(compact, seed=5):
    """The events of every sample in another order; the offsets stay."""
    off = compact['sample_event_offsets']
    rng = np.random.default_rng(seed)
    idx = np.concatenate([off[b] + rng.permutation(int(off[b + 1] - off[b])) for b in range(off.size - 1)]
                         + [np.arange(off[-1], compact['x'].size)]).astype(np.int64)
    return dict({k: compact[k][idx] for k in ('x', 'y', 'timestamp', 'polarity')}, sample_event_offsets=off)


def padded(compact, length, seed=3):
    """A tail of ``length`` slots past sample_event_offsets[B]: x = y = -1, NaN
    and huge timestamps, both polarity bytes."""
    rng = np.random.default_rng([seed, length])
    t = rng.choice(np.array([np.nan, 3e38, -3e38, 0.5, np.inf], np.float32), length)
    pol = np.arange(length) % 2 == 0
    tail = {'x': np.full(length, -1, np.int16), 'y': np.full(length, -1, np.int16), 'timestamp': t, 'polarity': pol}
    return dict({k: np.concatenate([compact[k], tail[k]]) for k in tail},
                sample_event_offsets=compact['sample_event_offsets'])


# ---------------------------------------------------------------------------
# The documented regions of the workspaces, as (first byte, one past the last)
# ---------------------------------------------------------------------------
def regions(kind, pyramid, F, M, shapes):
    """What the headers document of a workspace, by name.  The padding to 8
    bytes and the partials of the reductions (whose rows past the last level's
    are not written) stay out."""
    K = len(shapes)
    if kind == 'contrast' and not pyramid:
        (h, w), = shapes
        S = 16 * F * h * w
        return {'sums': (0, S), 'rec': (S, S + 32 * M), 'unit': (S + 32 * M, S + 32 * M + 8 * F)}
    if kind == 'contrast':
        lay = cpc.layout(F, M, shapes)
        return {'q': (0, lay['sums']), 'sums': (lay['sums'], lay['count']),
                'count': (lay['count'], lay['count'] + 4 * lay['P']), 'rec': (lay['rec'], lay['unit']),
                'unit': (lay['unit'], lay['stats'])}
    lay = apc.layout(F, M, shapes)
    assert lay['part'] - lay['rows'] == 32 * K * M
    return {'q': (0, lay['s']), 's': (lay['s'], lay['base']), 'base': (lay['base'], lay['sums']),
            'sums': (lay['sums'], lay['count']), 'count': (lay['count'], lay['count'] + 4 * lay['P']),
            'rec': (lay['rec'], lay['unit']), 'unit': (lay['unit'], lay['rows']), 'rows': (lay['rows'], lay['part'])}


# ---------------------------------------------------------------------------
# The device
# ---------------------------------------------------------------------------
def columns(form, compact, decoded, dev, null=False):
    """-> (the leading arguments of an entry point of that form, up to and
    including n_events; the tensors they point into)."""
    import torch
    if form == 'wire':
        held = [torch.from_numpy(np.array(decoded[k])).to(dev) for k in EVENT_KEYS]
        ptrs = [None if null else t.data_ptr() for t in held]
        return ptrs + [held[0].numel()], held
    held = [torch.from_numpy(np.array(compact[k])).to(dev) for k in ('x', 'y', 'timestamp')]
    held.append(torch.from_numpy(np.array(compact['polarity']).astype(np.uint8)).to(dev))
    held.append(torch.from_numpy(np.array(compact['sample_event_offsets'])).to(dev))
    assert held[0].dtype == torch.short and held[3].dtype == torch.uint8 and held[4].dtype == torch.long
    ptrs = [None if null else t.data_ptr() for t in held]
    return ptrs + [held[4].numel() - 1, held[0].numel()], held


def _filled(shape, dtype, fill, dev):
    import torch
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.reshape(-1).view(torch.uint8).fill_(fill)     # (reshape: a 0-dim tensor has no byte view)
    return t


def run(kind, pyramid, form, compact, c, mask, pol, weights=None, seed=1.0, weight=0.75, null=False, head=None):
    """One of the four pairs of calls (kind 'contrast' or 'avg_timestamp', one
    level or the pyramid) in one column form, forward then backward, into
    buffers and a workspace filled with FILLS[form] -> dict of numpy: the
    outputs, the documented regions of the workspace after the forward
    ('fwd:<name>') and after the backward ('bwd:<name>').  c: the case on the
    decoded columns (with 'flows' and 'level_shapes' for a pyramid).  head: the
    leading arguments, if not those of ``columns``."""
    import torch
    from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    fill = FILLS[form]
    suffix = '' if form == 'wire' else '_encoded'
    name = {('contrast', False): 'dvsof_contrast_multi', ('contrast', True): 'dvsof_contrast_pyramid',
            ('avg_timestamp', False): 'dvsof_avg_timestamp', ('avg_timestamp', True): 'dvsof_avg_timestamp_pyramid'}[
                (kind, pyramid)]
    fwd, bwd = getattr(lib, f'{name}_fwd{suffix}'), getattr(lib, f'{name}_bwd{suffix}')
    h, w = c['shape']
    F = len(c['fs'])
    M = F * len(mc.rhos(mask)) * (2 if pol else 1)
    if head is None:
        head, held = columns(form, compact, c, dev, null)
    ts, fs = (torch.from_numpy(np.array(c[k])).to(dev) for k in ('ts', 'fs'))
    seed_t = torch.tensor(seed, dtype=torch.float32, device=dev)
    out = {}
    if pyramid:
        shapes = tuple(c['level_shapes'])
        weights = [0.25] * len(shapes) if weights is None else weights
        flows = [torch.from_numpy(np.array(f)).to(dev) for f in c['flows']]
        grads = [_filled(f.shape, torch.float32, fill, dev) for f in flows]
        table = L.contrast_level_table((h, w), shapes, F, M, weights, [f.data_ptr() for f in flows],
                                       [g.data_ptr() for g in grads])
        nbytes = getattr(lib, f'{name}_workspace_bytes')(F, mask, int(pol), h, w, table)
        mid = [ts.data_ptr(), fs.data_ptr(), F, h, w, mask, int(pol), table]
        terms, value = _filled((len(shapes),), torch.float32, fill, dev), _filled((), torch.float32, fill, dev)
        outs = [terms.data_ptr(), value.data_ptr()]
        back = []
    else:
        shapes = ((h, w),)
        flow = torch.from_numpy(np.array(c['flow'])).to(dev)
        grads = [_filled(flow.shape, torch.float32, fill, dev)]
        nbytes = getattr(lib, f'{name}_workspace_bytes')(F, mask, int(pol), h, w)
        mid = [ts.data_ptr(), fs.data_ptr(), flow.data_ptr(), F, h, w, mask, int(pol)]
        term = _filled((), torch.float32, fill, dev)
        outs = [term.data_ptr()]
        back = [float(weight), grads[0].data_ptr()]
    ws = _filled((nbytes // 8,), torch.long, fill, dev)
    rows = q = count = None
    q_arg = []
    if kind == 'contrast':
        rows = _filled((len(shapes) * M, 48), torch.uint8, fill, dev)
        outs = [rows.data_ptr()] + outs
        if not pyramid:     # the one-level contrast calls have q and count as arguments, not in the workspace
            q, count = _filled((M, h, w), torch.long, fill, dev), _filled((M, h, w), torch.int32, fill, dev)
            outs = [q.data_ptr(), count.data_ptr()] + outs
            q_arg = [q.data_ptr()]
    out['rc_fwd'] = fwd(*head, *mid, *outs, ws.data_ptr(), nbytes, _lib.stream())
    after = ws.cpu().numpy().view(np.uint8)
    out['rc_bwd'] = bwd(*head, *mid, *q_arg, ws.data_ptr(), nbytes, seed_t.data_ptr(), *back, _lib.stream())
    torch.cuda.synchronize()
    final = ws.cpu().numpy().view(np.uint8)
    for label, a in (('fwd', after), ('bwd', final)):
        for region, (lo, hi) in regions(kind, pyramid, F, M, shapes).items():
            out[f'{label}:{region}'] = a[lo:hi].copy()
    out['grads'] = [g.cpu().numpy().view(np.uint32) for g in grads]
    if pyramid:
        out['terms'], out['value'] = terms.cpu().numpy().view(np.uint32), value.cpu().numpy().view(np.uint32)
    else:
        out['term'] = term.cpu().numpy().view(np.uint32)
    if rows is not None:
        out['rows_raw'] = rows.cpu().numpy()
        if out['rc_fwd'] == 0 and F > 0:
            out['rows'] = dev_eval.read_iwe_results(rows)
    if q is not None:
        out['q'], out['count'] = q.cpu().numpy(), count.cpu().numpy()
    return out


def same(a, b, skip=('rows_raw',)):
    """The names under which two results of ``run`` differ (floats are compared as their bits)."""
    bad = []
    for k in a:
        if k in skip:
            continue
        if k == 'grads':
            bad += [f'grads[{i}]' for i, (u, v) in enumerate(zip(a[k], b[k])) if not np.array_equal(u, v)]
        elif k == 'rows':
            bad += [f'rows.{n}' for n in a[k].dtype.names if not np.array_equal(a[k][n], b[k][n], equal_nan=True)]
        elif not np.array_equal(a[k], b[k]):
            bad.append(k)
    return bad


def untouched(result, form):
    """Every buffer and the whole of the regions still hold the fill: nothing was launched."""
    fill = FILLS[form]
    names = [k for k, v in result.items() if k not in ('rc_fwd', 'rc_bwd', 'grads', 'rows')
             and not (np.atleast_1d(np.asarray(v)).view(np.uint8) == fill).all()]
    names += [f'grads[{i}]' for i, g in enumerate(result['grads']) if not (g.view(np.uint8) == fill).all()]
    return names
