"""Shared pieces of the tests of the average-timestamp term on every flow scale
(docs/AVG_TIMESTAMP_SPEC.md sections 11-15): the cases are those of
tests/contrast_pyramid_cases.py (imported, not edited), the workspace layout
written out again, and the device calls.  Nothing here but the two
``*_device_run`` touches the package under test."""
import numpy as np

from tests import contrast_multi_cases as mc, contrast_pyramid_cases as pc

F32 = np.float32
SHAPES = ((24, 40), (21, 37))
REC_NAMES = ('S', 'S0', 'n', 'n0', 'peak', 'value', 'k2', 'gmax')
REC_DTYPE = np.dtype([(k, '<f8') for k in REC_NAMES])
ROW_DTYPE = np.dtype([('S', '<f8'), ('S0', '<f8'), ('peak', '<f8'), ('n', '<u4'), ('n0', '<u4')])


def partial_blocks(n):
    """min(max(ceil(n / 1024), 1), 128): the blocks per image of the fixed-order reduction."""
    return min(max(-(-n // 1024), 1), 128)


def layout(F, M, shapes):
    """Byte offsets of the workspace of include/dvsof_avg_timestamp_pyramid.h, written out again:
    q | s | base int64[P] | sums int64[S] | count uint32[P] | pad to 8 | K M records of 64 |
    K F units | K M rows of 32 | M nb rows of 32, nb the largest level's."""
    pixels = sum(h * w for h, w in shapes)
    P, S, K = M * pixels, 2 * F * pixels, len(shapes)
    rec = (24 * P + 8 * S + 4 * P + 7) // 8 * 8
    unit = rec + 64 * K * M
    rows = unit + 8 * K * F
    part = rows + 32 * K * M
    nb = max(partial_blocks(h * w) for h, w in shapes)
    return dict(P=P, S=S, s=8 * P, base=16 * P, sums=24 * P, count=24 * P + 8 * S, rec=rec, unit=unit, rows=rows,
                part=part, bytes=part + 32 * M * nb)


def images_of(c, mask, pol):
    return len(c['fs']) * len(mc.rhos(mask)) * (2 if pol else 1)


def device_run(c, mask, pol, weights, seed=1.0, fills=(0xAA, 0x55), guard=64):
    """dvsof_avg_timestamp_pyramid_fwd, then dvsof_avg_timestamp_pyramid_bwd once
    per fill pattern of the gradient buffers -> dict of numpy: per level q, s,
    base, count [M,h_k,w_k], rows, rec [M], unit [F]; grads (one list per fill);
    terms, value; sums_after_fwd and sums (after the last backward).  Behind the
    workspace, the terms and every gradient buffer stands a guard region, which
    must come back untouched; the backward may write the sums alone."""
    import torch
    from dvs_of_training_framework_amd import _lib, loss as L
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    h, w = c['shape']
    shapes, K, F = c['level_shapes'], len(c['level_shapes']), len(c['fs'])
    M = images_of(c, mask, pol)
    d = {k: torch.from_numpy(np.array(c[k])).to(dev) for k in ('x', 'y', 't', 'p', 's', 'ts', 'fs')}
    flows = [torch.from_numpy(np.array(f)).to(dev) for f in c['flows']]
    table = L.contrast_level_table((h, w), shapes, F, M, weights, [f.data_ptr() for f in flows])
    lay = layout(F, M, shapes)
    nbytes = lib.dvsof_avg_timestamp_pyramid_workspace_bytes(F, mask, int(pol), h, w, table)
    assert nbytes == lay['bytes'] and nbytes % 8 == 0, (nbytes, lay['bytes'])
    ws = torch.full((nbytes // 8 + guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=dev)
    out_buf = torch.full((K + 1 + guard,), float('nan'), device=dev)     # terms [K], value, guard
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [d['x'].numel()] + \
        [d['ts'].data_ptr(), d['fs'].data_ptr(), F, h, w, mask, int(pol)]
    assert lib.dvsof_avg_timestamp_pyramid_fwd(*head, table, out_buf.data_ptr(), out_buf[K:].data_ptr(),
                                               ws.data_ptr(), nbytes, _lib.stream()) == 0
    after = ws.cpu().numpy().view(np.uint8)
    seed_t = torch.tensor(seed, dtype=torch.float32, device=dev)
    grads = []
    for fill in fills:
        bufs = [torch.full((f.numel() + guard, 4), fill, dtype=torch.uint8, device=dev).view(torch.float32).reshape(-1)
                for f in flows]
        for k, b in enumerate(bufs):
            table.level[k].grad_flow = b.data_ptr()
        assert lib.dvsof_avg_timestamp_pyramid_bwd(*head, table, ws.data_ptr(), nbytes, seed_t.data_ptr(),
                                                   _lib.stream()) == 0
        got = [b.cpu().numpy() for b in bufs]
        for g, f in zip(got, flows):
            assert (g[f.numel():].view(np.uint8) == fill).all(), 'the guard behind a gradient buffer was written'
        grads.append([g[:f.numel()].reshape(tuple(f.shape)) for g, f in zip(got, flows)])
    torch.cuda.synchronize()
    final = ws.cpu().numpy().view(np.uint8)
    for buf in (after, final):
        assert (buf[nbytes:] == 0x5A).all(), 'the guard behind the workspace was written'
    assert final[:lay['sums']].tobytes() == after[:lay['sums']].tobytes()
    assert final[lay['count']:].tobytes() == after[lay['count']:].tobytes()
    host = out_buf.cpu().numpy()
    assert np.isnan(host[K + 1:]).all(), 'the guard behind the value was written'
    out = dict(terms=host[:K].copy(), value=host[K:K + 1].copy().reshape(()), grads=grads, levels=[],
               sums_after_fwd=after[lay['sums']:lay['count']].view(np.int64),
               sums=final[lay['sums']:lay['count']].view(np.int64))
    pixels = 0
    for k, (hk, wk) in enumerate(shapes):
        n = M * hk * wk
        lev = {}
        for name in ('q', 's', 'base'):
            at = {'q': 0, 's': lay['s'], 'base': lay['base']}[name] + 8 * M * pixels
            lev[name] = after[at:at + 8 * n].view(np.int64).reshape(M, hk, wk)
        at = lay['count'] + 4 * M * pixels
        lev['count'] = after[at:at + 4 * n].view(np.uint32).reshape(M, hk, wk)
        lev['rec'] = after[lay['rec'] + 64 * k * M:lay['rec'] + 64 * (k + 1) * M].view(REC_DTYPE)
        lev['unit'] = after[lay['unit'] + 8 * k * F:lay['unit'] + 8 * (k + 1) * F].view(np.float64)
        lev['rows'] = after[lay['rows'] + 32 * k * M:lay['rows'] + 32 * (k + 1) * M].view(ROW_DTYPE)
        out['levels'].append(lev)
        pixels += hk * wk
    return out


def one_level_device_run(c, mask, pol, weight, seed=1.0):
    """dvsof_avg_timestamp_fwd / _bwd on a case of tests/contrast_multi_cases.py -> dict of numpy:
    q, s, base, count, rows, rec, unit, term, grad."""
    import torch
    from dvs_of_training_framework_amd import _lib, loss as L
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    h, w = c['shape']
    F = len(c['fs'])
    M = images_of(c, mask, pol)
    P = M * h * w
    d = {k: torch.from_numpy(np.array(c[k])).to(dev) for k in mc.KEYS}
    term = torch.full((), float('nan'), device=dev)
    lay = L.avg_timestamp_layout(F, M, h, w)
    nbytes = lib.dvsof_avg_timestamp_workspace_bytes(F, mask, int(pol), h, w)
    ws = torch.empty((nbytes // 8,), dtype=torch.long, device=dev)
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [d['x'].numel()] + \
        [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, h, w, mask, int(pol)]
    assert lib.dvsof_avg_timestamp_fwd(*head, term.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()) == 0
    buf = ws.cpu().numpy().view(np.uint8)
    grad = torch.empty((F, 2, h, w), device=dev)
    seed_t = torch.tensor(seed, dtype=torch.float32, device=dev)
    assert lib.dvsof_avg_timestamp_bwd(*head, ws.data_ptr(), nbytes, seed_t.data_ptr(), float(weight),
                                       grad.data_ptr(), _lib.stream()) == 0
    torch.cuda.synchronize()

    def part(key, dtype, count):
        return buf[lay[key]:lay[key] + count * np.dtype(dtype).itemsize].view(dtype)
    return dict(q=part('q', np.int64, P).reshape(M, h, w), s=part('s', np.int64, P).reshape(M, h, w),
                base=part('base', np.int64, P).reshape(M, h, w), count=part('count', np.uint32, P).reshape(M, h, w),
                rec=part('rec', REC_DTYPE, M), unit=part('unit', np.float64, F), rows=part('rows', ROW_DTYPE, M),
                term=term.cpu().numpy(), grad=grad.cpu().numpy())
