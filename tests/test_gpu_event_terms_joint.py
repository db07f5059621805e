"""The joint calls of the two events-only terms (include/dvsof_event_terms_joint.h,
the last section of csrc/avg_timestamp.hip) against the two calls they stand
for, dvsof_contrast_pyramid_fwd / _bwd and dvsof_avg_timestamp_pyramid_fwd /
_bwd on the same inputs, byte for byte and from buffers of 0x5A / NaN: the
contrast rows, both terms' terms and values and both sets of gradients, on four
levels and on one, with the contrast references all or a part of the
average-timestamp ones, per event and tiled, on either form of the columns; the
refusals and the empty calls; and the loss with the flag through
``combined_loss`` against the loss without it."""
import functools

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L, training
from tests import contrast_multi_cases as cm
from tests.test_gpu_event_pyramids_tiled import DEV, FILL, run as twin_run, seam_case, table_of

pytestmark = pytest.mark.gpu
OPTIONS = [(1, 1, False), (1, 5, False), (1, 5, True), (2, 7, False), (4, 5, True), (7, 7, True)]
EINVAL, ENOSPACE = _lib.CONSTANTS['DVSOF_EINVAL'], _lib.CONSTANTS['DVSOF_ENOSPACE']


def one_level_case():
    full = seam_case()
    return dict(full, level_shapes=full['level_shapes'][:1], flows=full['flows'][:1])


def no_events_case():
    full = seam_case()
    return dict(full, **{k: full[k][:0] for k in ('x', 'y', 't', 'p', 's')})


CASES = {'seams': seam_case, 'one_level': one_level_case, 'no_events': no_events_case}


@functools.lru_cache(maxsize=None)
def twins(name, cmask, amask, pol, encoded):
    c = CASES[name]()
    return twin_run('contrast', c, cmask, pol, None, encoded), twin_run('avg_timestamp', c, amask, pol, None, encoded)


def joint(c, cmask, amask, pol, mode=-1, encoded=False, F=None, short=0, atable_case=None):
    """The joint forward and two backwards -> dict: rc, rows, cout and aout (terms, then the value),
    the workspace's bytes after a refused call, cgrads, agrads and those of the second backward."""
    lib = _lib.lib()
    h, w = c['shape']
    shapes, n = c['level_shapes'], c['x'].size
    F = len(c['fs']) if F is None else F
    C = 2 if pol else 1
    Mc, Ma = F * len(cm.rhos(cmask)) * C, F * len(cm.rhos(amask)) * C
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in ('x', 'y', 't', 'p', 's', 'ts', 'fs')}
    flows = [torch.from_numpy(np.array(f)).to(DEV) for f in c['flows']]
    ptrs = [f.data_ptr() for f in flows]
    ctable = table_of(c, F, Mc, ptrs)
    atable = table_of(c, F, Ma, ptrs) if atable_case is None else table_of(atable_case, F, Ma, ptrs)
    if encoded:     # the events are in sample order
        off = torch.from_numpy(np.searchsorted(c['s'], np.arange(3 + 1))).to(DEV)
        cols = [d['x'].short(), d['y'].short(), d['t'], (d['p'] > 0).to(torch.uint8), off]
        head, form = [k.data_ptr() for k in cols] + [off.numel() - 1, n], '_encoded'
    else:
        head, form = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n], ''
    head += [d['ts'].data_ptr(), d['fs'].data_ptr(), F, h, w, cmask, amask, int(pol), ctable, atable]
    nbytes = lib.dvsof_event_terms_joint_workspace_bytes(F, cmask, amask, int(pol), h, w, ctable, atable)
    ws = torch.full((max(nbytes, 64) // 8,), FILL, dtype=torch.long, device=DEV)
    rows = torch.full((max(len(shapes) * Mc, 1), 48), 0x5A, dtype=torch.uint8, device=DEV)
    cout, aout = (torch.full((len(shapes) + 1,), float('nan'), device=DEV) for _ in range(2))
    tiles, tile_bytes = None, 0
    if mode >= 0:
        tiles, tile_bytes = dev_eval.event_pyramids_tiled_workspace('avg_timestamp', F, amask, pol, h, w, atable, n, DEV)
        tiles.fill_(FILL)
    rc = getattr(lib, 'dvsof_event_terms_joint_fwd' + form)(
        *head, rows.data_ptr(), cout.data_ptr(), cout[-1:].data_ptr(), aout.data_ptr(), aout[-1:].data_ptr(),
        ws.data_ptr(), nbytes - short, _lib.stream(), _lib.ptr(tiles), tile_bytes, mode)
    got = dict(rc=rc, nbytes=nbytes, rows=rows.cpu().numpy().tobytes(), cout=cout.cpu().numpy(),
               aout=aout.cpu().numpy(), ws=ws.cpu().numpy())
    if rc != 0 or F == 0:
        return got
    seed = torch.ones((), device=DEV)
    for key in ('', '_again'):
        grads = [torch.full(f.shape, float('nan'), device=DEV) for f in flows + flows]
        for k in range(len(flows)):
            ctable.level[k].grad_flow, atable.level[k].grad_flow = grads[k].data_ptr(), grads[len(flows) + k].data_ptr()
        assert getattr(lib, 'dvsof_event_terms_joint_bwd' + form)(
            *head, ws.data_ptr(), nbytes, seed.data_ptr(), seed.data_ptr(), _lib.stream()) == 0
        got['cgrads' + key] = [g.cpu().numpy() for g in grads[:len(flows)]]
        got['agrads' + key] = [g.cpu().numpy() for g in grads[len(flows):]]
    return got


def same_as_twins(got, contrast, avg):
    assert got['rc'] == contrast['rc'] == avg['rc'] == 0
    assert got['rows'] == contrast['rows'], 'contrast_result'
    assert got['cout'].tobytes() == contrast['out'].tobytes() and got['aout'].tobytes() == avg['out'].tobytes()
    for key, twin in (('cgrads', contrast), ('agrads', avg)):
        for a, again, b in zip(got[key], got[key + '_again'], twin['grads']):
            assert a.tobytes() == b.tobytes(), key
            assert np.array_equal(np.isnan(a), np.isnan(b)) and not np.isnan(a).any()
            assert again.tobytes() == a.tobytes(), 'a second backward of the same forward'


@pytest.mark.parametrize('encoded', [False, True], ids=['wire', 'encoded'])
@pytest.mark.parametrize('mode', [-1, 1])
@pytest.mark.parametrize('cmask,amask,pol', OPTIONS)
@pytest.mark.parametrize('name', ['seams', 'one_level'])
def test_the_joint_calls_write_the_bytes_of_the_two_calls(name, cmask, amask, pol, mode, encoded):
    got = joint(CASES[name](), cmask, amask, pol, mode, encoded)
    same_as_twins(got, *twins(name, cmask, amask, pol, encoded))
    assert all(np.abs(g).max() > 0 for g in got['cgrads'] + got['agrads'])


def untouched(got):
    return (got['ws'] == FILL).all() and got['rows'] == b'\x5a' * len(got['rows']) and \
        np.isnan(got['cout']).all() and np.isnan(got['aout']).all()


def test_refusals_and_empty_calls():
    c = seam_case()
    got = joint(c, 2, 5, False)                                     # no subset
    assert got['rc'] == EINVAL and got['nbytes'] == 0 and untouched(got)
    got = joint(c, 1, 5, False, atable_case=seam_case((0, 1, 2, 2)))    # each table alone is accepted
    assert got['rc'] == EINVAL and got['nbytes'] == 0 and untouched(got)
    got = joint(c, 1, 5, False, short=8)
    assert got['rc'] == ENOSPACE and got['nbytes'] > 0 and untouched(got)
    assert joint(c, 1, 5, False, mode=2)['rc'] == EINVAL            # no such mode
    got = joint(c, 1, 5, False, F=0)
    assert got['rc'] == 0 and untouched(got)
    for mode in (-1, 1):
        got = joint(no_events_case(), 1, 5, True, mode)
        same_as_twins(got, *twins('no_events', 1, 5, True, False))
        assert not any(np.abs(g).max() > 0 for g in got['cgrads'] + got['agrads'])


@pytest.mark.parametrize('compact', [False, True], ids=['wire', 'compact'])
@pytest.mark.parametrize('scales', ['finest', 'all'])
def test_the_loss_with_the_flag_is_the_loss_without_it(scales, compact):
    c = seam_case()
    events = {k: torch.from_numpy(np.array(c[v])).to(DEV)
              for k, v in (('x', 'x'), ('y', 'y'), ('timestamp', 't'), ('polarity', 'p'), ('sample_index', 's'))}
    if compact:
        off = torch.from_numpy(np.searchsorted(c['s'], np.arange(3 + 1))).to(DEV)
        events = dict(x=events['x'].short(), y=events['y'].short(), timestamp=events['timestamp'],
                      polarity=events['polarity'] > 0, sample_event_offsets=off)
    ts, fs = torch.from_numpy(c['ts']).to(DEV), torch.from_numpy(c['fs']).to(DEV)
    losses = L.Losses(c['level_shapes'][::-1], 3, DEV)
    runs = []
    for flag in ({}, {'event_terms_joint': True}, {'event_terms_joint': True, 'event_pyramids_tiled': 'force'}):
        flows = [torch.from_numpy(np.nan_to_num(f)).to(DEV).requires_grad_(True) for f in c['flows'][::-1]]
        loss, terms = training.combined_loss(
            losses, flows, ts, fs, None, None, None, None, contrast_weight=0.25, events=events,
            contrast_polarity=True, avg_timestamp_polarity=True, contrast_scales=scales, avg_timestamp_scales=scales,
            avg_timestamp_weight=0.5, **flag)
        loss.backward()
        used = flows if scales == 'all' else flows[-1:]
        assert terms.contrast.shape == terms.avg_timestamp.shape == ((len(flows),) if scales == 'all' else ())
        assert all(f.grad.abs().max() > 0 for f in used)
        runs.append([t.detach().cpu().numpy().tobytes() for t in (loss, terms.contrast, terms.avg_timestamp)] +
                    [f.grad.cpu().numpy().tobytes() for f in flows])
    assert runs[0] == runs[1] == runs[2]
