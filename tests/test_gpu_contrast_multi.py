"""csrc/contrast.hip with its options on the device against the numpy
restatement of docs/CONTRAST_SPEC.md sections 11-14 (loss.contrast_multi_fwd_host /
contrast_multi_bwd_host), byte for byte: the images, the counts, the
statistics rows, the image records and frame units in the workspace, the term
and the flow gradient on every case of tests/contrast_multi_cases.py and on a
permuted copy of each; the existing entry points at mask = start without
polarity; the argument rules; and the term through autograd in a training
step.

The fixed-point sums are cleared by the kernel that converts them, inside the
same call that fills them, so the device's sums cannot be read before the
closing; what is read is that they are zeros after it, the unit they were
summed in, and the gradient converted from them (from buffers of 0xAA and of
0x55, and by a second backward of the same forward)."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L
from tests import contrast_cases as cc, contrast_multi_cases as mc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

_matrix = {}


def matrix():
    if not _matrix:
        _matrix.update(mc.device_matrix())
    return _matrix


CASE_IDS = list(matrix())


def device_run(c, mask, pol, seed=1.0, weight=1.0, fills=(0xAA, 0x55)):
    """dvsof_contrast_multi_fwd, then dvsof_contrast_multi_bwd once per fill
    pattern of the gradient buffer -> dict of numpy arrays: q, count, rows,
    term, rec [M,4] and unit [F] as the forward left them, grads (one per
    fill), sums (after the last backward)."""
    lib = _lib.lib()
    h, w = c['shape']
    F = len(c['fs'])
    M = F * len(mc.rhos(mask)) * (2 if pol else 1)
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in mc.KEYS}     # copies: the cases are read-only
    n = d['x'].numel()
    q = torch.full((M, h, w), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=DEV)
    count = torch.full((M, h, w), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rows = torch.full((M, 48), 0x5A, dtype=torch.uint8, device=DEV)
    term = torch.full((), float('nan'), device=DEV)
    nbytes = lib.dvsof_contrast_multi_workspace_bytes(F, mask, int(pol), h, w)
    stats = lib.dvsof_iwe_stats_workspace_bytes(M, h, w)
    assert nbytes == 16 * F * h * w + 32 * M + 8 * F + stats and stats >= 48 * M
    ws = torch.full((nbytes // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=DEV)
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n] + \
        [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, h, w, mask, int(pol)]
    assert lib.dvsof_contrast_multi_fwd(*head, q.data_ptr(), count.data_ptr(), rows.data_ptr(), term.data_ptr(),
                                        ws.data_ptr(), nbytes, _lib.stream()) == 0
    after_fwd = ws.cpu().numpy()
    seed_t = torch.tensor(seed, dtype=torch.float32, device=DEV)
    grads = []
    for fill in fills:
        grad = torch.full((F, 2, h, w), fill, dtype=torch.uint8, device=DEV).repeat_interleave(4, -1) \
            .view(torch.float32)
        assert tuple(grad.shape) == (F, 2, h, w) and grad.is_contiguous()
        assert lib.dvsof_contrast_multi_bwd(*head, q.data_ptr(), ws.data_ptr(), nbytes, seed_t.data_ptr(), weight,
                                            grad.data_ptr(), _lib.stream()) == 0
        grads.append(grad.cpu().numpy())
    torch.cuda.synchronize()
    n_sums = 2 * F * h * w
    assert not after_fwd[:n_sums].any(), 'the forward leaves the sums cleared'
    return dict(q=q.cpu().numpy(), count=count.cpu().numpy().view(np.uint32), rows=dev_eval.read_iwe_results(rows),
                term=term.cpu().numpy(), rec=after_fwd[n_sums:n_sums + 4 * M].view(np.float64).reshape(M, 4),
                unit=after_fwd[n_sums + 4 * M:n_sums + 4 * M + F].view(np.float64), grads=grads,
                sums=ws.cpu().numpy()[:n_sums])


def same_as_restatement(c, mask, pol, seed, weight):
    fwd = L.contrast_multi_fwd_host(*mc.args_of(c), mask, pol)
    want, _ = L.contrast_multi_bwd_host(*mc.args_of(c), fwd, seed=seed, weight=weight)
    got = device_run(c, mask, pol, seed, weight)
    assert np.array_equal(got['q'], fwd['q']), 'q'
    assert np.array_equal(got['count'], fwd['count']), 'count'
    for k in ('sum_q', 'max_q', 'count_sum', 'count_sq', 'count_max'):
        assert np.array_equal(got['rows'][k], fwd['result'][k]), k
    assert got['rows']['sum_sq'].tobytes() == fwd['result']['sum_sq'].tobytes(), 'sum_sq'
    assert got['term'].tobytes() == fwd['term'].tobytes(), (got['term'], fwd['term'])
    for i, k in enumerate(('mean', 'coef', 'gmax', 'image_term')):
        assert got['rec'][:, i].tobytes() == fwd[k].tobytes(), k
    assert got['unit'].tobytes() == fwd['unit'].tobytes(), 'unit'
    for g in got['grads']:                              # every element written, from either pattern
        assert g.tobytes() == want.tobytes(), int((g.view(np.uint32) != want.view(np.uint32)).sum())
    assert not got['sums'].any(), 'the closing kernel clears the sums'
    return fwd, want


@pytest.mark.parametrize('name', CASE_IDS)
def test_device_equals_the_restatement_byte_for_byte(name):
    c, mask, pol = matrix()[name]
    fwd, grad = same_as_restatement(c, mask, pol, 1.0, 0.25)
    again, grad_p = same_as_restatement(mc.permuted(c), mask, pol, 1.0, 0.25)
    assert np.array_equal(again['q'], fwd['q']) and grad_p.tobytes() == grad.tobytes()
    assert np.isfinite(grad).all() and np.isfinite(fwd['term'])
    if c['x'].size >= 255 and c['shape'] != (1, 1) and not name.startswith('degenerate'):
        assert fwd['count'].sum() > 0 and grad.any(), 'the case exercises nothing'


def test_the_cases_reach_what_they_are_there_for():
    """Host only: the classes of events and images the device test relies on exist."""
    c, mask, pol = matrix()['33x31_F3_n4097_m7_p1']
    assert (c['p'] == 0).any() and (c['p'] > 0).any() and (c['p'] < 0).any()
    assert np.isnan(c['flow']).any() and np.isinf(c['flow']).any()
    fwd = L.contrast_multi_fwd_host(*mc.args_of(c), mask, pol)
    q = fwd['q'].reshape(3, 3, 2, 33, 31)
    assert all(q[:, r, ch].any() for r in range(3) for ch in range(2))
    assert not np.array_equal(q[:, 0], q[:, 1]) and not np.array_equal(q[:, 1], q[:, 2])
    assert fwd['coef'].all() and len(fwd['q']) == 18
    one, mask, pol = matrix()['one_pixel_4097_m7_p1']
    assert L.contrast_multi_fwd_host(*mc.args_of(one), mask, pol)['count'].max() > 1500
    assert len(L.contrast_multi_fwd_host(*mc.args_of(matrix()['40x40_F3_n4097_m7_p1'][0]), 7, True)['q']) == 18


def test_seed_and_weight_reach_the_closing_kernel():
    c, _, _ = matrix()['33x31_F3_n257_m7_p1']
    _, a = same_as_restatement(c, 7, True, -1.5, 0.25)
    _, b = same_as_restatement(c, 7, True, 1.0, 1.0)
    assert a.any() and a.tobytes() != b.tobytes()


def test_a_second_backward_of_one_forward_gives_the_same_bytes():
    c, _, _ = matrix()['33x31_F3_n4097_m7_p1']
    got = device_run(c, 7, True, 1.0, 0.25, fills=(0xAA, 0x55, 0x00))
    assert got['grads'][0].any()
    assert got['grads'][0].tobytes() == got['grads'][1].tobytes() == got['grads'][2].tobytes()


def old_device_run(c, seed, weight):
    """dvsof_contrast_fwd / dvsof_contrast_bwd on the device."""
    lib = _lib.lib()
    h, w = c['shape']
    F = len(c['fs'])
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in cc.KEYS}
    q = torch.empty((F, h, w), dtype=torch.long, device=DEV)
    count = torch.empty((F, h, w), dtype=torch.int32, device=DEV)
    rows = torch.empty((F, 48), dtype=torch.uint8, device=DEV)
    term = torch.full((), float('nan'), device=DEV)
    nbytes = lib.dvsof_contrast_workspace_bytes(F, h, w)
    ws = torch.empty((nbytes // 8,), dtype=torch.long, device=DEV)
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 's')] + [d['x'].numel()] + \
        [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, h, w]
    assert lib.dvsof_contrast_fwd(*head, q.data_ptr(), count.data_ptr(), rows.data_ptr(), term.data_ptr(),
                                  ws.data_ptr(), nbytes, _lib.stream()) == 0
    grad = torch.empty((F, 2, h, w), device=DEV)
    seed_t = torch.tensor(seed, dtype=torch.float32, device=DEV)
    assert lib.dvsof_contrast_bwd(*head, q.data_ptr(), ws.data_ptr(), nbytes, seed_t.data_ptr(), weight,
                                  grad.data_ptr(), _lib.stream()) == 0
    torch.cuda.synchronize()
    return dict(q=q.cpu().numpy(), count=count.cpu().numpy().view(np.uint32), rows=rows.cpu().numpy(),
                term=term.cpu().numpy(), grad=grad.cpu().numpy())


@pytest.mark.parametrize('shape,F,n', [((5, 7), 1, 257), ((33, 31), 3, 4097), ((2, 3), 3, 257), ((40, 40), 3, 4097)])
def test_start_without_polarity_gives_the_bytes_of_the_existing_entry_points(shape, F, n):
    c = mc.with_polarity(cc.device_case(shape, F, n))
    old = old_device_run(c, -1.5, 0.25)
    lib = _lib.lib()
    h, w = shape
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in cc.KEYS}
    q = torch.empty((F, h, w), dtype=torch.long, device=DEV)
    count = torch.empty((F, h, w), dtype=torch.int32, device=DEV)
    rows = torch.empty((F, 48), dtype=torch.uint8, device=DEV)
    term = torch.full((), float('nan'), device=DEV)
    nbytes = lib.dvsof_contrast_multi_workspace_bytes(F, 1, 0, h, w)
    ws = torch.empty((nbytes // 8,), dtype=torch.long, device=DEV)
    head = [d[k].data_ptr() for k in ('x', 'y', 't')] + [None, d['s'].data_ptr(), n] + \
        [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, h, w, 1, 0]         # p is not read: null
    assert lib.dvsof_contrast_multi_fwd(*head, q.data_ptr(), count.data_ptr(), rows.data_ptr(), term.data_ptr(),
                                        ws.data_ptr(), nbytes, _lib.stream()) == 0
    grad = torch.empty((F, 2, h, w), device=DEV)
    seed_t = torch.tensor(-1.5, dtype=torch.float32, device=DEV)
    assert lib.dvsof_contrast_multi_bwd(*head, q.data_ptr(), ws.data_ptr(), nbytes, seed_t.data_ptr(), 0.25,
                                        grad.data_ptr(), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(q.cpu().numpy(), old['q']) and old['q'].any()
    assert np.array_equal(count.cpu().numpy().view(np.uint32), old['count'])
    assert rows.cpu().numpy().tobytes() == old['rows'].tobytes()
    assert term.cpu().numpy().tobytes() == old['term'].tobytes()
    assert grad.cpu().numpy().tobytes() == old['grad'].tobytes() and old['grad'].any()


def test_argument_rules_on_the_device_build():
    lib = _lib.lib()
    F, h, w, n, M = 2, 5, 7, 11, 12
    t = dict(x=torch.zeros(n, dtype=torch.long), y=torch.zeros(n, dtype=torch.long), t=torch.zeros(n),
             p=torch.ones(n, dtype=torch.long), s=torch.zeros(n, dtype=torch.long), ts=torch.zeros(2 * F),
             fs=torch.zeros(F, dtype=torch.long), flow=torch.zeros(F, 2, h, w),
             q=torch.full((M, h, w), 7, dtype=torch.long), count=torch.full((M, h, w), 7, dtype=torch.int32),
             result=torch.full((M, 48), 7, dtype=torch.uint8), term=torch.full((1,), 7.0),
             ws=torch.full((lib.dvsof_contrast_multi_workspace_bytes(F, 7, 1, h, w),), 7, dtype=torch.uint8),
             seed=torch.ones(1), grad=torch.full((F, 2, h, w), 7.0))
    t = {k: v.to(DEV) for k, v in t.items()}
    a = {k: v.data_ptr() for k, v in t.items()}
    a['n'] = n
    seen = 0
    for what, call, expect in mc.bad_calls(lib, a, F, h, w):
        assert call() == expect, what
        seen += 1
    torch.cuda.synchronize()
    assert seen >= 60
    for k in ('q', 'count', 'result', 'term', 'ws', 'grad'):
        assert bool((t[k] == 7).all()), k               # nothing was launched
    assert all(rc == 0 for rc in mc.empty_calls(lib))
    # a null p is refused only where it would be read
    for polarity, n_, expect in ((0, n, 0), (1, 0, 0), (1, n, mc.EINVAL)):
        rc = lib.dvsof_contrast_multi_fwd(a['x'], a['y'], a['t'], None, a['s'], n_, a['ts'], a['fs'], a['flow'], F, h,
                                          w, 7, polarity, a['q'], a['count'], a['result'], a['term'], a['ws'],
                                          t['ws'].numel(), None)
        assert rc == expect, (polarity, n_)
    torch.cuda.synchronize()


# ------------------------------------------------------- through autograd
# the smallest frame of tests/network_cases.py; 2500 events per sample keep the
# voxeliser on its fixed-point path (4096 events and up), where the network repeats its bits
B, H, W, DEPTH, EVENTS = 2, 32, 48, 3, 2500
WEIGHT = 0.25
ALL = dict(contrast_references=('start', 'middle', 'end'), contrast_polarity=True)


@pytest.fixture(scope='module')
def training_runs():
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    torch.manual_seed(0)
    model = Model(DEV, event_representation_depth=DEPTH).train()
    ev = init_losses((H, W), B, model, DEV, sequence_length=1)
    batch_np = synthetic.make_batch(7, B, H, W, EVENTS)

    def run(**kw):
        model.zero_grad(set_to_none=True)
        batch = synthetic.to_torch(batch_np, DEV)
        loss, terms, tags, out = process_minibatch(model, batch, FakeTimer(), DEV, True, ev, [0.5, 1, 1],
                                                   return_prediction=True, **kw)
        seen = []
        out['prediction'][-1].register_hook(lambda g: seen.append(g.detach().clone()))
        loss.backward()
        torch.cuda.synchronize()
        return dict(loss=loss.detach().clone(), terms=terms, flow=out['prediction'][-1].detach().clone(),
                    flow_grad=seen[0], flow_ts=out['flow_ts'], fsi=out['flow_sample_idx'], events=batch['events'],
                    grads=[p.grad.detach().clone() for p in model.parameters()])
    return dict(plain=run(), old=run(contrast_weight=WEIGHT),
                default=run(contrast_weight=WEIGHT, contrast_references=('start',), contrast_polarity=False),
                on=run(contrast_weight=WEIGHT, **ALL), again=run(contrast_weight=WEIGHT, **ALL))


def test_the_default_flags_are_the_step_without_the_keywords(training_runs):
    old, default = training_runs['old'], training_runs['default']
    assert torch.equal(old['loss'], default['loss']) and torch.equal(old['flow_grad'], default['flow_grad'])
    assert len(old['grads']) > 30
    for a, b in zip(old['grads'], default['grads']):
        assert torch.equal(a, b)
    assert old['terms'].contrast() == default['terms'].contrast() and old['terms'].contrast() is not None


def test_the_term_reaches_the_finest_flow_by_one_add(training_runs):
    plain, on, old = training_runs['plain'], training_runs['on'], training_runs['old']
    assert torch.equal(on['flow'], plain['flow'])               # the forward repeats its bits
    c = dict(x=on['events']['x'], y=on['events']['y'], t=on['events']['timestamp'], p=on['events']['polarity'],
             s=on['events']['sample_index'], ts=on['flow_ts'].contiguous().reshape(-1), fs=on['fsi'],
             flow=on['flow'])
    c = {k: v.cpu().numpy() for k, v in c.items()}
    c['shape'] = (H, W)
    got = device_run(c, 7, True, 1.0, WEIGHT, fills=(0xAA,))
    grad, term = got['grads'][0], got['term']
    assert got['count'].sum() == 3 * 2 * EVENTS and np.abs(grad).max() > 0
    want = plain['flow_grad'].cpu().numpy() + grad              # one float32 add per element
    assert want.dtype == np.float32 and on['flow_grad'].cpu().numpy().tobytes() == want.tobytes()
    # the loss is the fused loss plus weight times the logged term
    assert on['terms'].contrast() == float(term) and on['terms'].host() == plain['terms'].host()
    assert float(on['loss']) == float(np.float32(plain['loss'].item()) + np.float32(term) * np.float32(WEIGHT))
    assert any(not torch.equal(a, b) for a, b in zip(plain['grads'], on['grads']))
    assert on['terms'].contrast() != old['terms'].contrast()
    assert not torch.equal(on['flow_grad'], old['flow_grad'])


def test_two_runs_give_the_same_bits(training_runs):
    on, again = training_runs['on'], training_runs['again']
    assert torch.equal(on['loss'], again['loss']) and torch.equal(on['flow_grad'], again['flow_grad'])
    assert on['terms'].contrast() == again['terms'].contrast()
    for a, b in zip(on['grads'], again['grads']):
        assert torch.equal(a, b)
