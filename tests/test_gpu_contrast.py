"""csrc/contrast.hip on the device against the numpy restatement of
docs/CONTRAST_SPEC.md (loss.contrast_fwd_host / contrast_bwd_host), byte for
byte: the images, the counts, the statistics rows, the frames' records and
units in the workspace, the term and the flow gradient on every case of tests/contrast_cases.py and on a permuted copy of
each; the argument rules; and the term through autograd in a training step."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, eval as dev_eval, loss as L
from tests import contrast_cases as cc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

_cases = {}


def cases():
    if not _cases:
        _cases.update(cc.device_cases())
    return _cases


CASE_IDS = list(cases())


def device_run(c, seed=1.0, weight=1.0, fills=(0xAA, 0x55)):
    """dvsof_contrast_fwd, then dvsof_contrast_bwd once per fill pattern of the
    gradient buffer -> (q, count, rows, term, [grad per fill], rec [F,4] =
    {mean, coef, gmax, term} and unit [F] as the forward left them in the
    workspace behind the sums) as numpy."""
    lib = _lib.lib()
    h, w = c['shape']
    F = len(c['fs'])
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in cc.KEYS}     # copies: the cases are read-only
    n = d['x'].numel()
    q = torch.full((F, h, w), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=DEV)
    count = torch.full((F, h, w), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rows = torch.full((F, 48), 0x5A, dtype=torch.uint8, device=DEV)
    term = torch.full((), float('nan'), device=DEV)
    nbytes = lib.dvsof_contrast_workspace_bytes(F, h, w)
    assert nbytes >= 16 * F * h * w + 32 * F + 48 * F
    ws = torch.full((nbytes // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=DEV)
    cols = [d[k].data_ptr() for k in ('x', 'y', 't', 's')]
    tables = [d[k].data_ptr() for k in ('ts', 'fs', 'flow')]
    assert lib.dvsof_contrast_fwd(*cols, n, *tables, F, h, w, q.data_ptr(), count.data_ptr(), rows.data_ptr(),
                                  term.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()) == 0
    after_fwd = ws.cpu().numpy()
    seed_t = torch.tensor(seed, dtype=torch.float32, device=DEV)
    grads = []
    for fill in fills:
        grad = torch.full((F, 2, h, w), fill, dtype=torch.uint8, device=DEV).repeat_interleave(4, -1) \
            .view(torch.float32)
        assert tuple(grad.shape) == (F, 2, h, w) and grad.is_contiguous()
        assert lib.dvsof_contrast_bwd(*cols, n, *tables, F, h, w, q.data_ptr(), ws.data_ptr(), nbytes,
                                      seed_t.data_ptr(), weight, grad.data_ptr(), _lib.stream()) == 0
        grads.append(grad.cpu().numpy())
    torch.cuda.synchronize()
    n_sums = 2 * F * h * w
    return (q.cpu().numpy(), count.cpu().numpy().view(np.uint32), dev_eval.read_iwe_results(rows),
            term.cpu().numpy(), grads, after_fwd[n_sums:n_sums + 4 * F].view(np.float64).reshape(F, 4),
            after_fwd[n_sums + 4 * F:n_sums + 5 * F].view(np.float64))


def same_as_restatement(c, seed, weight):
    fwd = L.contrast_fwd_host(*cc.args_of(c))
    want, _ = L.contrast_bwd_host(*cc.args_of(c), fwd, seed=seed, weight=weight)
    q, count, rows, term, grads, rec, unit = device_run(c, seed, weight)
    assert np.array_equal(q, fwd['q']), 'q'
    assert np.array_equal(count, fwd['count']), 'count'
    for k in ('sum_q', 'max_q', 'count_sum', 'count_sq', 'count_max'):
        assert np.array_equal(rows[k], fwd['result'][k]), k
    assert rows['sum_sq'].tobytes() == fwd['result']['sum_sq'].tobytes(), 'sum_sq'
    assert term.tobytes() == fwd['term'].tobytes(), (term, fwd['term'])
    for i, k in ((0, 'mean'), (1, 'coef'), (3, 'frame_term')):
        assert rec[:, i].tobytes() == fwd[k].tobytes(), k
    assert unit.tobytes() == fwd['unit'].tobytes(), 'unit'  # a frame of one image: from the gmax its lane holds
    for g in grads:                                     # every element written, from either pattern
        assert g.tobytes() == want.tobytes(), int((g.view(np.uint32) != want.view(np.uint32)).sum())
    return fwd, want


@pytest.mark.parametrize('name', CASE_IDS)
def test_device_equals_the_restatement_byte_for_byte(name):
    c = cases()[name]
    fwd, grad = same_as_restatement(c, 1.0, 0.25)
    again, grad_p = same_as_restatement(cc.permuted(c), 1.0, 0.25)
    assert np.array_equal(again['q'], fwd['q']) and grad_p.tobytes() == grad.tobytes()
    assert np.isfinite(grad).all() and np.isfinite(fwd['term'])
    if c['x'].size >= 255 and c['shape'] != (1, 1) and name != 'degenerate_windows':
        assert fwd['count'].sum() > 0 and grad.any(), 'the case exercises nothing'


def test_the_cases_reach_what_they_are_there_for():
    """Host only: the classes of events the device test relies on exist."""
    c = cases()['33x31_F3_n4097']
    h, w = c['shape']
    ends = np.unique(c['ts'])
    assert all((c['t'] == e).any() for e in ends)                       # exactly on the ends
    assert (c['t'] == np.nextafter(ends[0], np.float32(-9))).any()      # just outside
    assert (c['x'] == -1).any() and (c['x'] == w).any() and (c['s'] < 0).any() and (c['s'] > 1).any()
    assert np.isnan(c['flow']).any() and np.isinf(c['flow']).any()
    fwd = L.contrast_fwd_host(*cc.args_of(c))
    assert fwd['count'].sum() > fwd['result']['sum_q'].sum() / 2.0 ** 32 > 0     # weight left the image
    one = cases()['one_pixel_4097']
    assert L.contrast_fwd_host(*cc.args_of(one))['count'].max() == 4097
    deg = L.contrast_fwd_host(*cc.args_of(cases()['degenerate_windows']))
    assert deg['count'][0].sum() > 0 and not deg['count'][1:].any()
    # d == 0: tau = 0 and every event stays where it is, unless its flow is not finite (0 * inf)
    finite = np.isfinite(cases()['degenerate_windows']['flow'][0]).all(0)
    assert np.array_equal(deg['q'][0][finite], deg['count'][0][finite].astype(np.int64) << 32)
    # var(c) = 0 in the frames without events: no coefficient, and the unit of gmax = 0
    assert deg['coef'][0] != 0 and not deg['coef'][1:].any() and (deg['unit'][1:] == 2.0 ** 40).all()
    # more frames than lanes: frames of every round of the closing wave have contrast and a gradient
    many = cases()['2x3_F130_n1040']
    fwd = L.contrast_fwd_host(*cc.args_of(many))
    grad, _ = L.contrast_bwd_host(*cc.args_of(many), fwd)
    assert len(many['fs']) == 130 and many['x'].size == 1040
    for lo, hi in ((0, 64), (64, 128), (128, 130)):
        assert fwd['coef'][lo:hi].any() and grad[lo:hi].any(), (lo, hi)


def test_seed_and_weight_reach_the_closing_kernel():
    c = cases()['16x16_F3_n257']
    _, a = same_as_restatement(c, -1.5, 0.25)
    _, b = same_as_restatement(c, 1.0, 1.0)
    assert a.any() and a.tobytes() != b.tobytes()


def test_argument_rules_on_the_device_build():
    lib = _lib.lib()
    F, h, w, n = 2, 5, 7, 11
    t = dict(x=torch.zeros(n, dtype=torch.long), y=torch.zeros(n, dtype=torch.long), t=torch.zeros(n),
             s=torch.zeros(n, dtype=torch.long), ts=torch.zeros(2 * F), fs=torch.zeros(F, dtype=torch.long),
             flow=torch.zeros(F, 2, h, w), q=torch.full((F, h, w), 7, dtype=torch.long),
             count=torch.full((F, h, w), 7, dtype=torch.int32), result=torch.full((F, 48), 7, dtype=torch.uint8),
             term=torch.full((1,), 7.0),
             ws=torch.full((lib.dvsof_contrast_workspace_bytes(F, h, w),), 7, dtype=torch.uint8),
             seed=torch.ones(1), grad=torch.full((F, 2, h, w), 7.0))
    t = {k: v.to(DEV) for k, v in t.items()}
    a = {k: v.data_ptr() for k, v in t.items()}
    a['n'] = n
    seen = 0
    for what, call, expect in cc.bad_calls(lib, a, F, h, w):
        assert call() == expect, what
        seen += 1
    torch.cuda.synchronize()
    assert seen >= 40
    for k in ('q', 'count', 'result', 'term', 'ws', 'grad'):
        assert bool((t[k] == 7).all()), k               # nothing was launched
    assert all(rc == 0 for rc in cc.empty_calls(lib))
    for F_, h_, w_ in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 32768)):
        assert lib.dvsof_contrast_workspace_bytes(F_, h_, w_) == 0


# ------------------------------------------------------- through autograd
# the smallest frame of tests/network_cases.py; 2500 events per sample keep the
# voxeliser on its fixed-point path (4096 events and up), where the network repeats its bits
B, H, W, DEPTH, EVENTS = 2, 32, 48, 3, 2500
WEIGHT = 0.25


@pytest.fixture(scope='module')
def training_runs():
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import process_minibatch
    from tests.network_cases import SMALL_FRAMES
    assert (B, H, W) == min(SMALL_FRAMES, key=lambda f: (f[1] * f[2], f[0]))
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
    return dict(plain=run(), zero=run(contrast_weight=0.0), on=run(contrast_weight=WEIGHT),
                again=run(contrast_weight=WEIGHT))


def test_weight_zero_is_the_step_without_the_keyword(training_runs):
    plain, zero = training_runs['plain'], training_runs['zero']
    assert torch.equal(plain['loss'], zero['loss']) and torch.equal(plain['flow_grad'], zero['flow_grad'])
    assert len(plain['grads']) > 30
    for a, b in zip(plain['grads'], zero['grads']):
        assert torch.equal(a, b)
    assert zero['terms'].contrast() is None and zero['terms'].host() == plain['terms'].host()


def test_the_term_reaches_the_finest_flow_by_one_add(training_runs):
    plain, on = training_runs['plain'], training_runs['on']
    assert torch.equal(on['flow'], plain['flow'])               # the forward repeats its bits
    c = dict(x=on['events']['x'], y=on['events']['y'], t=on['events']['timestamp'],
             s=on['events']['sample_index'], ts=on['flow_ts'].contiguous().reshape(-1), fs=on['fsi'],
             flow=on['flow'])
    c = {k: v.cpu().numpy() for k, v in c.items()}
    c['shape'] = (H, W)
    q, count, rows, term, (grad,), _, _ = device_run(c, 1.0, WEIGHT, fills=(0xAA,))
    assert count.sum() == 2 * EVENTS and np.abs(grad).max() > 0
    want = plain['flow_grad'].cpu().numpy() + grad              # one float32 add per element
    assert want.dtype == np.float32 and on['flow_grad'].cpu().numpy().tobytes() == want.tobytes()
    # the loss is the fused loss plus weight times the logged term
    assert on['terms'].contrast() == float(term) and on['terms'].host() == plain['terms'].host()
    assert float(on['loss']) == float(np.float32(plain['loss'].item()) + np.float32(term) * np.float32(WEIGHT))
    assert any(not torch.equal(a, b) for a, b in zip(plain['grads'], on['grads']))


def test_two_runs_give_the_same_bits(training_runs):
    on, again = training_runs['on'], training_runs['again']
    assert torch.equal(on['loss'], again['loss']) and torch.equal(on['flow_grad'], again['flow_grad'])
    assert on['terms'].contrast() == again['terms'].contrast()
    for a, b in zip(on['grads'], again['grads']):
        assert torch.equal(a, b)
