"""csrc/avg_timestamp.hip on the device against the numpy restatement of
docs/AVG_TIMESTAMP_SPEC.md (loss.avg_timestamp_fwd_host / avg_timestamp_bwd_host),
byte for byte: the four images of the workspace (q, s, base, count), the
statistics rows, the image records, the frame units, the term and the flow
gradient on every case of contrast_multi_cases.device_matrix(), on one 400x400
frame (the 128 partials of the statistics) and on a permuted copy of each; q
and count against dvsof_contrast_multi_fwd; the argument rules; and the term through autograd, in a training step and in
``training.train`` on a frameless recording.

The fixed-point sums are cleared by the kernel that converts them, so what is
read is that they are zeros after the forward and after every backward, and
the gradient converted from them (into buffers of 0xAA and of 0x55, and by a
second backward of the same forward)."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, loss as L
from tests import avg_timestamp_cases as ac, contrast_cases as cc, contrast_multi_cases as mc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

_matrix = {}


def matrix():
    if not _matrix:
        _matrix.update(ac.device_matrix())
        # the statistics' closing wave with the 128 partials allowed: two per lane, five rounds per thread
        _matrix['400x400_F1_n4097_m5_p0'] = (mc.with_polarity(cc.device_case((400, 400), 1, 4097)), 5, False)
    return _matrix


CASE_IDS = list(matrix())


def device_run(c, mask, pol, seed=1.0, weight=1.0, fills=(0xAA, 0x55)):
    """dvsof_avg_timestamp_fwd, then dvsof_avg_timestamp_bwd once per fill
    pattern of the gradient buffer -> dict of numpy arrays: q, s, base, count,
    rows, rec, unit and term as the forward left them, grads (one per fill),
    sums (after the last backward)."""
    lib = _lib.lib()
    h, w = c['shape']
    F = len(c['fs'])
    M = F * len(ac.rhos(mask)) * (2 if pol else 1)
    P = M * h * w
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in ac.KEYS}     # copies: the cases are read-only
    n = d['x'].numel()
    term = torch.full((), float('nan'), device=DEV)
    lay = L.avg_timestamp_layout(F, M, h, w)
    nbytes = lib.dvsof_avg_timestamp_workspace_bytes(F, mask, int(pol), h, w)
    assert nbytes == lay['bytes'] and nbytes % 8 == 0
    ws = torch.full((nbytes // 8,), 0x5A5A5A5A5A5A5A5A, dtype=torch.long, device=DEV)
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [n] + \
        [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, h, w, mask, int(pol)]
    assert lib.dvsof_avg_timestamp_fwd(*head, term.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()) == 0
    after_fwd = ws.cpu().numpy().view(np.uint8)
    seed_t = torch.tensor(seed, dtype=torch.float32, device=DEV)
    grads = []
    for fill in fills:
        grad = torch.full((F, 2, h, w), fill, dtype=torch.uint8, device=DEV).repeat_interleave(4, -1) \
            .view(torch.float32)
        assert tuple(grad.shape) == (F, 2, h, w) and grad.is_contiguous()
        assert lib.dvsof_avg_timestamp_bwd(*head, ws.data_ptr(), nbytes, seed_t.data_ptr(), weight, grad.data_ptr(),
                                           _lib.stream()) == 0
        grads.append(grad.cpu().numpy())
    torch.cuda.synchronize()
    after_bwd = ws.cpu().numpy().view(np.uint8)

    def part(buf, key, dtype, count):
        return buf[lay[key]:lay[key] + count * np.dtype(dtype).itemsize].view(dtype)
    n_sums = 2 * F * h * w
    assert not part(after_fwd, 'sums', np.int64, n_sums).any(), 'the forward leaves the sums cleared'
    # the backward writes the sums alone
    assert after_bwd[:lay['sums']].tobytes() == after_fwd[:lay['sums']].tobytes()
    assert after_bwd[lay['count']:].tobytes() == after_fwd[lay['count']:].tobytes()
    return dict(q=part(after_fwd, 'q', np.int64, P).reshape(M, h, w),
                s=part(after_fwd, 's', np.int64, P).reshape(M, h, w),
                base=part(after_fwd, 'base', np.int64, P).reshape(M, h, w),
                count=part(after_fwd, 'count', np.uint32, P).reshape(M, h, w),
                rec=part(after_fwd, 'rec', L.AVG_TIMESTAMP_REC_DTYPE, M), unit=part(after_fwd, 'unit', np.float64, F),
                rows=part(after_fwd, 'rows', L.AVG_TIMESTAMP_ROW_DTYPE, M), term=term.cpu().numpy(), grads=grads,
                sums=part(after_bwd, 'sums', np.int64, n_sums))


def same_as_restatement(c, mask, pol, seed, weight):
    fwd = L.avg_timestamp_fwd_host(*ac.args_of(c), mask, pol)
    want, _ = L.avg_timestamp_bwd_host(*ac.args_of(c), fwd, seed=seed, weight=weight)
    got = device_run(c, mask, pol, seed, weight)
    for k in ('q', 's', 'base', 'count'):
        assert np.array_equal(got[k], fwd[k]), k
    for k in ('n', 'n0'):
        assert np.array_equal(got['rows'][k], fwd['rows'][k]), k
    for k in ('S', 'S0', 'peak'):
        assert got['rows'][k].tobytes() == fwd['rows'][k].tobytes(), k
    for k in L.AVG_TIMESTAMP_REC_DTYPE.names:
        assert got['rec'][k].tobytes() == fwd['rec'][k].tobytes(), k
    assert got['unit'].tobytes() == fwd['unit'].tobytes(), 'unit'
    assert got['term'].tobytes() == fwd['term'].tobytes(), (got['term'], fwd['term'])
    for g in got['grads']:                              # every element written, from either pattern
        assert g.tobytes() == want.tobytes(), int((g.view(np.uint32) != want.view(np.uint32)).sum())
    assert not got['sums'].any(), 'the closing kernel clears the sums'
    return fwd, want


@pytest.mark.parametrize('name', CASE_IDS)
def test_device_equals_the_restatement_byte_for_byte(name):
    c, mask, pol = matrix()[name]
    fwd, grad = same_as_restatement(c, mask, pol, 1.0, 0.25)
    again, grad_p = same_as_restatement(ac.permuted(c), mask, pol, 1.0, 0.25)
    for k in ('q', 's', 'base', 'count', 'rec', 'unit', 'term'):
        assert again[k].tobytes() == fwd[k].tobytes(), k
    assert grad_p.tobytes() == grad.tobytes()
    assert np.isfinite(grad).all() and np.isfinite(fwd['term'])
    if c['x'].size >= 255 and c['shape'] != (1, 1) and not name.startswith('degenerate'):
        assert fwd['count'].sum() > 0 and fwd['s'].any() and grad.any(), 'the case exercises nothing'


def test_the_cases_reach_what_they_are_there_for():
    """Host only: the classes of events, flows and images the device test relies on exist."""
    c, mask, pol = matrix()['33x31_F3_n4097_m7_p1']
    assert (c['p'] == 0).any() and (c['p'] > 0).any() and (c['p'] < 0).any()            # polarity 0 is dropped
    assert (c['x'] < 0).any() and (c['x'] >= 31).any() and (c['y'] < 0).any()           # padded -1 events
    assert np.isnan(c['flow']).any() and np.isinf(c['flow']).any() and (np.abs(c['flow']) == 1e30).any()
    fwd = L.avg_timestamp_fwd_host(*ac.args_of(c), mask, pol)
    assert len(fwd['q']) == 18 and fwd['rec']['k2'].all() and (fwd['rec']['value'] > 0).all()
    # an event on a NaN or 1e30 flow is counted at its own pixel and splats nothing
    assert fwd['count'].sum() > (fwd['q'].sum() >> 32)
    kept = mc.restricted(c, (c['p'] != 0) & (c['x'] >= 0) & (c['x'] < 31) & (c['y'] >= 0) & (c['y'] < 33))
    clean = L.avg_timestamp_fwd_host(*ac.args_of(kept), mask, pol)
    assert all(clean[k].tobytes() == fwd[k].tobytes() for k in ('q', 's', 'base', 'count', 'term'))
    one, mask, pol = matrix()['one_pixel_4097_m7_p1']
    assert L.avg_timestamp_fwd_host(*ac.args_of(one), mask, pol)['count'].max() > 1500
    deg = L.avg_timestamp_fwd_host(*ac.args_of(matrix()['degenerate_windows_m7_p1'][0]), 7, True)
    assert (deg['rec']['value'] == 0).any() and (deg['rec']['k2'] == 0).any()            # images without a gradient
    assert len(L.avg_timestamp_fwd_host(*ac.args_of(matrix()['2x3_F130_n1040_m7_p1'][0]), 7, True)['q']) == 780


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


@pytest.mark.parametrize('name', ['33x31_F3_n4097_m7_p1', '5x7_F1_n257_m5_p0', '40x40_F3_n4097_m7_p1',
                                  '2x3_F130_n1040_m7_p1'])
def test_q_and_count_are_the_bytes_of_the_contrast_call(name):
    c, mask, pol = matrix()[name]
    lib = _lib.lib()
    h, w = c['shape']
    F = len(c['fs'])
    M = F * len(ac.rhos(mask)) * (2 if pol else 1)
    d = {k: torch.from_numpy(np.array(c[k])).to(DEV) for k in ac.KEYS}
    q = torch.empty((M, h, w), dtype=torch.long, device=DEV)
    count = torch.empty((M, h, w), dtype=torch.int32, device=DEV)
    rows = torch.empty((M, 48), dtype=torch.uint8, device=DEV)
    term = torch.empty((), device=DEV)
    nbytes = lib.dvsof_contrast_multi_workspace_bytes(F, mask, int(pol), h, w)
    ws = torch.empty((nbytes // 8,), dtype=torch.long, device=DEV)
    head = [d[k].data_ptr() for k in ('x', 'y', 't', 'p', 's')] + [d['x'].numel()] + \
        [d[k].data_ptr() for k in ('ts', 'fs', 'flow')] + [F, h, w, mask, int(pol)]
    assert lib.dvsof_contrast_multi_fwd(*head, q.data_ptr(), count.data_ptr(), rows.data_ptr(), term.data_ptr(),
                                        ws.data_ptr(), nbytes, _lib.stream()) == 0
    ours = device_run(c, mask, pol, fills=())
    assert np.array_equal(ours['q'], q.cpu().numpy()) and ours['q'].any()
    assert np.array_equal(ours['count'], count.cpu().numpy().view(np.uint32))


def test_argument_rules_on_the_device_build():
    lib = _lib.lib()
    F, h, w, n = 2, 5, 7, 11
    t = dict(x=torch.zeros(n, dtype=torch.long), y=torch.zeros(n, dtype=torch.long), t=torch.zeros(n),
             p=torch.ones(n, dtype=torch.long), s=torch.zeros(n, dtype=torch.long), ts=torch.zeros(2 * F),
             fs=torch.zeros(F, dtype=torch.long), flow=torch.zeros(F, 2, h, w), term=torch.full((1,), 7.0),
             ws=torch.full((lib.dvsof_avg_timestamp_workspace_bytes(F, 7, 1, h, w),), 7, dtype=torch.uint8),
             seed=torch.ones(1), grad=torch.full((F, 2, h, w), 7.0))
    t = {k: v.to(DEV) for k, v in t.items()}
    a = {k: v.data_ptr() for k, v in t.items()}
    a['n'] = n
    seen = 0
    for what, call, expect in ac.bad_calls(lib, a, F, h, w):
        assert call() == expect, what
        seen += 1
    torch.cuda.synchronize()
    assert seen >= 55
    for k in ('term', 'ws', 'grad'):
        assert bool((t[k] == 7).all()), k               # nothing was launched
    assert all(rc == 0 for rc in ac.empty_calls(lib))
    # a null p is refused only where it would be read
    for polarity, n_, expect in ((0, n, 0), (1, 0, 0), (1, n, ac.EINVAL)):
        rc = lib.dvsof_avg_timestamp_fwd(a['x'], a['y'], a['t'], None, a['s'], n_, a['ts'], a['fs'], a['flow'], F, h,
                                         w, 7, polarity, a['term'], a['ws'], t['ws'].numel(), None)
        assert rc == expect, (polarity, n_)
    torch.cuda.synchronize()


# ------------------------------------------------------- through autograd
# the smallest frame of tests/network_cases.py; 2500 events per sample keep the
# voxeliser on its fixed-point path (4096 events and up), where the network repeats its bits
B, H, W, DEPTH, EVENTS = 2, 32, 48, 3, 2500
WEIGHT = 0.5
ALL = dict(avg_timestamp_references=('start', 'middle', 'end'), avg_timestamp_polarity=True)


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
    return dict(plain=run(), absent=run(avg_timestamp_weight=0.0), on=run(avg_timestamp_weight=WEIGHT, **ALL),
                again=run(avg_timestamp_weight=WEIGHT, **ALL), default=run(avg_timestamp_weight=WEIGHT))


def test_with_the_weight_absent_the_step_is_the_step_without_the_keyword(training_runs):
    plain, absent = training_runs['plain'], training_runs['absent']
    assert torch.equal(plain['loss'], absent['loss']) and torch.equal(plain['flow_grad'], absent['flow_grad'])
    assert plain['terms'].host() == absent['terms'].host()
    assert absent['terms'].avg_timestamp() is None and absent['terms'].contrast() is None
    assert len(plain['grads']) > 30
    for a, b in zip(plain['grads'], absent['grads']):
        assert torch.equal(a, b)


def test_the_term_reaches_the_finest_flow_by_one_add_of_the_entry_points_gradient(training_runs):
    plain, on, default = training_runs['plain'], training_runs['on'], training_runs['default']
    assert torch.equal(on['flow'], plain['flow'])               # the forward repeats its bits
    c = dict(x=on['events']['x'], y=on['events']['y'], t=on['events']['timestamp'], p=on['events']['polarity'],
             s=on['events']['sample_index'], ts=on['flow_ts'].contiguous().reshape(-1), fs=on['fsi'],
             flow=on['flow'])
    c = {k: v.cpu().numpy() for k, v in c.items()}
    c['shape'] = (H, W)
    got = device_run(c, 7, True, 1.0, WEIGHT, fills=(0xAA,))
    grad, term = got['grads'][0], got['term']
    assert got['count'].sum() == 3 * EVENTS * B and np.abs(grad).max() > 0
    want = plain['flow_grad'].cpu().numpy() + grad              # one float32 add per element
    assert want.dtype == np.float32 and on['flow_grad'].cpu().numpy().tobytes() == want.tobytes()
    # the loss is the fused loss plus weight times the logged term
    assert on['terms'].avg_timestamp() == float(term) and on['terms'].host() == plain['terms'].host()
    assert float(on['loss']) == float(np.float32(plain['loss'].item()) + np.float32(term) * np.float32(WEIGHT))
    assert any(not torch.equal(a, b) for a, b in zip(plain['grads'], on['grads']))
    assert np.isfinite(default['terms'].avg_timestamp()) and 0 < default['terms'].avg_timestamp()
    assert default['terms'].avg_timestamp() != on['terms'].avg_timestamp()
    assert not torch.equal(on['flow_grad'], default['flow_grad'])


def test_two_runs_give_the_same_bits(training_runs):
    on, again = training_runs['on'], training_runs['again']
    assert torch.equal(on['loss'], again['loss']) and torch.equal(on['flow_grad'], again['flow_grad'])
    assert on['terms'].avg_timestamp() == again['terms'].avg_timestamp()
    for a, b in zip(on['grads'], again['grads']):
        assert torch.equal(a, b)


def test_two_training_steps_on_a_frameless_recording_with_both_terms():
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.optim import FusedAdamW
    from dvs_of_training_framework_amd.sequence import EventWindowLoader, WindowedEvents
    from dvs_of_training_framework_amd.timer import FakeTimer
    from dvs_of_training_framework_amd.training import train
    from tests.test_gpu_frameless import SENSOR, WINDOWS, moving_points
    recording = WindowedEvents.cut(moving_points(), SENSOR, boundaries=np.arange(WINDOWS + 1.0))
    torch.manual_seed(0)
    model = Model(DEV, event_representation_depth=DEPTH)
    opt = FusedAdamW(model.predictor.parameters(), lr=1e-3, amsgrad=True)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
    losses = init_losses((H, W), B, model, DEV, sequence_length=1)
    loader = EventWindowLoader(recording, (H, W), batch_size=B, augmentation=True, collapse_length=3,
                               rng=np.random.default_rng(4), steps=2)
    before = [p.detach().clone() for p in model.predictor.parameters()]
    seen = {}

    class Log:
        def add_scalar(self, tag, value, x):
            seen.setdefault(tag, []).append((x, value))
    train(model, DEV, loader, opt, 2, sch, Log(), losses, timers=FakeTimer(), contrast_weight=0.25,
          avg_timestamp_weight=WEIGHT)
    torch.cuda.synchronize()
    for tag in ('General/Train loss', 'Train/avg timestamp', 'Train/contrast'):
        assert [x for x, _ in seen[tag]] == [2, 4], tag
        assert all(np.isfinite(v) for _, v in seen[tag]), tag
    assert all(v > 0 for _, v in seen['Train/avg timestamp'])
    assert any(not torch.equal(a, b) for a, b in zip(before, model.predictor.parameters()))
