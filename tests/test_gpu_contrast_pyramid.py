"""The contrast term on every flow scale on the device
(docs/CONTRAST_SPEC.md sections 19-23): dvsof_contrast_pyramid_fwd / _bwd
against the numpy restatement loss.contrast_pyramid_fwd_host / _bwd_host byte
for byte -- per level the images, counts, rows, records, units and flow
gradient, and the terms and the value --, against dvsof_contrast_multi_fwd /
_bwd on the transformed columns, the argument rules, and the term through
autograd in a training step with and without frames.

As with the one-level calls the sums cannot be read between the kernel that
fills them and the one that clears them; what is read is that they are zeros
after the forward and after the closing, and the gradient converted from them
(from buffers of 0xAA and of 0x55, and by a further backward)."""
import ctypes

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, loss as L
from tests import contrast_multi_cases as mc, contrast_pyramid_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHAPES = ((24, 40), (21, 37))
WEIGHT = 0.25


def weights_of(K, weight=WEIGHT):
    return [np.float32(weight) / np.float32(K)] * K


def same_as_restatement(c, mask, pol, seed=1.0, fills=(0xAA, 0x55)):
    w = weights_of(len(c['flows']))
    fwd = L.contrast_pyramid_fwd_host(*pc.host_args(c), c['shape'], w, mask, pol)
    want = L.contrast_pyramid_bwd_host(*pc.host_args(c), fwd, seed=seed)
    got = pc.device_run(c, mask, pol, w, seed, fills)
    assert not got['sums_after_fwd'].any(), 'the forward leaves the sums cleared'
    assert not got['sums'].any(), 'the closing kernel clears the sums'
    assert got['terms'].tobytes() == fwd['terms'].tobytes(), (got['terms'], fwd['terms'])
    assert got['value'].tobytes() == fwd['value'].tobytes(), (got['value'], fwd['value'])
    for k, (dev, host) in enumerate(zip(got['levels'], fwd['levels'])):
        assert np.array_equal(dev['q'], host['q']), (k, 'q')
        assert np.array_equal(dev['count'], host['count']), (k, 'count')
        for name in ('sum_q', 'max_q', 'count_sum', 'count_sq', 'count_max'):
            assert np.array_equal(dev['rows'][name], host['result'][name]), (k, name)
        assert dev['rows']['sum_sq'].tobytes() == host['result']['sum_sq'].tobytes(), (k, 'sum_sq')
        for i, name in enumerate(('mean', 'coef', 'gmax', 'image_term')):
            assert dev['rec'][:, i].tobytes() == host[name].tobytes(), (k, name)
        assert dev['unit'].tobytes() == host['unit'].tobytes(), (k, 'unit')
        for per_fill in got['grads']:                   # every element written, from either pattern
            assert per_fill[k].tobytes() == want[k][0].tobytes(), \
                (k, int((per_fill[k].view(np.uint32) != want[k][0].view(np.uint32)).sum()))
    return fwd, [g for g, _ in want], got


@pytest.mark.parametrize('mask,pol', pc.OPTIONS)
@pytest.mark.parametrize('shape', SHAPES)
def test_device_equals_the_restatement_byte_for_byte(shape, mask, pol):
    c = pc.device_case(shape)
    fwd, grads, _ = same_as_restatement(c, mask, pol)
    again, grads_p, _ = same_as_restatement(pc.permuted(c), mask, pol, fills=(0xAA,))
    for k in range(len(grads)):
        assert np.array_equal(again['levels'][k]['q'], fwd['levels'][k]['q'])
        assert grads_p[k].tobytes() == grads[k].tobytes()
        assert fwd['levels'][k]['count'].sum() > 0 and grads[k].any(), 'the level exercises nothing'
        assert np.isfinite(grads[k]).all()
    assert np.isfinite(fwd['terms']).all() and fwd['terms'].all()


def test_the_cases_reach_what_they_are_there_for():
    """Host only: the classes of events the device test relies on exist."""
    for shape in SHAPES:
        c = pc.device_case(shape)
        h, w = shape
        assert c['x'].size == pc.N_EVENTS and len(c['fs']) == 3 and sorted(set(c['fs'])) == [0, 1]
        assert ((c['x'] == w) & (c['y'] >= 0) & (c['y'] < h)).any() and ((c['y'] == h) & (c['x'] >= 0)).any()
        assert ((c['x'] == -1) & (c['y'] >= 0)).any() and (c['p'] == 0).any()
        assert c['ts'][1] == c['ts'][2] and (c['t'] == c['ts'][1]).any()       # an edge two frames share
    # on 21x37 an inside test made after the shift would take the events at x = w and y = h in
    assert 37 >> 1 < 19 and 21 >> 1 < 11 and 37 >> 2 < 10 and 21 >> 2 < 6


def test_seed_and_weights_reach_the_closing_kernel():
    c = pc.device_case((21, 37))
    _, a, _ = same_as_restatement(c, 7, True, seed=-1.5, fills=(0xAA,))
    _, b, _ = same_as_restatement(c, 7, True, seed=1.0, fills=(0xAA,))
    assert all(x.any() and x.tobytes() != y.tobytes() for x, y in zip(a, b))
    w = [np.float32(0.5), np.float32(0.0), np.float32(-2.0), np.float32(0.125)]
    fwd = L.contrast_pyramid_fwd_host(*pc.host_args(c), c['shape'], w, 7, True)
    want = L.contrast_pyramid_bwd_host(*pc.host_args(c), fwd)
    got = pc.device_run(c, 7, True, w, fills=(0xAA,))
    assert got['value'].tobytes() == fwd['value'].tobytes() and got['terms'].tobytes() == fwd['terms'].tobytes()
    for k in range(4):
        assert got['grads'][0][k].tobytes() == want[k][0].tobytes()
    assert not got['grads'][0][1].any() and got['grads'][0][2].any()


def test_a_second_backward_of_one_forward_gives_the_same_bytes():
    c = pc.device_case((24, 40))
    got = pc.device_run(c, 7, True, weights_of(3), fills=(0xAA, 0x55, 0x00))
    for k in range(3):
        assert got['grads'][0][k].any()
        assert got['grads'][0][k].tobytes() == got['grads'][1][k].tobytes() == got['grads'][2][k].tobytes()


@pytest.mark.parametrize('shape,mask,pol', [((24, 40), 7, True), ((21, 37), 5, False), ((21, 37), 7, True)])
def test_each_level_equals_the_one_level_calls_on_the_transformed_columns(shape, mask, pol):
    c = pc.device_case(shape)
    w = weights_of(len(c['flows']))
    got = pc.device_run(c, mask, pol, w, seed=-1.5, fills=(0xAA,))
    for k in range(len(c['flows'])):
        one = pc.multi_device_run(pc.level_case(c, k), mask, pol, w[k], seed=-1.5)
        assert np.array_equal(got['levels'][k]['q'], one['q']) and one['q'].any(), k
        assert np.array_equal(got['levels'][k]['count'], one['count']), k
        assert got['levels'][k]['rows'].tobytes() == one['rows'].tobytes(), k
        assert got['terms'][k].tobytes() == one['term'].tobytes(), k
        assert got['grads'][0][k].tobytes() == one['grad'].tobytes() and one['grad'].any(), k


@pytest.mark.parametrize('shape', SHAPES)
def test_one_level_at_full_size_equals_the_one_level_calls_on_the_untouched_columns(shape):
    full = pc.device_case(shape)
    c = dict(full, level_shapes=full['level_shapes'][:1], flows=full['flows'][:1])
    got = pc.device_run(c, 7, True, [np.float32(0.25)], seed=-1.5, fills=(0xAA,))
    one = pc.multi_device_run(dict(c, flow=c['flows'][0]), 7, True, 0.25, seed=-1.5)
    assert np.array_equal(got['levels'][0]['q'], one['q']) and np.array_equal(got['levels'][0]['count'], one['count'])
    assert got['levels'][0]['rows'].tobytes() == one['rows'].tobytes()
    assert got['terms'][0].tobytes() == one['term'].tobytes()
    assert got['value'].tobytes() == np.float32(np.float64(np.float32(0.25)) * np.float64(
        L.contrast_pyramid_fwd_host(*pc.host_args(c), c['shape'], [0.25], 7, True)['terms64'][0])).tobytes()
    assert got['grads'][0][0].tobytes() == one['grad'].tobytes() and one['grad'].any()


def test_refusals_leave_the_outputs_untouched():
    lib = _lib.lib()
    F, h, w, n, mask, pol = 2, 21, 37, 11, 7, 1
    shapes = pc.LEVELS[(21, 37)]
    K, M = len(shapes), F * 3 * 2
    t = dict(x=torch.zeros(n, dtype=torch.long), y=torch.zeros(n, dtype=torch.long), t=torch.zeros(n),
             p=torch.ones(n, dtype=torch.long), s=torch.zeros(n, dtype=torch.long), ts=torch.zeros(2 * F),
             fs=torch.zeros(F, dtype=torch.long), seed=torch.ones(1))
    t = {k: v.to(DEV) for k, v in t.items()}
    flows = [torch.zeros(F, 2, *s, device=DEV) for s in shapes]
    nan = float('nan')
    grads = [torch.full((F, 2) + s, nan, device=DEV) for s in shapes]
    rows = torch.full((K * M, 12), nan, device=DEV)
    terms, value = torch.full((K,), nan, device=DEV), torch.full((1,), nan, device=DEV)

    def table(shapes_=shapes, K_=None, **change):
        tb = L.contrast_level_table((h, w), shapes_, F, M, [0.25] * len(shapes_), [f.data_ptr() for f in flows],
                                    [g.data_ptr() for g in grads])
        for k, v in change.items():
            name, level = k.rsplit('_', 1)
            setattr(tb.level[int(level)], name, v)
        if K_ is not None:
            tb.K = K_
        return tb
    need = lib.dvsof_contrast_pyramid_workspace_bytes(F, mask, pol, h, w, table())
    assert need > 0
    ws = torch.full((need // 4,), nan, device=DEV)
    a = {k: v.data_ptr() for k, v in t.items()}

    def fwd(tb=None, F=F, h=h, w=w, n=n, mask=mask, pol=pol, nbytes=need, **null):
        p = dict(a, rows=rows.data_ptr(), terms=terms.data_ptr(), value=value.data_ptr(), ws=ws.data_ptr())
        p.update({k: None for k in null})
        return lib.dvsof_contrast_pyramid_fwd(p['x'], p['y'], p['t'], p['p'], p['s'], n, p['ts'], p['fs'], F, h, w,
                                              mask, pol, tb or table(), p['rows'], p['terms'], p['value'], p['ws'],
                                              nbytes, None)

    def bwd(tb=None, F=F, h=h, w=w, n=n, mask=mask, pol=pol, nbytes=need, **null):
        p = dict(a, ws=ws.data_ptr())
        p.update({k: None for k in null})
        return lib.dvsof_contrast_pyramid_bwd(p['x'], p['y'], p['t'], p['p'], p['s'], n, p['ts'], p['fs'], F, h, w,
                                              mask, pol, tb or table(), p['ws'], nbytes, p['seed'], None)
    EINVAL, ENOSPACE = mc.EINVAL, mc.ENOSPACE
    seen = 0
    for call in (fwd, bwd):
        for kw in (dict(F=-1), dict(F=65536), dict(F=10923), dict(n=-1), dict(mask=0), dict(mask=8), dict(pol=2),
                   dict(pol=-1), dict(h=0), dict(w=0), dict(h=32768), dict(h=22), dict(w=38),
                   dict(tb=table(K_=0)), dict(tb=table(K_=9)), dict(tb=table(K_=-1)),
                   dict(tb=table(shift_1=2)), dict(tb=table(shift_1=-1)), dict(tb=table(shift_1=16)),
                   dict(tb=table(h_2=5)), dict(tb=table(w_3=6)), dict(tb=table(h_0=0)),
                   dict(tb=table(image_offset_1=0)), dict(tb=table(row_offset_2=M)), dict(tb=table(sums_offset_3=8)),
                   dict(tb=table(flow_2=None)), dict(x=1), dict(y=1), dict(t=1), dict(p=1), dict(s=1), dict(ts=1),
                   dict(fs=1)):
            assert call(**kw) == EINVAL, (call.__name__, {k: v for k, v in kw.items() if k != 'tb'})
            seen += 1
        for kw in (dict(ws=1), dict(nbytes=need - 1), dict(nbytes=0)):
            assert call(**kw) == ENOSPACE, (call.__name__, kw)
            seen += 1
    for k in ('rows', 'terms', 'value'):
        assert fwd(**{k: 1}) == EINVAL, k
    assert bwd(seed=1) == EINVAL and bwd(tb=table(grad_flow_1=None)) == EINVAL
    assert fwd(tb=table(grad_flow_1=None), n=0) == 0            # the forward does not look at grad_flow
    # 24x40 with a level of 12x21 is no halving: refused by the table's maker and by the library
    with pytest.raises(ValueError, match='halving'):
        L.contrast_level_table((24, 40), ((24, 40), (12, 21)), F, M, [0.5, 0.5])
    torch.cuda.synchronize()
    assert seen >= 70
    terms.fill_(nan)
    value.fill_(nan)
    rows.fill_(nan)
    ws.fill_(nan)
    torch.cuda.synchronize()
    for call in (fwd, bwd):
        assert call(mask=8) == EINVAL and call(tb=table(shift_1=2)) == EINVAL and call(nbytes=need - 1) == ENOSPACE
    torch.cuda.synchronize()
    for name, buf in [('rows', rows), ('terms', terms), ('value', value), ('ws', ws)] + \
            [(f'grad {k}', g) for k, g in enumerate(grads)]:
        assert bool(torch.isnan(buf).all()), name               # nothing was launched
    # F = 0 is fine and launches nothing, with no pointer at all
    empty = _lib.ContrastLevels()
    empty.K = 1
    assert lib.dvsof_contrast_pyramid_fwd(None, None, None, None, None, 0, None, None, 0, 4, 4, 7, 1, empty, None,
                                          None, None, None, 0, None) == 0
    assert lib.dvsof_contrast_pyramid_bwd(None, None, None, None, None, 0, None, None, 0, 4, 4, 7, 1, empty, None,
                                          0, None, None) == 0
    assert ctypes.sizeof(empty) == 456


# ------------------------------------------------------- through autograd
# the smallest frame of tests/network_cases.py, as tests/test_gpu_contrast_multi.py
B, H, W, DEPTH, EVENTS = 2, 32, 48, 3, 2500
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

    def run(frameless=False, **kw):
        model.zero_grad(set_to_none=True)
        batch = synthetic.to_torch(batch_np, DEV)
        if frameless:
            batch = dict(batch, images=None, shape=(H, W))
        loss, terms, tags, out = process_minibatch(model, batch, FakeTimer(), DEV, True, ev, [0.5, 1, 1],
                                                   return_prediction=True, **kw)
        seen = {}
        for k, flow in enumerate(out['prediction']):
            flow.register_hook(lambda g, k=k: seen.__setitem__(k, g.detach().clone()))
        loss.backward()
        torch.cuda.synchronize()
        return dict(loss=loss.detach().clone(), terms=terms, tags=list(tags),
                    flows=[f.detach().clone() for f in out['prediction']],
                    flow_grads=[seen[k] for k in range(len(out['prediction']))], flow_ts=out['flow_ts'],
                    fsi=out['flow_sample_idx'], events=batch['events'],
                    grads=[p.grad.detach().clone() for p in model.parameters()])
    w = dict(contrast_weight=WEIGHT)
    return dict(shapes=ev.shapes,
                plain=run(), old=run(**w), finest=run(**w, contrast_scales='finest'),
                on=run(**w, contrast_scales='all', **ALL), again=run(**w, contrast_scales='all', **ALL),
                frameless_finest=run(True, **w, **ALL),
                frameless_all=run(True, **w, contrast_scales='all', **ALL),
                frameless_again=run(True, **w, contrast_scales='all', **ALL))


def test_finest_is_the_step_without_the_keyword(training_runs):
    old, finest = training_runs['old'], training_runs['finest']
    assert torch.equal(old['loss'], finest['loss'])
    assert len(old['grads']) > 30
    for a, b in zip(old['grads'], finest['grads']):
        assert torch.equal(a, b)
    for a, b in zip(old['flow_grads'], finest['flow_grads']):
        assert torch.equal(a, b)
    assert old['terms'].contrast() == finest['terms'].contrast() and old['terms'].contrast() is not None
    assert finest['terms'].contrast_levels() is None


def _pyramid_of(run, shapes):
    """The device calls on the flows of a run -> (grads per level, terms, value)."""
    c = dict(x=run['events']['x'], y=run['events']['y'], t=run['events']['timestamp'], p=run['events']['polarity'],
             s=run['events']['sample_index'], ts=run['flow_ts'].contiguous().reshape(-1), fs=run['fsi'])
    c = {k: v.cpu().numpy() for k, v in c.items()}
    c.update(shape=(H, W), level_shapes=tuple(shapes), flows=[f.cpu().numpy() for f in run['flows']])
    got = pc.device_run(c, 7, True, weights_of(len(shapes)), fills=(0xAA,))
    return got['grads'][0], got['terms'], got['value'], got


@pytest.mark.parametrize('base,on', [('plain', 'on'), ('frameless_finest', 'frameless_all')])
def test_the_term_reaches_every_flow_by_one_add(training_runs, base, on):
    shapes = training_runs['shapes']
    plain, run = training_runs[base], training_runs[on]
    K = len(shapes)
    assert K == 4 and shapes[-1] == (H, W)
    for a, b in zip(run['flows'], plain['flows']):
        assert torch.equal(a, b)                                # the forward repeats its bits
    grads, terms, value, got = _pyramid_of(run, shapes)
    assert got['levels'][-1]['count'].sum() == 3 * 2 * EVENTS
    if base == 'plain':
        without = plain['flow_grads']
    else:
        # the frameless loss alone (smoothness and out-of-border) on the same flows
        from dvs_of_training_framework_amd.loss import Losses
        ev = Losses(shapes, B, DEV)
        leaves = [f.clone().requires_grad_(True) for f in run['flows']]
        loss0, _ = ev.frameless(leaves, weights=(0.5, 1))
        loss0.backward()
        torch.cuda.synchronize()
        without = [f.grad for f in leaves]
    for k in range(K):
        assert np.abs(grads[k]).max() > 0, k
        want = without[k].cpu().numpy() + grads[k]              # one float32 add per element
        assert want.dtype == np.float32 and run['flow_grads'][k].cpu().numpy().tobytes() == want.tobytes(), k
    levels = run['terms'].contrast_levels()
    assert levels == [float(v) for v in terms]
    assert run['terms'].contrast() == sum(levels) / K
    assert any(not torch.equal(a, b) for a, b in zip(plain['grads'], run['grads']))
    if base == 'plain':
        assert run['terms'].host() == plain['terms'].host()
        assert float(run['loss']) == float(np.float32(plain['loss'].item()) + np.float32(value))


def test_two_runs_give_the_same_bits(training_runs):
    for a_, b_ in (('on', 'again'), ('frameless_all', 'frameless_again')):
        on, again = training_runs[a_], training_runs[b_]
        assert torch.equal(on['loss'], again['loss'])
        for a, b in zip(on['flow_grads'], again['flow_grads']):
            assert torch.equal(a, b)
        assert on['terms'].contrast_levels() == again['terms'].contrast_levels()
        for a, b in zip(on['grads'], again['grads']):
            assert torch.equal(a, b)
