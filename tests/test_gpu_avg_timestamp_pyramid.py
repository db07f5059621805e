"""The average-timestamp term on every flow scale on the device
(docs/AVG_TIMESTAMP_SPEC.md sections 11-15): dvsof_avg_timestamp_pyramid_fwd /
_bwd against the numpy restatement loss.avg_timestamp_pyramid_fwd_host /
_bwd_host byte for byte -- per level q, s, base, count, the rows, the records,
the units and the flow gradient, and the terms and the value --, against
dvsof_avg_timestamp_fwd / _bwd on the transformed columns, the edge inputs, and
the term through autograd in a training step with and without frames.

The smallest shapes that still have three and four levels, an odd size, a frame
edge two frames share, out-of-frame events and events of polarity 0: 24x40 and
21x37, F = 3 (tests/contrast_pyramid_cases.py).  No tolerances: every comparison
is of bytes.  As with the one-level calls the sums cannot be read between the
kernel that fills them and the one that clears them; what is read is that they
are zeros after the forward and after the closing, and the gradient converted
from them (from buffers of 0xAA and of 0x55, and by further backwards)."""
import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, loss as L
from tests import avg_timestamp_pyramid_cases as apc, contrast_multi_cases as mc, contrast_pyramid_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHAPES = apc.SHAPES
WEIGHT = 0.25
F32 = np.float32


def weights_of(K, weight=WEIGHT):
    return [F32(weight) / F32(K)] * K


_host = {}


def restatement(c, mask, pol, weights, seed=1.0):
    """The host restatement, computed once per (case, options, weights, seed) and left unchanged."""
    key = (id(c), mask, pol, tuple(float(w) for w in weights), seed)
    if key not in _host:
        fwd = L.avg_timestamp_pyramid_fwd_host(*pc.host_args(c), c['shape'], weights, mask, pol)
        _host[key] = (c, fwd, L.avg_timestamp_pyramid_bwd_host(*pc.host_args(c), fwd, seed=seed))
    return _host[key][1:]


def levels_equal(dev, host, k):
    for name in ('q', 's', 'base', 'count'):
        assert np.array_equal(dev[name], host[name]), (k, name)
    for name in ('n', 'n0'):
        assert np.array_equal(dev['rows'][name], host['rows'][name]), (k, name)
    for name in ('S', 'S0', 'peak'):
        assert dev['rows'][name].tobytes() == host['rows'][name].tobytes(), (k, name)
    for name in apc.REC_NAMES:
        assert dev['rec'][name].tobytes() == host['rec'][name].tobytes(), (k, name)
    assert dev['unit'].tobytes() == host['unit'].tobytes(), (k, 'unit')


def same_as_restatement(c, mask, pol, seed=1.0, fills=(0xAA, 0x55), weights=None):
    w = weights_of(len(c['flows'])) if weights is None else weights
    fwd, want = restatement(c, mask, pol, w, seed)
    got = apc.device_run(c, mask, pol, w, seed, fills)
    assert not got['sums_after_fwd'].any(), 'the forward leaves the sums cleared'
    assert not got['sums'].any(), 'the closing kernel clears the sums'
    assert got['terms'].tobytes() == fwd['terms'].tobytes(), (got['terms'], fwd['terms'])
    assert got['value'].tobytes() == fwd['value'].tobytes(), (got['value'], fwd['value'])
    for k, (dev, host) in enumerate(zip(got['levels'], fwd['levels'])):
        levels_equal(dev, host, k)
        for per_fill in got['grads']:                   # every element written, from either pattern
            assert per_fill[k].tobytes() == want[k][0].tobytes(), \
                (k, int((per_fill[k].view(np.uint32) != want[k][0].view(np.uint32)).sum()))
    return fwd, [g for g, _ in want], got


@pytest.mark.parametrize('mask,pol', pc.OPTIONS)
@pytest.mark.parametrize('shape', SHAPES)
def test_device_equals_the_restatement_byte_for_byte(shape, mask, pol):
    c = pc.device_case(shape)
    fwd, grads, got = same_as_restatement(c, mask, pol)
    # a permutation of the events gives the same bytes (the restatement is not computed again)
    perm = apc.device_run(pc.permuted(c), mask, pol, weights_of(len(c['flows'])), fills=(0xAA,))
    assert perm['terms'].tobytes() == got['terms'].tobytes() and perm['value'].tobytes() == got['value'].tobytes()
    for k in range(len(grads)):
        levels_equal(perm['levels'][k], fwd['levels'][k], k)
        assert perm['grads'][0][k].tobytes() == grads[k].tobytes()
        assert fwd['levels'][k]['count'].sum() > 0 and grads[k].any(), 'the level exercises nothing'
        assert np.isfinite(grads[k]).all()
    assert np.isfinite(fwd['terms']).all() and (fwd['terms'] != 1).all()


@pytest.mark.parametrize('shape,mask,pol', [((24, 40), 7, True), ((21, 37), 5, False), ((21, 37), 7, True)])
def test_each_level_equals_the_one_level_calls_on_the_transformed_columns(shape, mask, pol):
    c = pc.device_case(shape)
    w = weights_of(len(c['flows']))
    got = apc.device_run(c, mask, pol, w, seed=-1.5, fills=(0xAA,))
    for k in range(len(c['flows'])):
        x, y = L.contrast_level_columns(c['x'], c['y'], c['shape'], L.contrast_level_shift(c['shape'],
                                                                                            c['level_shapes'][k]))
        mine = pc.level_case(c, k)                      # the transform written out in the cases module
        assert np.array_equal(x, mine['x']) and np.array_equal(y, mine['y'])
        one = apc.one_level_device_run(mine, mask, pol, w[k], seed=-1.5)
        dev = got['levels'][k]
        for name in ('q', 's', 'base', 'count'):
            assert np.array_equal(dev[name], one[name]) and one[name].any(), (k, name)
        for name in ('rows', 'rec', 'unit'):
            assert dev[name].tobytes() == one[name].tobytes(), (k, name)
        assert got['terms'][k].tobytes() == one['term'].tobytes(), k
        assert got['grads'][0][k].tobytes() == one['grad'].tobytes() and one['grad'].any(), k


@pytest.mark.parametrize('shape', SHAPES)
def test_one_level_at_full_size_equals_the_one_level_calls_on_the_untouched_columns(shape):
    full = pc.device_case(shape)
    c = dict(full, level_shapes=full['level_shapes'][:1], flows=full['flows'][:1])
    got = apc.device_run(c, 7, True, [F32(0.25)], seed=-1.5, fills=(0xAA,))
    one = apc.one_level_device_run(dict(c, flow=c['flows'][0]), 7, True, 0.25, seed=-1.5)
    dev = got['levels'][0]
    for name in ('q', 's', 'base', 'count'):
        assert np.array_equal(dev[name], one[name]), name
    for name in ('rows', 'rec', 'unit'):
        assert dev[name].tobytes() == one[name].tobytes(), name
    assert got['terms'][0].tobytes() == one['term'].tobytes()
    fwd, _ = restatement(c, 7, True, [F32(0.25)], -1.5)
    assert got['value'].tobytes() == F32(np.float64(F32(0.25)) * fwd['terms64'][0]).tobytes()
    assert got['grads'][0][0].tobytes() == one['grad'].tobytes() and one['grad'].any()


def test_a_second_and_a_third_backward_of_one_forward_give_the_same_bytes():
    c = pc.device_case((24, 40))
    got = apc.device_run(c, 7, True, weights_of(3), fills=(0xAA, 0x55, 0x00))
    for k in range(3):
        assert got['grads'][0][k].any()
        assert got['grads'][0][k].tobytes() == got['grads'][1][k].tobytes() == got['grads'][2][k].tobytes()


def test_seed_and_weights_reach_the_closing_kernel():
    c = pc.device_case((21, 37))
    _, a, _ = same_as_restatement(c, 7, True, seed=-1.5, fills=(0xAA,))
    _, b, _ = same_as_restatement(c, 7, True, seed=1.0, fills=(0xAA,))
    assert all(x.any() and x.tobytes() != y.tobytes() for x, y in zip(a, b))
    w = [F32(0.5), F32(0.0), F32(-2.0), F32(0.125)]
    fwd, grads, got = same_as_restatement(c, 7, True, fills=(0xAA,), weights=w)
    assert not got['grads'][0][1].any() and got['grads'][0][2].any()
    even = restatement(c, 7, True, weights_of(4))[0]
    assert got['value'].tobytes() == fwd['value'].tobytes() != even['value'].tobytes()


def test_without_events_the_terms_are_zero_and_every_element_is_written():
    full = pc.device_case((21, 37))
    c = dict(full, **{k: full[k][:0] for k in ('x', 'y', 't', 'p', 's')})
    got = apc.device_run(c, 7, True, weights_of(4))
    assert got['terms'].tobytes() == np.zeros(4, F32).tobytes() and got['value'].tobytes() == F32(0).tobytes()
    for per_fill in got['grads']:
        for g in per_fill:
            assert g.tobytes() == np.zeros_like(g).tobytes()        # +0.0 from either pattern
    for lev in got['levels']:
        assert not lev['q'].any() and not lev['count'].any() and not lev['rec']['value'].any()


def test_a_padded_batch_gives_the_bytes_of_the_unpadded_one():
    c = pc.device_case((21, 37))
    pad = 517
    padded = dict(c, x=np.concatenate([c['x'], np.full(pad, -1)]), y=np.concatenate([c['y'], np.full(pad, -1)]),
                  t=np.concatenate([c['t'], np.zeros(pad, F32)]), p=np.concatenate([c['p'], np.zeros(pad, np.int64)]),
                  s=np.concatenate([c['s'], np.zeros(pad, np.int64)]))
    for mask, pol in ((5, False), (7, True)):
        a = apc.device_run(c, mask, pol, weights_of(4), fills=(0xAA,))
        b = apc.device_run(padded, mask, pol, weights_of(4), fills=(0xAA,))
        assert a['terms'].tobytes() == b['terms'].tobytes() and a['value'].tobytes() == b['value'].tobytes()
        for k in range(4):
            for name in ('q', 's', 'base', 'count', 'rows', 'rec', 'unit'):
                assert a['levels'][k][name].tobytes() == b['levels'][k][name].tobytes(), (k, name)
            assert a['grads'][0][k].tobytes() == b['grads'][0][k].tobytes()


def test_f_zero_and_a_short_workspace_touch_nothing():
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
    out = torch.full((K + 1 + 64,), nan, device=DEV)
    tb = L.contrast_level_table((h, w), shapes, F, M, [0.25] * K, [f.data_ptr() for f in flows],
                                [g.data_ptr() for g in grads])
    need = lib.dvsof_avg_timestamp_pyramid_workspace_bytes(F, mask, pol, h, w, tb)
    assert need == apc.layout(F, M, shapes)['bytes']
    ws = torch.full((need // 4 + 64,), nan, device=DEV)
    a = {k: v.data_ptr() for k, v in t.items()}

    def fwd(F=F, nbytes=need, mask=mask):
        return lib.dvsof_avg_timestamp_pyramid_fwd(a['x'], a['y'], a['t'], a['p'], a['s'], n, a['ts'], a['fs'], F, h, w,
                                                   mask, pol, tb, out.data_ptr(), out[K:].data_ptr(), ws.data_ptr(),
                                                   nbytes, None)

    def bwd(F=F, nbytes=need, mask=mask):
        return lib.dvsof_avg_timestamp_pyramid_bwd(a['x'], a['y'], a['t'], a['p'], a['s'], n, a['ts'], a['fs'], F, h, w,
                                                   mask, pol, tb, ws.data_ptr(), nbytes, a['seed'], None)
    for call in (fwd, bwd):
        assert call(F=0) == 0                                   # nothing to do
        assert call(nbytes=need - 1) == mc.ENOSPACE and call(nbytes=0) == mc.ENOSPACE
        assert call(mask=8) == mc.EINVAL
    torch.cuda.synchronize()
    for name, buf in [('out', out), ('ws', ws)] + [(f'grad {k}', g) for k, g in enumerate(grads)]:
        assert bool(torch.isnan(buf).all()), name               # nothing was launched
    # and with exactly the bytes asked for the calls run, and stay inside them
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[need // 4:]).all()) and bool(torch.isnan(out[K + 1:]).all())
    assert not bool(torch.isnan(out[:K + 1]).any()) and not any(bool(torch.isnan(g).any()) for g in grads)


# ------------------------------------------------------- through autograd
# the smallest frame of tests/network_cases.py, as tests/test_gpu_contrast_pyramid.py
B, H, W, DEPTH, EVENTS = 2, 32, 48, 3, 2500
ALL = dict(avg_timestamp_references=('start', 'middle', 'end'), avg_timestamp_polarity=True)
CONTRAST = dict(contrast_weight=0.125)          # on the finest flow: the coarser heads then have two addends


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
    w = dict(avg_timestamp_weight=WEIGHT)
    return dict(shapes=ev.shapes, evaluator=ev,
                plain=run(), old=run(**w), finest=run(**w, avg_timestamp_scales='finest'),
                on=run(**w, avg_timestamp_scales='all', **ALL), again=run(**w, avg_timestamp_scales='all', **ALL),
                frameless_base=run(True, **CONTRAST),
                frameless_all=run(True, **CONTRAST, **w, avg_timestamp_scales='all', **ALL))


def test_finest_is_the_step_without_the_keyword(training_runs):
    plain, old, finest = (training_runs[k] for k in ('plain', 'old', 'finest'))
    assert torch.equal(old['loss'], finest['loss'])
    assert len(old['grads']) > 30
    for a, b in zip(old['grads'], finest['grads']):
        assert torch.equal(a, b)
    for a, b in zip(old['flow_grads'], finest['flow_grads']):
        assert torch.equal(a, b)
    assert old['terms'].avg_timestamp() == finest['terms'].avg_timestamp() and old['terms'].avg_timestamp() is not None
    assert finest['terms'].avg_timestamp_levels() is None
    # at 'finest' only the last flow head receives the term's gradient
    changed = [not torch.equal(a, b) for a, b in zip(plain['flow_grads'], old['flow_grads'])]
    assert changed == [False] * (len(changed) - 1) + [True]


def _pyramid_of(run, shapes):
    """The device calls and the restatement on the flows of a run."""
    c = dict(x=run['events']['x'], y=run['events']['y'], t=run['events']['timestamp'], p=run['events']['polarity'],
             s=run['events']['sample_index'], ts=run['flow_ts'].contiguous().reshape(-1), fs=run['fsi'])
    c = {k: v.cpu().numpy() for k, v in c.items()}
    c.update(shape=(H, W), level_shapes=tuple(shapes), flows=[f.cpu().numpy() for f in run['flows']])
    w = weights_of(len(shapes))
    got = apc.device_run(c, 7, True, w, fills=(0xAA,))
    fwd = L.avg_timestamp_pyramid_fwd_host(*pc.host_args(c), c['shape'], w, 7, True)
    return got['grads'][0], got['terms'], got['value'], fwd


@pytest.mark.parametrize('base,on', [('plain', 'on'), ('frameless_base', 'frameless_all')])
def test_the_term_reaches_every_flow_by_one_add(training_runs, base, on):
    shapes = training_runs['shapes']
    plain, run = training_runs[base], training_runs[on]
    K = len(shapes)
    assert K == 4 and shapes[-1] == (H, W)
    for a, b in zip(run['flows'], plain['flows']):
        assert torch.equal(a, b)                                # the forward repeats its bits
    grads, terms, value, fwd = _pyramid_of(run, shapes)
    assert terms.tobytes() == fwd['terms'].tobytes() and value.tobytes() == fwd['value'].tobytes()
    for k in range(K):
        assert np.abs(grads[k]).max() > 0, k                    # every head, where 'finest' reaches the last alone
        want = [plain['flow_grads'][k].cpu().numpy() + grads[k]]    # one float32 add per element
        if base != 'plain' and k == K - 1:
            # three addends meet on the finest flow (frameless loss, contrast term, this term):
            # autograd may add them in any order, and every order is a float32 sum of the same three
            ev = training_runs['evaluator']
            pieces = []
            for term in (lambda fl: ev.frameless(fl, weights=(0.5, 1))[0],
                         lambda fl: ev.contrast(fl, run['flow_ts'], run['fsi'], run['events'],
                                                weight=CONTRAST['contrast_weight'])[0]):
                leaves = [f.clone().requires_grad_(True) for f in run['flows']]
                term(leaves).backward()
                torch.cuda.synchronize()
                pieces.append(leaves[k].grad.cpu().numpy())
            f_, c_ = pieces
            assert (f_ + c_).tobytes() == plain['flow_grads'][k].cpu().numpy().tobytes()
            want += [(grads[k] + c_) + f_, (grads[k] + f_) + c_]
        assert all(w_.dtype == np.float32 for w_ in want)
        assert run['flow_grads'][k].cpu().numpy().tobytes() in [w_.tobytes() for w_ in want], k
    levels = run['terms'].avg_timestamp_levels()
    assert levels == [float(v) for v in terms]
    assert run['terms'].avg_timestamp() == sum(levels) / K
    assert any(not torch.equal(a, b) for a, b in zip(plain['grads'], run['grads']))
    assert run['terms'].host() == plain['terms'].host()
    assert float(run['loss']) == float(np.float32(plain['loss'].item()) + np.float32(value))
    if base != 'plain':
        assert run['terms'].contrast() == plain['terms'].contrast() is not None


def test_losses_avg_timestamp_scales_gives_the_value_and_a_gradient_on_every_head(training_runs):
    ev, run, shapes = training_runs['evaluator'], training_runs['on'], training_runs['shapes']
    grads, terms, value, fwd = _pyramid_of(run, shapes)
    call = (run['flow_ts'], run['fsi'], run['events'])

    def leaves():
        return [f.clone().requires_grad_(True) for f in run['flows']]
    flows = leaves()
    got, got_terms = ev.avg_timestamp_scales(flows, *call, weight=WEIGHT, references=('start', 'middle', 'end'),
                                             polarity=True, scales='all')
    got.backward()
    torch.cuda.synchronize()
    assert got.detach().cpu().numpy().tobytes() == fwd['value'].tobytes()
    assert got_terms.cpu().numpy().tobytes() == fwd['terms'].tobytes() and not got_terms.requires_grad
    for k, f in enumerate(flows):
        assert f.grad.cpu().numpy().tobytes() == grads[k].tobytes() and grads[k].any(), k
    flows = leaves()
    one, _ = ev.avg_timestamp_scales(flows, *call, weight=WEIGHT)     # 'finest': the last head alone
    one.backward()
    assert [f.grad is not None and bool(f.grad.any()) for f in flows] == [False] * 3 + [True]
    with pytest.raises(ValueError, match='unknown avg-timestamp scales'):
        ev.avg_timestamp_scales(leaves(), *call, scales='coarsest')


def test_two_runs_give_the_same_bits(training_runs):
    on, again = training_runs['on'], training_runs['again']
    assert torch.equal(on['loss'], again['loss'])
    for a, b in zip(on['flow_grads'], again['flow_grads']):
        assert torch.equal(a, b)
    assert on['terms'].avg_timestamp_levels() == again['terms'].avg_timestamp_levels()
    for a, b in zip(on['grads'], again['grads']):
        assert torch.equal(a, b)
