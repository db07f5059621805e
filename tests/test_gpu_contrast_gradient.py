"""The gradient-magnitude objective of the contrast term on the device
(docs/CONTRAST_SPEC.md sections 27-31): against a float64 definition within the
bounds section 31 derives (and reports the observed share of), by bytes where
it is exact, and through ``Losses.contrast(objective='gradient')``.  Inputs are
dyadic (section 7): the float32 warp is exact, q is the float64 image times 2^32."""
import functools

import numpy as np
import pytest
import torch

from dvs_of_training_framework_amd import _lib, loss as L
from tests import contrast_cases as cc, contrast_multi_cases as mc

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHAPES = ((1, 1), (1, 9), (9, 1), (16, 64), (17, 65), (33, 130))    # one tile, one past a seam, two seams
OPTIONS = ((1, False), (1, True), (7, False), (7, True))            # reference mask, polarity
SEED, WEIGHT = -1.5, 0.25
REC = L.CONTRAST_GRADIENT_RECORD


@functools.lru_cache(None)
def case(shape, n=4096):
    """Two frames of two samples, the wire columns and the compact ones they stand
    for: times k/16 (frame 1 ends at 1/2: later events take no part), flows on a 2^-4
    grid that carry footprints over every border, -1 slots on every 17th event."""
    h, w = shape
    rng = np.random.default_rng([7, h, w])
    s = np.sort(rng.integers(0, 2, n))
    x, y = rng.integers(0, w, n), rng.integers(0, h, n)
    x[::17], y[::17] = -1, -1
    flow = np.round(rng.normal(0, 2.0, (2, 2, h, w)) * 16) / 16
    whole = rng.random(flow.shape) < 0.125
    flow[whole] = np.round(flow[whole])
    pol = rng.integers(0, 2, n).astype(bool)
    compact = dict(x=x.astype(np.int16), y=y.astype(np.int16), t=(rng.integers(0, 17, n) / 16).astype(np.float32),
                   pol=pol, off=np.array([0, int((s == 0).sum()), n], np.int64))
    return dict(x=x.astype(np.int64), y=y.astype(np.int64), t=compact['t'], p=pol.astype(np.int64) * 2 - 1,
                s=s.astype(np.int64), ts=np.array([0, 1, 0, 0.5], np.float32), fs=np.array([0, 1], np.int64),
                flow=flow.astype(np.float32), shape=shape, compact=compact)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def filled(nbytes):
    return torch.full(((nbytes + 7) // 8 * 8,), 0x5A, dtype=torch.uint8, device=DEV)


def run(c, mask, pol, form='', backwards=1):
    """The C calls on buffers filled with 0x5A -> host arrays; sums: after the last backward."""
    lib = _lib.lib()
    h, w = c['shape']
    F = len(c['fs'])
    M = F * len(mc.rhos(mask)) * (2 if pol else 1)
    k = c['compact']
    if form:
        cols = [dev(k['x']), dev(k['y']), dev(k['t']), dev(k['pol'].view(np.uint8)), dev(k['off'])]
        head = [t.data_ptr() for t in cols] + [len(k['off']) - 1, k['x'].size]
    else:
        cols = [dev(c[n]) for n in ('x', 'y', 't', 'p', 's')]
        head = [t.data_ptr() for t in cols] + [c['x'].size]
    tables = [dev(c['ts']), dev(c['fs']), dev(c['flow'])]
    args = head + [t.data_ptr() for t in tables] + [F, h, w, mask, int(pol)]
    nbytes = lib.dvsof_contrast_gradient_workspace_bytes(F, mask, int(pol), h, w)
    q, count, term, ws = filled(8 * M * h * w), filled(4 * M * h * w), filled(4), filled(nbytes)
    _lib.check(getattr(lib, 'dvsof_contrast_gradient_fwd' + form)(
        *args, q.data_ptr(), count.data_ptr(), term.data_ptr(), ws.data_ptr(), nbytes, None), 'fwd')
    sums, lap, rec = L.contrast_gradient_workspace(ws.view(torch.long), F, M, h, w)
    out = dict(q=q.view(torch.long).view(M, h, w).cpu().numpy(), term=term.view(torch.float32)[0].item(),
               count=count.view(torch.int32)[:M * h * w].view(M, h, w).cpu().numpy().astype(np.int64),
               lap=lap.cpu().numpy(), rec=rec.cpu().numpy().view(REC).reshape(M), grad=[])
    seed = dev(np.array([SEED], np.float32))
    for _ in range(backwards):
        grad = filled(4 * F * 2 * h * w)
        _lib.check(getattr(lib, 'dvsof_contrast_gradient_bwd' + form)(
            *args, q.data_ptr(), ws.data_ptr(), nbytes, seed.data_ptr(), WEIGHT, grad.data_ptr(), None), 'bwd')
        out['grad'].append(grad.view(torch.float32).view(F, 2, h, w).cpu().numpy())
    out['sums'] = sums.cpu().numpy()
    return out


def gm(a):        # the definition: torch float64 on the CPU, the gradient by autograd
    return ((a[:, 1:] - a[:, :-1]) ** 2).sum() + ((a[1:, :] - a[:-1, :]) ** 2).sum()


def laplacian(a):
    out = np.zeros_like(a)
    out[:, 1:] += a[:, 1:] - a[:, :-1]
    out[:, :-1] += a[:, :-1] - a[:, 1:]
    out[1:, :] += a[1:, :] - a[:-1, :]
    out[:-1, :] += a[:-1, :] - a[1:, :]
    return out


def definition(c, mask, polarity):
    """-> term, grad = d term / d flow, ratio = mean_m GM(I_m)/GM(c_m), gmax [F], k [F,h,w], gm_c, gm_i [M]."""
    h, w = c['shape']
    F, R, C = len(c['fs']), len(mc.rhos(mask)), 2 if polarity else 1
    M = F * R * C
    flow = torch.tensor(c['flow'].astype(np.float64), requires_grad=True)
    term, ratio = torch.zeros((), dtype=torch.float64), 0.0
    gmax, k, gm_c, gm_i = np.zeros(F), np.zeros((F, h, w)), np.zeros(M, np.int64), np.zeros(M)
    for r, rho in enumerate(mc.rhos(mask)):
        for ch in range(C):
            for f, p in enumerate(mc.pairs64(c, rho, mc.channel_events(c, polarity, ch))):
                m = (f * R + r) * C + ch
                x, y, sig = (torch.from_numpy(p[n]) for n in ('x', 'y', 'sig'))
                count = torch.zeros(h * w, dtype=torch.float64).index_add(
                    0, y * w + x, torch.ones(len(x), dtype=torch.float64)).view(h, w)
                np.add.at(k[f], (p['y'], p['x']), 1)
                keep = torch.from_numpy(p['inside'])
                x, y, sig = x[keep], y[keep], sig[keep]
                xw, yw = x - sig * flow[f, 0, y, x], y - sig * flow[f, 1, y, x]
                bx, by = torch.floor(xw).detach(), torch.floor(yw).detach()
                fx, fy = xw - bx, yw - by
                image = torch.zeros(h * w, dtype=torch.float64)
                for j, wy in enumerate((1 - fy, fy)):
                    for i, wx in enumerate((1 - fx, fx)):
                        px, py = (bx + i).long(), (by + j).long()
                        ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
                        image = image.index_add(0, (py * w + px)[ok], (wy * wx)[ok])
                image = image.view(h, w)
                gm_c[m], gm_i[m] = int(gm(count)), float(gm(image).detach())
                if gm_c[m] > 0:
                    term = term + (1 - gm(image) / gm_c[m])
                    ratio += gm_i[m] / gm_c[m] / M
                    gmax[f] = max(gmax[f], 2 / gm_c[m] * np.abs(laplacian(image.detach().numpy())).max())
    term = term / M
    if term.requires_grad:
        term.backward()
    grad = flow.grad.numpy() if flow.grad is not None else np.zeros(flow.shape)
    return dict(term=float(term.detach()), grad=grad, ratio=ratio, gmax=gmax, k=k, gm_c=gm_c, gm_i=gm_i, M=M)


@functools.lru_cache(None)
def oracle64(shape, mask, polarity):
    o = definition(case(shape), mask, polarity)
    assert o['gm_i'].max(initial=0) < 2.0 ** 21     # its addends lie on a 2^-32 grid: the definition's sum is exact
    return o


@pytest.mark.parametrize('mask,pol', OPTIONS)
@pytest.mark.parametrize('shape', SHAPES)
def test_the_term_and_the_gradient_against_the_float64_definition(shape, mask, pol):
    """Section 31: |term - term64| <= (2N + 8) 2^-53 mean_m(GM(I_m)/GM(c_m)) + 2^-24 |term64|; per element
    |grad - seed weight grad64| <= |seed weight| / M k 2^-36 gmax_f + 2^-22 |seed weight grad64|."""
    o, got = oracle64(shape, mask, pol), run(case(shape), mask, pol)
    N = shape[0] * shape[1]
    b_term = (2 * N + 8) * 2.0 ** -53 * o['ratio'] + 2.0 ** -24 * abs(o['term'])
    want = SEED * WEIGHT * o['grad']
    b_grad = abs(SEED * WEIGHT) / o['M'] * o['k'][:, None] * 2.0 ** -36 * o['gmax'][:, None, None, None] \
        + 2.0 ** -22 * np.abs(want)
    e_term, e_grad = np.float64(abs(got['term'] - o['term'])), np.abs(got['grad'][0].astype(np.float64) - want)
    with np.errstate(all='ignore'):
        print(f'{shape} mask {mask} pol {pol}: error/bound term {e_term / b_term:.4f} '
              f'grad {np.nanmax(np.where(b_grad > 0, e_grad / b_grad, 0)):.4f}')
    assert e_term <= b_term and (e_grad <= b_grad).all()
    assert np.array_equal(got['rec']['gm_c'].astype(np.int64), o['gm_c'])
    assert N == 1 or (np.abs(want).max() > 0 and got['term'] != 0.0)


@pytest.mark.parametrize('mask,pol', OPTIONS)
@pytest.mark.parametrize('shape', SHAPES)
def test_what_is_exact_is_exact_by_bytes(shape, mask, pol):
    """lap is the integer Laplacian of q, GM(c) the integer sum over count; a second backward, a
    permuted copy of the events and the encoded columns give the same bytes everywhere."""
    c = case(shape)
    a = run(c, mask, pol, backwards=2)
    assert a['count'].sum() > 0 and np.array_equal(a['lap'], np.stack([laplacian(q) for q in a['q']]))
    assert np.array_equal(a['rec']['gm_c'], np.array([gm(n) for n in a['count']], np.uint64))
    assert np.array_equal(a['rec']['lap_max'], np.abs(a['lap']).reshape(len(a['lap']), -1).max(1))
    flat = a['rec']['gm_c'] == 0
    assert not a['rec']['coef'][flat].any() and not a['rec']['term'][flat].any() and (a['rec']['coef'][~flat] < 0).all()
    assert not flat.all() or (a['term'] == 0.0 and not a['grad'][0].any())
    assert a['grad'][0].tobytes() == a['grad'][1].tobytes() and not a['sums'].any()
    idx = np.random.default_rng(5).permutation(c['x'].size)
    shuffled = dict(c, **{n: c[n][idx] for n in ('x', 'y', 't', 'p', 's')})
    for b in (run(shuffled, mask, pol), run(c, mask, pol, form='_encoded')):
        assert np.float32(a['term']).tobytes() == np.float32(b['term']).tobytes()
        for n in ('q', 'count', 'lap', 'rec', 'sums'):
            assert a[n].tobytes() == b[n].tobytes(), n
        assert a['grad'][0].tobytes() == b['grad'][0].tobytes()


@pytest.mark.parametrize('shape', SHAPES)
def test_a_zero_flow_gives_zero_and_a_flat_count_image_takes_no_part(shape):
    """Zero flow: q = c 2^32, GM(I) has the bits of (double) GM(c), the term is 0.0.
    Two events on every pixel under any flow: GM(c) = 0 for every image."""
    c, (h, w) = case(shape), shape
    got = run(dict(c, flow=np.zeros_like(c['flow'])), 7, True)
    assert got['rec']['gm_i'].tobytes() == got['rec']['gm_c'].astype(np.float64).tobytes()
    assert got['term'] == 0.0 and got['count'].sum() > 0
    yy, xx = (np.tile(a.ravel(), 4) for a in np.mgrid[:h, :w])
    n = xx.size
    got = run(dict(c, x=xx, y=yy, t=np.full(n, 0.25, np.float32), p=np.ones(n, np.int64),
                   s=(np.arange(n) >= n // 2).astype(np.int64)), 7, False)
    assert (got['count'] == 2).all() and not got['rec']['gm_c'].any() and not got['rec']['coef'].any()
    assert got['term'] == 0.0 and not got['grad'][0].any() and (got['rec']['gm_i'] > 0).any() == (h * w > 1)


def events_of(c, compact):
    k = c['compact']
    if compact:
        return dict(x=dev(k['x']), y=dev(k['y']), timestamp=dev(k['t']), polarity=dev(k['pol']),
                    sample_event_offsets=dev(k['off']))
    return dict(x=dev(c['x']), y=dev(c['y']), timestamp=dev(c['t']), polarity=dev(c['p']), sample_index=dev(c['s']))


@pytest.mark.parametrize('compact', (False, True))
@pytest.mark.parametrize('mask,pol', ((1, False), (7, True)))
def test_losses_contrast_with_the_gradient_objective_gives_the_bytes_of_the_calls(mask, pol, compact):
    c = case((17, 65))
    want = run(c, mask, pol)
    losses = L.Losses([c['shape']], 2, DEV)
    flow = dev(c['flow']).requires_grad_()
    names = tuple(n for b, n in enumerate(('start', 'middle', 'end')) if mask >> b & 1)
    value, term = losses.contrast([flow], dev(c['ts']), dev(c['fs']), events_of(c, compact), weight=WEIGHT,
                                  references=names, polarity=pol, objective='gradient')
    value.backward(torch.tensor(SEED, device=DEV))
    assert float(term) == want['term'] and float(value) == float(np.float32(want['term']) * np.float32(WEIGHT))
    assert flow.grad.cpu().numpy().tobytes() == want['grad'][0].tobytes()


def test_the_default_objective_is_the_call_as_it_was():
    """Without the keyword and with 'variance': the bytes of the restatement the variance kernels are pinned to."""
    c = case((17, 65))
    losses = L.Losses([c['shape']], 2, DEV)
    got = []
    for kw in ({}, {'objective': 'variance'}):
        flow = dev(c['flow']).requires_grad_()
        value, term = losses.contrast([flow], dev(c['ts']), dev(c['fs']), events_of(c, False), weight=WEIGHT,
                                      references=('start', 'end'), polarity=True, **kw)
        value.backward()
        got.append((float(term), flow.grad.cpu().numpy().tobytes()))
    assert got[0] == got[1]
    host = L.contrast_multi_fwd_host(*mc.args_of(c), references=('start', 'end'), polarity=True)
    assert got[0][0] == float(host['term'])
    assert got[0][1] == L.contrast_multi_bwd_host(*mc.args_of(c), host, weight=WEIGHT)[0].tobytes()


def test_ten_gradient_steps_on_a_translating_pattern_lower_the_term_at_every_step():
    """From half the true flow a constant flow of two parameters follows the device's gradient in steps of 0.25."""
    true = np.array([3.0, -2.0])
    p = cc.translating_pattern(flow=tuple(true))
    losses = L.Losses([p['shape']], 1, DEV)
    events = dict(x=dev(p['x']), y=dev(p['y']), timestamp=dev(p['t']), polarity=dev(np.ones_like(p['x'])),
                  sample_index=dev(p['s']))
    uv, terms = (true / 2).astype(np.float32), []
    for step in range(11):
        flow = dev(cc.constant_flow(p['shape'], uv)).requires_grad_()
        term = losses.contrast([flow], dev(p['ts']), dev(p['fs']), events, objective='gradient')
        terms.append(float(term))
        term.backward()
        uv = (uv - np.float32(0.25) * flow.grad.sum((0, 2, 3)).cpu().numpy()).astype(np.float32)
    print('terms', terms, 'flow', uv)
    assert all(b < a for a, b in zip(terms, terms[1:])) and np.linalg.norm(uv - true) < np.linalg.norm(true / 2)
