"""The census term on the device (docs/CENSUS_SPEC.md) against its definition,
items 1-6 of the spec in torch float64 on the CPU with the gradient by autograd:
the C calls on buffers filled with 0x5A, ``Losses.census`` and
``combined_loss(census_weight=)``.

Bounds: eight times the largest error observed on an MI355X over the cases
(docs/CENSUS_SPEC.md section 9 lists them), headroom for another rounding of
1/sqrt, the reciprocal, log2 and exp2; all below the project's 1e-3.  The
warped frame is exact on these inputs and is held to that."""
import functools

import pytest
import torch

from dvs_of_training_framework_amd import _lib, loss as L, training

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CASES = {'6x9': [(6, 9)], '7x7': [(7, 7)], '16x64': [(16, 64)], '17x65': [(17, 65)], '23x70': [(23, 70)],
         '33x130': [(33, 130)], 'two': [(9, 12), (17, 65)]}
N, D, START, STOP = 2, 3, (2, 0), (1, 2)
SEED, WEIGHT = -1.5, 0.25
# relative (8 x 1.42e-7), relative to the case's max |gradient| (8 x 1.24e-5); Bw of integer frames < 2^8 with
# weights that are multiples of 2^-4 is exact in float32 (every product and sum fits 24 bits): no error at all
TERM_BOUND, GRAD_BOUND, WARP_BOUND = 1.2e-6, 1e-4, 0.0


@functools.lru_cache(None)
def case(name):
    """Per level D frames of integers 0..255, frame 2 = frame 0 + 40 + noise (the
    pair of prediction 1), and flows k/16 with k odd, |k| <= 47: no sample
    position on a pixel or on the border of m, some outside the image."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    frames, flows = [], []
    for h, w in CASES[name]:
        f = torch.randint(0, 256, (D, h, w), generator=g)
        f[0].clamp_(max=210)
        f[2] = f[0] + 40 + torch.randint(-3, 4, (h, w), generator=g)
        frames.append(f.float())
        flows.append((2 * torch.randint(-24, 24, (N, 2, h, w), generator=g) + 1).float() / 16)
    return frames, flows


def definition(frames, flows, weight):
    """-> value, terms [K], d value / d flow per level, Bw per level; float64."""
    terms, warped = [], []
    flows = [f.double().requires_grad_() for f in flows]
    for fr, U in zip(frames, flows):
        fr = fr.double()
        A, B = fr[list(START)], fr[list(STOP)]
        h, w = A.shape[-2:]
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
        sx, sy = xs + U[:, 0], ys + U[:, 1]
        x0, y0 = sx.floor(), sy.floor()
        fx, fy = sx - x0, sy - y0

        def tap(yy, xx):
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            at = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).long().reshape(N, -1)
            return B.reshape(N, -1).gather(1, at).reshape(N, h, w) * ok
        Bw = (1 - fx) * (1 - fy) * tap(y0, x0) + fx * (1 - fy) * tap(y0, x0 + 1) \
            + (1 - fx) * fy * tap(y0 + 1, x0) + fx * fy * tap(y0 + 1, x0 + 1)
        warped.append(Bw.detach())
        if h < 7 or w < 7:
            terms.append(U.sum() * 0)
            continue
        m = ((sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1))[:, 3:h - 3, 3:w - 3].double()

        def ternary(img):
            diff = [img[:, dy:dy + h - 6, dx:dx + w - 6] - img[:, 3:h - 3, 3:w - 3]
                    for dy in range(7) for dx in range(7) if (dy, dx) != (3, 3)]
            diff = torch.stack(diff)
            return diff / torch.sqrt(0.81 + diff * diff)
        s = (ternary(A) - ternary(Bw)) ** 2
        dist = (s / (0.1 + s)).sum(0)
        terms.append((m * (dist ** 2 + 1e-6) ** 0.45).sum() / m.sum().clamp(min=1))
    value = weight * torch.stack(terms).mean()
    value.backward()
    return value.item(), [t.item() for t in terms], [f.grad for f in flows], warped


@functools.lru_cache(None)
def expected(name):
    return definition(*case(name), WEIGHT)


def filled(like=None, nbytes=None):
    nbytes = like.numel() * 4 if nbytes is None else nbytes
    return torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV).view(torch.float32)


def relative(got, want):
    return abs(got - want) / abs(want) if want else abs(got)


def grad_error(got, want):
    top = max(w.abs().max().item() for w in want)
    worst = max((g.double().cpu() - w).abs().max().item() for g, w in zip(got, want))
    return worst / top if top else worst


@pytest.mark.parametrize('name', CASES)
def test_the_term_and_its_gradient_against_the_definition(name):
    frames, flows = case(name)
    value, terms, grads, warped = expected(name)
    shapes, K, lib = CASES[name], len(CASES[name]), _lib.lib()
    start, stop = (torch.tensor(i, dtype=torch.int32, device=DEV) for i in (START, STOP))
    fr, fl = [f.to(DEV) for f in frames], [f.to(DEV) for f in flows]
    out = [[filled(f) for f in fl] for _ in range(2)]
    arr = [L._scale_array(fr, fl, [g.view_as(f) for g, f in zip(o, fl)]) for o in out]
    nbytes = lib.dvsof_census_workspace_bytes(arr[0], K, N)
    assert nbytes == 4 * (L.CENSUS_HEADER_WORDS + sum(2 * N * h * w for h, w in shapes))
    ws, got_terms, got_value = filled(nbytes=nbytes), filled(nbytes=4 * K), filled(nbytes=4)
    assert lib.dvsof_census_fwd(arr[0], K, N, start.data_ptr(), stop.data_ptr(), WEIGHT, got_terms.data_ptr(),
                                got_value.data_ptr(), ws.data_ptr(), nbytes - 4, None) == _lib.CONSTANTS['DVSOF_ENOSPACE']
    _lib.check(lib.dvsof_census_fwd(arr[0], K, N, start.data_ptr(), stop.data_ptr(), WEIGHT, got_terms.data_ptr(),
                                    got_value.data_ptr(), ws.data_ptr(), nbytes, None), 'dvsof_census_fwd')
    seed = torch.tensor([SEED], device=DEV)
    for a in arr:       # two backwards on the same workspace
        _lib.check(lib.dvsof_census_bwd(a, K, N, start.data_ptr(), stop.data_ptr(), seed.data_ptr(), ws.data_ptr(),
                                        nbytes, None), 'dvsof_census_bwd')
    errors = dict(
        term=max(relative(g, t) for g, t in zip(got_terms.tolist(), terms)),
        value=relative(got_value.item(), value),
        grad=grad_error([g.view_as(f) for g, f in zip(out[0], fl)], [SEED * g for g in grads]),
        warp=max((bw.double().cpu() - w).abs().max().item()
                 for (bw, _), w in zip(L.census_workspace(ws, shapes, N), warped)))
    # and through Losses.census, whose frames are the levels of the pyramid of the finest frames
    losses = L.Losses(shapes, N, DEV)
    leaves = [f.clone().requires_grad_() for f in fl]
    v, t = losses.census(leaves, None, None, fr[-1], None, None, weight=WEIGHT, frame_indices=(start, stop))
    torch.autograd.backward(v, grad_tensors=seed[0])
    pyramid = [p.cpu() for p in losses._pyramid(fl, fr[-1])]
    assert K > 1 or torch.equal(pyramid[0], frames[0])      # one level of the frames' size: the frames themselves
    value_, terms_, grads_, _ = expected(name) if K == 1 else definition(pyramid, flows, WEIGHT)
    errors.update(losses_term=max(relative(g, w) for g, w in zip(t.tolist(), terms_)),
                  losses_value=relative(v.item(), value_),
                  losses_grad=grad_error([f.grad for f in leaves], [SEED * g for g in grads_]))
    print(f'census {name}:', ' '.join(f'{k}={e:.3g}' for k, e in errors.items()))
    assert all(torch.equal(a, b) for a, b in zip(*out)), 'two backwards, different bytes'
    assert max(errors['term'], errors['value'], errors['losses_term'], errors['losses_value']) <= TERM_BOUND, errors
    assert max(errors['grad'], errors['losses_grad']) <= GRAD_BOUND and errors['warp'] <= WARP_BOUND, errors
    if name == '6x9':
        assert got_terms.tolist() == [0.0] and got_value.item() == 0.0 and not out[0][0].any()


def test_combined_loss_adds_the_weighted_mean_and_carries_the_terms():
    frames, flows = case('two')
    shapes = CASES['two']
    losses = L.Losses(shapes, N, DEV)
    images = frames[-1].to(DEV)
    indices = tuple(torch.tensor(i, dtype=torch.int32, device=DEV) for i in (START, STOP))
    leaves = [f.to(DEV).requires_grad_() for f in flows]
    call = (losses, leaves, None, None, images, None, None, None)
    plain, _ = training.combined_loss(*call, frame_indices=indices)
    zero, terms0 = training.combined_loss(*call, frame_indices=indices, census_weight=0)
    assert torch.equal(zero, plain) and not hasattr(terms0, 'census')
    loss, terms = training.combined_loss(*call, frame_indices=indices, census_weight=WEIGHT)
    pyramid = [p.cpu() for p in losses._pyramid(leaves, images)]
    value = definition(pyramid, flows, WEIGHT)[0]
    want = plain.item() + value
    # the census value within its bound, and the float32 sum's one rounding
    print(f'census combined: error={abs(loss.item() - want):.3g} value={value:.6g}')
    assert abs(loss.item() - want) <= TERM_BOUND * abs(value) + 2.0 ** -23 * abs(want)
    assert torch.equal(terms.census, losses.census(leaves, None, None, images, None, None, weight=WEIGHT,
                                                   frame_indices=indices)[1])
    assert terms.contrast is None and terms.packed is not None
