"""The references of tests/head_fold_cases.py against float64 autograd through conv2d / cat /
interpolate, the range of the integer-grid cases, the paths the case tables are there for, and
the Mish yardstick of tests/test_gpu_head_fold.py.  No GPU.

K32_FWD / K32_BWD: the largest error, in the units of head_fold_cases.mish_fwd_unit /
mish_bwd_unit, of the kernels' own formulas (act_fwd / act_bwd of csrc/conv_common.h)
evaluated in NumPy float32 with every operation correctly rounded, over the sweep points in
[-87, 100].  Measured with

    python -m tests.test_head_fold_oracle

which prints them per range, ATen float32's error on the same points in the same units (for
information) and the largest partial magnitude of every integer-grid case;
test_k32_constants fails if a change of the sweep or of the formulas makes the constants too
small (or idle).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_fold_cases as hc

F32 = np.float32


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


# ---- references against autograd ---------------------------------------------------------
@pytest.mark.parametrize('act', [None, hc.ACT_NONE, hc.ACT_RELU, hc.ACT_MISH])
def test_head_references_equal_float64_autograd(act):
    d = hc.head_inputs(16, (3, 5, 7), 'rnd')
    t = lambda a: torch.tensor(a, dtype=torch.float64)       # noqa: E731
    x = t(d['x']).permute(0, 3, 1, 2).requires_grad_(True)
    w, b = t(d['w']).requires_grad_(True), t(d['bias']).requires_grad_(True)
    flow = F.conv2d(x, w[:, :, None, None], b)
    assert rel(hc.head_fwd_ref(d, True)[0], flow.detach().numpy()) < 1e-14
    assert rel(hc.head_fwd_ref(d, False)[0], (flow - b[None, :, None, None]).detach().numpy()) < 1e-14
    flow.backward(t(d['gflow']))
    s = t(d['actsrc']).requires_grad_(True)
    if act == hc.ACT_MISH:
        da = torch.autograd.grad(F.mish(s).sum(), s)[0]
    elif act == hc.ACT_RELU:
        da = (s > 0).double()
    else:
        da = torch.ones_like(s)
    for gx_in in (False, True):
        r = hc.head_bwd_ref(d, gx_in, act)
        want = (x.grad.permute(0, 2, 3, 1) + (t(d['gx_in']) if gx_in else 0)) * da.detach()
        assert rel(r['gx'], want.numpy()) < 1e-13
        assert rel(r['dw'], w.grad.numpy()) < 1e-14 and rel(r['db'], b.grad.numpy()) < 1e-14


def small_fold(layout):
    """A decoder stage in small: x, skip at 2x3, the layer on the 2x nearest upsampled
    cat of the three members in `layout` order -> (inputs dict as fold_inputs makes it,
    autograd results)."""
    B, Cx, Cs, Cout, h, w_ = 2, 3, 2, 4, 2, 3
    r = hc.rng(9, *[ord(c) for c in layout])
    t = lambda shape: torch.tensor(r.standard_normal(shape).astype(F32), dtype=torch.float64)  # noqa: E731
    x, sk = t((B, Cx, h, w_)), t((B, Cs, h, w_))
    wh, bh = t((2, Cx)).requires_grad_(True), t(2).requires_grad_(True)
    ctot = Cx + Cs + 2
    w, bias = t((Cout, ctot, 3, 3)).requires_grad_(True), t(Cout)
    flow = F.conv2d(x, wh[:, :, None, None], bh)
    members = {'x': x, 's': sk, 'f': flow}
    inp = F.interpolate(torch.cat([members[m] for m in layout], 1), scale_factor=2, mode='nearest')
    z = F.conv2d(inp, w, bias, padding=1)
    gz = t(z.shape)
    z.backward(gz)
    cx, cf, cs = hc.fold_offsets(layout, Cx, Cs)
    phys = lambda a: a.detach().permute(0, 2, 3, 1).reshape(Cout, 9, ctot).numpy()     # noqa: E731
    dW = phys(w.grad).copy()
    d = dict(Cx=Cx, Cs=Cs, Cout=Cout, B=B, H=2 * h, W=2 * w_, Ctot=ctot, cx_off=cx, cf_off=cf,
             cs_off=cs, w=phys(w), wh=wh.detach().numpy(), bh=bh.detach().numpy(),
             bias=bias.numpy(), dW=dW, g=gz.permute(0, 2, 3, 1).numpy(),
             dwh0=np.zeros((2, Cx)), dbh0=np.zeros(2), db=gz.sum((0, 2, 3)).numpy())
    auto = dict(flow_cols=dW[:, :, cf:cf + 2].copy(), dwh=wh.grad.numpy(), dbh=bh.grad.numpy(),
                z=z.detach(), x=x, sk=sk, bias=bias)
    return d, auto


@pytest.mark.parametrize('layout', ['xsf', 'fsx', 'sfx'])
def test_fold_references_equal_float64_autograd(layout):
    d, auto = small_fold(layout)
    r = hc.fold_grads_ref(d)
    assert rel(r['flow'], auto['flow_cols']) < 1e-13
    assert rel(r['dwh'], auto['dwh']) < 1e-13 and rel(r['dbh'], auto['dbh']) < 1e-13
    # forward fold: the layer on cat[x, skip] with Weff, bias_eff and the bias of the
    # pixel's border class is the layer on all three members
    weff = hc.fold_weights_ref(d)[0]
    eff, _, cls, _, _ = hc.fold_bias_ref(d, True)
    Ce = d['Ctot'] - 2
    w2 = torch.tensor(weff.reshape(d['Cout'], 3, 3, Ce)).permute(0, 3, 1, 2)
    two = [m for m in layout if m != 'f']
    inp = F.interpolate(torch.cat([{'x': auto['x'], 's': auto['sk']}[m] for m in two], 1),
                        scale_factor=2, mode='nearest')
    z2 = F.conv2d(inp, w2, torch.tensor(eff), padding=1)
    H, W = d['H'], d['W']
    cy = np.array([1 if y == 0 else 2 if y == H - 1 else 0 for y in range(H)])
    cxx = np.array([1 if x == 0 else 2 if x == W - 1 else 0 for x in range(W)])
    c = 3 * cy[:, None] + cxx[None, :]
    assert sorted(set(c.ravel())) == list(range(9))
    z2 = z2 + torch.tensor(cls[c]).permute(2, 0, 1)[None]
    assert rel(z2.numpy(), auto['z'].numpy()) < 1e-13
    assert rel(hc.fold_bias_ref(d, False)[0], eff - d['bias']) < 1e-13


def test_mish_reference_equals_float64_autograd():
    p = hc.sweep()
    p = p[np.abs(p) <= 30][::7]
    x = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    f = F.mish(x)
    d1, = torch.autograd.grad(f.sum(), x, create_graph=True)
    d2, = torch.autograd.grad(d1.sum(), x)
    g, g1, g2 = hc.mish64(p)
    # (ATen forms 1 - tanh^2 by subtraction: 1e-16 absolute, hence the absolute floors)
    assert np.abs(g - f.detach().numpy()).max() < 1e-13
    assert np.abs(g1 - d1.detach().numpy()).max() < 1e-13
    assert np.abs(g2 - d2.numpy()).max() < 1e-12
    th, q = hc.mish_parts(p)
    assert np.abs(th + p.astype(np.float64) * q - g1).max() < 1e-15


# ---- the integer grid stays exact ----------------------------------------------------------
def int_partials():
    out = {}
    for C in hc.WIDTHS:
        for shape in hc.head_shapes(C) + [hc.stride_shape(C)]:
            d = hc.head_inputs(C, shape, 'int')
            key = f'head C={C} {shape}'
            out[key + ' fwd'] = hc.head_fwd_ref(d, True)[2]
            out[key + ' bwd'] = hc.head_bwd_ref(d, True, hc.ACT_RELU)['partial']
    for name in hc.FOLD_CASES:
        d = hc.fold_inputs(name, 'int')
        out[f'fold {name} weights'] = hc.fold_weights_ref(d)[2]
        out[f'fold {name} bias'] = hc.fold_bias_ref(d, True)[4]
        out[f'fold {name} grads'] = hc.fold_grads_ref(d)['partial']
    return out


def test_integer_grid_cases_stay_below_2_24():
    for where, partial in int_partials().items():
        print(f'{where}: largest partial magnitude {partial:.0f}')
        hc.assert_exact_range(partial, where)


def test_integer_references_are_integers():
    d = hc.head_inputs(64, (3, 5, 7), 'int')
    r = hc.head_bwd_ref(d, True, hc.ACT_RELU)
    for a in (hc.head_fwd_ref(d, True)[0], r['gx'], r['dw'], r['db']):
        assert np.array_equal(a, np.rint(a))
    z = d['actsrc'].reshape(-1)
    assert (z == 0).any() and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    r = hc.fold_grads_ref(hc.fold_inputs('xsf_20_5_6x10', 'int'))
    for a in (r['flow'], r['dwh'], r['dbh']):
        assert np.array_equal(a, np.rint(a))


# ---- the tables reach the paths they name --------------------------------------------------
def test_head_tables_reach_their_paths():
    assert sorted(hc.ppw(C) for C in hc.WIDTHS) == [1, 2, 4, 8, 16]
    for C in hc.WIDTHS:
        p = hc.ppw(C)
        B, H, W = hc.stride_shape(C)
        total = B * H * W
        assert B == 3 and hc.bwd_rows(total, C) == hc.BWD_CAP and hc.bwd_iters(total, C) == 2
        assert total > 2048 * p and (p == 1 or total % p)
        assert not any(3 * hw > 2048 * p and (p == 1 or (3 * hw) % p) for hw in range(1, H * W))
        assert all(hc.bwd_rows(b * h * w, C) < hc.BWD_CAP and hc.bwd_iters(b * h * w, C) == 1
                   for b, h, w in hc.head_shapes(C))
    assert hc.stride_shape(16)[1] * hc.stride_shape(16)[2] * 3 == 32769
    blocks = lambda c: [hc.fwd_blocks(c['B'] * h * w, C) for C, h, w in c['heads']]        # noqa: E731
    assert sorted(len(c['heads']) for c in hc.HEADS_CASES.values()) == [1, 2, 3, 4, 4]
    b = blocks(hc.HEADS_CASES['n3_one_block_between'])
    assert b[1] == 1 and b[0] > 1 and b[2] > 1
    for c in hc.HEADS_CASES.values():
        assert len({(C, h, w) for C, h, w in c['heads']}) == len(c['heads'])
    full = hc.bwd_options(True)
    # gx None x dbias, and the whole cross product behind a gx
    assert len(full) == len(set(full)) == 2 + 3 * 4 * 2 * 2
    assert {o[3] for o in full if not o[0]} == {True, False}
    assert {o[1:] for o in full if o[0]} == {
        (i, a, b, h) for i in ('given', None, 'same') for a in (None, 0, 1, 2) for b in (True, False)
        for h in (True, False)}
    assert {o[1] for o in full} == {'given', None, 'same'}
    assert {o[2] for o in full} == {None, hc.ACT_NONE, hc.ACT_RELU, hc.ACT_MISH}
    for k in (0, 3, 4):
        assert {o[k] for o in full} == {True, False}
    for gx_in in ('given', None, 'same'):
        assert {o[2] for o in full if o[1] == gx_in} == {None, 0, 1, 2}


def test_fold_table_reaches_its_paths():
    cs = hc.FOLD_CASES
    both, wonly = cs['xsf_20_256_30x37'], cs['sfx_64_64_16x120']
    assert hc.takes_unrolled(both[3], both[5]) and hc.takes_unrolled(both[3], both[6])
    assert not hc.takes_unrolled(both[3], 28)       # the smallest sides at this width: 29
    assert hc.takes_unrolled(wonly[3], wonly[6]) and not hc.takes_unrolled(wonly[3], wonly[5])
    assert not any(hc.takes_unrolled(c[3], max(c[5], c[6])) for n, c in cs.items()
                   if c not in (both, wonly))
    assert {c[0] for c in cs.values()} == {'xsf', 'fsx', 'sfx'} and any(c[2] == 0 for c in cs.values())
    assert {1, 20, 64, 96} <= {c[1] for c in cs.values()}
    assert {1, 5, 32, 1030} <= {c[3] for c in cs.values()}
    assert {(1, 1), (1, 9), (9, 1), (2, 2), (6, 10)} <= {(c[5], c[6]) for c in cs.values()}
    assert {c[4] for c in cs.values()} == {1, 3}
    assert hc.fold_offsets('fsx', 20, 3) == (5, 0, 2) and hc.fold_offsets('sfx', 20, 3) == (5, 3, 0)
    assert hc.fold_offsets('xsf', 20, 3) == (0, 23, 20)


# ---- Mish yardstick --------------------------------------------------------------------------
def measure():
    """-> per-range units of the float32 emulation (fwd, bwd) and of ATen float32 (fwd, bwd)."""
    p = hc.sweep()
    d1 = hc.mish64(p)[1]
    ub = hc.mish_bwd_unit(p)
    x = torch.tensor(p, requires_grad=True)
    y = F.mish(x)
    g, = torch.autograd.grad(y.sum(), x)
    rows = []
    for fwd, got in ((True, hc.emu_mish_fwd(p)), (False, hc.emu_mish_bwd(p)), (True, y.detach().numpy()),
                     (False, g.numpy())):
        units = hc.mish_fwd_units(got, p) if fwd else np.abs(got.astype(np.float64) - d1) / ub
        rows.append(hc.units_by_range(p, units))
    return rows


def test_k32_constants():
    emu_f, emu_b, aten_f, aten_b = measure()
    for name, row in (('emulation fwd', emu_f), ('emulation bwd', emu_b), ('ATen f32 fwd', aten_f),
                      ('ATen f32 bwd', aten_b)):
        print(f'{name:14s} units per range {hc.RANGES}: ' + ' '.join(f'{v:.2f}' for v in row))
    k_f, k_b = max(emu_f[1:]), max(emu_b[1:])       # [-87, 100]
    print(f'K32_FWD measured {k_f:.3f} (constant {hc.K32_FWD}), K32_BWD measured {k_b:.3f} '
          f'(constant {hc.K32_BWD})')
    assert k_f <= hc.K32_FWD and k_b <= hc.K32_BWD
    assert k_f >= 0.5 * hc.K32_FWD and k_b >= 0.5 * hc.K32_BWD      # not idle either


def test_clamped_product_changes_no_bit_where_training_is_and_mends_the_rest():
    """act_bwd with min(s, 20) in the product: the same bits as with s itself on the whole
    sweep (|s| <= 104) and up to 1e9 (at 2e9 the term reaches half an ulp of
    th = 1 - 2^-24); beyond, the unclamped product drifted away from 1.  +inf gives what 20
    gives, NaN stays NaN."""
    p = np.concatenate([hc.sweep(), np.array([1e6, 1e8, 1e9], F32)])
    assert np.array_equal(hc.emu_mish_bwd(p).view(np.int32), hc.emu_mish_bwd(p, fixed=False).view(np.int32))
    big = hc.BWD_LARGE
    old, new = hc.emu_mish_bwd(big, fixed=False), hc.emu_mish_bwd(big)
    assert abs(float(old[big == F32(1e12)][0]) - 1.0000169) < 1e-6 and old[-2] > 1e13
    assert np.all(np.abs(new.astype(np.float64) - 1) <= hc.mish_bwd_unit(big))
    edge = hc.emu_mish_bwd(np.array([np.inf, 20, np.nan], F32))
    assert edge[0] == edge[1] and abs(float(edge[1]) - 1) <= hc.U and np.isnan(edge[2])


if __name__ == '__main__':
    test_k32_constants()
    for k, v in int_partials().items():
        print(f'{k}: largest partial magnitude {v:.0f}')
