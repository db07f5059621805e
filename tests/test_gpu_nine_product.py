"""The nine-product decoder kernels (csrc/fwd_min.hip, csrc/dgrad_min.hip):
every epilogue option against a float64 reference, the kernel each case runs
(dvsof_conv2d_last_kernel), bitwise-repeatable results, grid edges of the
persistent launches, and the pointer contract the prepared Wt / W' forms
impose (include/dvsof.h, dvsof_conv2d_fwd / _dgrad)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def close64(got, want, rtol=RTOL):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs().max().item()
    ref = want.abs().max().item()
    assert err <= rtol * ref, (err, ref)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


def from_nhwc(t):
    return t.permute(0, 3, 1, 2)


def path(kind):
    from dvs_of_training_framework_amd import conv as C
    fam, mode = C.last_kernel(kind)
    return C.KERNEL_NAMES[fam], mode


def class_bias(b_cls, Ho, Wo):
    """[9][Cout] border-class bias as a [Cout][Ho][Wo] float64 map (dvsof_conv_desc_t.bias_cls)."""
    ys, xs = torch.arange(Ho), torch.arange(Wo)
    vy = torch.where(ys == 0, 1, torch.where(ys == Ho - 1, 2, 0))
    vx = torch.where(xs == 0, 1, torch.where(xs == Wo - 1, 2, 0))
    cls = 3 * vy[:, None] + vx[None, :]
    tab = b_cls.double().clone()
    tab[0] = 0                                     # row 0 (interior) is not read
    return tab[cls].permute(2, 0, 1)


def act64(z, act):
    return F.relu(z) if act == 'relu' else F.mish(z) if act == 'mish' else z


def act_grad64(z, act):
    if act == 'relu':
        return (z > 0).double()
    z = z.detach().clone().requires_grad_(True)
    return torch.autograd.grad(F.mish(z).sum(), z)[0]


# (B, H, W, Cx, Cs, Cout, fwd family, dgrad family)
SHAPES = [
    # 4-row forward blocks (8 workgroups); dgrad_min<1> (16 items: fewer than 512)
    (2, 16, 32, 64, 64, 32, 'fwd_min4', 'dgrad_min1'),
    # 8-row blocks on 270 persistent workgroups (270 % 8 = 6: the XCD split's remainder);
    # dgrad_min<0> with 540 items over its 256 resident workgroups (uneven items per group)
    (6, 72, 80, 64, 64, 32, 'fwd_min8', 'dgrad_min0'),
    # the boundary: exactly 256 forward workgroups, exactly 512 data-gradient items
    (8, 64, 64, 64, 64, 32, 'fwd_min8', 'dgrad_min0'),
]


def _layer(B, H, W, Cx, Cs, Cout, act, seed):
    from dvs_of_training_framework_amd import conv as C
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cx, H, W, generator=g, dtype=torch.float64)
    sk = torch.randn(B, Cs, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cx + Cs, 3, 3, generator=g, dtype=torch.float64) / ((Cx + Cs) * 9) ** 0.5
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    # f32 values on both sides: the reference is float64 arithmetic on the same inputs
    x, sk, w, b = (t.float().double() for t in (x, sk, w, b))
    xd, sd = nhwc(x), nhwc(sk)
    a = {'relu': C.ACT_RELU, 'mish': C.ACT_MISH, 'none': C.ACT_NONE}[act]
    d = C.make_desc([(xd, Cx, C.NHWC), (sd, Cs, C.NHWC)], B, H, W, Cout, 3, 1, 1, True, a)
    d._keep = (xd, sd)
    return C, g, x, sk, w, b, d


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%dH%dW%d' % s[:3])
def test_fwd_min_every_epilogue_option_vs_float64(shape):
    """fwd_min (4- and 8-row blocks): with / without the z copy, with / without
    the border-class bias of a folded flow member, ReLU / Mish / none."""
    B, H, W, Cx, Cs, Cout, fam, _ = shape
    C, g, x, sk, w, b, _ = _layer(B, H, W, Cx, Cs, Cout, 'relu', seed=B * 1000 + H)
    b_cls = torch.randn(9, Cout, generator=g, dtype=torch.float64).float().double() * 0.5
    inp = F.interpolate(torch.cat([x, sk], 1), scale_factor=2, mode='nearest')
    z0 = F.conv2d(inp, w, b, padding=1)
    zc = z0 + class_bias(b_cls, 2 * H, 2 * W)[None]
    w_dev = w.float().permute(0, 2, 3, 1).contiguous().cuda()
    for act in ('relu', 'mish', 'none'):
        *_, d = _layer(B, H, W, Cx, Cs, Cout, act, seed=B * 1000 + H)
        w_f, _ = C.prepare(d, w_dev, False)
        for cls in (False, True):
            z_ref = zc if cls else z0
            y_ref = act64(z_ref, act)
            for want_z in (False, True):
                outs = []
                for _rep in range(2):
                    y, z = C.conv_fwd(d, w_f, b.float().cuda(), 'cuda', None, want_z=want_z,
                                      bias_cls=b_cls.float().cuda() if cls else None)
                    torch.cuda.synchronize()
                    assert path(0) == (fam, 0), (act, cls, want_z, path(0))
                    outs.append((y, z))
                (y, z), (y2, z2) = outs
                assert torch.equal(y, y2)
                close64(from_nhwc(y), y_ref)
                if want_z:
                    assert torch.equal(z, z2)
                    close64(from_nhwc(z), z_ref)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%dH%dW%d' % s[:3])
@pytest.mark.parametrize('act', ['relu', 'mish'])
def test_dgrad_min_every_epilogue_option_vs_float64(shape, act):
    """dgrad_min <0> / <1>: addend, addend2 and act'(actsrc) on member 0; the flow
    head on member 0 folded in (head_w / head_gflow), alone and with its own weight
    gradient from NaN-prefilled per-block partials (head_x / head_part + head_reduce)."""
    B, H, W, Cx, Cs, Cout, _, fam = shape
    C, g, x, sk, w, b, d = _layer(B, H, W, Cx, Cs, Cout, act, seed=B * 77 + H)
    x.requires_grad_(True)
    sk.requires_grad_(True)
    inp = F.interpolate(torch.cat([x, sk], 1), scale_factor=2, mode='nearest')
    z = F.conv2d(inp, w, b, padding=1)
    gz = torch.randn(z.shape, generator=g, dtype=torch.float64).float().double()
    z.backward(gz)
    gx, gs = x.grad, sk.grad
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # noqa: E731
    a1, a2, src = r(x.shape), r(x.shape), r(x.shape)
    wh, gf, hx = r(2, Cx) / Cx ** 0.5, r(B, 2, H, W), r(x.shape)
    dact = act_grad64(src, act)
    head = torch.einsum('kc,bkyx->bcyx', wh, gf)
    bact = C.ACT_RELU if act == 'relu' else C.ACT_MISH
    _, wt = C.prepare(d, w.float().permute(0, 2, 3, 1).contiguous().cuda(), True)
    gz_d, a1d, a2d, srcd = nhwc(gz), nhwc(a1), nhwc(a2), nhwc(src)
    whd, gfd, hxd = wh.float().cuda(), gf.float().cuda(), nhwc(hx)
    options = [
        ('plain', {}, gx),
        ('addend', dict(addend=a1d), gx + a1),
        ('addends+act', dict(addend=a1d, addend2=a2d, actsrc=srcd), (gx + a1 + a2) * dact),
        ('act', dict(actsrc=srcd), gx * dact),
        ('head', dict(addend=a1d, actsrc=srcd, head_w=whd, head_gflow=gfd), (gx + a1 + head) * dact),
        ('head+part', dict(addend=a1d, addend2=a2d, actsrc=srcd, head_w=whd, head_gflow=gfd, head_x=hxd),
         (gx + a1 + a2 + head) * dact),
    ]
    for name, opt, want0 in options:
        results = []
        for _rep in range(2):
            b0 = torch.full((B, H, W, Cx), float('nan'), device='cuda')
            b1 = torch.full((B, H, W, Cs), float('nan'), device='cuda')
            dst0 = dict(p=b0, **opt)
            part = None
            if 'head_x' in opt:
                part = C.dgrad_head_part(d, Cx, 'cuda')
                part.fill_(float('nan'))        # every element is written
                dst0['head_part'] = part
            C.conv_dgrad(d, wt, gz_d, [dst0, dict(p=b1)], bact)
            torch.cuda.synchronize()
            assert path(1) == (fam, 0), (name, path(1))
            results.append((b0, b1, part))
        (b0, b1, part), (b0b, b1b, partb) = results
        assert torch.equal(b0, b0b) and torch.equal(b1, b1b), name
        close64(from_nhwc(b0), want0)
        close64(from_nhwc(b1), gs)
        if part is not None:
            assert torch.equal(part, partb)
            dw = torch.empty(2, Cx, device='cuda')
            db = torch.empty(2, device='cuda')
            C.head_reduce(part, Cx, dw, db)
            close64(dw, torch.einsum('bkyx,bcyx->kc', gf, hx))
            close64(db, gf.sum((0, 2, 3)))


def test_flow_member_folded_into_weight_space_forward_on_eight_row_blocks():
    """The folded flow member's border-class bias (dvsof_flow_fold_bias) on the 8-row
    fwd_min blocks, against the unfolded layer cat[x, skip, flow] in float64."""
    from dvs_of_training_framework_amd import conv as C
    B, H, W, Cx, Cs, Cout = 6, 72, 80, 64, 64, 32
    g = torch.Generator().manual_seed(17)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # noqa: E731
    x, sk = r(B, Cx, H, W), r(B, Cs, H, W)
    wh, bh = r(2, Cx) / Cx ** 0.5, r(2)
    ctot = Cx + Cs + 2
    w, b = r(Cout, ctot, 3, 3) / (ctot * 9) ** 0.5, r(Cout)
    flow = F.conv2d(x, wh[:, :, None, None], bh)
    z_ref = F.conv2d(F.interpolate(torch.cat([x, sk, flow], 1), scale_factor=2, mode='nearest'),
                     w, b, padding=1)
    xd, sd = nhwc(x), nhwc(sk)
    w_d = w.float().permute(0, 2, 3, 1).contiguous().cuda()
    d2 = C.make_desc([(xd, Cx, C.NHWC), (sd, Cs, C.NHWC)], B, H, W, Cout, 3, 1, 1, True)
    w_eff = C.flow_fold_weights(w_d, Cout, ctot, 0, Cx, Cx + Cs, wh.float().cuda().contiguous())
    w_f, _ = C.prepare(d2, w_eff, False)
    b_eff, b_cls = C.flow_fold_bias(w_d, Cout, ctot, Cx + Cs, bh.float().cuda(), b.float().cuda())
    _, z = C.conv_fwd(d2, w_f, b_eff, 'cuda', None, want_z=True, bias_cls=b_cls)
    assert path(0) == ('fwd_min8', 0)
    close64(from_nhwc(z), z_ref)


def _lib():
    from dvs_of_training_framework_amd import _lib as L
    return L.lib()


def test_nine_product_layers_refuse_misaligned_pointers_and_a_residual():
    """Once Wt / W' are prepared no other kernel can take the layer: dvsof_conv2d_fwd /
    _dgrad return DVSOF_EINVAL on the host, before any launch, for a pointer that is
    not 16-byte aligned and for a forward residual -- and leave the outputs alone.
    (Every refused pointer is a +4-byte view inside a live allocation.)"""
    from dvs_of_training_framework_amd import conv as C
    B, H, W, Cx, Cs, Cout = 2, 8, 32, 64, 64, 32
    C, g, x, sk, w, b, d = _layer(B, H, W, Cx, Cs, Cout, 'relu', seed=3)
    w_f, wt = C.prepare(d, w.float().permute(0, 2, 3, 1).contiguous().cuda(), True)
    lib, EINVAL = _lib(), -1
    xd, sd = d._keep
    bias = torch.randn(Cout + 4, device='cuda')
    b_cls = torch.randn(9 * Cout + 4, device='cuda')
    res = torch.randn(B, 2 * H, 2 * W, Cout + 1, device='cuda')
    y = torch.full((B, 2 * H, 2 * W, Cout), float('nan'), device='cuda')
    xoff = torch.empty(xd.numel() + 4, device='cuda')
    xoff[1:1 + xd.numel()] = xd.flatten()
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)  # noqa: E731

    def fwd(src0=None, bias_p=None, cls_p=None, res_p=None):
        d.src[0].p = (src0 or p(xd)).value
        d.bias_cls = cls_p.value if cls_p is not None else None
        rc = lib.dvsof_conv2d_fwd(ctypes.byref(d), p(w_f), bias_p or p(bias), res_p, p(y), None, None)
        d.src[0].p = xd.data_ptr()
        d.bias_cls = None
        return rc
    assert fwd() == 0
    torch.cuda.synchronize()
    assert path(0) == ('fwd_min4', 0)
    y.fill_(float('nan'))
    for name, kw in (('src', dict(src0=p(xoff, 1))), ('bias', dict(bias_p=p(bias, 1))),
                     ('bias_cls', dict(cls_p=p(b_cls, 1))), ('residual', dict(res_p=p(res)))):
        assert fwd(**kw) == EINVAL, name
        assert path(0) == ('none', 0), name
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
    # data gradient: misaligned gout, addend and head_w; the destinations stay NaN
    gz = torch.randn(B * 2 * H * 2 * W * Cout + 4, device='cuda')
    add = torch.randn(B * H * W * Cx + 4, device='cuda')
    whd = torch.randn(2 * Cx + 4, device='cuda')
    gf = torch.randn(B, 2, H, W, device='cuda')
    g0 = torch.full((B, H, W, Cx), float('nan'), device='cuda')
    g1 = torch.full((B, H, W, Cs), float('nan'), device='cuda')

    def dgrad(gout=None, addend=None, head_w=None):
        arr = (C.GradDst * 2)()
        arr[0].p, arr[1].p = g0.data_ptr(), g1.data_ptr()
        arr[0].addend = addend.value if addend is not None else None
        if head_w is not None:
            arr[0].head_w, arr[0].head_gflow = head_w.value, gf.data_ptr()
        return lib.dvsof_conv2d_dgrad(ctypes.byref(d), p(wt), gout or p(gz), arr, C.ACT_NONE, None)
    for name, kw in (('gout', dict(gout=p(gz, 1))), ('addend', dict(addend=p(add, 1))),
                     ('head_w', dict(head_w=p(whd, 1)))):
        assert dgrad(**kw) == EINVAL, name
        assert path(1) == ('none', 0), name
    torch.cuda.synchronize()
    assert torch.isnan(g0).all() and torch.isnan(g1).all()
    assert dgrad() == 0
    torch.cuda.synchronize()
    assert path(1) == ('dgrad_min1', 0) and not torch.isnan(g0).any()
