"""HIP conv stack (through the C ABI) against plain PyTorch fp32 CPU ops.
Tolerance: 1e-3 relative to the tensor's peak magnitude (north star: flow
fields within 1e-3 relative fp32); typical error is ~1e-6."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.conv_cases import (CASES, F32_ONLY, TWIN_LAYERS, WGRAD_TWIN_CASES,  # noqa: F401
                              assert_path, build, from_nhwc, nhwc, torch_fwd, wphys)

pytestmark = pytest.mark.gpu
RTOL = 1e-4


def close(got, want, rtol=RTOL):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err = (got - want).abs().max().item()
    ref = want.abs().max().item()
    assert err <= rtol * ref + 1e-7, (err, ref)


# bf16 mode: operands rounded to bf16 (2^-9 relative) inside the MFMA kernels,
# f32 accumulation and storage; bound on the error relative to the peak
BF16_RTOL = 2e-2


# bf16x3: hi/lo split operands, three products: ~2^-16 per product
BF16X3_RTOL = 1e-4


@pytest.mark.parametrize('mfma', ['f32', 'bf16', 'bf16x3'])
@pytest.mark.parametrize('ci', range(len(CASES)))
def test_conv_fwd_dgrad_wgrad(ci, mfma, close=close):
    case = CASES[ci]
    C, xs, w, b, desc, act, o = build(case, seed=ci)
    if mfma != 'f32':
        desc.mfma = C.MFMA_BF16 if mfma == 'bf16' else C.MFMA_BF16X3
        exact, tol = close, BF16_RTOL if mfma == 'bf16' else BF16X3_RTOL

        def close(got, want):                      # noqa: F811
            exact(got, want, tol)
    xs = [x.requires_grad_(True) for x in xs]
    w.requires_grad_(True)
    b.requires_grad_(True)
    ho, wo = C.out_size(desc)
    res = torch.randn(case['B'], case['Cout'], ho, wo) if case.get('residual') else None
    y_ref, z_ref = torch_fwd(xs, w, b, o, act, C, res)
    import ctypes
    first = C._lib.lib().dvsof_conv2d_kernel_generation(ctypes.byref(desc), 0) == 3
    assert first == (bool(case.get('first')) or ci == 0)       # (case 0 has the first layer's shape too)
    nscratch = C._lib.lib().dvsof_conv2d_scratch_bytes(ctypes.byref(desc))
    # the Winograd path is the one under test (bf16-rounded operands stay direct)
    assert (nscratch > 0) == (bool(case.get('wino')) and mfma != 'bf16')
    w_dev = wphys(w.detach())
    w_fwd, wt = C.prepare(desc, w_dev, True)     # sub-pixel forms for up-layers
    # (Winograd layers: the weight gradient below reuses the forward's transformed
    # input when both run the same tile form -- the last case; the others recompute)
    y, z = C.conv_fwd(desc, w_fwd, b.cuda(), 'cuda',
                      nhwc(res) if res is not None else None, want_z=True,
                      keep_input_transform=bool(case.get('wino')))
    mi = ['f32', 'bf16', 'bf16x3'].index(mfma)
    fam = case['path'][mi].split()
    assert_path(0, fam[0], mi)
    close(from_nhwc(y), y_ref)
    close(from_nhwc(z), z_ref)
    # backward w.r.t. the pre-activation output
    gz = torch.randn(z_ref.shape, generator=torch.Generator().manual_seed(99))
    z_ref.backward(gz)
    gz_d = nhwc(gz)
    ctot = sum(c for c, _ in case['src'])
    dsts, holders = [], []
    for x, (c, lay) in zip(xs, case['src']):
        buf = torch.empty(x.shape if lay == 'nchw' else
                          (x.shape[0], x.shape[2], x.shape[3], c), device='cuda')
        holders.append((buf, lay))
        dsts.append(dict(p=buf))
    C.conv_dgrad(desc, wt, gz_d, dsts)
    assert_path(1, fam[1], mi)
    for (buf, lay), x in zip(holders, xs):
        close(buf if lay == 'nchw' else from_nhwc(buf), x.grad)
    dw = torch.empty(case['Cout'], o['k'], o['k'], ctot, device='cuda')
    db = torch.empty(case['Cout'], device='cuda')
    C.conv_wgrad(desc, gz_d, dw, db)
    assert_path(2, fam[2], mi)
    close(dw.permute(0, 3, 1, 2), w.grad)
    close(db, b.grad)


@pytest.mark.parametrize('case', WGRAD_TWIN_CASES)
def test_wgrad_on_bf16_twins_equals_the_operand_mode(case):
    """mfma mode 3: the vector members' weight gradient streams the bf16 TWINS
    of gout and of the sources through LDS (ds_read_b64_tr_b16 transposed
    fragment reads, K = pixels).  Mode 1 rounds the same f32 values to bf16 in
    registers, so both multiply identical operands: equal up to f32 summation
    order.  Bias gradient: sums of the bf16-rounded gout (2^-9 per element).
    The twins are really read: built from OTHER tensors, the result is mode 1's
    on those tensors rounded to bf16 (the planar flow member has no twin)."""
    C, xs, w, b, desc, act, o = build(case, seed=11)
    ho, wo = C.out_size(desc)
    g = torch.Generator().manual_seed(5)
    gz = torch.randn(case['B'], case['Cout'], ho, wo, generator=g)
    gz_d = nhwc(gz)
    ctot = sum(c for c, _ in case['src'])
    fam3 = 'wgrad_patch' if case.get('up') else 'general_v2'
    alt = [torch.randn(t.shape, generator=g).cuda() if lay == 'nhwc' else t
           for t, (_, lay) in zip(desc._keepalive, case['src'])]
    gz_alt = torch.randn(gz_d.shape, generator=g).cuda()

    def run(mode, twins, f32=None, t16=None, gout=None, gout16=None):
        f32 = desc._keepalive if f32 is None else f32
        t16 = f32 if t16 is None else t16
        srcs = []
        for t, u, (c, lay) in zip(f32, t16, case['src']):
            u16 = u.to(torch.bfloat16) if (twins and lay == 'nhwc') else None
            srcs.append((t, c, C.NCHW if lay == 'nchw' else C.NHWC, u16))
        d = C.make_desc(srcs, case['B'], case['H'], case['W'], case['Cout'], o['k'], o['stride'],
                        o['pad'], o['up'], act, mode)
        d._keep = srcs
        dw = torch.empty(case['Cout'], o['k'], o['k'], ctot, device='cuda')
        db = torch.empty(case['Cout'], device='cuda')
        gout = gz_d if gout is None else gout
        gout16 = gout if gout16 is None else gout16
        C.conv_wgrad(d, gout, dw, db, gout16.to(torch.bfloat16) if twins else None)
        torch.cuda.synchronize()
        return dw, db
    dw1, db1 = run(C.MFMA_BF16, False)
    assert_path(2, 'general_v2', 1)
    dw3, db3 = run(C.MFMA_BF16_TWINS, True)
    assert_path(2, fam3, 3)
    close(dw3, dw1, 1e-5)
    close(db3, db1, 1e-2)
    dw3b, _ = run(C.MFMA_BF16_TWINS, True)
    assert torch.equal(dw3, dw3b)                 # fixed-order reductions
    # and both stay within the bf16 bound of the exact gradient
    dwx, _ = run(C.MFMA_F32, False)
    close(dw3, dwx, BF16_RTOL)
    # twins of other tensors: the vector members' columns follow the twins, the flat ones x
    dwd, _ = run(C.MFMA_BF16_TWINS, True, t16=alt, gout16=gz_alt)
    assert_path(2, fam3, 3)
    rounded = [t.to(torch.bfloat16).float() if lay == 'nhwc' else t
               for t, (_, lay) in zip(alt, case['src'])]
    dwr, _ = run(C.MFMA_BF16, False, f32=rounded, gout=gz_alt.to(torch.bfloat16).float())
    col = 0
    for t, (c, lay) in zip(alt, case['src']):
        if lay == 'nhwc':
            close(dwd[..., col:col + c], dwr[..., col:col + c], 1e-5)
        col += c


@pytest.mark.parametrize('B,H,W,act,cls,want_z', [
    (1, 2, 16, 'relu', False, False),       # one block: every patch row / column border at once
    (2, 8, 16, 'relu', True, True),         # border-class bias of a folded flow member, z copy
    (3, 10, 48, 'mish', True, True),        # strips shared between workgroups, ragged last range
    (8, 64, 64, 'relu', True, False),       # 512 persistent workgroups x 4 blocks
    (8, 128, 128, 'relu', False, False),    # the benchmark's finest stage: 8 blocks per workgroup
])
def test_finest_decoder_forward_on_bf16_twins_equals_the_operand_mode(B, H, W, act, cls, want_z):
    """csrc/fwd_patch.hip (mode 3, cat[x 64, skip 64] -> 32, sub-pixel phases):
    input patch resident in LDS, weights in registers.  Mode 1 rounds the same
    f32 values to bf16 in registers, so both multiply identical operands: equal
    up to f32 summation order; the bf16 twin of y is y rounded; and both stay
    within the bf16 bound of the exact layer."""
    from dvs_of_training_framework_amd import conv as C
    g = torch.Generator().manual_seed(B * 131 + H)
    x = nhwc(torch.randn(B, 64, H, W, generator=g))
    sk = nhwc(torch.randn(B, 64, H, W, generator=g))
    w = wphys(torch.randn(32, 128, 3, 3, generator=g) / (128 * 9) ** 0.5)
    b = torch.randn(32, generator=g).cuda()
    b_cls = (torch.randn(9, 32, generator=g).cuda() * 0.3) if cls else None
    a = {'relu': C.ACT_RELU, 'mish': C.ACT_MISH}[act]

    def run(mode, srcs=(x, sk), twin_srcs=None, w_twin=None, w_f32=w):
        twins = mode == C.MFMA_BF16_TWINS
        twin_srcs = srcs if twin_srcs is None else twin_srcs
        s = [(t, 64, C.NHWC, u.to(torch.bfloat16) if twins else None) for t, u in zip(srcs, twin_srcs)]
        d = C.make_desc(s, B, H, W, 32, 3, 1, 1, True, a, mode)
        d._keep = s
        if twins:
            w_f, _, w_f16, _ = C.prepare(d, w_f32, False, want16=True)
            if w_twin is not None:      # the twin of another weight's forward form
                w_f16 = C.prepare(d, w_twin, False, want16=True)[2]
        else:
            (w_f, _), w_f16 = C.prepare(d, w_f32, False), None
        y, z = C.conv_fwd(d, w_f, b, 'cuda', None, want_z=want_z, weight16=w_f16, bias_cls=b_cls)
        torch.cuda.synchronize()
        return y, z, d._y16
    y1, z1, _ = run(C.MFMA_BF16)
    assert_path(0, 'general_v2', 1)
    y3, z3, y16 = run(C.MFMA_BF16_TWINS)
    assert_path(0, 'fwd_patch', 3)
    close(y3, y1, 1e-5)
    if want_z:
        close(z3, z1, 1e-5)
    assert torch.equal(y16.view(y3.shape), y3.to(torch.bfloat16))
    y3b, _, _ = run(C.MFMA_BF16_TWINS)
    assert torch.equal(y3, y3b)
    yx, _, _ = run(C.MFMA_F32)
    close(y3, yx, BF16_RTOL)
    # twins of OTHER tensors (sources and weights): the result follows the twins -- mode 1 on
    # the twins' values (the weight form of w2 rounds to the same bf16 in both)
    x2, sk2 = (nhwc(torch.randn(B, 64, H, W, generator=g)) for _ in range(2))
    w2 = wphys(torch.randn(32, 128, 3, 3, generator=g) / (128 * 9) ** 0.5)
    yd, zd, yd16 = run(C.MFMA_BF16_TWINS, twin_srcs=(x2, sk2), w_twin=w2)
    assert_path(0, 'fwd_patch', 3)
    yr, zr, _ = run(C.MFMA_BF16, srcs=(x2.to(torch.bfloat16).float(), sk2.to(torch.bfloat16).float()),
                    w_f32=w2)
    close(yd, yr, 1e-5)
    if want_z:
        close(zd, zr, 1e-5)
    assert torch.equal(yd16.view(yd.shape), yd.to(torch.bfloat16))


@pytest.mark.parametrize('B,H,W,Cx,Cs,Cout', [
    (2, 8, 8, 32, 32, 32),
    (3, 6, 10, 64, 32, 64),          # odd frame sides, unequal members
    (8, 32, 32, 64, 64, 32),         # a decoder-stage shape (K splits, sub-pixel fold)
])
def test_flow_member_folded_into_weight_space(B, H, W, Cx, Cs, Cout):
    """Backward of a decoder stage whose input is cat[x, skip, flow] with
    flow = Wh x + bh (the previous stage's head): the data gradient on
    cat[x, skip] with the folded weights, the weight gradient with the flow
    columns derived from the x columns + border sums, and the head's gradient
    additions (csrc/flowfold.hip) against ATen autograd through
    cat / interpolate / conv2d."""
    from dvs_of_training_framework_amd import conv as C
    g = torch.Generator().manual_seed(B * 7 + Cout)
    x = torch.randn(B, Cx, H, W, generator=g, requires_grad=True)
    sk = torch.randn(B, Cs, H, W, generator=g, requires_grad=True)
    wh = (torch.randn(2, Cx, generator=g) / Cx ** 0.5).requires_grad_(True)
    bh = torch.randn(2, generator=g, requires_grad=True)
    ctot = Cx + Cs + 2
    w = (torch.randn(Cout, ctot, 3, 3, generator=g) / (ctot * 9) ** 0.5).requires_grad_(True)
    b = torch.randn(Cout, generator=g, requires_grad=True)
    flow = F.conv2d(x, wh[:, :, None, None], bh)
    inp = F.interpolate(torch.cat([x, sk, flow], 1), scale_factor=2, mode='nearest')
    z = F.conv2d(inp, w, b, padding=1)
    gz = torch.randn(z.shape, generator=g)
    z.backward(gz)

    x_d, sk_d = nhwc(x.detach()), nhwc(sk.detach())
    flow_d = flow.detach().cuda().contiguous()
    w_d, wh_d, bh_d = wphys(w.detach()), wh.detach().cuda().contiguous(), bh.detach().cuda()
    gz_d = nhwc(gz)
    # data gradient: two vector members, folded weights
    d2 = C.make_desc([(x_d, Cx, C.NHWC), (sk_d, Cs, C.NHWC)], B, H, W, Cout, 3, 1, 1, True)
    w_eff = C.flow_fold_weights(w_d, Cout, ctot, 0, Cx, Cx + Cs, wh_d)
    w_f, w_dg = C.prepare(d2, w_eff, True)
    # forward on cat[x, skip]: the head's bias arrives through the in-frame flow
    # taps only -> a bias per border class of the output pixel
    b_eff, b_cls = C.flow_fold_bias(w_d, Cout, ctot, Cx + Cs, bh_d, b.detach().cuda())
    y_f, z_f = C.conv_fwd(d2, w_f, b_eff, 'cuda', None, want_z=True, bias_cls=b_cls)
    close(from_nhwc(z_f), z)
    d3f = C.make_desc([(x_d, Cx, C.NHWC), (sk_d, Cs, C.NHWC), (flow_d, 2, C.NCHW)], B, H, W, Cout,
                      3, 1, 1, True)
    w_f3, _ = C.prepare(d3f, w_d, False)
    _, z_3 = C.conv_fwd(d3f, w_f3, b.detach().cuda(), 'cuda', None, want_z=True)
    close(from_nhwc(z_f), from_nhwc(z_3), 1e-5)
    gx = torch.empty(B, H, W, Cx, device='cuda')
    gs = torch.empty(B, H, W, Cs, device='cuda')
    C.conv_dgrad(d2, w_dg, gz_d, [dict(p=gx), dict(p=gs)])
    close(from_nhwc(gx), x.grad)          # includes the path through the flow head
    close(from_nhwc(gs), sk.grad)
    # weight gradient: vector members on the matrix cores, flow columns in weight space
    d3 = C.make_desc([(x_d, Cx, C.NHWC), (sk_d, Cs, C.NHWC), (flow_d, 2, C.NCHW)], B, H, W, Cout,
                     3, 1, 1, True)
    dw = torch.full((Cout, 3, 3, ctot), float('nan'), device='cuda')
    db = torch.empty(Cout, device='cuda')
    C.conv_wgrad(d3, gz_d, dw, db, skip_flat=True)
    dwh = torch.zeros(2, Cx, device='cuda')
    dbh = torch.zeros(2, device='cuda')
    C.flow_fold_grads(dw, w_d, Cout, ctot, 0, Cx, Cx + Cs, wh_d, bh_d, db, gz_d, B, 2 * H, 2 * W,
                      dwh, dbh)
    close(dw.permute(0, 3, 1, 2), w.grad)
    close(db, b.grad)
    close(dwh, wh.grad)
    close(dbh, bh.grad)
    # the unfused path (flat-member kernels) gives the same weight gradient
    dw2 = torch.empty(Cout, 3, 3, ctot, device='cuda')
    C.conv_wgrad(d3, gz_d, dw2, db)
    close(dw, dw2, 1e-5)


@pytest.mark.parametrize('B,H,W,Cin,Cout,act', [
    (2, 8, 12, 32, 64, 'relu'),
    (1, 5, 7, 64, 48, 'mish'),        # odd sizes, Cout not a tile multiple
    (8, 32, 32, 128, 64, 'relu'),     # a decoder-stage shape
])
def test_transposed_conv_layer(B, H, W, Cin, Cout, act):
    """upsample = UP_ZERO: 2x zero insertion + 3x3/pad 1 = transposed
    convolution with stride 2 (north star: "strided conv / transposed-conv /
    Mish stack"), run as four output-parity phases on the matrix cores.
    Forward, data gradient (a stride-2 convolution of the output gradient) and
    weight / bias gradient (the adjoint stride-2 layer's, flip-transposed)
    against ATen on the zero-inserted input and against conv_transpose2d."""
    from dvs_of_training_framework_amd import conv as C
    g = torch.Generator().manual_seed(B * 100 + H)
    a = {'relu': C.ACT_RELU, 'mish': C.ACT_MISH}[act]
    x = torch.randn(B, Cin, H, W, generator=g, requires_grad=True)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).requires_grad_(True)
    b = torch.randn(Cout, generator=g, requires_grad=True)
    xw = torch.stack([x, torch.zeros_like(x)], dim=-1).reshape(B, Cin, H, 2 * W)
    xz = torch.stack([xw, torch.zeros_like(xw)], dim=-2).reshape(B, Cin, 2 * H, 2 * W)
    assert torch.equal(xz[:, :, ::2, ::2], x) and int((xz != 0).sum()) == int((x != 0).sum())
    z_ref = F.conv2d(xz, w, b, padding=1)
    z_t = F.conv_transpose2d(x, w.flip(2, 3).transpose(0, 1), b, stride=2, padding=1,
                             output_padding=1)
    close(z_t, z_ref, 1e-5)       # the layer IS conv_transpose2d (flipped kernel)
    y_ref = F.relu(z_ref) if act == 'relu' else F.mish(z_ref)
    x_d = nhwc(x.detach())
    desc = C.make_desc([(x_d, Cin, C.NHWC)], B, H, W, Cout, 3, 1, 1, C.UP_ZERO, a)
    assert C.out_size(desc) == (2 * H, 2 * W)
    w_fwd, w_dg = C.prepare(desc, wphys(w.detach()), True)
    assert w_fwd.numel() == 16 * Cout * Cin and w_dg.numel() == 9 * Cout * Cin
    y, z = C.conv_fwd(desc, w_fwd, b.detach().cuda(), 'cuda', None, want_z=True)
    assert_path(0, 'transposed', 0)
    close(from_nhwc(z), z_ref)
    close(from_nhwc(y), y_ref)
    gz = torch.randn(z_ref.shape, generator=g)
    z_ref.backward(gz)
    gz_d = nhwc(gz)
    gx = torch.empty(B, H, W, Cin, device='cuda')
    C.conv_dgrad(desc, w_dg, gz_d, [dict(p=gx)])
    assert_path(1, 'general_v2', 0)       # a plain stride-2 convolution of gout
    close(from_nhwc(gx), x.grad)
    dw = torch.empty(Cout, 3, 3, Cin, device='cuda')
    db = torch.empty(Cout, device='cuda')
    C.conv_wgrad(desc, gz_d, dw, db)
    close(dw.permute(0, 3, 1, 2), w.grad)
    close(db, b.grad)


def test_transposed_conv_rejects_what_it_does_not_implement():
    from dvs_of_training_framework_amd import conv as C
    x = torch.zeros(1, 4, 4, 32, device='cuda')
    for bad in (dict(ksize=5, pad=2), dict(stride=2)):
        kw = dict(ksize=3, stride=1, pad=1)
        kw.update(bad)
        d = C.make_desc([(x, 32, C.NHWC)], 1, 4, 4, 32, upsample=C.UP_ZERO, **kw)
        with pytest.raises(RuntimeError):
            C.conv_fwd(d, torch.zeros(32 * 16 * 32, device='cuda'), None, 'cuda')
    x5 = torch.zeros(1, 5, 4, 4, device='cuda')      # planar 5-channel source
    d = C.make_desc([(x5, 5, C.NCHW)], 1, 4, 4, 32, upsample=C.UP_ZERO)
    with pytest.raises(RuntimeError):
        C.conv_fwd(d, torch.zeros(32 * 16 * 5, device='cuda'), None, 'cuda')


@pytest.mark.parametrize('case', [
    dict(B=2, H=8, W=8, src=[(32, 'nhwc')], Cout=64, stride=2),
    dict(B=8, H=16, W=8, src=[(256, 'nhwc')], Cout=256, stride=1),     # Winograd F(4x4,3x3)
])
def test_dgrad_epilogue_addends_and_act(case):
    from dvs_of_training_framework_amd import conv as C
    C, xs, w, b, desc, act, o = build(case, seed=3)
    x = xs[0].requires_grad_(True)
    _, z_ref = torch_fwd([x], w, b, o, act, C)
    gz = torch.randn(z_ref.shape)
    z_ref.backward(gz)
    a1, a2 = torch.randn(x.shape), torch.randn(x.shape)
    ysrc = torch.randn(x.shape)
    want = (x.grad + a1 + a2) * (ysrc > 0).float()
    buf = torch.empty(case['B'], case['H'], case['W'], case['src'][0][0], device='cuda')
    _, wt = C.prepare(desc, wphys(w), True)
    C.conv_dgrad(desc, wt, nhwc(gz), [dict(p=buf, addend=nhwc(a1), addend2=nhwc(a2),
                                           actsrc=nhwc(ysrc))], C.ACT_RELU)
    close(from_nhwc(buf), want)


def test_decoder_dgrad_nine_product_form_epilogue():
    """csrc/dgrad_min.hip (two members of 64 | C, 8 | H): the gradient lands in
    the member its channel tile belongs to; addends and act' on one member only
    (the decoder's first stage: x = the last residual output)."""
    from dvs_of_training_framework_amd import conv as C
    case = dict(B=2, H=16, W=32, src=[(128, 'nhwc'), (64, 'nhwc')], Cout=48 + 16, up=True)
    C, xs, w, b, desc, act, o = build(case, seed=5)
    xs = [x.requires_grad_(True) for x in xs]
    _, z_ref = torch_fwd(xs, w, b, o, act, C)
    gz = torch.randn(z_ref.shape)
    z_ref.backward(gz)
    a1, a2, ysrc = (torch.randn(xs[0].shape) for _ in range(3))
    want0 = (xs[0].grad + a1 + a2) * (ysrc > 0).float()
    bufs = [torch.empty(2, 16, 32, c, device='cuda') for c, _ in case['src']]
    _, wt = C.prepare(desc, wphys(w), True)
    C.conv_dgrad(desc, wt, nhwc(gz), [dict(p=bufs[0], addend=nhwc(a1), addend2=nhwc(a2),
                                           actsrc=nhwc(ysrc)), dict(p=bufs[1])], C.ACT_RELU)
    close(from_nhwc(bufs[0]), want0)
    close(from_nhwc(bufs[1]), xs[1].grad)
    # a flow head on member 0 folded into the epilogue (dvsof_grad_dst_t.head_w):
    # + W_h^T g_flow ahead of act'; the head's own weight gradient with gx=None
    assert C.dgrad_fuses_head(desc)
    wh, gf = torch.randn(2, 128) / 8, torch.randn(2, 2, 16, 32)
    want_h = (xs[0].grad + a1 + torch.einsum('kc,bkyx->bcyx', wh, gf)) * (ysrc > 0).float()
    C.conv_dgrad(desc, wt, nhwc(gz), [dict(p=bufs[0], addend=nhwc(a1), actsrc=nhwc(ysrc),
                                           head_w=wh.cuda(), head_gflow=gf.cuda()),
                                      dict(p=bufs[1])], C.ACT_RELU)
    close(from_nhwc(bufs[0]), want_h)
    close(from_nhwc(bufs[1]), xs[1].grad)
    dw, db = torch.empty(2, 128, device='cuda'), torch.empty(2, device='cuda')
    C.head_bwd(nhwc(ysrc), wh.cuda(), gf.cuda(), None, None, C.ACT_RELU, None, dw, db,
               2, 16, 32, 128)
    close(dw, torch.einsum('bkyx,bcyx->kc', gf, ysrc))
    close(db, gf.sum((0, 2, 3)))
    # ... or from per-block partials the same epilogue leaves (head_x / head_part), with the
    # head's input apart from actsrc (Mish) and the same tensor (ReLU)
    for hx in (torch.randn(ysrc.shape), ysrc):
        part = C.dgrad_head_part(desc, 128, 'cuda')
        assert part is not None and part.shape == (2 * (16 // 8) * (32 // 16), 2 * 128 + 2)
        part.fill_(float('nan'))        # every element is written
        hx_d = nhwc(hx)
        as_d = nhwc(ysrc) if hx is not ysrc else hx_d
        C.conv_dgrad(desc, wt, nhwc(gz), [dict(p=bufs[0], addend=nhwc(a1), actsrc=as_d,
                                               head_w=wh.cuda(), head_gflow=gf.cuda(),
                                               head_x=hx_d, head_part=part),
                                          dict(p=bufs[1])], C.ACT_RELU)
        close(from_nhwc(bufs[0]), want_h)
        dw2, db2 = torch.empty(2, 128, device='cuda'), torch.empty(2, device='cuda')
        C.head_reduce(part, 128, dw2, db2)
        close(dw2, torch.einsum('bkyx,bcyx->kc', gf, hx))
        close(db2, gf.sum((0, 2, 3)))
    # the same fold in the general kernels' epilogue (here: bf16 operands, where the layer's data
    # gradient is the 4x4 stride-2 form on gconv2) -- and with a third, planar member beside it
    desc.mfma = C.MFMA_BF16
    assert C.dgrad_fuses_head(desc)
    _, wt16 = C.prepare(desc, wphys(w), True)
    C.conv_dgrad(desc, wt16, nhwc(gz), [dict(p=bufs[0], addend=nhwc(a1), actsrc=nhwc(ysrc),
                                             head_w=wh.cuda(), head_gflow=gf.cuda()),
                                        dict(p=bufs[1])], C.ACT_RELU)
    close(from_nhwc(bufs[0]), want_h, BF16_RTOL)
    close(from_nhwc(bufs[1]), xs[1].grad, BF16_RTOL)
    desc.mfma = C.MFMA_F32
    # ... and refused where the kernel is another one (here: stride 1, no up-sampling)
    case2 = dict(B=1, H=8, W=16, src=[(64, 'nhwc')], Cout=64, up=False)
    C2, xs2, w2, b2, desc2, act2, o2 = build(case2, seed=6)
    assert not C.dgrad_fuses_head(desc2)
    _, wt2 = C.prepare(desc2, wphys(w2), True)
    with pytest.raises(Exception):
        C.conv_dgrad(desc2, wt2, torch.zeros(1, 8, 16, 64, device='cuda'),
                     [dict(p=torch.empty(1, 8, 16, 64, device='cuda'), head_w=wh.cuda(),
                           head_gflow=gf.cuda())], C.ACT_RELU)


@pytest.mark.parametrize('B,H,W', [(8, 16, 16), (4, 8, 32), (2, 24, 32)])
def test_winograd_chain_forms_are_the_consumers_own(B, H, W):
    """dvsof_conv_desc_t.winograd_next / winograd_next_gout / winograd_pre /
    winograd_gout (csrc/winograd.hip wino_chain_kernel): a Winograd layer's
    output transform also writes its consumer's transformed input and gradient
    form.  Bitwise the same outputs, gradients and weight gradients as the
    three separate transforms -- forward with residual and Mish (pre-activation
    copy), data gradient with addend and act'."""
    from dvs_of_training_framework_amd import conv as C
    Cc = 256
    case = dict(B=B, H=H, W=W, src=[(Cc, 'nhwc')], Cout=Cc, stride=1, act='mish')
    C, xs, w1, b1, d1, act, o = build(case, seed=3)
    _, _, w2, b2, d2, _, _ = build(case, seed=4)
    assert C.winograd_tile(d1, 0) == 4 and C.winograd_chain(d1, 0) and C.winograd_chain(d1, 1)
    dev = 'cuda'
    u1, u1t = C.prepare(d1, wphys(w1), True)
    u2, u2t = C.prepare(d2, wphys(w2), True)
    res = nhwc(torch.randn(B, Cc, H, W))

    def layer2_src(y):      # layer 2 reads layer 1's output
        d2.src[0].p = y.data_ptr()
        return y
    # ---- plain: every call makes its own transforms
    y1, z1 = C.conv_fwd(d1, u1, b1.cuda(), dev, residual=res, want_z=True, keep_input_transform=True)
    layer2_src(y1)
    y2, _ = C.conv_fwd(d2, u2, b2.cuda(), dev, keep_input_transform=True)
    g2 = nhwc(torch.randn(B, Cc, H, W))
    add = nhwc(torch.randn(B, Cc, H, W))
    g1 = torch.empty_like(y1)
    C.conv_dgrad(d2, u2t, g2, [dict(p=g1, addend=add, actsrc=z1)], act)
    dw1, db1 = torch.empty(Cc * 9 * Cc, device=dev), torch.empty(Cc, device=dev)
    C.conv_wgrad(d1, g1, dw1, db1)
    g0 = torch.empty_like(y1)
    C.conv_dgrad(d1, u1t, g1, [dict(p=g0)], act)
    # ---- chained
    v2 = C.winograd_form(d1, Cc, dev)
    y1c, z1c = C.conv_fwd(d1, u1, b1.cuda(), dev, residual=res, want_z=True,
                          keep_input_transform=True, wino_next=v2)
    layer2_src(y1c)
    y2c, _ = C.conv_fwd(d2, u2, b2.cuda(), dev, keep_input_transform=True, wino_pre=v2)
    vg, zg = C.winograd_form(d2, Cc, dev), C.winograd_form(d2, Cc, dev)
    g1c = torch.empty_like(y1)
    C.conv_dgrad(d2, u2t, g2, [dict(p=g1c, addend=add, actsrc=z1c)], act,
                 wino_next=vg, wino_next_gout=zg)
    dw1c, db1c = torch.empty_like(dw1), torch.empty_like(db1)
    C.conv_wgrad(d1, g1c, dw1c, db1c, wino_gout=zg if C.winograd_tile(d1, 2) == 4 else None)
    g0c = torch.empty_like(y1)
    C.conv_dgrad(d1, u1t, g1c, [dict(p=g0c)], act, wino_pre=vg)
    for a, b_ in ((y1, y1c), (z1, z1c), (y2, y2c), (g1, g1c), (dw1, dw1c), (db1, db1c), (g0, g0c)):
        assert torch.equal(a, b_)
    # a layer that is not a Winograd evaluation refuses the options
    case3 = dict(B=1, H=8, W=16, src=[(64, 'nhwc')], Cout=64, up=False)
    C3, xs3, w3, b3, d3, act3, o3 = build(case3, seed=6)
    assert not C.winograd_chain(d3, 0)
    with pytest.raises(Exception):
        C.conv_fwd(d3, wphys(w3), b3.cuda(), dev, wino_next=v2)


@pytest.mark.parametrize('Cc,act', [(32, 'relu'), (256, 'relu'), (64, 'mish')])
def test_flow_head(Cc, act):
    from dvs_of_training_framework_amd import conv as C
    B, H, W = 2, 12, 20
    aid = C.ACT_RELU if act == 'relu' else C.ACT_MISH
    x = torch.randn(B, Cc, H, W, requires_grad=True)
    w = (torch.randn(2, Cc, 1, 1) / Cc ** 0.5).requires_grad_(True)
    b = torch.randn(2, requires_grad=True)
    zsrc = torch.randn(B, Cc, H, W)      # stand-in for the producer's y / z
    f_ref = F.conv2d(x, w, b)
    f = C.head_fwd(nhwc(x), w.view(2, Cc).cuda().contiguous(), b.cuda(), B, H, W, Cc)
    close(f, f_ref)
    gf, gx_in = torch.randn(f_ref.shape), torch.randn(x.shape)
    f_ref.backward(gf)
    dact = (zsrc > 0).float() if act == 'relu' else \
        torch.autograd.grad(F.mish(zsrc.requires_grad_(True)).sum(), zsrc)[0]
    want_gx = (x.grad + gx_in) * dact
    gx = torch.empty(B, H, W, Cc, device='cuda')
    dw, db = torch.empty(2, Cc, device='cuda'), torch.empty(2, device='cuda')
    C.head_bwd(nhwc(x), w.view(2, Cc).cuda().contiguous(), gf.cuda(), nhwc(gx_in),
               nhwc(zsrc.detach()), aid, gx, dw, db, B, H, W, Cc)
    close(from_nhwc(gx), want_gx)
    close(dw, w.grad.view(2, Cc))
    close(db, b.grad)


@pytest.mark.parametrize('mish,shape', [(False, (2, 5, 32, 48)), (True, (2, 5, 32, 48)),
                                        # residual stage 8 x 8 x 8: 128 2x2 tiles -> Winograd
                                        (False, (8, 5, 128, 128))])
def test_predictor_vs_torch_reference(mish, shape):
    """Whole predictor forward + backward (explicit schedule) vs ATen autograd."""
    from dvs_of_training_framework_amd.predictor import Predictor
    from oracle.ref_model import ref_predictor
    torch.manual_seed(1)
    B, Cin, H, W = shape
    act = torch.nn.Mish() if mish else torch.nn.ReLU()
    net = Predictor(Cin, act)
    x = torch.randn(B, Cin, H, W)
    state = {k: v.detach().clone().requires_grad_(True)
             for k, v in net.state_dict().items()}
    ref_flows = ref_predictor(state, x, mish)
    gfl = [torch.randn(f.shape) for f in ref_flows]
    sum((f * g).sum() for f, g in zip(ref_flows, gfl)).backward()
    net = net.cuda()
    flows = net(x.cuda())
    assert [tuple(f.shape) for f in flows] == [(B, 2, H // 8, W // 8), (B, 2, H // 4, W // 4),
                                               (B, 2, H // 2, W // 2), (B, 2, H, W)]
    for f, r in zip(flows, ref_flows):
        close(f, r, 1e-3)
    sum((f * g.cuda()).sum() for f, g in zip(flows, gfl)).backward()
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        close(p.grad, state[name].grad, 1e-3)


@pytest.mark.parametrize('ci', range(len(TWIN_LAYERS)))
def test_layer_on_bf16_twins(ci):
    """Mode 3 (bf16 twins), forward and data gradient of the layers the predictor runs
    on the general kernels: (a) the kernel ran in mode 3 (no silent fallback to mode 1);
    (b) equal to mode 1 on the same f32 tensors up to summation order; (c) every twin
    output is its f32 output rounded to nearest even; (d) twins built from OTHER tensors
    (sources, gout, weights) are what the vector members read -- the result is mode 1's
    on the twins' values, the planar flow member reads its f32 tensor; (e) within the
    bf16 bound of float64.  Data gradient with addend and act'(actsrc) in the epilogue."""
    from dvs_of_training_framework_amd import conv as C
    case, ffam, dfam = TWIN_LAYERS[ci]
    _, xs, w, b, desc, act, o = build(case, seed=40 + ci)
    B, H, W, Cout = case['B'], case['H'], case['W'], case['Cout']
    g = torch.Generator().manual_seed(70 + ci)
    vec = [lay == 'nhwc' for _, lay in case['src']]
    ho, wo = C.out_size(desc)
    res = torch.randn(B, Cout, ho, wo, generator=g) if case.get('residual') else None
    res_d = nhwc(res) if res is not None else None
    bias = b.cuda()
    f32 = desc._keepalive
    alt = [nhwc(torch.randn(x.shape, generator=g)) if v else d for x, d, v in zip(xs, f32, vec)]
    w2 = torch.randn(w.shape, generator=g) / w[0].numel() ** 0.5
    rnd = lambda t: t.to(torch.bfloat16).float()          # noqa: E731

    def desc_for(mode, srcs, twins=None):
        twins = srcs if twins is None else twins
        s = [(t, c, C.NHWC if v else C.NCHW, u.to(torch.bfloat16) if (mode == 3 and v) else None)
             for t, u, (c, _), v in zip(srcs, twins, case['src'], vec)]
        d = C.make_desc(s, B, H, W, Cout, o['k'], o['stride'], o['pad'], o['up'], act, mode)
        d._keep = s
        return d

    def fwd(mode, srcs=f32, twins=None, wf=w, w16=None):
        d = desc_for(mode, srcs, twins)
        w_f, _, w_f16, _ = C.prepare(d, wphys(wf), True, want16=True)
        if w16 is not None:
            w_f16 = C.prepare(d, wphys(w16), True, want16=True)[2]
        y, z = C.conv_fwd(d, w_f, bias, 'cuda', res_d, want_z=True,
                          weight16=w_f16 if mode == 3 else None)
        torch.cuda.synchronize()
        return y, z, d._y16
    y1, z1, _ = fwd(C.MFMA_BF16)
    assert_path(0, ffam, 1)
    y3, z3, y16 = fwd(C.MFMA_BF16_TWINS)
    assert_path(0, ffam, 3)                                              # (a)
    close(y3, y1, 1e-5)                                                  # (b)
    close(z3, z1, 1e-5)
    assert torch.equal(y16.view(y3.shape), y3.to(torch.bfloat16))       # (c)
    yd, zd, yd16 = fwd(C.MFMA_BF16_TWINS, twins=alt, w16=w2)             # (d)
    assert_path(0, ffam, 3)
    yr, zr, _ = fwd(C.MFMA_BF16, srcs=[rnd(t) if v else t for t, v in zip(alt, vec)], wf=w2)
    close(yd, yr, 1e-5)
    close(zd, zr, 1e-5)
    assert torch.equal(yd16.view(yd.shape), yd.to(torch.bfloat16))
    xs64 = [x.double().requires_grad_(True) for x in xs]
    y_ref, z_ref = torch_fwd(xs64, w.double(), b.double(), o, act, C,
                             res.double() if res is not None else None)
    close(from_nhwc(y3), y_ref, BF16_RTOL)                               # (e)

    # data gradient: addend + act' on every member, bf16 twins of the NHWC gradients
    gz = torch.randn(z_ref.shape, generator=g)
    gz2 = nhwc(torch.randn(z_ref.shape, generator=g))
    adds = [torch.randn(x.shape, generator=g) for x in xs]
    acts = [torch.randn(x.shape, generator=g) for x in xs]
    dev = lambda t, v: nhwc(t) if v else t.cuda().contiguous()       # noqa: E731
    adds_d = [dev(t, v) for t, v in zip(adds, vec)]
    acts_d = [dev(t, v) for t, v in zip(acts, vec)]
    gz_d = nhwc(gz)

    def dgrad(mode, gout=gz_d, gout16=None, wf=w, w16=None):
        d = desc_for(mode, f32)
        _, w_dg, _, w_dg16 = C.prepare(d, wphys(wf), True, want16=True)
        if w16 is not None:
            w_dg16 = C.prepare(d, wphys(w16), True, want16=True)[3]
        bufs, dsts = [], []
        for x, v, a_, s_ in zip(xs, vec, adds_d, acts_d):
            p = torch.full(s_.shape, float('nan'), device='cuda')
            p16 = torch.empty(s_.shape, dtype=torch.bfloat16, device='cuda') if v else None
            bufs.append((p, p16))
            dsts.append(dict(p=p, p16=p16, addend=a_, actsrc=s_))
        g16 = (gout if gout16 is None else gout16).to(torch.bfloat16) if mode == 3 else None
        C.conv_dgrad(d, w_dg, gout, dsts, C.ACT_RELU, weight16=w_dg16 if mode == 3 else None,
                     gout16=g16)
        torch.cuda.synchronize()
        return bufs
    g1 = dgrad(C.MFMA_BF16)
    assert_path(1, dfam, 1)
    g3 = dgrad(C.MFMA_BF16_TWINS)
    assert_path(1, dfam, 3)                                              # (a)
    for (p1, _), (p3, p16), v in zip(g1, g3, vec):
        close(p3, p1, 1e-5)                                              # (b)
        if v:
            assert torch.equal(p16, p3.to(torch.bfloat16))              # (c)
    gd = dgrad(C.MFMA_BF16_TWINS, gout16=gz2, w16=w2)                    # (d)
    assert_path(1, dfam, 3)
    gr = dgrad(C.MFMA_BF16, gout=rnd(gz2), wf=w2)
    for (pd, pd16), (pr, _), (p3, _), v in zip(gd, gr, g3, vec):
        if v:
            close(pd, pr, 1e-5)
            assert torch.equal(pd16, pd.to(torch.bfloat16))
        else:   # a planar member's gradient: from the f32 gout and f32 weights (dvsof.h)
            assert torch.equal(pd, p3)
    z_ref.backward(gz.double())
    for (p3, _), x, a_, s_, v in zip(g3, xs64, adds, acts, vec):         # (e)
        want = (x.grad + a_.double()) * (s_.double() > 0)
        close(from_nhwc(p3) if v else p3, want, BF16_RTOL)


@pytest.mark.parametrize('Cc', [64, 128])
def test_flow_head_backward_bf16_twin_of_gx(Cc):
    """dvsof_flow_head_bwd with gx16 (mode 3: the twin the next data gradient reads):
    the twin is gx rounded to nearest even, gx within 1e-4 of float64."""
    from dvs_of_training_framework_amd import conv as C
    B, H, W = 2, 12, 20
    g = torch.Generator().manual_seed(Cc)
    x = torch.randn(B, Cc, H, W, generator=g, dtype=torch.float64).float()
    w = torch.randn(2, Cc, generator=g).float() / Cc ** 0.5
    gf, gx_in, zsrc = (torch.randn(s, generator=g) for s in ((B, 2, H, W), x.shape, x.shape))
    want = (torch.einsum('kc,bkyx->bcyx', w.double(), gf.double()) + gx_in.double()) * \
        (zsrc.double() > 0)
    gx = torch.full((B, H, W, Cc), float('nan'), device='cuda')
    gx16 = torch.empty((B, H, W, Cc), dtype=torch.bfloat16, device='cuda')
    dw, db = torch.empty(2, Cc, device='cuda'), torch.empty(2, device='cuda')
    C.head_bwd(nhwc(x), w.cuda().contiguous(), gf.cuda(), nhwc(gx_in), nhwc(zsrc), C.ACT_RELU, gx, dw,
               db, B, H, W, Cc, gx16=gx16)
    torch.cuda.synchronize()
    close(from_nhwc(gx), want)
    assert torch.equal(gx16, gx.to(torch.bfloat16))
    close(dw, torch.einsum('bkyx,bcyx->kc', gf.double(), x.double()))


def test_first_layer_writes_the_bf16_twin_of_y():
    """csrc/first.hip in mode 3: exact f32 arithmetic, y16 = y rounded (nearest even),
    the witness reports the twin written."""
    from dvs_of_training_framework_amd import conv as C
    case = dict(B=2, H=32, W=48, src=[(5, 'nchw')], Cout=64, stride=2, act='mish')
    _, xs, w, b, d0, act, o = build(case, seed=9)
    d = C.make_desc([(d0._keepalive[0], 5, C.NCHW)], 2, 32, 48, 64, 3, 2, 1, False, act, 3)
    d._keep = d0._keepalive
    y, z = C.conv_fwd(d, wphys(w), b.cuda(), 'cuda', None, want_z=True)
    torch.cuda.synchronize()
    assert_path(0, 'first', 3)
    assert torch.equal(d._y16.view(y.shape), y.to(torch.bfloat16))
    y_ref, z_ref = torch_fwd([x.double() for x in xs], w.double(), b.double(), o, act, C)
    close(from_nhwc(z), z_ref)
    close(from_nhwc(y), y_ref)
    d.mfma = C.MFMA_F32
    yf, _ = C.conv_fwd(d, wphys(w), b.cuda(), 'cuda', None)
    assert_path(0, 'first', 0)
    assert torch.equal(yf, y)
