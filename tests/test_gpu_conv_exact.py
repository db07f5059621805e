"""Conv kernels without tolerance, and the bf16 rounding contract emulated exactly.

1. Integer-grid oracle: operands on a small integer grid keep every product and every
   partial sum an integer below 2^24 (the premise is checked per pass, conv_cases.
   exact_bound), so every family in every operand mode must equal the float64 result
   BIT FOR BIT -- f32 or bf16 matrix cores, the bf16x3 split (lo = 0), the sub-pixel,
   nine-product and F(2x2) Winograd forms.  Exceptions, each with its non-dyadic step:
   F(4x4) Winograd (1/6, 1/12, 1/24 in its transforms) and Mish.
2. The bf16 operand modes against float64 arithmetic on the operands rounded as
   include/dvsof.h documents (conv_cases.operand_pairs), with a separation check that
   the wrong rounding could not pass.
3. dvsof_to_bf16 / _many bit for bit against torch's round to nearest even."""
import pytest
import torch
import torch.nn.functional as F

from tests.conv_cases import (CASES, F32_ONLY, GRID, TWIN_LAYERS, WGRAD_TWIN_CASES,
                              assert_exact_premise, EMU_TAU, EMU_TAU_DB, contract_errors, dyadic_weights,
                              effective_mode, emulate_dgrad, emulate_fwd, emulate_wgrad,
                              int_grid, is_subpixel, layer_geometry, reference64, rel_l2, rne_bf16,
                              run_layer, twins_apply)

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24
# Tolerances of the non-dyadic exceptions, in units of 2^-24 * sum|a||b| per element
# (sum|a||b|: the conv on absolute values, plus |bias| and |residual|); set at <= 4x the
# worst error of the first run on an MI355X, and never looser than 1e-4 of the peak.
WINO4_ULPS = 90.0       # F(4x4,3x3): transforms with 1/6, 1/12, 1/24 (csrc/winograd.hip)
MISH_ULPS = 4.0         # Mish: v_exp / v_rcp approximations (conv_common.h mish_t)


def out_hw(case):
    o = layer_geometry(case)
    hv = case['H'] * (2 if o['up'] else 1)
    wv = case['W'] * (2 if o['up'] else 1)
    return ((hv + 2 * o['pad'] - o['k']) // o['stride'] + 1,
            (wv + 2 * o['pad'] - o['k']) // o['stride'] + 1)


def int_layer(case, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W, Cout = case['B'], case['H'], case['W'], case['Cout']
    k = case.get('k', 3)
    ctot = sum(c for c, _ in case['src'])
    ho, wo = out_hw(case)
    xs = [int_grid(g, (B, c, H, W), GRID['x']) for c, _ in case['src']]
    w = int_grid(g, (Cout, ctot, k, k), GRID['w'])
    b = int_grid(g, (Cout,), GRID['b'])
    res = int_grid(g, (B, Cout, ho, wo), GRID['b']) if case.get('residual') else None
    gz = int_grid(g, (B, Cout, ho, wo), GRID['g'])
    return xs, w, b, res, gz


# float64 references, made once per case and reused across the modes (tests run case-major)
_REF = {}


def case_data(key, case, seed, need_abs):
    if key not in _REF:
        _REF.clear()
        xs, w, b, res, gz = int_layer(case, seed)
        ref = reference64(case, xs, w, b, res, gz)
        absref = None
        if need_abs:
            absref = reference64(case, [x.abs() for x in xs], w.abs(), b.abs(),
                                 res.abs() if res is not None else None, gz.abs())
        _REF[key] = (xs, w, b, res, gz, ref, absref)
    return _REF[key]


def pass_bounds(case, fams):
    """Assert the exactness premise of each pass; -> the three bounds."""
    B, H, W, Cout = case['B'], case['H'], case['W'], case['Cout']
    o = layer_geometry(case)
    ctot = sum(c for c, _ in case['src'])
    ho, wo = out_hw(case)
    k2 = o['k'] ** 2
    # a sub-pixel layer (up-sampling, 3x3 / pad 1) multiplies phase forms, sums of up to four
    # taps, and its weight gradient reduces over the B H W low-resolution pixels.  Any other
    # up-sampling layer reads the raw taps from the up-sampled frame: growth 1, a weight
    # gradient over the B Ho Wo output pixels -- and a data gradient that sums the 2x2 quad
    # of up-sampled pixels (growth 4, like the sub-pixel 4x4 form)
    sub = is_subpixel(o)
    return (assert_exact_premise(ctot * k2, GRID['x'], GRID['w'], fams[0], sub,
                                 extra=2 * GRID['b']),
            assert_exact_premise(Cout * k2, GRID['g'], GRID['w'], fams[1], o['up'], extra=2 * GRID['b']),
            assert_exact_premise(B * H * W if sub else B * ho * wo, GRID['g'], GRID['x'], fams[2],
                                 sub))


def within_ulps(got, want, absref, ulps):
    """Worst |got - want| in units of 2^-24 * absref; asserts <= ulps and <= 1e-4 of the peak."""
    got, want = got.double(), want.double()
    err = (got - want).abs()
    worst = (err / (EPS24 * absref.double()).clamp_min(EPS24)).max().item()
    assert worst <= ulps, worst
    assert err.max().item() <= 1e-4 * want.abs().max().item(), (err.max().item(), want.abs().max().item())
    return worst


def check_layer(case, mode, out, ref, absref, wino4_ulps=WINO4_ULPS, mish_ulps=MISH_ULPS):
    """Compare every output of run_layer with the float64 reference: -> list of mismatches
    (empty = all bitwise, or within the named exception's tolerance), worst exception errors."""
    bad, worst = [], {}

    def same(name, got, want):
        if not torch.equal(got.double(), want.double()):
            d = (got.double() - want.double()).abs()
            i = int(d.flatten().argmax())
            bad.append((name, int((d != 0).sum()), d.max().item(), i, tuple(got.shape)))

    def approx(name, got, want, a, ulps):
        try:
            worst[name] = within_ulps(got, want, a, ulps)
        except AssertionError as e:
            bad.append((name, 'tolerance', str(e)))
    fams = out['fam']
    # F(4x4,3x3) Winograd: non-dyadic transforms
    if fams[0] == 'wino4':
        approx('z', out['z'], ref['z'], absref['z'], wino4_ulps)
    else:
        same('z', out['z'], ref['z'])
    if case.get('act') == 'mish':
        # Mish: y = z tanh(softplus(z)) is not an exact f32 function of z (after F(4x4):
        # the error of z dominates)
        approx('y', out['y'], ref['y'], absref['z'] + 1, wino4_ulps if fams[0] == 'wino4' else mish_ulps)
    elif fams[0] == 'wino4':
        approx('y', out['y'], ref['y'], absref['z'], wino4_ulps)
    else:
        same('y', out['y'], ref['y'])
    for i, (got, want) in enumerate(zip(out['dx'], ref['dx'])):
        if fams[1] == 'wino4':
            approx('dx%d' % i, got, want, absref['dx'][i], wino4_ulps)
        else:
            same('dx%d' % i, got, want)
    if fams[2] == 'wino4':
        approx('dw', out['dw'], ref['dw'], absref['dw'], wino4_ulps)
    else:
        same('dw', out['dw'], ref['dw'])
    same('db', out['db'], ref['db'])
    if out['y16'] is not None:
        same('y16', out['y16'].float(), out['y'].to(torch.bfloat16).float())
    for i, (d16, d) in enumerate(zip(out['dx16'], out['dx'])):
        if d16 is not None:
            same('dx16_%d' % i, d16.float(), d.to(torch.bfloat16).float())
    return bad, worst


def check_families(case, mode, out):
    want = case['path'][mode].split()
    for kind in range(3):
        assert (out['fam'][kind], out['modes'][kind]) == \
            (want[kind], effective_mode(kind, want[kind], mode)), (kind, out['fam'], out['modes'], want)


EXACT_PARAMS = [(ci, m) for ci in range(len(CASES)) for m in (0, 1, 2, 3)
                if m != 3 or twins_apply(CASES[ci])]


@pytest.mark.parametrize('ci,mode', EXACT_PARAMS)
def test_every_conv_path_is_exact_on_an_integer_grid(ci, mode):
    case = CASES[ci]
    need_abs = case.get('act') == 'mish' or bool(case.get('wino'))
    xs, w, b, res, gz, ref, absref = case_data(('case', ci), case, 1000 + ci, need_abs)
    out = run_layer(case, mode, xs, w, b, res, gz, p16=True)
    check_families(case, mode, out)
    pass_bounds(case, out['fam'])
    bad, _ = check_layer(case, mode, out, ref, absref)
    assert not bad, bad


# mode-3 weight gradients of test_wgrad_on_bf16_twins_... that CASES does not hold already
def _key(c):
    return (c['B'], c['H'], c['W'], tuple(c['src']), c['Cout'], c.get('stride', 1), c.get('up', False))


_CASE_KEYS = {_key(c) for c in CASES}
WGRAD_TWIN_EXTRA = [c for c in WGRAD_TWIN_CASES if _key(c) not in _CASE_KEYS]


@pytest.mark.parametrize('wi', range(len(WGRAD_TWIN_EXTRA)))
def test_wgrad_on_bf16_twins_is_exact_on_an_integer_grid(wi):
    case = WGRAD_TWIN_EXTRA[wi]
    xs, w, b, res, gz, ref, _ = case_data(('wtwin', wi), case, 2000 + wi, False)
    out = run_layer(case, 3, xs, w, b, res, gz)
    assert out['modes'][2] == 3 and out['fam'][2] == ('wgrad_patch' if case.get('up') else 'general_v2'), out
    pass_bounds(case, out['fam'])
    assert torch.equal(out['dw'].double(), ref['dw'])
    assert torch.equal(out['db'].double(), ref['db'])


@pytest.mark.parametrize('ci', range(len(TWIN_LAYERS)))
@pytest.mark.parametrize('mode', [1, 3])
def test_twin_layers_with_epilogue_are_exact_on_an_integer_grid(ci, mode):
    """TWIN_LAYERS: forward with residual, data gradient with addend + act'(actsrc) (ReLU,
    relu'(0) = 0 as in ATen: act_bwd is s > 0) on every member, the twins of y and dx."""
    case, ffam, dfam = TWIN_LAYERS[ci]
    xs, w, b, res, gz, ref, absref = case_data(('twin', ci), case, 3000 + ci, case.get('act') == 'mish')
    g = torch.Generator().manual_seed(3100 + ci)
    epi = [dict(addend=int_grid(g, x.shape, GRID['b']), actsrc=int_grid(g, x.shape, 1)) for x in xs]
    out = run_layer(case, mode, xs, w, b, res, gz, p16=True, epi=epi, bwd_act=1)
    assert out['fam'][:2] == [ffam, dfam] and out['modes'][:2] == [mode, mode], out['fam']
    pass_bounds(case, out['fam'])
    want = dict(ref)
    want['dx'] = [(d + e['addend'].cuda()) * (e['actsrc'].cuda() > 0).double() for d, e in zip(ref['dx'], epi)]
    for d, e in zip(out['dx'], epi):       # ReLU' at exactly 0 is 0: the integer actsrc hits it
        zero = e['actsrc'] == 0
        assert zero.any() and (d.cpu()[zero] == 0).all()
    bad, _ = check_layer(case, mode, out, want, absref)
    assert not bad, bad


# ---------------------------------------------------------------------------
# nine-product decoder kernels (csrc/fwd_min.hip, csrc/dgrad_min.hip): every epilogue option
# ---------------------------------------------------------------------------
NINE = [(2, 16, 32, 64, 64, 32, 'fwd_min4', 'dgrad_min1'),
        (6, 72, 80, 64, 64, 32, 'fwd_min8', 'dgrad_min0')]


def _class_bias(b_cls, Ho, Wo):
    ys, xs = torch.arange(Ho), torch.arange(Wo)
    vy = torch.where(ys == 0, 1, torch.where(ys == Ho - 1, 2, 0))
    vx = torch.where(xs == 0, 1, torch.where(xs == Wo - 1, 2, 0))
    tab = b_cls.double().clone()
    tab[0] = 0
    return tab[3 * vy[:, None] + vx[None, :]].permute(2, 0, 1)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


@pytest.mark.parametrize('shape', NINE, ids=lambda s: 'B%dH%dW%d' % s[:3])
def test_nine_product_epilogues_are_exact_on_an_integer_grid(shape):
    from dvs_of_training_framework_amd import conv as C
    B, H, W, Cx, Cs, Cout, ffam, dfam = shape
    g = torch.Generator().manual_seed(B * 31 + H)
    x, sk = int_grid(g, (B, Cx, H, W), 1), int_grid(g, (B, Cs, H, W), 1)
    w, b = int_grid(g, (Cout, Cx + Cs, 3, 3), 2), int_grid(g, (Cout,), 4)
    b_cls = int_grid(g, (9, Cout), 4)
    assert_exact_premise((Cx + Cs) * 9, 1, 2, ffam, True, extra=8)
    xd, sd = _nhwc(x), _nhwc(sk)
    inp = F.interpolate(torch.cat([x, sk], 1), scale_factor=2, mode='nearest')
    z0 = F.conv2d(inp, w, b, padding=1)
    zc = z0 + _class_bias(b_cls, 2 * H, 2 * W)[None]
    w_dev = w.float().permute(0, 2, 3, 1).contiguous().cuda()
    worst = 0.0
    for act in ('relu', 'none', 'mish'):
        a = {'relu': C.ACT_RELU, 'mish': C.ACT_MISH, 'none': C.ACT_NONE}[act]
        d = C.make_desc([(xd, Cx, C.NHWC), (sd, Cs, C.NHWC)], B, H, W, Cout, 3, 1, 1, True, a)
        w_f, _ = C.prepare(d, w_dev, False)
        for cls in (False, True):
            z_ref = zc if cls else z0
            y, z = C.conv_fwd(d, w_f, b.float().cuda(), 'cuda', None, want_z=True,
                              bias_cls=b_cls.float().cuda() if cls else None)
            torch.cuda.synchronize()
            assert C.KERNEL_NAMES[C.last_kernel(0)[0]] == ffam
            if act != 'mish':
                assert torch.equal(y.permute(0, 3, 1, 2).double().cpu(),
                                   F.relu(z_ref) if act == 'relu' else z_ref), (act, cls)
            assert torch.equal(z.permute(0, 3, 1, 2).double().cpu(), z_ref), (act, cls)
            if act == 'mish':     # Mish: not an exact f32 function of z
                absz = F.conv2d(inp.abs(), w.abs(), b.abs(), padding=1) + 4
                worst = max(worst, within_ulps(y.permute(0, 3, 1, 2).cpu(), F.mish(z_ref), absz + 1,
                                               MISH_ULPS))
    # the folded flow member (dvsof_flow_fold_weights / _bias) against the unfolded layer
    wh, bh = int_grid(g, (2, Cx), 2), int_grid(g, (2,), 4)
    wf = int_grid(g, (Cout, Cx + Cs + 2, 3, 3), 2)
    flow = F.conv2d(x, wh[:, :, None, None], bh)
    zf = F.conv2d(F.interpolate(torch.cat([x, sk, flow], 1), scale_factor=2, mode='nearest'),
                  wf, b, padding=1)
    assert_exact_premise((Cx + Cs) * 9, 1, 2 + 2 * 2 * Cx, ffam, True, extra=4 + 2 * 9 * 2 * 4)
    ctot = Cx + Cs + 2
    wf_d = wf.float().permute(0, 2, 3, 1).contiguous().cuda()
    d2 = C.make_desc([(xd, Cx, C.NHWC), (sd, Cs, C.NHWC)], B, H, W, Cout, 3, 1, 1, True, C.ACT_NONE)
    w_eff = C.flow_fold_weights(wf_d, Cout, ctot, 0, Cx, Cx + Cs, wh.float().cuda().contiguous())
    w_f, _ = C.prepare(d2, w_eff, False)
    b_eff, b_cls2 = C.flow_fold_bias(wf_d, Cout, ctot, Cx + Cs, bh.float().cuda(), b.float().cuda())
    _, z = C.conv_fwd(d2, w_f, b_eff, 'cuda', None, want_z=True, bias_cls=b_cls2)
    torch.cuda.synchronize()
    assert C.KERNEL_NAMES[C.last_kernel(0)[0]] == ffam
    assert torch.equal(z.permute(0, 3, 1, 2).double().cpu(), zf)

    # data gradient: addends, act' (ReLU: relu'(0) = 0; Mish: tolerance), the folded head
    gz = int_grid(g, (B, Cout, 2 * H, 2 * W), 1)
    xr, skr = x.clone().requires_grad_(True), sk.clone().requires_grad_(True)
    F.conv2d(F.interpolate(torch.cat([xr, skr], 1), scale_factor=2, mode='nearest'), w, b,
             padding=1).backward(gz)
    gx, gs = xr.grad, skr.grad
    assert_exact_premise(Cout * 9, 1, 2, dfam, True, extra=3 * 4 + 2 * 2 * 1)
    a1, a2 = int_grid(g, x.shape, 4), int_grid(g, x.shape, 4)
    src, hx = int_grid(g, x.shape, 1), int_grid(g, x.shape, 1)
    hw, gf = int_grid(g, (2, Cx), 2), int_grid(g, (B, 2, H, W), 1)
    head = torch.einsum('kc,bkyx->bcyx', hw, gf)
    _, wt = C.prepare(d, w_dev, True)
    gz_d = _nhwc(gz)
    a1d, a2d, srcd, hxd = _nhwc(a1), _nhwc(a2), _nhwc(src), _nhwc(hx)
    whd, gfd = hw.float().cuda(), gf.float().cuda()
    relu_d = (src > 0).double()
    zs = src.clone().requires_grad_(True)
    mish_d = torch.autograd.grad(F.mish(zs).sum(), zs)[0]
    options = [
        ('plain', {}, C.ACT_NONE, gx, None),
        ('addend', dict(addend=a1d), C.ACT_NONE, gx + a1, None),
        ('addends+relu', dict(addend=a1d, addend2=a2d, actsrc=srcd), C.ACT_RELU, (gx + a1 + a2) * relu_d, None),
        ('head+relu', dict(addend=a1d, actsrc=srcd, head_w=whd, head_gflow=gfd), C.ACT_RELU,
         (gx + a1 + head) * relu_d, None),
        ('head+part', dict(addend=a1d, addend2=a2d, actsrc=srcd, head_w=whd, head_gflow=gfd, head_x=hxd),
         C.ACT_RELU, (gx + a1 + a2 + head) * relu_d, None),
        # Mish act': not an exact f32 function of actsrc
        ('addends+mish', dict(addend=a1d, addend2=a2d, actsrc=srcd), C.ACT_MISH, (gx + a1 + a2) * mish_d,
         (gx.abs() + 8) * mish_d.abs()),
    ]
    for name, opt, bact, want0, tol_scale in options:
        b0 = torch.full((B, H, W, Cx), float('nan'), device='cuda')
        b1 = torch.full((B, H, W, Cs), float('nan'), device='cuda')
        dst0, part = dict(p=b0, **opt), None
        if 'head_x' in opt:
            part = C.dgrad_head_part(d, Cx, 'cuda')
            part.fill_(float('nan'))
            dst0['head_part'] = part
        C.conv_dgrad(d, wt, gz_d, [dst0, dict(p=b1)], bact)
        torch.cuda.synchronize()
        assert C.KERNEL_NAMES[C.last_kernel(1)[0]] == dfam, name
        got0 = b0.permute(0, 3, 1, 2).cpu()
        if tol_scale is None:
            assert torch.equal(got0.double(), want0), name
        else:
            worst = max(worst, within_ulps(got0, want0, tol_scale + 1, MISH_ULPS))
        if 'actsrc' in opt and bact == C.ACT_RELU:
            assert (src == 0).any() and (got0[src == 0] == 0).all(), name
        assert torch.equal(b1.permute(0, 3, 1, 2).double().cpu(), gs), name
        if part is not None:
            dwh, dbh = torch.empty(2, Cx, device='cuda'), torch.empty(2, device='cuda')
            C.head_reduce(part, Cx, dwh, dbh)
            assert torch.equal(dwh.double().cpu(), torch.einsum('bkyx,bcyx->kc', gf, hx)), name
            assert torch.equal(dbh.double().cpu(), gf.sum((0, 2, 3))), name
    assert worst <= MISH_ULPS


# ---------------------------------------------------------------------------
# 2. The bf16 rounding contract, emulated exactly (random operands)
# ---------------------------------------------------------------------------
# layers whose passes reach every (family, pass) the bf16 modes run in CASES / TWIN_LAYERS /
# WGRAD_TWIN_CASES: general_v2 forward / data / weight gradient, stride2_phased data
# gradient, wgrad_patch and fwd_patch (mode 3), and the f32-only families of modes 1-2
# (the stride-2 layer's general_v1 weight gradient: exact products).  Winograd in mode 2 rounds its TRANSFORMED
# operands; it is covered bitwise by the integer grid above and by test_gpu_conv.py's 1e-4.
EMU_LAYERS = [
    # sub-pixel forms of an up-sampling layer, a planar flow member beside two vector members
    dict(B=2, H=8, W=16, src=[(64, 'nhwc'), (32, 'nhwc'), (2, 'nchw')], Cout=32, up=True, act='none',
         path={1: 'general_v2 general_v2 general_v2', 2: 'general_v2 general_v2 general_v2',
               3: 'general_v2 general_v2 wgrad_patch'}),
    # stride 2: the phased data gradient
    dict(B=2, H=16, W=16, src=[(64, 'nhwc')], Cout=128, stride=2, act='none',
         path={1: 'general_v2 stride2_phased general_v1', 2: 'general_v2 stride2_phased general_v1',
               3: 'general_v2 stride2_phased general_v1'}),
    # stride 1, one member
    dict(B=2, H=8, W=16, src=[(64, 'nhwc')], Cout=64, stride=1, act='none',
         path={1: 'general_v2 general_v2 general_v2', 2: 'general_v2 general_v2 general_v2',
               3: 'general_v2 general_v2 general_v2'}),
    # the finest decoder stage: fwd_patch in mode 3
    dict(B=1, H=4, W=16, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True, act='none',
         path={1: 'general_v2 general_v2 general_v2', 2: 'general_v2 general_v2 general_v2',
               3: 'fwd_patch general_v2 wgrad_patch'}),
]
TAU, TAU_DB = EMU_TAU, EMU_TAU_DB


def emu_rounding(mode, family, kind):
    if effective_mode(kind, family, mode) == 0 and family in F32_ONLY:
        return 'exact'
    return 'x3' if mode == 2 else 'rne'


def emu_alternatives(rounding):
    """Roundings a wrong kernel might use instead: each must be far from the contract."""
    return {'rne': ('trunc', 'exact'), 'x3': ('x3_no_cross',), 'exact': ('rne',)}[rounding]


def emu_data(case, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W, Cout = case['B'], case['H'], case['W'], case['Cout']
    ctot = sum(c for c, _ in case['src'])
    ho, wo = out_hw(case)
    k = case.get('k', 3)
    xs = [torch.randn(B, c, H, W, generator=g).double() for c, _ in case['src']]
    w = dyadic_weights(g, (Cout, ctot, k, k))
    b = torch.randn(Cout, generator=g).float().double()
    gz = torch.randn(B, Cout, ho, wo, generator=g).float().double()
    return xs, w, b, gz


def emu_measure(ei, mode):
    return emu_measure_case(EMU_LAYERS[ei], 500 + ei, mode)


def emu_measure_case(case, seed, mode, planar_dx_exact=True):
    """-> (families, {pass: (rounding, rel, elem, {alternative: rel distance})})
    planar_dx_exact: the planar members' data gradient runs beside the matrix-core launch in
    exact f32 (csrc/gconv.hip peels narrow trailing planar destinations off a plain or
    sub-pixel data gradient); False where it stays in the matrix-core problem and rounds
    like every other column (quad rows, zero-inserted gout)."""
    xs, w, b, gz = emu_data(case, seed)
    out = run_layer(case, mode, xs, w, b, None, gz)
    o = layer_geometry(case)
    x = torch.cat(xs, 1).cuda()
    wc, gc = w.cuda(), gz.cuda()
    ax, aw, ag = x.abs(), wc.abs(), gc.abs()
    # channels of the planar (NCHW) members: their data gradient and weight-gradient columns
    # are computed in exact f32 in every mode (dvsof.h, dvsof_conv_desc_t.mfma)
    planar, c0 = [], 0
    for c, lay in case['src']:
        if lay == 'nchw':
            planar.append((c0, c0 + c))
        c0 += c
    res = {}

    def one(name, kind, fn, absval, got, per_member=False):
        r = emu_rounding(mode, out['fam'][kind], kind)
        if name == 'dx' and not planar_dx_exact:
            per_member = False

        def emu(rr):
            t = fn(rr)
            if per_member and rr != 'exact' and planar:
                ex = fn('exact')
                for lo, hi in planar:
                    t[:, lo:hi] = ex[:, lo:hi]
            return t
        ref = emu(r)
        rel, elem = contract_errors(got, ref, absval)
        res[name] = (r, rel, elem, {alt: rel_l2(emu(alt), ref) for alt in emu_alternatives(r)})
    one('z', 0, lambda r: emulate_fwd(x, wc, o, r) + b.cuda()[None, :, None, None],
        emulate_fwd(ax, aw, o, 'exact') + b.cuda().abs()[None, :, None, None], out['z'])
    one('dx', 1, lambda r: emulate_dgrad(x.shape, wc, gc, o, r),
        emulate_dgrad(x.shape, aw, ag, o, 'exact'), torch.cat(out['dx'], 1), per_member=True)
    one('dw', 2, lambda r: emulate_wgrad(x, w.shape, gc, o, r),
        emulate_wgrad(ax, w.shape, ag, o, 'exact'), out['dw'], per_member=True)
    # bias gradient: channel sums of gout in f32, of its bf16 twin where the mode-3 weight
    # gradient streams the twins
    twin = mode == 3 and out['fam'][2] not in F32_ONLY
    db_ref = (rne_bf16(gc) if twin else gc).sum((0, 2, 3))
    db_alt = (gc if twin else rne_bf16(gc)).sum((0, 2, 3))
    res['db'] = ('rne' if twin else 'exact', rel_l2(out['db'], db_ref), 0.0,
                 {'rne' if not twin else 'exact': rel_l2(db_alt, db_ref)})
    return out['fam'], res


@pytest.mark.parametrize('mode', [1, 2, 3])
@pytest.mark.parametrize('ei', range(len(EMU_LAYERS)))
def test_bf16_modes_round_as_documented(ei, mode):
    fams, res = emu_measure(ei, mode)
    assert fams == EMU_LAYERS[ei]['path'][mode].split(), fams
    for name, (r, rel, elem, alts) in res.items():
        tau = TAU[mode] if name != 'db' else TAU_DB
        assert rel <= tau, (name, r, rel)
        assert elem <= 1.0, (name, r, elem)
        for alt, dist in alts.items():       # the check could not pass the wrong rounding
            assert dist >= 100 * tau, (name, r, alt, dist)


# ---------------------------------------------------------------------------
# 3. dvsof_to_bf16 / dvsof_to_bf16_many bit for bit
# ---------------------------------------------------------------------------
def _bits_f32(vals):
    return torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in vals], dtype=torch.int32).view(torch.float32)


SPECIAL = _bits_f32([
    0x3f808000, 0x3f818000, 0x3f808001, 0x3f817fff, 0xbf808000, 0xbf818000,     # ties: even / odd
    0x00000000, 0x80000000,                                                       # +-0
    0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff, 0xff7f8000,                   # largest finite
    0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffc00001, 0x7fffffff,       # inf, NaN
    0x00000001, 0x00008000, 0x00018000, 0x00017fff, 0x007fffff, 0x807fffff,       # subnormals
    0x80008000, 0x00400000, 0x00800000, 0x00ff8000])


def _same_bf16(got, src):
    want = src.to(torch.bfloat16)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16)), \
        [(hex(int(s)), int(a), int(b_)) for s, a, b_ in zip(src.view(torch.int32)[~nan],
                                                            got[~nan].view(torch.int16),
                                                            want[~nan].view(torch.int16)) if a != b_]


def test_to_bf16_special_values_bit_for_bit():
    from dvs_of_training_framework_amd import conv as C
    src = SPECIAL.cuda()
    _same_bf16(C.to_bf16(src).cpu(), SPECIAL)


def test_to_bf16_lengths_and_offsets_bit_for_bit():
    """Lengths 0-37 from offsets of +1..+3 elements (unaligned heads and tails); the
    element past the end is not written."""
    from dvs_of_training_framework_amd import _lib
    g = torch.Generator().manual_seed(7)
    base = torch.cat([SPECIAL, torch.randn(64, generator=g)]).cuda()
    lib = _lib.lib()
    for off in (0, 1, 2, 3):
        for n in range(38):
            src = base[off:off + n]
            dst = torch.full((n + 8,), -7.0, dtype=torch.bfloat16, device='cuda')
            _lib.check(lib.dvsof_to_bf16(base.data_ptr() + 4 * off, dst.data_ptr(), n, _lib.stream()),
                       'dvsof_to_bf16')
            d = dst.cpu()
            _same_bf16(d[:n], src.cpu())
            assert (d[n:] == -7.0).all(), (off, n)


def test_to_bf16_many_uneven_tensors_bit_for_bit():
    from dvs_of_training_framework_amd import conv as C
    g = torch.Generator().manual_seed(8)
    sizes = [1, 0, 37, 3, 1000, 17, 4096 + 5, 2, 33, 64, 5, 129, 7, 1, 250, 31]
    base = torch.cat([SPECIAL, torch.randn(sum(sizes) + 64, generator=g)]).cuda()
    srcs, pos = [], 0
    for i, n in enumerate(sizes):
        pos += 1 + i % 3                       # uneven offsets
        srcs.append(base[pos:pos + n])
        pos += n
    outs = C.to_bf16_many(srcs)
    for s, o in zip(srcs, outs):
        _same_bf16(o.cpu(), s.cpu())
