"""Every layer geometry the conv entry points accept, off the 3x3 / pad-1 forms the other conv
tests run: ksize 1 | 3 | 5, stride 1 | 2, any pad in 0 .. ksize-1, 2x nearest up-sampling in
front of any of those at stride 1 (conv_cases.GEOMETRY; csrc/conv_api.hip: desc_ok,
conv_classify).  These reach the general forward with the `Y >> 1` gather, the data-gradient
forms DG_PLAIN with pad' = ksize - 1 - pad, DG_ZERO2 (zero-inserted gout) and DG_QUAD (rows
ordered (b, y, x, dy, dx), 2x2 sum in the epilogue), the flip-transposed weight form for
ksize != 3, and the general weight gradient on the up-sampled frame -- on the v1 and the v2
kernels of each pass.

1. Integer grid: every output of every case in every operand mode equals float64 bit for bit.
2. Random data against float64 at the bars of test_gpu_conv.py.
3. Every element of every output is written, nothing beyond it is; input pixels that no
   output reads get a gradient of exactly +0 (act'(actsrc) * addend with an epilogue).
4. The data-gradient epilogue (addend, addend2, act') on the quad and zero-insertion forms.
5. The bf16 rounding contract (include/dvsof.h) on an up-sampled 5x5 and a 1x1 layer.
6. Descriptors outside the accepted set are refused by every entry point.
No tolerance here is new: bitwise, RTOL / BF16_RTOL / BF16X3_RTOL, EMU_TAU, MISH_ULPS."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.conv_cases import (EMU_TAU, EMU_TAU_DB, GEOMETRY, GRID, geometry_id, int_grid, layer_geometry, nhwc, reference64, run_layer, split_path,
                              twins_apply, wphys)
from tests.test_gpu_conv import BF16_RTOL, BF16X3_RTOL, RTOL, close
from tests.test_gpu_conv_exact import (MISH_ULPS, case_data, check_layer, emu_measure_case, int_layer,
                                       out_hw, pass_bounds, within_ulps)

pytestmark = pytest.mark.gpu

IDS = [geometry_id(c) for c in GEOMETRY]
assert len(set(IDS)) == len(IDS)


def case_of(name):
    return GEOMETRY[IDS.index(name)]


def modes_of(case):
    """Operand modes 0, 1, 2, and 3 where every NHWC member has 32 | C."""
    assert len(case['path']) == (4 if twins_apply(case) else 3), case
    return range(len(case['path']))


def check_path(case, mode, out):
    """The three passes ran the families, in the operand modes, derived from the dispatch."""
    assert list(zip(out['fam'], out['modes'])) == split_path(case, mode), (out['fam'], out['modes'], case['path'][mode])


EXACT_PARAMS = [pytest.param(ci, m, id='%s-m%d' % (IDS[ci], m)) for ci in range(len(GEOMETRY))
                for m in modes_of(GEOMETRY[ci])]


# ---------------------------------------------------------------------------
# 1. Integer grid, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('ci,mode', EXACT_PARAMS)
def test_every_geometry_is_exact_on_an_integer_grid(ci, mode):
    """y, z, every dx, dw, db and the bf16 twins of y and dx against float64: all general-family
    kernels with ReLU, so no non-dyadic exception applies and nothing has a tolerance."""
    case = GEOMETRY[ci]
    assert case.get('act', 'relu') == 'relu' and not case.get('residual')
    xs, w, b, res, gz, ref, _ = case_data(('geometry', ci), case, 7000 + ci, False)
    out = run_layer(case, mode, xs, w, b, res, gz, p16=True)
    check_path(case, mode, out)
    assert all(f in ('general_v1', 'general_v2', 'flat_valu') for f in out['fam']), out['fam']
    pass_bounds(case, out['fam'])
    bad, worst = check_layer(case, mode, out, ref, None)
    assert not bad and not worst, (bad, worst)
    if case.get('no_wino'):     # one field off the Winograd gate: planned as a direct layer too
        from dvs_of_training_framework_amd import conv as C
        x = torch.empty(1, device='cuda')
        o = layer_geometry(case)
        for m in range(4):
            d = C.make_desc([(x, c, C.NHWC) for c, _ in case['src']], case['B'], case['H'], case['W'],
                            case['Cout'], o['k'], o['stride'], o['pad'], o['up'], C.ACT_RELU, m)
            lib = C._lib.lib()
            assert [lib.dvsof_conv2d_winograd_tile(ctypes.byref(d), k) for k in range(3)] == [0, 0, 0]
            assert lib.dvsof_conv2d_scratch_bytes(ctypes.byref(d)) == 0


def test_the_cases_reach_every_general_kernel_of_every_pass():
    """The derived paths between them: v1 and v2 in all three passes, a flat weight-gradient
    family, and the quad and zero-insertion data gradients on v1 and on v2."""
    seen = {(kind, fam) for c in GEOMETRY for p in c['path'] for kind, fam in
            enumerate(t.partition(':')[0] for t in p.split())}
    assert {(k, f) for k in range(3) for f in ('general_v1', 'general_v2')} <= seen, seen
    assert (2, 'flat_valu') in seen
    dg = {(('quad' if c['up'] else 'zero2'), c['path'][0].split()[1]) for c in GEOMETRY
          if c['up'] or c['stride'] == 2}
    assert dg == {(f, g) for f in ('quad', 'zero2') for g in ('general_v1', 'general_v2')}, dg


def test_mode3_falls_back_on_a_narrow_member():
    """Mode 3 needs 32 | C of every NHWC member: beside a 16-channel member the up-sampled 5x5
    layer's forward runs as mode 1 (its data gradient reads gout alone: 32 channels, twins),
    with the same bits on the integer grid."""
    case = case_of('B2H5W6_32+16+2p_32_k5s1p2up')
    assert not twins_apply(case)
    xs, w, b, res, gz, ref, _ = case_data(('geometry', IDS.index(geometry_id(case))), case,
                                          7000 + GEOMETRY.index(case), False)
    out = run_layer(case, 3, xs, w, b, res, gz, p16=True)
    assert out['fam'] == ['general_v2', 'general_v2', 'general_v1'], out['fam']
    assert out['modes'] == [1, 3, 0], out['modes']
    pass_bounds(case, out['fam'])
    bad, _ = check_layer(case, 3, out, ref, None)
    assert not bad, bad


# ---------------------------------------------------------------------------
# 2. Random data against float64
# ---------------------------------------------------------------------------
_RANDOM = {}


def random_layer(ci):
    if ci not in _RANDOM:
        _RANDOM.clear()
        case = GEOMETRY[ci]
        g = torch.Generator().manual_seed(8000 + ci)
        B, H, W, Cout = case['B'], case['H'], case['W'], case['Cout']
        ctot = sum(c for c, _ in case['src'])
        ho, wo = out_hw(case)
        xs = [torch.randn(B, c, H, W, generator=g) for c, _ in case['src']]
        w = torch.randn(Cout, ctot, case['k'], case['k'], generator=g) / (ctot * case['k'] ** 2) ** 0.5
        b = torch.randn(Cout, generator=g)
        gz = torch.randn(B, Cout, ho, wo, generator=g)
        _RANDOM[ci] = (xs, w, b, gz, reference64(case, xs, w, b, None, gz))
    return _RANDOM[ci]


@pytest.mark.parametrize('ci,mode', [pytest.param(ci, m, id='%s-%s' % (IDS[ci], ('f32', 'bf16', 'bf16x3')[m]))
                                     for ci in range(len(GEOMETRY)) for m in range(3)])
def test_every_geometry_against_float64(ci, mode):
    case = GEOMETRY[ci]
    xs, w, b, gz, ref = random_layer(ci)
    out = run_layer(case, mode, xs, w, b, None, gz)
    check_path(case, mode, out)
    tol = (RTOL, BF16_RTOL, BF16X3_RTOL)[mode]
    close(out['y'], ref['y'], tol)
    close(out['z'], ref['z'], tol)
    for got, want in zip(out['dx'], ref['dx']):
        close(got, want, tol)
    close(out['dw'], ref['dw'], tol)
    close(out['db'], ref['db'], tol)


# ---------------------------------------------------------------------------
# 3. Every element written, nothing beyond
# ---------------------------------------------------------------------------
GUARD = 4096            # sentinel words on either side of a payload
SENTINEL = 0x7FC5A5A5   # a NaN no kernel produces


class Arena:
    """A payload of n floats, prefilled with NaN, between two runs of sentinel words."""

    def __init__(self, n):
        self.all = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.int32, device='cuda')
        self.n = n
        self.pay = self.all[GUARD:GUARD + n].view(torch.float32)
        self.pay.fill_(float('nan'))

    def check(self, what):
        assert bool((self.all[:GUARD] == SENTINEL).all()) and bool((self.all[GUARD + self.n:] == SENTINEL).all()), what
        assert bool(torch.isfinite(self.pay).all()), (what, int((~torch.isfinite(self.pay)).sum()), self.n)


def read_mask(n_in, n_out, k, stride, pad, up):
    """Which of n_in input rows (columns) some output row (column) reads."""
    hit = torch.zeros(n_in, dtype=torch.bool)
    for o in range(n_out):
        for t in range(k):
            v = o * stride - pad + t
            if 0 <= v < n_in * (2 if up else 1):
                hit[v >> 1 if up else v] = True
    return hit


UNREAD = {'B2H8W10_32_32_k3s2p0': (1, 1), 'B2H6W7_32_32_k1s2p0': (3, 3), 'B1H8W12_32_32_k5s2p0': (1, 1),
          'B1H8W8_5p_64_k3s2p0': (1, 1)}


def test_the_unread_rows_are_the_ones_the_cases_name():
    """(rows, columns) no output reads, per case: row 7 / column 9, every odd position,
    row 7 / column 11, row 7 / column 7 -- and none anywhere else in the list."""
    got = {}
    for name, case in zip(IDS, GEOMETRY):
        o = layer_geometry(case)
        ho, wo = out_hw(case)
        rows = read_mask(case['H'], ho, o['k'], o['stride'], o['pad'], o['up'])
        cols = read_mask(case['W'], wo, o['k'], o['stride'], o['pad'], o['up'])
        if not (rows.all() and cols.all()):
            got[name] = (int((~rows).sum()), int((~cols).sum()))
    assert got == UNREAD, got


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('ci', range(len(GEOMETRY)), ids=IDS)
def test_every_output_element_is_written_and_nothing_beyond(ci, mode):
    from dvs_of_training_framework_amd import conv as C
    case, o = GEOMETRY[ci], layer_geometry(GEOMETRY[ci])
    B, H, W, Cout = case['B'], case['H'], case['W'], case['Cout']
    ctot = sum(c for c, _ in case['src'])
    ho, wo = out_hw(case)
    lib = C._lib.lib()
    xs, w, b, _, gz = int_layer(case, 9000 + ci)
    dev = [(x.float().cuda().contiguous() if lay == 'nchw' else nhwc(x.float()))
           for x, (_, lay) in zip(xs, case['src'])]
    srcs = [(d, c, C.NCHW if lay == 'nchw' else C.NHWC) for d, (c, lay) in zip(dev, case['src'])]
    desc = C.make_desc(srcs, B, H, W, Cout, o['k'], o['stride'], o['pad'], o['up'], C.ACT_RELU, mode)
    w_f, w_dg = C.prepare(desc, wphys(w.float()), True)
    y, z = Arena(B * ho * wo * Cout), Arena(B * ho * wo * Cout)
    bias = b.float().cuda()
    C._lib.check(lib.dvsof_conv2d_fwd(ctypes.byref(desc), w_f.data_ptr(), bias.data_ptr(), None,
                                      y.pay.data_ptr(), z.pay.data_ptr(), C._lib.stream()), 'dvsof_conv2d_fwd')
    torch.cuda.synchronize()
    y.check('y')
    z.check('z')
    gz_d = nhwc(gz.float())
    rows = read_mask(H, ho, o['k'], o['stride'], o['pad'], o['up'])
    cols = read_mask(W, wo, o['k'], o['stride'], o['pad'], o['up'])
    unread = ~(rows[:, None] & cols[None, :])          # [H][W]
    assert bool(unread.any()) == (IDS[ci] in UNREAD)
    g = torch.Generator().manual_seed(9100 + ci)
    for with_epilogue in (False, True):
        dx = [Arena(B * c * H * W) for c, _ in case['src']]
        dsts, epi = [], []
        for a, x, (c, lay) in zip(dx, xs, case['src']):
            d = dict(p=a.pay)
            if with_epilogue:
                add, src = int_grid(g, x.shape, GRID['b']), int_grid(g, x.shape, 1)
                epi.append((add, src))
                put = (lambda t: t.float().cuda().contiguous()) if lay == 'nchw' else (lambda t: nhwc(t.float()))
                d.update(addend=put(add), actsrc=put(src))
            dsts.append(d)
        C.conv_dgrad(desc, w_dg, gz_d, dsts, C.ACT_RELU if with_epilogue else C.ACT_NONE)
        torch.cuda.synchronize()
        for i, (a, (c, lay)) in enumerate(zip(dx, case['src'])):
            a.check(('dx', i, with_epilogue))
            if not unread.any():
                continue
            t = a.pay.view(B, c, H, W) if lay == 'nchw' else a.pay.view(B, H, W, c).permute(0, 3, 1, 2)
            got = t.cpu()[:, :, unread]
            if with_epilogue:   # exactly act'(actsrc) * addend
                add, src = epi[i]
                assert torch.equal(got.double(), (add * (src > 0))[:, :, unread]), (i, 'epilogue')
            else:               # exactly +0: no set bit
                assert not bool(got.contiguous().view(torch.int32).any()), (i, got.abs().max().item())
    dw, db = Arena(Cout * o['k'] ** 2 * ctot), Arena(Cout)
    C.conv_wgrad(desc, gz_d, dw.pay, db.pay)
    torch.cuda.synchronize()
    dw.check('dw')
    db.check('db')


# ---------------------------------------------------------------------------
# 4. The data-gradient epilogue on the quad and the zero-insertion forms
# ---------------------------------------------------------------------------
EPILOGUE = ['B2H5W6_32+16+2p_32_k5s1p2up',     # DG_QUAD on v2 with a planar member
            'B1H5W6_20_24_k5s1p2up',           # DG_QUAD on v1
            'B2H9W11_24+2p_32_k3s2p1',         # DG_ZERO2 on v2 with a planar member
            'B2H9W11_32_32_k3s2p1',            # DG_ZERO2 on v2, mode 3 with the twins of dx
            'B2H9W11_32_24_k3s2p1']            # DG_ZERO2 on v1


@pytest.mark.parametrize('name,mode', [pytest.param(n, m, id='%s-m%d' % (n, m)) for n in EPILOGUE
                                       for m in modes_of(case_of(n)) if m != 2])
def test_dgrad_epilogue_on_the_quad_and_zero_insertion_forms(name, mode):
    """addend, addend2 and act'(actsrc) on every member: ReLU bit for bit with relu'(0) = 0,
    Mish within MISH_ULPS of (|dx| + |addends|) |mish'| like the nine-product epilogue."""
    from dvs_of_training_framework_amd import conv as C
    case = case_of(name)
    ci = IDS.index(name)
    xs, w, b, res, gz, ref, _ = case_data(('geometry', ci), case, 7000 + ci, False)
    g = torch.Generator().manual_seed(7500 + ci)
    a1 = [int_grid(g, x.shape, GRID['b']) for x in xs]
    a2 = [int_grid(g, x.shape, GRID['b']) for x in xs]
    src = [int_grid(g, x.shape, 1) for x in xs]
    want_fam = case['path'][mode].split()[1].partition(':')[0]
    form = 'quad' if case['up'] else 'zero2'

    def run(epi, bwd_act):
        out = run_layer(case, mode, xs, w, b, res, gz, p16=True, epi=epi, bwd_act=bwd_act)
        assert out['fam'][1] == want_fam, (form, out['fam'])
        pass_bounds(case, out['fam'])       # (its data-gradient bound leaves room for two addends)
        return out
    # one addend alone
    out = run([dict(addend=a) for a in a1], C.ACT_NONE)
    for i, (got, d, a) in enumerate(zip(out['dx'], ref['dx'], a1)):
        assert torch.equal(got.double(), d + a.cuda()), ('addend', i)
    # both addends and ReLU'
    out = run([dict(addend=a, addend2=c, actsrc=s) for a, c, s in zip(a1, a2, src)], C.ACT_RELU)
    want = dict(ref)
    want['dx'] = [(d + a.cuda() + c.cuda()) * (s.cuda() > 0).double() for d, a, c, s in zip(ref['dx'], a1, a2, src)]
    bad, _ = check_layer(case, mode, out, want, None)       # (and the twins of dx in mode 3)
    assert not bad, bad
    for got, s in zip(out['dx'], src):
        assert (s == 0).any() and (got.cpu()[s == 0] == 0).all()
    # both addends and Mish'
    out = run([dict(addend=a, addend2=c, actsrc=s) for a, c, s in zip(a1, a2, src)], C.ACT_MISH)
    for i, (got, d, a, c, s) in enumerate(zip(out['dx'], ref['dx'], a1, a2, src)):
        zs = s.clone().requires_grad_(True)
        mish_d = torch.autograd.grad(F.mish(zs).sum(), zs)[0].cuda()
        within_ulps(got, (d + a.cuda() + c.cuda()) * mish_d, (d.abs() + 2 * GRID['b']) * mish_d.abs() + 1, MISH_ULPS)


# ---------------------------------------------------------------------------
# 5. The bf16 rounding contract
# ---------------------------------------------------------------------------
# (name, the planar member's data gradient is exact f32): a general up-sampling layer rounds
# the RAW taps (conv_cases.fwd_form); in the quad form the planar member's columns stay in the
# matrix-core problem and round like the others (include/dvsof.h)
CONTRACT = [('B2H5W6_32+16+2p_32_k5s1p2up', False), ('B2H5W7_32_48_k1s1p0', True),
            ('B1H4W8_32+32_32_k3s1p0up', True)]


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('name,planar_exact', CONTRACT, ids=[n for n, _ in CONTRACT])
def test_bf16_modes_round_as_documented_off_the_subpixel_form(name, planar_exact, mode):
    case = dict(case_of(name), act='none')
    fams, res = emu_measure_case(case, 600 + IDS.index(name), mode, planar_dx_exact=planar_exact)
    assert fams == [t.partition(':')[0] for t in case['path'][mode].split()], fams
    for what, (r, rel, elem, alts) in res.items():
        tau = EMU_TAU[mode] if what != 'db' else EMU_TAU_DB
        assert rel <= tau, (what, r, rel)
        assert elem <= 1.0, (what, r, elem)
        for alt, dist in alts.items():       # the check could not pass the wrong rounding
            assert dist >= 100 * tau, (what, r, alt, dist)


# ---------------------------------------------------------------------------
# 6. Refusals
# ---------------------------------------------------------------------------
EINVAL = -1
ROOM = 1 << 16      # floats per buffer: more than any accepted neighbour of these descriptors needs
REFUSED = [
    ('pad == ksize (3x3)', dict(pad=3)), ('pad == ksize (1x1)', dict(k=1, pad=1)),
    ('pad == ksize (5x5)', dict(k=5, pad=5)), ('pad < 0', dict(pad=-1)),
    ('ksize 2', dict(k=2, pad=1)), ('ksize 4', dict(k=4, pad=1)), ('ksize 7', dict(k=7, pad=3)),
    ('stride 0', dict(stride=0)), ('stride 3', dict(stride=3)),
    ('up-sampling with stride 2', dict(up=True, stride=2)),
    ('frame too small for the taps', dict(H=4, W=4, k=5, pad=0)),
]


class Buffers:
    def __init__(self):
        f = lambda: torch.full((ROOM,), 7.0, device='cuda')     # noqa: E731
        self.x, self.bias, self.gout, self.ws = f(), f(), f(), f()
        self.w = torch.full((ROOM,), 0.5, device='cuda')        # (a copy of it is no 7.0 either)
        self.outs = dict(y=f(), z=f(), wf=f(), wd=f(), dx=f(), dw=f(), db=f())

    def touched(self):
        torch.cuda.synchronize()
        return [k for k, t in self.outs.items() if not bool((t == 7.0).all())]


def all_entry_points(C, desc, buf, dst):
    lib, r, st = C._lib.lib(), ctypes.byref(desc), C._lib.stream()
    o = buf.outs
    return dict(
        prepare=lib.dvsof_conv2d_prepare(r, buf.w.data_ptr(), o['wf'].data_ptr(), o['wd'].data_ptr(), st),
        fwd=lib.dvsof_conv2d_fwd(r, buf.w.data_ptr(), buf.bias.data_ptr(), None, o['y'].data_ptr(),
                                 o['z'].data_ptr(), st),
        dgrad=lib.dvsof_conv2d_dgrad(r, buf.w.data_ptr(), buf.gout.data_ptr(), dst, 0, st),
        wgrad=lib.dvsof_conv2d_wgrad(r, buf.gout.data_ptr(), o['dw'].data_ptr(), o['db'].data_ptr(),
                                     buf.ws.data_ptr(), ROOM * 4, st))


@pytest.mark.parametrize('what,change', REFUSED, ids=[w for w, _ in REFUSED])
def test_descriptors_outside_the_accepted_set_are_refused(what, change):
    """DVSOF_EINVAL from dvsof_conv2d_prepare, _fwd, _dgrad and _wgrad; nothing is written."""
    from dvs_of_training_framework_amd import conv as C
    f = dict(B=1, H=8, W=8, k=3, stride=1, pad=1, up=False)
    f.update(change)
    buf = Buffers()
    desc = C.make_desc([(buf.x, 32, C.NHWC)], f['B'], f['H'], f['W'], 32, f['k'], f['stride'], f['pad'], f['up'])
    dst = (C.GradDst * 1)()
    dst[0].p = buf.outs['dx'].data_ptr()
    rcs = all_entry_points(C, desc, buf, dst)
    assert rcs == dict(prepare=EINVAL, fwd=EINVAL, dgrad=EINVAL, wgrad=EINVAL), (what, rcs)
    assert buf.touched() == [], what
    # ... while the accepted neighbour runs in the same buffers
    ok = C.make_desc([(buf.x, 32, C.NHWC)], 1, 8, 8, 32, 3, 1, 1, False)
    rcs = all_entry_points(C, ok, buf, dst)
    assert rcs == dict(prepare=0, fwd=0, dgrad=0, wgrad=0), rcs
    assert sorted(buf.touched()) == sorted(buf.outs), 'the accepted neighbour writes every output'


def test_a_flow_head_is_refused_on_a_quad_layer():
    """head_w / head_gflow fold into the sub-pixel data gradients only: on an up-sampling layer
    that is not 3x3 / pad 1 (DG_QUAD) dvsof_conv2d_dgrad returns DVSOF_EINVAL and writes nothing."""
    from dvs_of_training_framework_amd import conv as C
    buf = Buffers()
    lib, st = C._lib.lib(), C._lib.stream()
    head_w, head_g = torch.zeros(2, 32, device='cuda'), torch.zeros(1, 2, 8, 8, device='cuda')
    for pad, want in ((0, EINVAL), (2, EINVAL), (1, 0)):
        desc = C.make_desc([(buf.x, 32, C.NHWC), (buf.x, 32, C.NHWC)], 1, 8, 8, 32, 3, 1, pad, True)
        assert lib.dvsof_conv2d_dgrad_fuses_head(ctypes.byref(desc)) == (1 if want == 0 else 0)
        assert lib.dvsof_conv2d_dgrad_head_rows(ctypes.byref(desc)) == 0
        assert lib.dvsof_conv2d_prepare(ctypes.byref(desc), buf.w.data_ptr(), buf.outs['wf'].data_ptr(),
                                        buf.outs['wd'].data_ptr(), st) == 0
        buf.outs['wf'].fill_(7.0)
        buf.outs['wd'].fill_(7.0)
        dx1 = torch.full((ROOM,), 7.0, device='cuda')
        dst = (C.GradDst * 2)()
        dst[0].p, dst[1].p = buf.outs['dx'].data_ptr(), dx1.data_ptr()
        dst[0].head_w, dst[0].head_gflow = head_w.data_ptr(), head_g.data_ptr()
        rc = lib.dvsof_conv2d_dgrad(ctypes.byref(desc), buf.w.data_ptr(), buf.gout.data_ptr(), dst, 0, st)
        assert rc == want, (pad, rc)
        torch.cuda.synchronize()
        if want == EINVAL:
            assert buf.touched() == [] and bool((dx1 == 7.0).all()), pad
            dst[0].head_w = dst[0].head_gflow = None       # ... and without the head it runs
            assert lib.dvsof_conv2d_dgrad(ctypes.byref(desc), buf.w.data_ptr(), buf.gout.data_ptr(), dst, 0, st) == 0
            assert C.KERNEL_NAMES[C.last_kernel(1)[0]] == 'general_v2'
            torch.cuda.synchronize()
            assert buf.touched() == ['dx'] and not bool((dx1 == 7.0).all())
            buf.outs['dx'].fill_(7.0)
