"""The weight gradient's workspace invariant (csrc/wgrad_plan.hip): the size that
dvsof_conv2d_wgrad_workspace_bytes answers from the shape alone covers the plan of every
call of that shape -- with or without a bias gradient, in mode 3 with the bf16 twins bound or
not.  For every layer of tests/conv_cases.py (the last five of CASES are there for the plan
outcomes the others miss; GEOMETRY adds the layers off the 3x3 / pad-1 forms) the call runs in a workspace of exactly that many bytes, placed inside a
larger tensor whose remainder holds a sentinel: it returns DVSOF_OK, leaves the sentinel
alone and writes, bit for bit, the dW and dbias of the same call in a generous workspace."""
import ctypes

import pytest
import torch

from tests.conv_cases import CASES, GEOMETRY, TWIN_LAYERS, WGRAD_TWIN_CASES, layer_geometry, twins_apply

pytestmark = pytest.mark.gpu

GUARD = 4096            # sentinel floats on either side of the workspace
SENTINEL = 0x7FC5A5A5   # a NaN no kernel produces


def _key(c):
    return (c['B'], c['H'], c['W'], tuple(c['src']), c['Cout'], c.get('k', 3), c.get('stride', 1),
            c.get('pad', 1), c.get('up', False))


LAYERS = list({_key(c): c for c in CASES + [c for c, _, _ in TWIN_LAYERS] + WGRAD_TWIN_CASES + GEOMETRY}.values())
PARAMS = [(li, m) for li in range(len(LAYERS)) for m in range(4) if m != 3 or twins_apply(LAYERS[li])]


def out_hw(case):
    o = layer_geometry(case)
    up = 2 if o['up'] else 1
    return ((case['H'] * up + 2 * o['pad'] - o['k']) // o['stride'] + 1,
            (case['W'] * up + 2 * o['pad'] - o['k']) // o['stride'] + 1)


@pytest.mark.parametrize('li,mode', PARAMS)
def test_sized_workspace_covers_every_call_of_the_shape(li, mode):
    from dvs_of_training_framework_amd import conv as C
    case, o = LAYERS[li], layer_geometry(LAYERS[li])
    B, H, W, Cout = case['B'], case['H'], case['W'], case['Cout']
    lib = C._lib.lib()
    g = torch.Generator(device='cuda').manual_seed(li)
    small = lambda *s: torch.randint(-1, 2, s, generator=g, device='cuda').float()   # noqa: E731
    xs = [small(B, c, H, W) if lay == 'nchw' else small(B, H, W, c) for c, lay in case['src']]
    ho, wo = out_hw(case)
    gout = small(B, ho, wo, Cout)
    ctot = sum(c for c, _ in case['src'])

    def desc(twins):
        srcs = [(x, c, C.NCHW if lay == 'nchw' else C.NHWC,
                 x.to(torch.bfloat16) if (twins and lay == 'nhwc') else None)
                for x, (c, lay) in zip(xs, case['src'])]
        d = C.make_desc(srcs, B, H, W, Cout, o['k'], o['stride'], o['pad'], o['up'], C.ACT_RELU, mode)
        d._keep = srcs
        return d
    # sized from the shape: no twin, no gout is known yet
    need = lib.dvsof_conv2d_wgrad_workspace_bytes(ctypes.byref(desc(False)))
    assert need % 4 == 0
    arena = torch.empty(2 * GUARD + need // 4, dtype=torch.int32, device='cuda')
    roomy = torch.empty(4 * (need // 4) + (1 << 18), dtype=torch.float32, device='cuda')

    def run(d, g16, with_bias, ws_ptr, ws_bytes):
        dw = torch.full((Cout, o['k'], o['k'], ctot), float('nan'), device='cuda')
        db = torch.full((Cout,), float('nan'), device='cuda') if with_bias else None
        d.gout16 = C._lib.ptr(g16)
        rc = lib.dvsof_conv2d_wgrad(ctypes.byref(d), gout.data_ptr(), dw.data_ptr(), C._lib.ptr(db),
                                    ws_ptr, ws_bytes, C._lib.stream())
        return rc, dw, db, C.last_kernel(2)

    for twins in ((False, True) if mode == 3 else (False,)):
        d = desc(twins)
        g16 = gout.to(torch.bfloat16) if twins else None
        for with_bias in (False, True):
            rc0, dw0, db0, k0 = run(d, g16, with_bias, roomy.data_ptr(), roomy.numel() * 4)
            arena.fill_(SENTINEL)
            rc, dw, db, k = run(d, g16, with_bias, arena.data_ptr() + 4 * GUARD, need)
            torch.cuda.synchronize()
            what = (case, mode, twins, with_bias, need, k)
            assert rc0 == 0 and rc == 0, (rc0, rc, what)
            assert k == k0, (k0, what)
            assert bool((arena[:GUARD] == SENTINEL).all()) and bool((arena[GUARD + need // 4:] == SENTINEL).all()), what
            assert not torch.isnan(dw).any() and torch.equal(dw, dw0), what
            if with_bias:
                assert not torch.isnan(db).any() and torch.equal(db, db0), what
