"""Argument rules of dvsof_conv2d_prepare16 / _fwd / _dgrad (include/dvsof.h): every
combination the entry points reject returns DVSOF_EINVAL, and one accepted neighbour of each
returns DVSOF_OK.  The combinations were read off the dispatch as it stood before the form
of a layer was classified in one place (csrc/conv_api.hip: conv_classify) and confirmed by
running that commit.  Every pointer is a real device buffer of the size its role needs, so
a call that is wrongly accepted is a harmless launch and a failed assert.

Layers (the smallest that select each form): sub-pixel 32 + 32 -> 32 at 8 x 16 (nine-product
forward, general data gradient), 64 + 64 -> 32 at 8 x 16 (nine-product data gradient too),
32 + 32 -> 32 at 6 x 16 (the nine-product gate refuses: 4 does not divide H), Winograd at its
gate (B 2, 16 x 16, 512 -> 512: 128 tiles of 2 x 2), transposed 16 -> 16 at 4 x 4, stride 2
16 -> 32 at 8 x 8."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

EINVAL, OK = -1, 0


class Layer:
    """A descriptor with every buffer a call on it may name."""

    def __init__(self, B, H, W, chans, Cout, stride=1, up=0):
        from dvs_of_training_framework_amd import conv as C
        self.C, self.B, self.H, self.W, self.chans, self.Cout = C, B, H, W, chans, Cout
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')   # noqa: E731
        self.x = [z(B, H, W, c) for c in chans]
        self.desc = C.make_desc([(x, c, C.NHWC) for x, c in zip(self.x, chans)], B, H, W, Cout,
                                3, stride, 1, up)
        lib, ref = C._lib.lib(), ctypes.byref(self.desc)
        ctot = sum(chans)
        nf, nd = lib.dvsof_conv2d_fwd_weight_elems(ref), lib.dvsof_conv2d_dgrad_weight_elems(ref)
        assert nf >= 9 * Cout * ctot and nd >= 9 * Cout * ctot
        # (the raw weight as large as the forward form: an in-place call that is wrongly
        # accepted stays inside it)
        self.w = z(max(nf, 9 * Cout * ctot))
        self.wf, self.wd = z(nf), z(nd)
        self.wf16, self.wd16 = z(nf, dt=torch.bfloat16), z(nd, dt=torch.bfloat16)
        ho, wo = C.out_size(self.desc)
        self.y, self.gout = z(B, ho, wo, Cout), z(B, ho, wo, Cout)
        self.dx = [z(B, H, W, c) for c in chans]
        nscr = lib.dvsof_conv2d_scratch_bytes(ref)
        self.scratch = z(max(nscr // 4, 4))
        self.desc.scratch, self.desc.scratch_bytes = self.scratch.data_ptr(), nscr
        # a Winograd form of this frame, whichever channel count and tile it is for
        self.form = z(36 * B * (max(H, 4) // 2) * (max(W, 4) // 2) * max(Cout, ctot))
        # a flow head on member 0: weights, the flow's gradient, partials of its weight gradient
        self.head_w, self.head_g = z(2, chans[0]), z(B, 2, H, W)
        rows = lib.dvsof_conv2d_dgrad_head_rows(ref)
        self.head_rows = rows
        self.head_part = z(max(rows, 1), 2 * chans[0] + 2)

    def prepare16(self, weight=None, w_fwd=None, w_dgrad=None, w_fwd16=None, w_dgrad16=None):
        p = self.C._lib.ptr
        return self.C._lib.lib().dvsof_conv2d_prepare16(
            ctypes.byref(self.desc), p(weight), p(w_fwd), p(w_dgrad), p(w_fwd16), p(w_dgrad16),
            self.C._lib.stream())

    def _chain(self, pre=None, nxt=None, nxt_gout=None):
        p = self.C._lib.ptr
        self.desc.winograd_pre, self.desc.winograd_next = p(pre), p(nxt)
        self.desc.winograd_next_gout = p(nxt_gout)

    def fwd(self, **chain):
        self._chain(**chain)
        rc = self.C._lib.lib().dvsof_conv2d_fwd(
            ctypes.byref(self.desc), self.wf.data_ptr(), None, None, self.y.data_ptr(), None,
            self.C._lib.stream())
        self._chain()
        return rc

    def dgrad(self, heads=None, **chain):
        """heads: per member dict(head_w=, head_gflow=, head_x=, head_part=)."""
        arr = (self.C.GradDst * len(self.chans))()
        for i, t in enumerate(self.dx):
            arr[i].p = t.data_ptr()
            for k, v in ((heads or {}).get(i) or {}).items():
                setattr(arr[i], k, self.C._lib.ptr(v))
        self._chain(**chain)
        rc = self.C._lib.lib().dvsof_conv2d_dgrad(
            ctypes.byref(self.desc), self.wd.data_ptr(), self.gout.data_ptr(), arr, 0,
            self.C._lib.stream())
        self._chain()
        return rc


@pytest.fixture(scope='module')
def layers():
    L = dict(sub9=Layer(1, 8, 16, (32, 32), 32, up=1),        # nine-product forward only
             sub9d=Layer(1, 8, 16, (64, 64), 32, up=1),       # ... and data gradient
             sub=Layer(1, 6, 16, (32, 32), 32, up=1),         # refused by the nine-product gate
             wino=Layer(2, 16, 16, (512,), 512),
             tr=Layer(1, 4, 4, (16,), 16, up=2),
             s2=Layer(1, 8, 8, (16,), 32, stride=2))
    yield L
    torch.cuda.synchronize()


def check(table):
    got = [(name, rc, want) for name, rc, want in table]
    for name, rc, want in got:
        print(f'{name}: rc {rc} (want {want})')
    wrong = [g for g in got if g[1] != g[2]]
    assert not wrong, wrong


def test_the_layers_take_the_forms_they_are_here_for(layers):
    C = layers['s2'].C
    lib = C._lib.lib()
    rows = {k: v.head_rows for k, v in layers.items()}
    assert rows['sub9d'] > 0 and all(v == 0 for k, v in rows.items() if k != 'sub9d'), rows
    tile = {k: lib.dvsof_conv2d_winograd_tile(ctypes.byref(v.desc), 0) for k, v in layers.items()}
    assert tile['wino'] == 2 and all(v == 0 for k, v in tile.items() if k != 'wino'), tile
    fam = {}
    for k, v in layers.items():
        assert v.prepare16(v.w, v.wf, v.wd) == OK, k
        assert v.fwd() == OK and v.dgrad() == OK, k
        fam[k] = (C.KERNEL_NAMES[C.last_kernel(0)[0]], C.KERNEL_NAMES[C.last_kernel(1)[0]])
    torch.cuda.synchronize()
    assert fam.pop('sub9d')[1].startswith('dgrad_min'), fam
    assert fam == dict(sub9=('fwd_min4', 'general_v2'),
                       sub=('general_v2', 'general_v2'), wino=('wino2', 'wino2'),
                       tr=('transposed', 'general_v2'), s2=('general_v2', 'stride2_phased')), fam


def test_prepare16_argument_rules(layers):
    t = []
    for k, v in layers.items():     # a data-gradient twin goes with its form
        if k != 'wino':
            t.append((f'{k}: w_dgrad16 without w_dgrad', v.prepare16(v.w, v.wf, None, None, v.wd16), EINVAL))
    for k in ('sub', 's2', 'tr'):
        v = layers[k]
        t.append((f'{k}: w_dgrad16 with w_dgrad', v.prepare16(v.w, v.wf, v.wd, None, v.wd16), OK))
    for k in ('sub9', 'sub9d', 'sub'):
        v = layers[k]
        t += [(f'{k}: neither weight nor w_fwd', v.prepare16(None, None, v.wd), EINVAL),
              (f'{k}: nothing to make', v.prepare16(v.w, None, None), EINVAL),
              (f'{k}: w_fwd given, no weight, no w_dgrad', v.prepare16(None, v.wf, None), EINVAL),
              (f'{k}: data-gradient form from the raw weights', v.prepare16(v.w, None, v.wd), OK),
              (f'{k}: forward form alone', v.prepare16(v.w, v.wf, None), OK)]
    sub, sub9, sub9d = layers['sub'], layers['sub9'], layers['sub9d']
    t += [('sub: data-gradient form from the phase kernels', sub.prepare16(None, sub.wf, sub.wd), OK),
          ('sub: ... with both twins', sub.prepare16(None, sub.wf, sub.wd, sub.wf16, sub.wd16), OK),
          ('sub: forward form with its twin', sub.prepare16(sub.w, sub.wf, None, sub.wf16), OK),
          ('sub9: no weight', sub9.prepare16(None, sub9.wf, sub9.wd), EINVAL),
          ('sub9: nine-product forward form with a twin', sub9.prepare16(sub9.w, sub9.wf, None, sub9.wf16), EINVAL),
          ('sub9: ... without', sub9.prepare16(sub9.w, sub9.wf, sub9.wd), OK),
          ('sub9: twin of the general data-gradient form', sub9.prepare16(sub9.w, None, sub9.wd, None, sub9.wd16), OK),
          ('sub9d: nine-product data-gradient form with a twin',
           sub9d.prepare16(sub9d.w, None, sub9d.wd, None, sub9d.wd16), EINVAL),
          ('sub9d: ... without', sub9d.prepare16(sub9d.w, sub9d.wf, sub9d.wd), OK)]
    w = layers['wino']
    t += [('wino: w_fwd16', w.prepare16(w.w, w.wf, w.wd, w.wf16, None), EINVAL),
          ('wino: w_dgrad16', w.prepare16(w.w, w.wf, w.wd, None, w.wd16), EINVAL),
          ('wino: no weight', w.prepare16(None, w.wf, w.wd), EINVAL),
          ('wino: nothing to make', w.prepare16(w.w, None, None), EINVAL),
          ('wino: both forms', w.prepare16(w.w, w.wf, w.wd), OK),
          ('wino: one form', w.prepare16(w.w, None, w.wd), OK)]
    tr = layers['tr']
    t += [('tr: w_fwd == weight', tr.prepare16(tr.w, tr.w, tr.wd), EINVAL),
          ('tr: no weight', tr.prepare16(None, tr.wf, tr.wd), EINVAL),
          ('tr: nothing to make', tr.prepare16(tr.w, None, None), EINVAL),
          ('tr: both forms with twins', tr.prepare16(tr.w, tr.wf, tr.wd, tr.wf16, tr.wd16), OK)]
    s2 = layers['s2']
    t += [('s2: no weight', s2.prepare16(None, s2.wf, s2.wd), EINVAL),
          ('s2: w_fwd == weight', s2.prepare16(s2.w, s2.w, s2.wd, s2.wf16, s2.wd16), OK),
          ('s2: the raw twin alone', s2.prepare16(s2.w, None, None, s2.wf16, None), OK),
          ('s2: weight alone', s2.prepare16(s2.w), OK)]
    torch.cuda.synchronize()
    check(t)


def test_fwd_argument_rules(layers):
    t = []
    for k, v in layers.items():
        assert v.prepare16(v.w, v.wf, v.wd) == OK
        t.append((f'{k}: winograd_next_gout on a forward', v.fwd(nxt_gout=v.form), EINVAL))
        if k != 'wino':
            t += [(f'{k}: winograd_pre off the Winograd path', v.fwd(pre=v.form), EINVAL),
                  (f'{k}: winograd_next off the Winograd path', v.fwd(nxt=v.form), EINVAL)]
        t.append((f'{k}: plain forward', v.fwd(), OK))
    torch.cuda.synchronize()
    check(t)


def test_dgrad_argument_rules(layers):
    t = []
    for k, v in layers.items():
        assert v.prepare16(v.w, v.wf, v.wd) == OK
        hw, hg, hp = v.head_w, v.head_g, v.head_part
        folds = k in ('sub9', 'sub9d', 'sub')
        if k not in ('wino', 'sub9d'):      # (the nine-product data gradient never looked at them)
            t += [(f'{k}: winograd_pre off the Winograd path', v.dgrad(pre=v.form), EINVAL),
                  (f'{k}: winograd_next_gout off the Winograd path', v.dgrad(nxt_gout=v.form), EINVAL)]
        t += [(f'{k}: plain data gradient', v.dgrad(), OK),
              (f'{k}: head_w without head_gflow', v.dgrad({0: dict(head_w=hw)}), EINVAL),
              (f'{k}: head_gflow without head_w', v.dgrad({0: dict(head_gflow=hg)}), EINVAL),
              (f'{k}: head_part without head_x', v.dgrad({0: dict(head_w=hw, head_gflow=hg, head_part=hp)}), EINVAL),
              (f'{k}: head_part without head_w', v.dgrad({0: dict(head_x=v.x[0], head_part=hp)}), EINVAL),
              (f'{k}: head folded on member 0', v.dgrad({0: dict(head_w=hw, head_gflow=hg)}), OK if folds else EINVAL),
              (f'{k}: head_part', v.dgrad({0: dict(head_w=hw, head_gflow=hg, head_x=v.x[0], head_part=hp)}),
               OK if k == 'sub9d' else EINVAL)]
        if len(v.chans) > 1:
            t.append((f'{k}: head_w on member 1', v.dgrad({1: dict(head_w=hw, head_gflow=hg)}), EINVAL))
    torch.cuda.synchronize()
    check(t)
