"""EV_FlowNet predictor (docs/MODEL_SPEC.md) on the HIP conv stack.

The reference imports ``EV_FlowNet.net.Model`` whose source is an un-vendored
submodule; what the reference pins is the contract:
4 flow maps coarse to fine at ``imsize // 2**i`` (DummyNet/net.py:59-66,
tests/training/test_training.py:45-46), attribute ``predictor`` with
state-dict names ``predictor.enc.N.conv.*`` (train_flownet.py:50-54,79-85).
The architecture is the canonical EV-FlowNet (Zhu et al., RSS 2018):

  enc.i   3x3 stride-2 conv + act,  C -> 64 -> 128 -> 256 -> 512
  res.i   x + conv2(act(conv1(x))), then act          (2 blocks at 512)
  dec.i   3x3 conv + act on the 2x nearest-upsampled concat[x, skip, flow]
          -> 256, 128, 64, 32;  dec.i.flow = 1x1 conv -> 2 (linear head)

``LAYERS`` is the one description of these 12 conv layers (members, frames,
parameters, gradient units); modules, parameter order, FLOPs, the forward's
loop and the backward's lookups all read it.

Forward and backward are ONE autograd node with an explicit schedule: the
backward pass is ~45 launches of the gather-conv / wgrad / head kernels with
the gradient sums and activation derivatives folded into kernel epilogues
(no autograd graph, no cat/upsample tensors, no elementwise passes).
"""
import contextlib
import math
import os
from typing import NamedTuple

import torch
from torch import nn

from . import conv as C

_SIDE_STREAMS = {}      # device index -> the second backward stream

ENC_CH = (64, 128, 256, 512)
DEC_CH = (256, 128, 64, 32)
NUM_RES = 2

VOXELS = -1             # Layer.inputs: the network's input


class Layer(NamedTuple):
    """One conv layer of the network: everything about it that is no tensor."""
    unit: tuple         # gradient unit key: ('enc', i) | ('res', i, 1 | 2) | ('dec', i)
    srcs: tuple         # source members (channels, layout); channels None: the input's
    inputs: tuple       # per member VOXELS | the layer whose output it is | ('flow', layer)
    cout: int
    stride: int
    up: bool            # 2x nearest upsampling of the concatenated members
    shift: int          # its frame is (H >> shift, W >> shift)
    params: tuple       # indices in param_list(): w, b and, with a flow head, flow w, flow b
    residual: object    # the layer whose output is added ahead of the activation, or None
    chained: tuple      # (its producer, its consumer) is a Winograd layer of the same frame

    @property
    def name(self):
        return '.'.join(map(str, self.unit))


def _layer_table():
    """The 12 conv layers in forward order; parameters numbered as they come."""
    table = []

    def add(unit, srcs, inputs, cout, shift, stride=1, up=False, residual=None,
            chained=(False, False), head=False):
        first = table[-1].params[-1] + 1 if table else 0
        table.append(Layer(unit, tuple(srcs), tuple(inputs), cout, stride, up, shift,
                           tuple(range(first, first + (4 if head else 2))), residual, chained))
        return len(table) - 1
    c, lay, x, deep = None, C.NCHW, VOXELS, len(ENC_CH)
    for i, cout in enumerate(ENC_CH):
        x = add(('enc', i), [(c, lay)], [x], cout, i, stride=2)
        c, lay = cout, C.NHWC
    skips = list(range(deep))
    for i in range(NUM_RES):
        t = add(('res', i, 1), [(c, lay)], [x], c, deep, chained=(i > 0, True))
        x = add(('res', i, 2), [(c, lay)], [t], c, deep, residual=x,
                chained=(True, i + 1 < NUM_RES))
    for i, cout in enumerate(DEC_CH):
        skip = skips.pop()
        srcs, inputs = [(c, lay), (ENC_CH[skip], lay)], [x, skip]
        if i > 0:       # the flow of the stage below
            srcs.append((2, C.NCHW))
            inputs.append(('flow', x))
        x = add(('dec', i), srcs, inputs, cout, deep - i, up=True, head=True)
        c = cout
    return tuple(table)


LAYERS = _layer_table()
# layer indices by part of the network (the backward walks them in reverse)
_ENC = tuple(i for i, l in enumerate(LAYERS) if l.unit[0] == 'enc')
_RES = tuple((l.inputs[0], i) for i, l in enumerate(LAYERS) if l.residual is not None)
_DEC = tuple(i for i, l in enumerate(LAYERS) if l.unit[0] == 'dec')


def activation_id(activation):
    """nn.ReLU -> ACT_RELU, Mish-like module -> ACT_MISH
    (reference: utils/options.py:341-347 passes nn.ReLU() or Mish())."""
    if activation is None or isinstance(activation, nn.ReLU):
        return C.ACT_RELU
    if isinstance(activation, nn.Identity):
        return C.ACT_NONE
    if type(activation).__name__.lower() == 'mish':
        return C.ACT_MISH
    raise ValueError(f'unsupported activation {activation!r}: the HIP conv '
                     'stack fuses ReLU or Mish')


class ConvParams(nn.Module):
    """weight [Cout,Cin,k,k] stored channels_last = physical [Cout][k][k][Cin]
    (the K-contiguous layout the MFMA kernels stream), bias [Cout]."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.cin, self.cout, self.k = cin, cout, k
        w = torch.empty(cout, cin, k, k).contiguous(
            memory_format=torch.channels_last)
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.empty(cout))
        self.reset_parameters()

    def reset_parameters(self):
        # nn.Conv2d's default init
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1 / math.sqrt(self.cin * self.k * self.k)
        nn.init.uniform_(self.bias, -bound, bound)


class _Named(nn.Module):
    def __init__(self, **mods):
        super().__init__()
        for k, v in mods.items():
            self.add_module(k, v)


def _prep(desc, weight, want_dgrad, phase_weights=None, want16=False):
    """conv.prepare -> always (w_fwd, w_dgrad, w_fwd16, w_dgrad16)."""
    out = C.prepare(desc, weight, want_dgrad, phase_weights, want16)
    return out if want16 else (out[0], out[1], None, None)


def _phys(w):
    """Physical [Cout][k][k][Cin] buffer of a channels_last OIHW weight."""
    assert w.permute(0, 2, 3, 1).is_contiguous(), \
        'conv weights must stay in channels_last memory format'
    return w


class _NoTensor:
    """Source member of a descriptor made before the layer's inputs exist: conv.prepare and
    the planning queries read the shape fields only, and want an address that is not NULL."""
    @staticmethod
    def data_ptr():
        return 4096


class _Fold(NamedTuple):
    """Decoder stage run on cat[x, skip], its flow member folded into weight space
    (csrc/flowfold.hip): what forward and backward share."""
    desc: object        # the two-member descriptor forward and data gradient run on
    w: object           # the stage's raw weight
    cx: int             # channels of x = column where the skip member starts
    cf_off: int         # column where the flow member starts
    ctot: int
    head: tuple         # param_list() indices of (w, b) of the head below, whose flow it is
    keep: tuple         # forms made on the second stream and read on the main one


class _Done(NamedTuple):
    """A layer as the forward leaves it for the backward."""
    desc: object
    y: object
    z: object
    srcs: list
    w_dg: object
    w_dg16: object
    fold: object


class _Plan:
    """The weight forms of one step: which stream makes each, and where the main stream
    first waits for them."""
    # Training with the second stream, that stream makes, in this order: the bf16 twins of
    # the raw weights, every prepared FORWARD form (Winograd-domain weights of the residual
    # layers, sub-pixel phase kernels of the decoder: not needed before the encoder has
    # run), then layer by layer beside the forward the data-gradient forms, which only the
    # backward needs.  The main stream waits once for the twins and once for the forward
    # forms, each at the first layer that takes one.  A forward form that was not made ahead
    # is made on the main stream where it is used, and the second stream waits for it.
    # Without the second stream (DVSOF_WGRAD_STREAM=0, inference) everything is made on the
    # main stream: folded decoder stages at the top, the rest where it is used.

    def __init__(self, module, dims, params, want_grad, dev):
        self.dims, self.act, self.mfma = dims, module.act, module.mfma
        self.params, self.want_grad = params, want_grad
        self.twins = twins = module.mfma == C.MFMA_BF16_TWINS
        self.main = torch.cuda.current_stream(dev)
        self.side = side = module._wgrad_stream(dev) if want_grad else None
        begin = module._take_step_begin()
        # The second stream first waits for everything enqueued so far (the optimizer's
        # update of the weights; the previous backward's readers of the buffers it is about
        # to reuse) ...
        if side is not None:
            # ... or, when the caller marked the start of the step (mark_step_begin, ahead
            # of the voxeliser), only for what preceded THAT: nothing made here reads the
            # event volume, so the forms run beside the voxeliser and the first layers
            if begin is not None:
                side.wait_event(begin)
            else:
                side.wait_stream(self.main)
        self.pending = {}       # 'raw16' | 'fwd' -> event the main stream has yet to wait for
        # bf16-twins mode: the twins of the weights that are used as they are
        # (stride-2 encoder layers, direct residual layers) in ONE launch; the
        # twins of prepared forms come from the kernels that make the forms
        self.raw16 = {}         # layer -> twin of its raw weight
        if twins:
            raws = [li for li, l in enumerate(LAYERS) if not l.up]
            # on the second stream when there is one (16 us off the forward's lane)
            with self._on_side():
                self.raw16 = dict(zip(raws, C.to_bf16_many(
                    [_phys(params[LAYERS[li].params[0]]) for li in raws])))
                self._record('raw16')
        self.fwd, self.folds = {}, {}       # layer -> (w_fwd, w_fwd16) | folded forms
        if want_grad:
            with self._on_side():
                for li, l in enumerate(LAYERS):
                    if len(l.srcs) == 3:
                        # decoder stage with a flow member: when training, forward AND
                        # backward run on cat[x, skip] with the head folded into the
                        # weights; in inference the member stays a member
                        self.folds[li] = self._fold_forms(l)
                    elif side is not None and l.stride == 1:    # (the encoder's: where used)
                        w = params[l.params[0]]
                        w_f, _, w_f16, _ = _prep(self.desc(l)[1], _phys(w), False, want16=twins)
                        if w_f is not w:
                            self.fwd[li] = (w_f, w_f16)
                self._record('fwd')
        # (Measured and not kept: the data-gradient weight forms issued late, beside the
        # decoder's kernels instead of layer by layer beside the encoder / residual layers:
        # 2.522-2.530 ms wherever they run -- the step is bound by total work, and the forms
        # cost 63 us of it: 2.451 ms with the forms of the first step reused, which is wrong.)

    def _on_side(self):
        return torch.cuda.stream(self.side) if self.side is not None \
            else contextlib.nullcontext()

    def _record(self, what):
        if self.side is not None:
            self.pending[what] = torch.cuda.Event()
            self.pending[what].record(self.side)

    def _await(self, what):
        ev = self.pending.pop(what, None)
        if ev is not None:
            self.main.wait_event(ev)

    def desc(self, l, members=()):
        """-> (srcs, descriptor) of table layer ``l`` on ``members``, its first sources as
        (tensor, bf16 twin or None); none: shapes only."""
        B, Cin, H, W = self.dims
        members = members or ((_NoTensor, None),) * len(l.srcs)
        srcs = [(t, c or Cin, lay, t16) for (c, lay), (t, t16) in zip(l.srcs, members)]
        return srcs, C.make_desc(srcs, B, H >> l.shift, W >> l.shift, l.cout, 3, l.stride,
                                 1, l.up, self.act, self.mfma)

    def _fold_forms(self, l):
        (cx, _), (cs, _) = l.srcs[:2]
        ctot = cx + cs + 2
        w, bias = (self.params[i] for i in l.params[:2])
        head = LAYERS[l.inputs[2][1]].params[2:]
        wh, bh = (self.params[i] for i in head)
        w_eff = C.flow_fold_weights(_phys(w), l.cout, ctot, 0, cx, cx + cs, wh)
        b_eff, b_cls = C.flow_fold_bias(_phys(w), l.cout, ctot, cx + cs, bh, bias)
        d2 = self.desc(l, ((_NoTensor, None),) * 2)[1]
        w_f, _, w_f16, _ = _prep(d2, w_eff, False, want16=self.twins)
        return _Fold(None, w, cx, cx + cs, ctot, head, (w_eff, w_f, w_f16, b_eff, b_cls))

    def layer(self, li, l, d, members):
        """-> (descriptor to run on, forward form, its twin, bias, bias table, data-gradient
        form, its twin, _Fold or None) of layer ``li`` = ``l`` described by ``d``."""
        twins, side = self.twins, self.side
        w, bias = (self.params[i] for i in l.params[:2])
        fold = self.folds.get(li)
        if fold is not None:
            self._await('fwd')
            w_eff, w_f, w_f16, b_eff, b_cls = fold.keep
            d2 = self.desc(l, members[:2])[1]
            with self._on_side():
                _, w_dg, _, w_dg16 = _prep(d2, w_eff, True, phase_weights=w_f, want16=twins)
            return d2, w_f, w_f16, b_eff, b_cls, w_dg, w_dg16, fold._replace(desc=d2)
        # the voxel input needs no data gradient
        need_dg = self.want_grad and l.inputs[0] != VOXELS
        if side is not None and need_dg:
            if li in self.fwd:          # made ahead on the second stream
                w_fwd, w_fwd16 = self.fwd[li]
                self._await('fwd')
            else:
                w_fwd, w_fwd16 = C.prepare(d, _phys(w), False)[0], None
                if w_fwd is not w:      # prepared form made on main
                    ev = torch.cuda.Event()
                    ev.record(self.main)
                    side.wait_event(ev)
            with torch.cuda.stream(side):
                _, w_dg, _, w_dg16 = _prep(d, _phys(w), True, phase_weights=w_fwd,
                                           want16=twins)
        else:
            w_fwd, w_dg, w_fwd16, w_dg16 = _prep(d, _phys(w), need_dg, want16=twins)
        if twins and w_fwd16 is None:
            self._await('raw16')
            w_fwd16 = self.raw16.get(li)
            if w_fwd16 is None or w_fwd is not w:
                w_fwd16 = C.to_bf16(w_fwd)
        return d, w_fwd, w_fwd16, bias, None, w_dg, w_dg16, None

    def close(self):
        """-> the event after the last data-gradient form (None: all on the main stream)."""
        self._record('dg')
        return self.pending.pop('dg', None)


class _PredictorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, module, want_grad, *params):
        dev, act = x0.device, module.act
        B, Cin, H, W = dims = tuple(x0.shape)
        mish = act == C.ACT_MISH
        plan = _Plan(module, dims, params, want_grad, dev)
        L = []                          # per conv layer: _Done
        # what the layers read: activations travel as (f32 tensor, bf16 twin or None)
        outs = {VOXELS: (x0, None)}
        flows, heads = [], []
        chain = None    # Winograd form a layer made for its consumer: the transformed input
        # travels from output transform to GEMM (dvsof_conv_desc_t.winograd_next)
        for li, l in enumerate(LAYERS):
            members = [outs[k] for k in l.inputs]
            srcs, d = plan.desc(l, members)
            d_run, w_fwd, w_fwd16, bias, bias_cls, w_dg, w_dg16, fold = \
                plan.layer(li, l, d, members)
            v_pre = chain if l.chained[0] else None
            chain = C.winograd_form(d, l.cout, dev) \
                if l.chained[1] and C.winograd_chain(d, 0) else None
            y, z = C.conv_fwd(d_run, w_fwd, bias, dev,
                              None if l.residual is None else outs[l.residual][0], mish,
                              keep_input_transform=want_grad, weight16=w_fwd16,
                              bias_cls=bias_cls, wino_pre=v_pre, wino_next=chain)
            L.append(_Done(d, y, z, srcs, w_dg, w_dg16, fold))
            # in the bf16-twins mode the same kernel wrote the output's bf16 copy
            outs[li] = (y, d_run._y16)
            if len(l.params) == 4:
                h, w = C.out_size(d)
                head = (y, params[l.params[2]], params[l.params[3]], h, w, l.cout)
                if want_grad:
                    # folded: no later stage reads this flow -- all four heads run in
                    # one launch after the last stage (the tensor is only named here)
                    flow = torch.empty(B, 2, h, w, dtype=torch.float32, device=dev)
                    heads.append(head)
                else:
                    flow = C.head_fwd(*head[:3], B, h, w, l.cout)
                outs['flow', li] = (flow, None)
                flows.append(flow)
        if heads:
            C.heads_fwd(heads, B, out=flows)
        if want_grad:
            ctx.dg_ready = plan.close()
            ctx.L, ctx.act, ctx.dims = L, act, dims
            ctx.raw16 = plan.raw16  # made on the second stream, read on this one: alive until backward
            ctx.params = params
            ctx.module = module
            # a learnable event representation (net.LearnedVoxelGrid) below the
            # predictor: the backward then ends with enc.0's data gradient
            ctx.grid_grad = ctx.needs_input_grad[0]
        return tuple(flows)

    @staticmethod
    def backward(ctx, *gflows):
        L, act, (B, Cin, H, W) = ctx.L, ctx.act, ctx.dims
        params = ctx.params
        dev = gflows[0].device
        mish = act == C.ACT_MISH
        grads, finish = ctx.module._grad_targets(params)
        gflows = [g.contiguous() for g in gflows]
        gflow = dict(zip(_DEC, gflows))         # by decoder layer

        def asrc(layer):        # what act' is evaluated on
            return layer.z if mish else layer.y

        def new(t):
            return torch.empty_like(t)

        twins = ctx.module.mfma == C.MFMA_BF16_TWINS

        def tw(t):          # bf16 twin of a gradient a later data gradient reads
            return C.twin(t) if twins else None

        # The data-gradient chain is the critical path; every weight gradient
        # only needs its layer's output gradient.  They run on a second HIP
        # stream so that their split-K reduces, bias sums and small-grid tails
        # fill the CUs the dgrad kernels leave idle.  ``keep`` holds the
        # tensors the side stream reads until the streams are joined.
        main = torch.cuda.current_stream(dev)
        side = ctx.module._wgrad_stream(dev)
        if ctx.dg_ready is not None:
            main.wait_event(ctx.dg_ready)
        keep = []

        # (One side stream: the weight gradients dealt round-robin to two or three of them
        # measured no gain.)

        # Flow member folded into weight space (csrc/flowfold.hip): a stage's
        # weight gradient leaves its flow columns to dvsof_flow_fold_grads, which
        # also ADDS the stage's share to the gradients of the head below -- so it
        # runs once that head's own backward has written them: at the next
        # weight gradient, ahead of it on the same stream.
        pending = []

        def wgrad(li, gz, gz16=None, fold=None, first=None, wino_gout=None):
            desc, unit = L[li].desc, LAYERS[li].unit
            gw, gb = (grads[i] for i in LAYERS[li].params[:2])

            def body():
                if first is not None:
                    first()
                for job in pending:
                    job()
                del pending[:]
                C.conv_wgrad(desc, gz, gw, gb, gz16, skip_flat=fold is not None,
                             wino_gout=wino_gout)
                if fold is None:
                    finish(unit)
                else:
                    pending.append(fold_job(desc, gz, gw, gb, unit, fold))
            if side is None:
                body()
                return
            ready = torch.cuda.Event()
            ready.record(main)
            side.wait_event(ready)
            with torch.cuda.stream(side):
                body()
            keep.extend((gz, gz16))

        def fold_job(desc, gz, gw, gb, unit, fold):
            ho, wo = C.out_size(desc)
            (wh, gwh), (bh, gbh) = ((params[i], grads[i]) for i in fold.head)

            def job():
                C.flow_fold_grads(gw, _phys(fold.w), desc.Cout, fold.ctot, 0,
                                  fold.cx, fold.cf_off, wh, bh, gb, gz, B, ho,
                                  wo, gwh, gbh)
                finish(unit)
            return job

        # ---- decoder, fine to coarse
        g_x = None          # gradient w.r.t. this stage's y from the finer stage
        g_f = gflows[-1]    # total gradient of the flow of this stage
        g_skip = {}         # encoder layer -> gradient into its output from the decoder
        g_r = g_r16 = None
        head_in_dgrad = False
        g_x16 = g_in16 = None
        # (The head's weight gradient is its own pass over the tensor on the other stream.  From
        # per-block partials of the data gradient's epilogue instead, dvsof_grad_dst_t.head_part:
        # measured 2.58 against 2.53 ms wherever the encoder's weight gradients go -- the
        # shuffles, the extra barrier and the partial stores sit on the data-gradient chain.)
        for li in reversed(_DEC):
            lay, (below, skip) = L[li], LAYERS[li].inputs[:2]
            d = lay.desc
            h, w = C.out_size(d)
            y = lay.y
            pfw, pfb = LAYERS[li].params[2:]
            head_w = None
            if head_in_dgrad:
                # the finer stage's data gradient already wrote d/d(pre-activation)
                # of this stage (head path and act' in its epilogue): only the
                # head's own weight / bias gradient is left, off the critical chain
                gz, gz16 = g_x, g_x16

                def head_w(y=y, wf=params[pfw], g=g_f, gw=grads[pfw], gb=grads[pfb],
                           h=h, w=w, c=d.Cout):
                    C.head_bwd(y, wf, g, None, None, act, None, gw, gb, B, h, w, c)
            else:
                gz, gz16 = new(y), tw(y)
                C.head_bwd(y, params[pfw], g_f, g_x, asrc(lay), act, gz,
                           grads[pfw], grads[pfb], B, h, w, d.Cout, gx16=gz16)
            fold = lay.fold
            wgrad(li, gz, gz16, fold, first=head_w)
            srcs = lay.srcs
            g_in = new(srcs[0][0])
            g_e = new(srcs[1][0])
            dsts = [dict(p=g_in), dict(p=g_e)]
            head_in_dgrad = False
            lowest = below not in _DEC
            if lowest:
                # x = r (last residual output): single consumer -> its dz,
                # which the residual chain's data gradients read next
                dsts[0]['actsrc'] = asrc(L[below])
                g_r16 = dsts[0]['p16'] = tw(g_in)
            if fold is not None:
                # cat[x, skip] with the folded weights: g_in already holds the
                # path through the flow head, which then sees the loss gradient only
                g_fprev = gflow[below]
                wf_prev = params[fold.head[0]]
                # (only the nine-product kernels, dgrad_head_rows > 0.  The general kernels can
                # fold a head too, conv_epilogue: bf16s 5 146 against 5 234 samples/s without,
                # bf16 3 941 / 3 912, bf16x3 the same -- their epilogue cannot start its loads
                # ahead of the K loop's end)
                if (C.dgrad_fuses_head(fold.desc)
                        and C.dgrad_head_rows(fold.desc) > 0
                        and wf_prev.data_ptr() % 16 == 0):
                    # ... and the head below goes into this data gradient's epilogue
                    # (dvsof_grad_dst_t.head_w): g_in leaves as the stage below's dz
                    head_in_dgrad = True
                    g_in16 = tw(g_in)       # (twins mode: the data gradient below reads its bf16 copy)
                    dsts[0].update(head_w=wf_prev, head_gflow=g_fprev,
                                   actsrc=asrc(L[below]), p16=g_in16)
            elif len(srcs) == 3:
                g_fprev = new(srcs[2][0])
                dsts.append(dict(p=g_fprev, addend=gflow[below]))
            C.conv_dgrad(d if fold is None else fold.desc, lay.w_dg, gz, dsts, act,
                         weight16=lay.w_dg16, gout16=gz16)
            keep.append(gz16)
            g_skip[skip] = g_e
            if lowest:
                g_r = g_in
            else:
                g_x, g_f = g_in, g_fprev
                g_x16 = g_in16 if head_in_dgrad else None
        # ---- residual blocks (g_r is already d/d pre-activation)
        gs, gs16 = g_r, g_r16
        # Winograd forms along the chain (dvsof_conv_desc_t.winograd_next /
        # winograd_next_gout): a data gradient's output transform also makes the
        # transformed input of the data gradient below and the gradient form of
        # the weight gradient below
        v_pre = z_pre = None

        def forms(producer, consumer):
            if not C.winograd_chain(producer, 1):
                return None, None
            c_out = consumer.Cout
            v = C.winograd_form(producer, c_out, dev)
            z = C.winograd_form(producer, c_out, dev) \
                if C.winograd_tile(consumer, 2) == 4 else None
            keep.extend((v, z))
            return v, z
        for li1, li2 in reversed(_RES):
            l1, l2 = L[li1], L[li2]
            wgrad(li2, gs, gs16, wino_gout=z_pre)
            g_t, g_t16 = new(l1.y), tw(l1.y)
            v_n, z_n = forms(l2.desc, l1.desc)
            C.conv_dgrad(l2.desc, l2.w_dg, gs,
                         [dict(p=g_t, actsrc=asrc(l1), p16=g_t16)], act,
                         weight16=l2.w_dg16, gout16=gs16, wino_pre=v_pre,
                         wino_next=v_n, wino_next_gout=z_n)
            v_pre, z_pre = v_n, z_n
            wgrad(li1, g_t, g_t16, wino_gout=z_pre)
            li0 = LAYERS[li1].inputs[0]     # another block's output, or the encoder's
            below = L[li0]
            g_prev, g_prev16 = new(below.y), tw(below.y)
            dst = dict(p=g_prev, addend=gs, actsrc=asrc(below), p16=g_prev16)
            if li0 in _ENC:
                dst['addend2'] = g_skip[li0]    # the coarsest decoder stage's skip
            v_n, z_n = forms(l1.desc, below.desc) if li0 not in _ENC else (None, None)
            C.conv_dgrad(l1.desc, l1.w_dg, g_t, [dst], act,
                         weight16=l1.w_dg16, gout16=g_t16, wino_pre=v_pre,
                         wino_next=v_n, wino_next_gout=z_n)
            v_pre, z_pre = v_n, z_n
            keep.extend((gs16, g_t16))
            gs, gs16 = g_prev, g_prev16
        # ---- encoder.  Its weight gradients are issued on the MAIN stream after
        # the last data gradient: by then the second stream still holds the
        # residual blocks' weight gradients, and the main stream would only
        # wait for it -- this way both streams drain the tail together.
        gz, gz16 = gs, gs16
        deferred = []
        # (measured, batch 8: exact f32 on one GPU with the nine-product decoder kernels 3; the
        # bf16 modes and every data-parallel rank 2)
        red_ = getattr(ctx.module, 'reducer', None)
        alone_ = red_ is None or not red_.active()   # (under the exchange marks 2 again: 2.72 vs 2.84 ms)
        n_side = 3 if ctx.module.mfma == 0 and alone_ else 2
        g_grid = None
        for li in reversed(_ENC):
            lay, li0 = L[li], LAYERS[li].inputs[0]
            if li0 == VOXELS and ctx.grid_grad:
                # gz is d/d(pre-activation) of enc.0 (the layer above applied act'), the
                # tensor the weight gradient below reads.  Ahead of that weight gradient:
                # its bucket may be updated as soon as it closes (optim.fuse_into_backward)
                g_grid = C.first_dgrad(gz, _phys(params[LAYERS[li].params[0]]), B, Cin, H, W)
            if LAYERS[li].unit[1] >= n_side:
                wgrad(li, gz, gz16)     # second stream (it is about to run dry)
            else:
                deferred.append((li, gz, gz16))     # main stream, after the last data gradient
            if li0 == VOXELS:
                break
            below = L[li0]
            g_prev, g_prev16 = new(below.y), tw(below.y)
            C.conv_dgrad(lay.desc, lay.w_dg, gz,
                         [dict(p=g_prev, addend=g_skip[li0],
                               actsrc=asrc(below), p16=g_prev16)], act,
                         weight16=lay.w_dg16, gout16=gz16)
            keep.append(gz16)
            gz, gz16 = g_prev, g_prev16
        for li, g, g16 in deferred:
            if side is None:
                wgrad(li, g, g16)
            else:
                gw, gb = (grads[i] for i in LAYERS[li].params[:2])
                C.conv_wgrad(L[li].desc, g, gw, gb, g16)
                finish(LAYERS[li].unit)
        if side is not None:
            main.wait_stream(side)
        del keep
        ctx.L = None
        return (g_grid,) + (None,) * (2 + len(params))


class Predictor(nn.Module):
    def __init__(self, in_channels, activation=None, compute_dtype='f32'):
        super().__init__()
        self.in_channels = in_channels
        self.act = activation_id(activation)
        # 'f32': exact f32 matrix cores.  'bf16': conv operands rounded to bf16
        # in registers (v_mfma_f32_32x32x16_bf16), f32 accumulation; weights,
        # activations, gradients and optimizer state all stay f32 in memory.
        # 'bf16x3': operands split into bf16 hi + lo, three products (error
        # ~2^-16 per product instead of 2^-24): f32-like accuracy at the bf16
        # matrix rate.
        # 'bf16s': bf16 operands as in 'bf16', but the forward / data-gradient
        # kernels stream bf16 TWINS of the activations, gradients and prepared
        # weights through LDS (half the LDS-DMA bytes 'bf16' is bound by);
        # every f32 tensor is still written (weight gradients, heads and loss
        # read those), master weights / optimizer state stay f32.
        modes = {'f32': C.MFMA_F32, 'bf16': C.MFMA_BF16, 'bf16x3': C.MFMA_BF16X3,
                 'bf16s': C.MFMA_BF16_TWINS}
        assert compute_dtype in modes, compute_dtype
        self.compute_dtype = compute_dtype
        self.mfma = modes[compute_dtype]
        self.reducer = None      # parallel.GradReducer for data parallelism
        # enc.i.conv, res.i.conv1 / conv2, dec.i.conv / flow, created in table order
        groups = {'enc': {}, 'res': {}, 'dec': {}}
        self._convs = []        # the ConvParams in param_list() order
        for l in LAYERS:
            kind, i, *j = l.unit
            convs = {'conv%d' % j[0] if j else 'conv':
                     ConvParams(sum(c or in_channels for c, _ in l.srcs), l.cout, 3)}
            if len(l.params) == 4:
                convs['flow'] = ConvParams(l.cout, 2, 1)
            groups[kind].setdefault(i, {}).update(convs)
            self._convs += convs.values()
        for kind, group in groups.items():
            setattr(self, kind, nn.ModuleList(_Named(**convs) for convs in group.values()))

    # Gradient buckets in the order the backward completes them (fine decoder
    # stages first, encoder last): persistent flat buffers that the wgrad
    # kernels write into, that ``p.grad`` views, that the DP reducer
    # all-reduces and that the fused optimizer reads.
    UNIT_PARAMS = {l.unit: l.params for l in LAYERS}
    BUCKETS = (
        (('dec', 3), ('dec', 2), ('dec', 1)),
        (('dec', 0),),
        (('res', 1, 2),), (('res', 1, 1),), (('res', 0, 2),), (('res', 0, 1),),
        (('enc', 3),),
        (('enc', 2), ('enc', 1), ('enc', 0)),
    )

    def _wgrad_stream(self, dev):
        """Second stream of the backward (None: DVSOF_WGRAD_STREAM=0)."""
        if os.environ.get('DVSOF_WGRAD_STREAM', '1') == '0':
            return None
        # ONE second stream per device, shared by every model of the process:
        # ROCclr deals streams round-robin onto the hardware queues, and a third
        # or fourth stream lands on the main stream's queue (the two backward
        # chains then alternate instead of overlapping: 3.4 vs 2.4 ms per step
        # measured on the third model built in one process)
        key = torch.device(dev).index if torch.device(dev).index is not None \
            else torch.cuda.current_device()
        if key not in _SIDE_STREAMS:
            _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
        return _SIDE_STREAMS[key]

    def mark_step_begin(self, dev):
        """Called by the model wrapper before it voxelises: the second stream's
        work of the coming forward (weight twins, prepared forms) depends on the
        optimizer's update only, and may start HERE instead of behind the
        voxeliser (78 us of small kernels off the forward's lane at batch 8)."""
        if self._wgrad_stream(dev) is None:
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self._step_begin = ev

    def _take_step_begin(self):
        ev, self._step_begin = getattr(self, '_step_begin', None), None
        return ev

    def _buckets(self, params):
        dev = params[0].device
        key = (dev, tuple(p.numel() for p in params))
        if getattr(self, '_bucket_key', None) != key:
            self._bucket_key = key
            self._bucket_flat, self._bucket_slot = [], {}
            for b, units in enumerate(self.BUCKETS):
                off = 0
                for u in units:
                    for i in self.UNIT_PARAMS[u]:
                        self._bucket_slot[i] = (b, off)
                        off += params[i].numel()
                self._bucket_flat.append(
                    torch.empty(off, dtype=torch.float32, device=dev))
            # every parameter's slice of its bucket, shaped and strided as the parameter
            self._bucket_views = []
            for i, p in enumerate(params):
                b, off = self._bucket_slot[i]
                self._bucket_views.append(self._bucket_flat[b][off:off + p.numel()]
                                          .as_strided(p.shape, p.stride()))
        return self._bucket_flat, self._bucket_slot

    def attach_bucket_grads(self):
        """``p.grad`` = the parameter's slice of its gradient bucket wherever
        ``p.grad`` is unset.  After a captured micro-batch that only wrote or
        accumulated gradients (capture.py roles 'first' / 'middle') this is
        Python's view of what the replay did: the next eager micro-batch of
        the same optimizer step then accumulates into the buckets."""
        params = self.param_list()
        self._buckets(params)
        for p, v in zip(params, self._bucket_views):
            if p.grad is None:
                p.grad = v

    def _grad_targets(self, params):
        """-> (targets, finish): per-parameter tensors the backward writes
        into, and a callback to call when a unit's gradients are enqueued.
        A parameter without .grad gets a view of its bucket as .grad; one that
        already has a gradient (micro-batch accumulation,
        reference utils/training.py:156-167) is accumulated into."""
        flats, _ = self._buckets(params)
        views = self._bucket_views
        accumulate = [p.grad is not None for p in params]
        targets = [torch.empty_like(p) if acc else v
                   for p, v, acc in zip(params, views, accumulate)]
        remaining = [len(units) for units in self.BUCKETS]
        unit_bucket = {u: b for b, units in enumerate(self.BUCKETS)
                       for u in units}
        reducer = self.reducer
        dev, on_gpu = params[0].device, params[0].is_cuda
        # The units of one bucket may be enqueued on different streams (the
        # backward splits weight gradients between its two streams).  Whoever
        # closes the bucket hands it to the reducer / the fused optimizer on
        # ITS stream, so that stream first waits for the other units' writes.
        marks = [[] for _ in self.BUCKETS]

        def finish(unit):
            for i in self.UNIT_PARAMS[unit]:
                p = params[i]
                if accumulate[i]:
                    p.grad.add_(targets[i])
                else:
                    p.grad = views[i]
            b = unit_bucket[unit]
            remaining[b] -= 1
            if on_gpu and len(self.BUCKETS[b]) > 1:
                cur = torch.cuda.current_stream(dev)
                if remaining[b] != 0:
                    done = torch.cuda.Event()
                    done.record(cur)
                    marks[b].append((cur, done))
                else:
                    for stream, done in marks[b]:
                        if stream != cur:
                            cur.wait_event(done)
            if remaining[b] != 0:
                return
            hook = getattr(self, 'bucket_hook', None)    # optim.fuse_into_backward
            after = None
            if hook is not None:
                bparams = [params[i] for u in self.BUCKETS[b]
                           for i in self.UNIT_PARAMS[u]]
                after = lambda: hook(b, bparams)            # noqa: E731
            if reducer is not None and reducer.active():
                owned = all(params[i].grad.data_ptr() == views[i].data_ptr()
                            for u in self.BUCKETS[b]
                            for i in self.UNIT_PARAMS[u])
                assert owned, 'DP needs .grad to live in the bucket buffers'
                reducer.bucket_ready(flats[b], after)
            elif after is not None:
                after()
        return targets, finish

    def param_list(self):
        return [t for m in self._convs for t in (m.weight, m.bias)]

    def forward(self, voxels):
        """voxels: float32 [B,C,H,W] (NCHW dense), H and W multiples of 16.
        -> tuple of 4 flows [B,2,H/8..H,W/8..W] coarse to fine."""
        B, Cin, H, W = voxels.shape
        assert Cin == self.in_channels
        assert H % 16 == 0 and W % 16 == 0, \
            'the predictor needs H and W divisible by 16'
        params = self.param_list()
        want_grad = torch.is_grad_enabled() and (
            voxels.requires_grad or any(p.requires_grad for p in params))
        return _PredictorFn.apply(voxels.contiguous(), self, want_grad,
                                  *params)

    def flops_per_sample(self, H, W):
        """Algorithmic forward FLOPs (2*MACs), SURVEY.md section 8d formula."""
        total = 0
        for l in LAYERS:
            scale = 2 if l.up else 1
            pixels = ((H >> l.shift) * scale // l.stride) * ((W >> l.shift) * scale // l.stride)
            cin = sum(c or self.in_channels for c, _ in l.srcs)
            total += 2 * pixels * l.cout * (9 * cin + (2 if len(l.params) == 4 else 0))
        return total
