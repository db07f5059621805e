"""TEST INFRASTRUCTURE ONLY (see oracle/dvsof_oracle.c header).

Plain PyTorch fp32 restatement of docs/MODEL_SPEC.md (CPU or GPU, ATen ops
only) -- the floating-point reference the HIP conv stack is compared with.
Upstream's EV_FlowNet source is absent ("parity unpinned"), so this
file and the spec define the network; it takes the SAME state_dict as
dvs_of_training_framework_amd.predictor.Predictor."""
import torch
import torch.nn.functional as F


def _act(x, mish):
    return F.mish(x) if mish else F.relu(x)


def ref_predictor(state, x, mish=False, prefix=''):
    """state: dict name -> tensor (names as Predictor.state_dict()).
    x: [B,C,H,W].  -> list of 4 flows coarse to fine."""
    g = lambda n: state[prefix + n]
    e = []
    for i in range(4):
        x = _act(F.conv2d(x, g(f'enc.{i}.conv.weight'), g(f'enc.{i}.conv.bias'),
                          stride=2, padding=1), mish)
        e.append(x)
    r = x
    for i in range(2):
        t = _act(F.conv2d(r, g(f'res.{i}.conv1.weight'),
                          g(f'res.{i}.conv1.bias'), padding=1), mish)
        r = _act(F.conv2d(t, g(f'res.{i}.conv2.weight'),
                          g(f'res.{i}.conv2.bias'), padding=1) + r, mish)
    flows, x, f = [], r, None
    for i in range(4):
        parts = [x, e[3 - i]] + ([f] if f is not None else [])
        inp = F.interpolate(torch.cat(parts, 1), scale_factor=2, mode='nearest')
        x = _act(F.conv2d(inp, g(f'dec.{i}.conv.weight'),
                          g(f'dec.{i}.conv.bias'), padding=1), mish)
        f = F.conv2d(x, g(f'dec.{i}.flow.weight'), g(f'dec.{i}.flow.bias'))
        flows.append(f)
    return flows


class _ReluMasked(torch.autograd.Function):
    """relu(z) whose derivative is read from `src`: 1 where src > 0 (at_zero: where src >= 0)."""

    @staticmethod
    def forward(ctx, z, src, at_zero):
        ctx.save_for_backward((src >= 0) if at_zero else (src > 0))
        return z.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask.to(g.dtype), None, None


WRONG_RELU = ('act_at_zero', 'actsrc_neighbour')      # mis-wirings that need an activation


def wrong_variants(act):
    """Every name `wrong` may take with activation `act` ('relu' | 'none')."""
    out = ['skip_grad_%d' % i for i in range(4)]
    out += ['flow_path_%d' % i for i in range(1, 4)]
    out += ['%s_%d' % (k, i) for k in ('residual_fwd', 'residual_bwd') for i in range(2)]
    out += ['member_order_%d' % i for i in range(4)]
    out += ['fold_bias_border_%d' % i for i in range(1, 4)]
    return out + (list(WRONG_RELU) if act == 'relu' else [])


def ref_predictor_trace(state, x, act='relu', wrong=None, prefix=''):
    """ref_predictor's arithmetic in the dtype of its inputs, keeping what it passes through.

    act: 'relu' | 'none'.  -> (flows, trace): trace maps 'enc.0' ... 'dec.3' (the names of
    predictor.LAYERS) to the layer's output y, name + '/z' to its pre-activation, 'flow.i' to
    the flows and 'dec.i/x', 'dec.i/skip', 'dec.i/flow' to the members as stage i reads them,
    every one with retain_grad set: after a backward .grad of 'enc.0/z' is the gradient the
    layer's weight gradient reads, of 'dec.i/skip' the decoder's share of a skip gradient.

    wrong: None, or one deliberate mis-wiring of this restatement (wrong_variants): what a
    test uses to show that its data would detect such an error in the network under test.
      skip_grad_<i>       stage i reads its skip detached (the skip gradient is lost)
      flow_path_<i>       stage i reads its flow member detached
      residual_fwd_<i>    residual block i without its residual add
      residual_bwd_<i>    ... with the add in the forward only
      member_order_<i>    stage i runs on cat[skip, x] instead of cat[x, skip]
      act_at_zero         relu'(0) = 1
      actsrc_neighbour    the residual layers take act' of the layer below, not their own
      fold_bias_border_<i> stage i sees the flow head's bias through the taps that fall in the
                          zero padding too, as a folded bias applied uniformly would have it"""
    assert act in ('relu', 'none'), act
    assert wrong is None or wrong in wrong_variants(act), wrong
    g = lambda n: state[prefix + n]        # noqa: E731
    trace = {}
    is_wrong = lambda kind, i: wrong == '%s_%d' % (kind, i)     # noqa: E731

    def keep(name, t):
        if t.requires_grad:
            t.retain_grad()
        trace[name] = t
        return t

    def tap(name, t):           # the same values under a name of their own
        t = t.view_as(t)
        return keep(name, t)

    def activate(name, z, below=None):
        z = keep(name + '/z', z)
        if act == 'none':
            y = z.view_as(z)
        elif wrong == 'act_at_zero':
            y = _ReluMasked.apply(z, z, True)
        elif wrong == 'actsrc_neighbour' and below is not None:
            y = _ReluMasked.apply(z, below, False)
        else:
            y = F.relu(z)
        return keep(name, y)

    e = []
    for i in range(4):
        x = activate(f'enc.{i}', F.conv2d(x, g(f'enc.{i}.conv.weight'), g(f'enc.{i}.conv.bias'),
                                          stride=2, padding=1))
        e.append(x)
    r = x
    for i in range(2):
        t = activate(f'res.{i}.1', F.conv2d(r, g(f'res.{i}.conv1.weight'),
                                            g(f'res.{i}.conv1.bias'), padding=1), below=r)
        z = F.conv2d(t, g(f'res.{i}.conv2.weight'), g(f'res.{i}.conv2.bias'), padding=1)
        if is_wrong('residual_bwd', i):
            z = z + r.detach()
        elif not is_wrong('residual_fwd', i):
            z = z + r
        r = activate(f'res.{i}.2', z, below=t)
    flows, x, f = [], r, None
    for i in range(4):
        skip = e[3 - i].detach() if is_wrong('skip_grad', i) else e[3 - i]
        parts = [tap(f'dec.{i}/x', x), tap(f'dec.{i}/skip', skip)]
        if is_wrong('member_order', i):
            parts.reverse()
        if f is not None:
            parts.append(tap(f'dec.{i}/flow', f.detach() if is_wrong('flow_path', i) else f))
        inp = F.interpolate(torch.cat(parts, 1), scale_factor=2, mode='nearest')
        w = g(f'dec.{i}.conv.weight')
        z = F.conv2d(inp, w, g(f'dec.{i}.conv.bias'), padding=1)
        if is_wrong('fold_bias_border', i):
            wf = w[:, -2:]
            bh = g(f'dec.{i - 1}.flow.bias').view(1, 2, 1, 1).expand(1, 2, *z.shape[2:])
            z = z + F.conv2d(F.pad(bh, (1, 1, 1, 1), mode='replicate'), wf) \
                - F.conv2d(bh, wf, padding=1)
        x = activate(f'dec.{i}', z)
        f = keep(f'flow.{i}', F.conv2d(x, g(f'dec.{i}.flow.weight'), g(f'dec.{i}.flow.bias')))
        flows.append(f)
    return flows, trace
