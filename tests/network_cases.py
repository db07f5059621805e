"""Shared pieces of the tests that pin the network at evaluation-size frames
(test_gpu_network_layers.py, test_gpu_network_repeat.py): the small frames, the predictor's
conv layers at those frames in the conv_cases.CASES format, a poison for the memory
torch.empty hands out next, and a way to forget the device scratch that survives a call.
Nothing here touches the GPU at import."""
import torch

# (B, H, W): the evaluation box of tests/eval_cases.py at batches of one to three frames, the
# training frame of test_gpu_resume.py and the frame of test_gpu_model.py's training step.
# Every one of them is run by some other test already.
SMALL_FRAMES = ((1, 32, 64), (2, 32, 64), (3, 32, 64), (2, 64, 64), (2, 32, 48))
DEPTHS = (3, 5)


def _key(case):
    return (case['B'], case['H'], case['W'], tuple(case['src']), case['Cout'], case['stride'],
            case['up'], case['residual'], case['act'])


def case_id(case):
    """'dec.1 B2 8x16 256n+256n+2p->128 s1 up relu': the key of the committed path table."""
    src = '+'.join('%d%s' % (c, 'p' if lay == 'nchw' else 'n') for c, lay in case['src'])
    return '%s B%d %dx%d %s->%d s%d%s%s %s' % (
        case['name'], case['B'], case['H'], case['W'], src, case['Cout'], case['stride'],
        ' up' if case['up'] else '', ' res' if case['residual'] else '', case['act'])


def layer_cases(B, H, W, bins, act='relu'):
    """The conv layers of predictor.LAYERS at frame (B, H, W) with `bins` input channels, as
    conv_cases.CASES dicts (plus 'name': LAYERS[i].name, '/folded' where the flow member is
    folded away, and 'layer': i).  Derived from the table the way the planning goldens are
    (tools/make_goldens_conv_plan.predictor_layers): every decoder stage with a flow member
    appears as cat[x, skip, flow] and as cat[x, skip]."""
    from dvs_of_training_framework_amd.predictor import LAYERS
    from tools import make_goldens_conv_plan as gen
    descs = gen.predictor_layers(B, H, W, 0, bins)
    # predictor_layers walks LAYERS in order, a three-member layer twice
    owners = [(li, len(l.srcs) == 3 and fold) for li, l in enumerate(LAYERS)
              for fold in ((False, True) if len(l.srcs) == 3 else (False,))]
    assert len(owners) == len(descs)
    out, seen = [], set()
    for d, (li, folded) in zip(descs, owners):
        assert (d['ksize'], d['pad'], d['nsrc']) == (3, 1, len(d['src']))
        case = dict(B=d['B'], H=d['H'], W=d['W'],
                    src=[(c, 'nchw' if lay == gen.NCHW else 'nhwc') for c, lay in d['src']],
                    Cout=d['Cout'], stride=d['stride'], up=bool(d['upsample']),
                    residual=LAYERS[li].residual is not None, act=act,
                    name=LAYERS[li].name + ('/folded' if folded else ''), layer=li)
        if _key(case) not in seen:
            seen.add(_key(case))
            out.append(case)
    return out


def all_layer_cases():
    """Every layer of every SMALL_FRAMES entry at both depths with ReLU, and the batch of two
    evaluation frames with Mish as well (its epilogues: the z copy, act' of z); no layer twice."""
    out, seen = [], set()
    todo = [(f, bins, 'relu') for f in SMALL_FRAMES for bins in DEPTHS]
    todo += [((2, 32, 64), bins, 'mish') for bins in DEPTHS]
    for (B, H, W), bins, act in todo:
        for case in layer_cases(B, H, W, bins, act):
            if _key(case) not in seen:
                seen.add(_key(case))
                out.append(case)
    return out


# ---------------------------------------------------------------------------
# poison: what torch.empty hands out next
# ---------------------------------------------------------------------------
POISONS = {0xFF: 'NaN', 0x00: 'zero', 0x7F: 'large finite'}
_MIB = 1 << 20
# Block sizes, largest first, all held at once: the caching allocator serves a request from the
# smallest cached free block that fits before it asks the driver, so every free fragment of
# at least the size of some rung ends up in one of these tensors.  Requests of up to 1 MiB come
# from the small pool (2 MiB segments, 512-byte granules), larger ones from the large pool,
# whose fragments are larger than 1 MiB.
_LARGE = ((1, 768 * _MIB), (4, 64 * _MIB), (8, 16 * _MIB), (16, 4 * _MIB), (48, _MIB + 512))
_SMALL = ((16, _MIB), (32, 256 << 10), (64, 64 << 10), (64, 16 << 10), (128, 4 << 10), (256, 512))


def _streams():
    """The streams the network allocates on: the current one and the predictor's second."""
    from dvs_of_training_framework_amd import predictor
    out = [torch.cuda.current_stream()]
    out += [s for s in predictor._SIDE_STREAMS.values() if s not in out]
    return out


def _fill_free_memory(pattern):
    """Fill the allocator's free memory of every stream of _streams() with `pattern` bytes and
    free it again (a stub of this is how the self-check is shown to fail)."""
    torch.cuda.synchronize()
    for stream in _streams():
        with torch.cuda.stream(stream):
            held = [torch.empty(size, dtype=torch.uint8, device='cuda')
                    for count, size in _LARGE + _SMALL for _ in range(count)]
            for t in held:
                t.fill_(pattern)
            del held, t
    torch.cuda.synchronize()


def poison_took(pattern):
    """-> '' when a fresh torch.empty of 1 KiB and one of 4 MiB on every stream read back the
    pattern, else what did not."""
    for si, stream in enumerate(_streams()):
        with torch.cuda.stream(stream):
            for size in (1 << 10, 4 * _MIB):
                t = torch.empty(size, dtype=torch.uint8, device='cuda')
                wrong = int((t != pattern).sum())
                if wrong:
                    return 'stream %d: %d of %d fresh bytes are not 0x%02X' % (si, wrong, size, pattern)
                del t
    torch.cuda.synchronize()
    return ''


def poison(pattern):
    """The next torch.empty hands out `pattern` bytes (0xFF: NaN, 0x00, 0x7F: 3.4e38), on the
    current stream and on the predictor's second one.  A kernel that reads memory it did not
    write then computes from the pattern, and two patterns give two results.  Self-checked: a
    poison that did not take fails the test (AssertionError), it proves nothing."""
    assert pattern in POISONS, pattern
    _fill_free_memory(pattern)
    failed = poison_took(pattern)
    assert not failed, 'poison(0x%02X) did not take: %s' % (pattern, failed)


# ---------------------------------------------------------------------------
# forget: device scratch that survives a call
# ---------------------------------------------------------------------------
def forget_caches(*models):
    """Drop what the package keeps on the device between calls, so that the next call is a
    first call again:

    - voxel._WORKSPACES, learned_voxel._WORKSPACES: the voxelisers' workspaces (control words
      zero-filled once, then left clean by the kernels);
    - loss._UNIT: the cached device 1.0 that seeds unit_backward;
    - conv._PLAN: planning answers per descriptor (host integers; dropped with the rest so
      that a first call asks the library again);
    - per Model passed: _layout_cache and _fast (index vectors of the uniform layout);
    - per Predictor (a Model's .predictor or one passed itself): the gradient buckets
      (_bucket_key, _bucket_flat, _bucket_views; every .grad is a view of them, so the
      gradients go too) and a pending _step_begin mark;
    - per OpticalFlow: _graphs (captured graphs with their static inputs and outputs).

    Streams (predictor._SIDE_STREAMS, feed._COPY_STREAMS, parallel._*_STREAMS) and
    _audit._LAYOUTS (host tables) hold no device tensors and stay.  The HIP library itself
    keeps no device memory between calls (csrc/ allocates none: every workspace is passed in)."""
    from dvs_of_training_framework_amd import conv, learned_voxel, loss, voxel
    torch.cuda.synchronize()
    voxel._WORKSPACES.clear()
    learned_voxel._WORKSPACES.clear()
    loss._UNIT.clear()
    conv._PLAN.clear()
    for m in models:
        if hasattr(m, '_graphs'):           # OpticalFlow
            m._graphs.clear()
            m = m._net
        if hasattr(m, '_layout_cache'):     # Model
            m._layout_cache.clear()
            m._fast = None
            m = m.predictor
        if hasattr(m, '_bucket_key'):       # Predictor that ran a backward
            for p in m.parameters():
                p.grad = None
            m._bucket_key = None
            m._bucket_flat, m._bucket_views, m._bucket_slot = [], [], {}
        if hasattr(m, '_step_begin'):
            m._step_begin = None


def first_difference(a, b):
    """-> None when a and b hold the same bits, else (flat index, a there, b there, count)."""
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    ia = a.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]).flatten()
    ib = b.view(ia.dtype).flatten()
    ne = ia != ib
    n = int(ne.sum())
    if n == 0:
        return None
    i = int(ne.nonzero()[0])
    return i, float(a.flatten()[i]), float(b.flatten()[i]), n
