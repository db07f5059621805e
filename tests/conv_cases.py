"""Tables and helpers shared by the conv tests (test_gpu_conv.py, test_gpu_conv_exact.py,
test_gpu_conv_geometry.py, test_conv_emulation.py): the layer cases with the kernel family each operand mode runs, the
descriptor builder, and the float64 references."""
import torch
import torch.nn.functional as F


def nhwc(t):   # logical NCHW -> dense NHWC buffer on the GPU
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def from_nhwc(t):
    return t.permute(0, 3, 1, 2)


def wphys(w):  # OIHW -> [O][kh][kw][I] on the GPU
    return w.permute(0, 2, 3, 1).contiguous().cuda()


CASES = [
    # B, H, W, chans(list, layouts), Cout, k, stride, up, act; path: the families of the
    # forward, data and weight gradient in operand modes 0, 1, 2 and -- where every NHWC
    # member has 32 | C -- 3 (bf16 twins)
    dict(B=2, H=16, W=16, src=[(5, 'nchw')], Cout=64, stride=2,
         path=('first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first')),
    dict(B=1, H=13, W=19, src=[(3, 'nchw')], Cout=32, stride=2,
         path=('general_v1 general_v2 flat_valu', 'general_v1 general_v2 flat_valu', 'general_v1 general_v2 flat_valu', 'general_v1 general_v2 flat_valu')),
    dict(B=2, H=12, W=20, src=[(64, 'nhwc')], Cout=128, stride=2,
         path=('general_v2 stride2_phased general_v1', 'general_v2 stride2_phased general_v1', 'general_v2 stride2_phased general_v1', 'general_v2 stride2_phased general_v1')),
    dict(B=3, H=8, W=8, src=[(32, 'nhwc')], Cout=32, stride=1, residual=True,
         path=('general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1')),
    dict(B=2, H=8, W=12, src=[(32, 'nhwc'), (16, 'nhwc'), (2, 'nchw')], Cout=32,
         up=True,
         path=('general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1')),
    dict(B=1, H=4, W=4, src=[(512, 'nhwc'), (512, 'nhwc')], Cout=256, up=True,
         path=('general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1')),
    dict(B=2, H=9, W=7, src=[(20, 'nhwc')], Cout=48, stride=1, k=5, pad=2,
         path=('general_v1 general_v2 general_v1', 'general_v1 general_v2 general_v1', 'general_v1 general_v2 general_v1')),
    dict(B=2, H=16, W=16, src=[(64, 'nhwc'), (64, 'nhwc'), (2, 'nchw')], Cout=32,
         up=True, act='mish',
         path=('general_v2 general_v2 wgrad_min', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 wgrad_patch')),
    # wide 3x3 stride-1 layers with enough tiles: Winograd.  F(2x2,3x3) (W % 4 != 0),
    # forward, data and weight gradient
    dict(B=4, H=8, W=18, src=[(256, 'nhwc')], Cout=320, stride=1, residual=True, wino=True,
         path=('wino2 wino2 wino2', 'general_v2 general_v2 general_v1', 'wino2 wino2 wino2', 'general_v2 general_v2 general_v1')),
    # F(4x4,3x3) forward / data gradient (64 tiles), F(2x2) weight gradient
    dict(B=8, H=8, W=16, src=[(320, 'nhwc')], Cout=256, stride=1, act='mish', wino=True,
         path=('wino4 wino4 wino2', 'general_v2 general_v2 general_v2', 'wino2 wino2 wino2', 'general_v2 general_v2 general_v2')),
    # fewer than 64 4x4 tiles: the 2x2 form on a 4-aligned image
    dict(B=6, H=8, W=16, src=[(256, 'nhwc')], Cout=384, stride=1, wino=True,
         path=('wino2 wino2 wino2', 'general_v2 general_v2 general_v2', 'wino2 wino2 wino2', 'general_v2 general_v2 general_v2')),
    # >= 128 4x4 tiles: the weight gradient takes the F(4x4,3x3) form too and
    # reuses the forward's transformed input
    dict(B=8, H=16, W=16, src=[(256, 'nhwc')], Cout=256, stride=1, wino=True,
         path=('wino4 wino4 wino4', 'general_v2 general_v2 general_v2', 'wino2 wino2 wino2', 'general_v2 general_v2 general_v2')),
    # large up-sampling layer with a flow member: four-lanes-per-pixel flow-gradient rows
    # and the matrix-core flat-member weight gradient
    dict(B=8, H=64, W=64, src=[(32, 'nhwc'), (32, 'nhwc'), (2, 'nchw')], Cout=64, up=True,
         path=('general_v2 general_v2 wgrad_patch', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 wgrad_patch')),
    # too few tiles: the direct kernel (transformed weights would dominate)
    dict(B=1, H=8, W=8, src=[(256, 'nhwc')], Cout=256, stride=1,
         path=('general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1', 'general_v2 general_v2 general_v1')),
    # the first encoder layer's own kernels (csrc/first.hip: planar input, 64 outputs,
    # 8 x 32-pixel tiles, K = 9 C): ragged tiles in both directions, every column-block
    # count of the weight gradient (K + 1 = 28 .. 145 columns), Mish with its z copy
    dict(B=2, H=20, W=72, src=[(5, 'nchw')], Cout=64, stride=2, first=True,
         path=('first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first')),
    dict(B=1, H=16, W=64, src=[(12, 'nchw')], Cout=64, stride=2, act='mish', first=True,
         path=('first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first')),
    dict(B=3, H=34, W=18, src=[(9, 'nchw')], Cout=64, stride=2, first=True,
         path=('first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first')),
    dict(B=1, H=8, W=8, src=[(16, 'nchw')], Cout=64, stride=2, first=True,
         path=('first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first')),
    dict(B=1, H=8, W=8, src=[(3, 'nchw')], Cout=64, stride=2, first=True,
         path=('first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first')),
    dict(B=8, H=128, W=128, src=[(5, 'nchw')], Cout=64, stride=2, first=True,
         path=('first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first', 'first stride2_phased first')),   # 256 tiles: one per group
    # decoder stages whose weight gradient takes the patch-resident kernel in the twins mode
    # (csrc/wgrad_patch.hip, test_wgrad_on_bf16_twins_... below) and, every vector member
    # 64 | C, the nine-product wgrad_min in exact f32: 64 input channels per workgroup
    # (swapped halves of odd patch slots), 144 blocks over 64 splits with a flat member
    # beside the vector members
    dict(B=4, H=32, W=32, src=[(128, 'nhwc'), (128, 'nhwc')], Cout=64, up=True,
         path=('fwd_min4 dgrad_min1 wgrad_min', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 wgrad_patch')),
    dict(B=3, H=32, W=48, src=[(64, 'nhwc'), (192, 'nhwc'), (2, 'nchw')], Cout=64, up=True,
         path=('general_v2 general_v2 wgrad_min', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 wgrad_patch')),
    # the finest decoder stage with its flow member folded away (two members of 64 -> 32):
    # forward by csrc/fwd_patch.hip (weights in registers, patch in LDS)
    dict(B=1, H=2, W=16, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True,
         path=('fwd_patch general_v2 wgrad_min', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'fwd_patch general_v2 wgrad_patch')),
    dict(B=3, H=10, W=48, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True, act='mish',
         path=('fwd_patch general_v2 wgrad_min', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'fwd_patch general_v2 wgrad_patch')),
    dict(B=2, H=62, W=64, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True,
         path=('fwd_patch general_v2 wgrad_min', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'fwd_patch general_v2 wgrad_patch')),
    # decoder stages whose exact-f32 forward is the nine-product form (csrc/fwd_min.hip: 4 | H,
    # 16 | W, two NHWC members of multiples of 32 channels): 4-row blocks with the K split over
    # the waves / 8-row blocks, members of different widths, Mish with its pre-activation copy,
    # blocks on every border of the frame, the coarsest benchmark stage's channel counts
    dict(B=2, H=12, W=32, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True, act='mish',
         path=('fwd_min4 general_v2 wgrad_min', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'fwd_patch general_v2 wgrad_patch')),
    dict(B=1, H=8, W=16, src=[(32, 'nhwc'), (96, 'nhwc')], Cout=64, up=True,
         path=('fwd_min4 general_v2 wgrad_patch', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 wgrad_patch')),
    dict(B=3, H=24, W=48, src=[(64, 'nhwc'), (32, 'nhwc')], Cout=96, up=True, act='none',
         path=('fwd_min4 general_v2 wgrad_patch', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 wgrad_patch')),
    dict(B=8, H=16, W=16, src=[(256, 'nhwc'), (256, 'nhwc')], Cout=128, up=True,
         path=('fwd_min4 dgrad_min1 wgrad_min', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 wgrad_patch')),
    dict(B=16, H=64, W=32, src=[(32, 'nhwc'), (32, 'nhwc')], Cout=32, up=True,
         path=('fwd_min8 general_v2 wgrad_patch', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 wgrad_patch')),
    # the coarsest and the finest decoder stage EXACTLY as benchmarked (batch 8, 256 x 256
    # input): 512 + 512 -> 256 at 16 x 16 (4-row blocks, K split over the waves, 32 chunks)
    # and 64 + 64 -> 32 at 128 x 128 (8-row blocks, 1 024 workgroups)
    dict(B=8, H=16, W=16, src=[(512, 'nhwc'), (512, 'nhwc')], Cout=256, up=True,
         path=('fwd_min4 dgrad_min1 wgrad_min', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 wgrad_patch')),
    dict(B=8, H=128, W=128, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True,
         path=('fwd_min8 dgrad_min0 wgrad_min', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'fwd_patch general_v2 wgrad_patch')),
    # outcomes of the weight gradient's plan (csrc/wgrad_plan.hip) the layers above do not reach,
    # each at the smallest size that takes it (tests/test_gpu_wgrad_plan.py):
    # a 4-channel planar member beside a sub-pixel layer's vector members: its columns on the v1
    # tiles beside v2, both into the phase slabs, with the patch kernels' split count
    dict(B=1, H=8, W=16, src=[(32, 'nhwc'), (32, 'nhwc'), (4, 'nchw')], Cout=32, up=True,
         path=('general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2', 'general_v2 general_v2 general_v2')),
    # rows that are no whole 16-pixel groups: v1 tiles for the vector member, direct; the flow
    # member on the VALU kernel; the bias by the scalar column-sum pass (Cout % 4 != 0)
    dict(B=2, H=9, W=11, src=[(24, 'nhwc'), (2, 'nchw')], Cout=30,
         path=('general_v1 general_v1 general_v1', 'general_v1 general_v1 general_v1', 'general_v1 general_v1 general_v1')),
    # a flat-only layer of M = 262144 pixels: the matrix-core flat kernel, the bias gradient as
    # its extra output column
    dict(B=1, H=512, W=512, src=[(2, 'nchw')], Cout=32,
         path=('general_v1 general_v2 flat_valu', 'general_v1 general_v2 flat_valu', 'general_v1 general_v2 flat_valu', 'general_v1 general_v2 flat_valu')),
    # flat members no flat kernel takes (36 / 72 + 36 columns): on the v1 tiles, direct / over
    # K-split slabs, the bias by the column-sum pass
    dict(B=1, H=16, W=16, src=[(4, 'nchw')], Cout=32,
         path=('general_v1 general_v2 general_v1', 'general_v1 general_v2 general_v1', 'general_v1 general_v2 general_v1', 'general_v1 general_v2 general_v1')),
    dict(B=2, H=16, W=32, src=[(8, 'nhwc'), (4, 'nchw')], Cout=12,
         path=('general_v1 general_v1 general_v1', 'general_v1 general_v1 general_v1', 'general_v1 general_v1 general_v1')),
]


# kernels that compute in exact f32 whatever the operand mode (dvsof_conv2d_last_kernel
# reports mode 0 for them)
F32_ONLY = {'first', 'general_v1', 'flat_valu', 'fwd_min4', 'fwd_min8', 'dgrad_min0',
            'dgrad_min1', 'dgrad_min2', 'wgrad_min'}


def effective_mode(kind, family, mode):
    """The operand mode dvsof_conv2d_last_kernel reports for `family` in a call of `mode`."""
    return mode if family not in F32_ONLY else 3 if (family == 'first' and kind == 0 and mode == 3) else 0


def assert_path(kind, family, mode):
    """The last conv call of `kind` (0 fwd, 1 dgrad, 2 wgrad) ran `family` in operand mode
    `mode` (after every fallback; the f32-only kernels report 0, the first layer's forward 3
    when it wrote the twin of y)."""
    from dvs_of_training_framework_amd import conv as C
    fam, m = C.last_kernel(kind)
    want = effective_mode(kind, family, mode)
    assert (C.KERNEL_NAMES[fam], m) == (family, want), (kind, C.KERNEL_NAMES[fam], m, family, want)


def build(case, seed=0):
    from dvs_of_training_framework_amd import conv as C
    g = torch.Generator().manual_seed(seed)
    B, H, W = case['B'], case['H'], case['W']
    k, stride = case.get('k', 3), case.get('stride', 1)
    pad, up = case.get('pad', 1), case.get('up', False)
    act = {'relu': C.ACT_RELU, 'mish': C.ACT_MISH, 'none': C.ACT_NONE}[
        case.get('act', 'relu')]
    xs = [torch.randn(B, c, H, W, generator=g) for c, _ in case['src']]
    ctot = sum(c for c, _ in case['src'])
    w = torch.randn(case['Cout'], ctot, k, k, generator=g) / (ctot * k * k) ** 0.5
    b = torch.randn(case['Cout'], generator=g)
    dev = [(x.cuda().contiguous() if lay == 'nchw' else nhwc(x))
           for x, (_, lay) in zip(xs, case['src'])]
    srcs = [(d, c, C.NCHW if lay == 'nchw' else C.NHWC)
            for d, (c, lay) in zip(dev, case['src'])]
    desc = C.make_desc(srcs, B, H, W, case['Cout'], k, stride, pad, up, act)
    desc._keepalive = dev   # the descriptor only holds raw pointers
    return C, xs, w, b, desc, act, dict(k=k, stride=stride, pad=pad, up=up)


def torch_fwd(xs, w, b, o, act, C, residual=None):
    inp = torch.cat(xs, 1)
    if o['up']:
        inp = F.interpolate(inp, scale_factor=2, mode='nearest')
    z = F.conv2d(inp, w, b, stride=o['stride'], padding=o['pad'])
    if residual is not None:
        z = z + residual
    y = F.relu(z) if act == C.ACT_RELU else F.mish(z) if act == C.ACT_MISH else z
    return y, z


TWIN_LAYERS = [
    # (case, fwd family, dgrad family): what mode 3 runs in the predictor
    (dict(B=2, H=32, W=32, src=[(64, 'nhwc')], Cout=128, stride=2), 'general_v2', 'stride2_phased'),
    (dict(B=2, H=16, W=16, src=[(256, 'nhwc')], Cout=256, stride=1, residual=True),   # no Winograd
     'general_v2', 'general_v2'),
    (dict(B=2, H=16, W=16, src=[(64, 'nhwc'), (64, 'nhwc'), (2, 'nchw')], Cout=32, up=True,
          act='mish'), 'general_v2', 'general_v2'),
    (dict(B=2, H=16, W=16, src=[(128, 'nhwc'), (128, 'nhwc')], Cout=64, up=True),
     'general_v2', 'general_v2'),
]


# layers of test_wgrad_on_bf16_twins_equals_the_operand_mode: mode 3 weight gradient on the twins
WGRAD_TWIN_CASES = [
    dict(B=2, H=16, W=32, src=[(64, 'nhwc')], Cout=64, stride=1),
    dict(B=3, H=32, W=32, src=[(32, 'nhwc')], Cout=128, stride=2),        # odd number of 16-pixel groups per split
    dict(B=2, H=16, W=16, src=[(64, 'nhwc'), (32, 'nhwc'), (2, 'nchw')], Cout=32, up=True),   # sub-pixel phases + a flat member
    dict(B=8, H=64, W=64, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True),                # 32 x 128 tile, many K splits
    dict(B=4, H=16, W=16, src=[(256, 'nhwc')], Cout=256, stride=1),                          # direct wide layer (no Winograd in mode 3)
    # the patch-resident decoder kernel (csrc/wgrad_patch.hip; the 64 x 64 case above too):
    # 16-pixel rows (every group is its own row: top / bottom / left / right borders in one
    # group), two output-channel tiles, unequal members, an odd number of groups per split
    dict(B=3, H=16, W=16, src=[(64, 'nhwc'), (32, 'nhwc')], Cout=64, up=True),
    dict(B=2, H=8, W=32, src=[(32, 'nhwc')], Cout=32, up=True),
    dict(B=1, H=16, W=48, src=[(96, 'nhwc'), (32, 'nhwc')], Cout=96, up=True),
    # 64 input channels per workgroup (members of 64 | C and >= 512 workgroups): 128-byte
    # pixel slots with the swizzled halves; 144 blocks over 64 splits (empty splits write zeros)
    dict(B=4, H=32, W=32, src=[(128, 'nhwc'), (128, 'nhwc')], Cout=64, up=True),
    dict(B=3, H=32, W=48, src=[(64, 'nhwc'), (192, 'nhwc'), (2, 'nchw')], Cout=64, up=True),
    # the finest decoder stage with its flow member folded away (two members of 64 -> 32):
    # forward by csrc/fwd_patch.hip (weights in registers, patch in LDS)
    dict(B=1, H=2, W=16, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True),
    dict(B=3, H=10, W=48, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True, act='mish'),
    dict(B=2, H=64, W=64, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True),
    # decoder stages whose exact-f32 forward is the nine-product form (csrc/fwd_min.hip: 4 | H,
    # 16 | W, two NHWC members of multiples of 32 channels): 4-row blocks with the K split over
    # the waves / 8-row blocks, members of different widths, Mish with its pre-activation copy,
    # blocks on every border of the frame, the coarsest benchmark stage's channel counts
    dict(B=2, H=12, W=32, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True, act='mish'),
    dict(B=1, H=8, W=16, src=[(32, 'nhwc'), (96, 'nhwc')], Cout=64, up=True),
    dict(B=3, H=24, W=48, src=[(64, 'nhwc'), (32, 'nhwc')], Cout=96, up=True, act='none'),
    dict(B=8, H=16, W=16, src=[(256, 'nhwc'), (256, 'nhwc')], Cout=128, up=True),
    dict(B=16, H=16, W=32, src=[(32, 'nhwc'), (32, 'nhwc')], Cout=32, up=True),
    # the coarsest and the finest decoder stage EXACTLY as benchmarked (batch 8, 256 x 256
    # input): 512 + 512 -> 256 at 16 x 16 (4-row blocks, K split over the waves, 32 chunks)
    # and 64 + 64 -> 32 at 128 x 128 (8-row blocks, 1 024 workgroups)
    dict(B=8, H=16, W=16, src=[(512, 'nhwc'), (512, 'nhwc')], Cout=256, up=True),
    dict(B=8, H=128, W=128, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True),
]


# ---------------------------------------------------------------------------
# Every accepted geometry off the 3x3 / pad-1 forms (tests/test_gpu_conv_geometry.py): ksize
# 1 | 3 | 5, stride 1 | 2, pad 0 .. ksize-1, 2x nearest up-sampling in front of any of them.
# All of these run the general family; `path` is derived from the dispatch:
#   forward (gconv_launch):  v2 when every vector member (NHWC, 4 | C, C >= 16) has 16 | C,
#                            else v1; no vector member: v1
#   data gradient:           the same test on gout, i.e. on Cout; its form by conv_classify:
#                            DG_PLAIN, DG_ZERO2 (stride 2), DG_QUAD (up-sampling)
#   weight gradient (wgrad_plan): v2 when 16 | Wo and the layer does not up-sample, else
#                            the v1 tiles; a flat-only layer takes flat_valu when its
#                            ksize^2 C columns are 18, 27, 45, 81 or 108, else the v1 tiles
# A family written 'general_v2:1' reports operand mode 1 in that call: mode 3 falls back to
# mode 1 on v2 when a vector operand is no multiple of 32 channels (gconv2_launch).
# Each case is the smallest frame at which its path can still go wrong.
# ---------------------------------------------------------------------------
_V221 = ('general_v2 general_v2 general_v1',) * 4
_V222 = ('general_v2 general_v2 general_v2',) * 4
_ONE = [(32, 'nhwc')]
GEOMETRY = [
    # ---- plain layers: FWD_GENERAL, DG_PLAIN (pad' = ksize - 1 - pad), WG_GENERAL
    # 1x1 / pad 0; Cout = 48: the mode-3 data gradient reads 48 channels of gout, no whole
    # 64-byte slices of bf16
    dict(B=2, H=5, W=7, src=_ONE, Cout=48, k=1, pad=0,
         path=_V221[:3] + ('general_v2 general_v2:1 general_v1',)),
    # ... on the v1 tiles with a flat member of 3 columns and Cout % 4 != 0 (gout is a flat
    # operand of the data gradient)
    dict(B=2, H=5, W=7, src=[(20, 'nhwc'), (3, 'nchw')], Cout=10, k=1, pad=0,
         path=('general_v1 general_v1 general_v1',) * 3),
    dict(B=2, H=6, W=9, src=_ONE, Cout=32, pad=0, path=_V221),
    # the output (6 x 7) is larger than the input: corner outputs see one input pixel
    dict(B=2, H=4, W=5, src=_ONE, Cout=32, pad=2, path=_V221),
    # 5x5 at every pad but 2 (CASES holds that one); 24 channels of gout: v1 data gradient
    dict(B=1, H=7, W=9, src=[(16, 'nhwc'), (2, 'nchw')], Cout=24, k=5, pad=0,
         path=('general_v2 general_v1 general_v1',) * 3),
    dict(B=1, H=7, W=9, src=[(16, 'nhwc'), (2, 'nchw')], Cout=24, k=5, pad=1,
         path=('general_v2 general_v1 general_v1',) * 3),
    dict(B=1, H=7, W=9, src=[(16, 'nhwc'), (2, 'nchw')], Cout=24, k=5, pad=3,
         path=('general_v2 general_v1 general_v1',) * 3),
    dict(B=1, H=7, W=9, src=[(16, 'nhwc'), (2, 'nchw')], Cout=24, k=5, pad=4,
         path=('general_v2 general_v1 general_v1',) * 3),
    # one-pixel frames
    dict(B=3, H=1, W=1, src=_ONE, Cout=32, k=1, pad=0, path=_V221),
    dict(B=3, H=1, W=1, src=_ONE, Cout=32, path=_V221),
    dict(B=3, H=1, W=1, src=_ONE, Cout=32, k=5, pad=4, path=_V221),     # 5 x 5 output
    # ---- stride 2 off the phased form: DG_ZERO2 (zero-inserted gout)
    dict(B=2, H=9, W=11, src=_ONE, Cout=32, stride=2, path=_V221),      # odd frame
    dict(B=2, H=9, W=11, src=[(24, 'nhwc'), (2, 'nchw')], Cout=32, stride=2,   # v1 forward, planar destination
         path=('general_v1 general_v2 general_v1',) * 3),
    dict(B=2, H=8, W=10, src=_ONE, Cout=32, stride=2, pad=0, path=_V221),      # row 7, column 9 unread
    dict(B=2, H=8, W=8, src=_ONE, Cout=32, stride=2, pad=2, path=_V221),
    dict(B=2, H=6, W=7, src=_ONE, Cout=32, k=1, stride=2, pad=0, path=_V221),  # odd positions unread
    dict(B=1, H=9, W=12, src=_ONE, Cout=32, k=5, stride=2, pad=2, path=_V221),
    dict(B=1, H=8, W=12, src=_ONE, Cout=32, k=5, stride=2, pad=0, path=_V221),  # row 7, column 11 unread
    # ---- up-sampling off the sub-pixel form: general forward, DG_QUAD, general weight gradient
    dict(B=1, H=4, W=8, src=[(32, 'nhwc'), (32, 'nhwc')], Cout=32, up=True, pad=0, path=_V221),
    dict(B=1, H=4, W=8, src=[(32, 'nhwc'), (32, 'nhwc')], Cout=32, up=True, pad=2, path=_V221),
    # a planar destination in the quad epilogue (mode 3 falls back to mode 1 on the
    # 16-channel member: test_mode3_falls_back_on_a_narrow_member)
    dict(B=2, H=5, W=6, src=[(32, 'nhwc'), (16, 'nhwc'), (2, 'nchw')], Cout=32, up=True, k=5, pad=2,
         path=_V221[:3]),
    dict(B=1, H=5, W=6, src=[(20, 'nhwc')], Cout=24, up=True, k=5, pad=2,      # the quad rows on v1
         path=('general_v1 general_v1 general_v1',) * 3),
    dict(B=2, H=3, W=5, src=_ONE, Cout=32, up=True, k=1, pad=0, path=_V221),
    # the nine-product gate's shape with only `pad` changed
    dict(B=1, H=8, W=16, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True, pad=0, path=_V221),
    # ---- one field away from a special kernel
    # not `first` (planar 5 -> 64, stride 2): pad 0, 5x5 / pad 2 (125 flat columns: on the v1
    # tiles), 3x3 / pad 1 on an odd frame
    dict(B=1, H=8, W=8, src=[(5, 'nchw')], Cout=64, stride=2, pad=0,
         path=('general_v1 general_v2 flat_valu',) * 4),
    dict(B=1, H=8, W=8, src=[(5, 'nchw')], Cout=64, stride=2, k=5, pad=2,
         path=('general_v1 general_v2 general_v1',) * 4),
    dict(B=1, H=9, W=8, src=[(5, 'nchw')], Cout=64, stride=2,
         path=('general_v1 general_v2 flat_valu',) * 4),
    # not Winograd (B2 16x16 256 -> 256 is at its gate with pad 1)
    dict(B=2, H=16, W=16, src=[(256, 'nhwc')], Cout=256, pad=0, path=_V221, no_wino=True),
    dict(B=2, H=16, W=16, src=[(256, 'nhwc')], Cout=256, pad=2, path=_V221, no_wino=True),
    # not fwd_patch
    dict(B=1, H=2, W=16, src=[(64, 'nhwc'), (64, 'nhwc')], Cout=32, up=True, pad=2, path=_V221),
    # ---- added to the issue's list because the dispatch needs them
    # DG_ZERO2 through the v1 VECTOR loader: v1 reads gout as a vector operand only when
    # 4 | Cout, Cout >= 16 and 16 does not divide Cout (32 channels of gout go to v2)
    dict(B=2, H=9, W=11, src=_ONE, Cout=24, stride=2,
         path=('general_v2 general_v1 general_v1',) * 4),
    # the v2 weight gradient needs rows of whole 16-pixel groups (16 | Wo), which no frame
    # above has: 3x3 / pad 0 on 5 x 18 and 5x5 / pad 3 on 4 x 14 (Wo = 16; the latter is also
    # the 5x5 DG_PLAIN data gradient on v2 with pad' = 1)
    dict(B=1, H=5, W=18, src=_ONE, Cout=32, pad=0, path=_V222),
    dict(B=1, H=4, W=14, src=_ONE, Cout=32, k=5, pad=3, path=_V222),
]
for _c in GEOMETRY:     # every case carries its geometry in full
    _c.update(k=_c.get('k', 3), stride=_c.get('stride', 1), pad=_c.get('pad', 1), up=_c.get('up', False))


def geometry_id(case):
    o = layer_geometry(case)
    return 'B%dH%dW%d_%s_%d_k%ds%dp%d%s' % (
        case['B'], case['H'], case['W'], '+'.join('%d%s' % (c, 'p' if lay == 'nchw' else '') for c, lay in case['src']),
        case['Cout'], o['k'], o['stride'], o['pad'], 'up' if o['up'] else '')


def split_path(case, mode):
    """-> [(family, reported operand mode)] x 3 of `case` in a call of operand mode `mode`."""
    out = []
    for kind, tok in enumerate(case['path'][mode].split()):
        fam, _, m = tok.partition(':')
        out.append((fam, int(m) if m else effective_mode(kind, fam, mode)))
    return out


# ---------------------------------------------------------------------------
# Integer-grid data: every product and every partial sum is an integer (or a
# dyadic fraction) far below 2^24, so f32 arithmetic in any order, the bf16
# operand modes (integers of at most 8 bits are exact bf16, lo = 0 in the
# split) and the prepared forms made of integer sums are all exact.
# ---------------------------------------------------------------------------
GRID = dict(x=1, w=2, b=4, g=1)      # |x|, |gout| <= 1; |w| <= 2; biases / addends <= 4
EXACT_LIMIT = 2 ** 24

# growth of the worst-case partial sum over (reduction length x max|a| x max|b|) by
# the family's transform: sub-pixel phase forms sum up to four taps; the nine-product
# forms (G w G^T, D x) and Winograd transform both operands and the result
TRANSFORM_GROWTH = {'fwd_min4': 36, 'fwd_min8': 36, 'dgrad_min0': 36, 'dgrad_min1': 36,
                    'dgrad_min2': 36, 'wgrad_min': 36, 'wino2': 36, 'wino4': 36}


def int_grid(g, shape, m):
    """Integers in [-m, m], as float64."""
    return torch.randint(-m, m + 1, shape, generator=g).double()


def exact_bound(K, amax, bmax, family, up=False, extra=0.0):
    """Worst-case magnitude of any partial sum of a pass: reduction length x max|a| x
    max|b| x the growth of the family's transform (4 for the sub-pixel forms of an
    up-sampling layer), plus what the epilogue adds."""
    growth = TRANSFORM_GROWTH.get(family, 4 if up else 1)
    return K * amax * bmax * growth + extra


def assert_exact_premise(K, amax, bmax, family, up=False, extra=0.0):
    bound = exact_bound(K, amax, bmax, family, up, extra)
    assert bound < EXACT_LIMIT, ('integer grid too wide for exact f32', K, amax, bmax, family, bound)
    return bound


# ---------------------------------------------------------------------------
# The bf16 rounding contract (include/dvsof.h, dvsof_conv_desc_t.mfma), emulated in
# float64.  An operand is rounded from its f32 value:
#   modes 1, 3: a * b -> RNE(a) * RNE(b)
#   mode 2:     a * b -> hi(a) hi(b) + hi(a) lo(b) + lo(a) hi(b),  hi = RNE(a), lo = RNE(a - hi)
# where the weight operand of a sub-pixel layer (up-sampling, 3x3 / pad 1) is its phase
# form (sums of taps made in f32, then rounded); any other up-sampling layer rounds the raw
# taps.  Bias, residual, addends and the epilogue stay f32.
# ---------------------------------------------------------------------------
# relative L2 error a bf16 pass may have against its emulation, per mode: f32 summation
# order only (4x the worst of the first run on an MI355X, test_gpu_conv_exact.py)
EMU_TAU = {1: 7.5e-7, 2: 7.5e-7, 3: 7.5e-7}
EMU_TAU_DB = 1e-6       # bias gradient: a plain f32 channel sum


def rne_bf16(t):
    return t.float().to(torch.bfloat16).double()


def trunc_bf16(t):
    """bf16 by truncation (round toward zero): the rounding a kernel must NOT use."""
    i = t.float().contiguous().view(torch.int32) & -65536
    return i.view(torch.float32).double()


def split_bf16(t, rnd=rne_bf16):
    hi = rnd(t)
    return hi, rnd(t.float().double() - hi)        # a - hi is exact in f32


def operand_pairs(a, b, rounding):
    """The products a kernel forms from operands a, b: [(a', b'), ...] summed.
    rounding: 'exact' | 'rne' | 'trunc' | 'x3' | 'x3_no_cross' (one cross term dropped)."""
    if rounding == 'exact':
        return [(a, b)]
    if rounding in ('rne', 'trunc'):
        r = rne_bf16 if rounding == 'rne' else trunc_bf16
        return [(r(a), r(b))]
    (ah, al), (bh, bl) = split_bf16(a), split_bf16(b)
    if rounding == 'x3':
        return [(ah, bh), (ah, bl), (al, bh)]
    assert rounding == 'x3_no_cross'
    return [(ah, bh), (ah, bl)]


def phase_forms(w):
    """[Cout][Ci][3][3] -> [2][2][Cout][Ci][2][2]: the sub-pixel phase kernels of a 2x
    nearest-upsampled 3x3 / pad-1 layer.  Rows: phase a = 0 reads input rows (i-1 | i)
    with (w0 | w1 + w2), a = 1 rows (i | i+1) with (w0 + w1 | w2); columns alike."""
    def fold(v, axis, a):
        t0, t1, t2 = v.unbind(axis)
        return torch.stack((t0, t1 + t2) if a == 0 else (t0 + t1, t2), axis)
    return torch.stack([torch.stack([fold(fold(w, 2, a), 3, b) for b in (0, 1)]) for a in (0, 1)])


def is_subpixel(o):
    """The layer runs as sub-pixel phases: 2x nearest up-sampling in front of 3x3 / pad 1
    (csrc/conv_api.hip, conv_classify).  Every other up-sampling layer gathers the raw taps
    from the up-sampled frame."""
    return bool(o['up']) and o.get('k', 3) == 3 and o.get('pad', 1) == 1 and o.get('stride', 1) == 1


def lin_fwd(x, wf, o):
    """The layer's bilinear part on NCHW x with the forward weight form wf (raw OIHW, or
    phase_forms for a sub-pixel layer)."""
    if not is_subpixel(o):
        xv = F.interpolate(x, scale_factor=2, mode='nearest') if o['up'] else x
        return F.conv2d(xv, wf, stride=o['stride'], padding=o['pad'])
    B, _, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    out = x.new_zeros(B, wf.shape[2], 2 * H, 2 * W)
    for a in (0, 1):
        for b in (0, 1):
            out[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], wf[a, b])
    return out


def fwd_form(w, o):
    return phase_forms(w) if is_subpixel(o) else w


def emulate_fwd(x, w, o, rounding):
    """Sum of the products the forward multiplies (no bias)."""
    return sum(lin_fwd(a, b, o) for a, b in operand_pairs(x, fwd_form(w, o), rounding))


def emulate_dgrad(x_shape, w, g, o, rounding):
    """Data gradient: operands gout and the forward weight form (the data-gradient forms
    hold the same values), by autograd through lin_fwd."""
    total = 0
    for ga, wa in operand_pairs(g, fwd_form(w, o), rounding):
        x0 = torch.zeros(x_shape, dtype=torch.float64, device=g.device, requires_grad=True)
        total = total + torch.autograd.grad(lin_fwd(x0, wa, o), x0, ga)[0]
    return total


def emulate_wgrad(x, w_shape, g, o, rounding):
    """Weight gradient of the raw 3x3 taps on the (up-sampled) input: operands gout and x."""
    total = 0
    for ga, xa in operand_pairs(g, x, rounding):
        xv = F.interpolate(xa, scale_factor=2, mode='nearest') if o['up'] else xa
        w0 = torch.zeros(w_shape, dtype=torch.float64, device=g.device, requires_grad=True)
        z = F.conv2d(xv, w0, stride=o['stride'], padding=o['pad'])
        total = total + torch.autograd.grad(z, w0, ga)[0]
    return total


def dyadic_weights(g, shape, e=16):
    """Weights m * 2^-e with |m| < 2^11: the f32 sums of up to four of them (the phase
    forms) are exact, so only the bf16 rounding of the form is non-trivial."""
    return torch.randint(-2047, 2048, shape, generator=g).double() * 2.0 ** -e


def contract_errors(got, ref, absref):
    """(relative L2 error, worst |got - ref| / (2^-16 sum|a||b|)) of a pass."""
    got, ref, absref = got.double(), ref.double(), absref.double()
    d = got - ref
    rel = (d.norm() / ref.norm()).item()
    elem = (d.abs() / (2.0 ** -16 * absref).clamp_min(1e-300)).max().item()
    return rel, elem


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def old_bar_passes(got, want, rtol=2e-2):
    """The bar test_gpu_conv.py holds a bf16 pass to: 2e-2 of the tensor's peak."""
    got, want = got.double(), want.double()
    return (got - want).abs().max().item() <= rtol * want.abs().max().item() + 1e-7


def twins_apply(case):
    """Mode 3 runs as itself when every NHWC member has C % 32 == 0."""
    return all(c % 32 == 0 for c, lay in case['src'] if lay == 'nhwc')


def layer_geometry(case):
    return dict(k=case.get('k', 3), stride=case.get('stride', 1), pad=case.get('pad', 1),
                up=case.get('up', False))


def run_layer(case, mode, xs, w, b, res, gz, p16=False, epi=None, bwd_act=0):
    """Forward (with z), data gradient and weight gradient of a CASES-style layer through
    the C ABI in operand mode `mode` (3: twins of the NHWC members, gout and the weight
    forms made by .to(bfloat16) / dvsof_conv2d_prepare16).  Inputs are NCHW CPU tensors of
    any float type; outputs are NCHW float32 on the GPU, with the family of each pass.
    epi: per member dict(addend=, addend2=, actsrc=) NCHW tensors for the data-gradient
    epilogue, act'(actsrc) of kind bwd_act."""
    from dvs_of_training_framework_amd import conv as C
    B, H, W, Cout = case['B'], case['H'], case['W'], case['Cout']
    o = layer_geometry(case)
    act = {'relu': C.ACT_RELU, 'mish': C.ACT_MISH, 'none': C.ACT_NONE}[case.get('act', 'relu')]
    twins = mode == C.MFMA_BF16_TWINS
    dev = [(x.float().cuda().contiguous() if lay == 'nchw' else nhwc(x.float()))
           for x, (_, lay) in zip(xs, case['src'])]
    srcs = [(d, c, C.NCHW if lay == 'nchw' else C.NHWC,
             d.to(torch.bfloat16) if (twins and lay == 'nhwc') else None)
            for d, (c, lay) in zip(dev, case['src'])]
    desc = C.make_desc(srcs, B, H, W, Cout, o['k'], o['stride'], o['pad'], o['up'], act, mode)
    desc._keep = srcs
    if twins:
        w_f, w_dg, w_f16, w_dg16 = C.prepare(desc, wphys(w.float()), True, want16=True)
    else:
        (w_f, w_dg), w_f16, w_dg16 = C.prepare(desc, wphys(w.float()), True), None, None
    out = {}
    y, z = C.conv_fwd(desc, w_f, b.float().cuda(), 'cuda',
                      nhwc(res.float()) if res is not None else None, want_z=True,
                      keep_input_transform=bool(case.get('wino')), weight16=w_f16)
    out['fam'] = [C.KERNEL_NAMES[C.last_kernel(0)[0]]]
    out['modes'] = [C.last_kernel(0)[1]]
    out['y'], out['z'] = from_nhwc(y), from_nhwc(z)
    out['y16'] = from_nhwc(desc._y16.view(y.shape)) if twins else None
    gz_d = nhwc(gz.float())
    dsts, bufs = [], []
    put = lambda t, lay: None if t is None else (t.float().cuda().contiguous() if lay == 'nchw'  # noqa: E731
                                                 else nhwc(t.float()))
    for i, (x, (c, lay)) in enumerate(zip(xs, case['src'])):
        shape = x.shape if lay == 'nchw' else (x.shape[0], x.shape[2], x.shape[3], c)
        buf = torch.full(shape, float('nan'), device='cuda')
        b16 = torch.empty(shape, dtype=torch.bfloat16, device='cuda') \
            if (p16 and twins and lay == 'nhwc') else None
        bufs.append((buf, b16, lay))
        e = (epi or [{}] * len(xs))[i]
        dsts.append(dict(p=buf, p16=b16, **{k: put(v, lay) for k, v in e.items()}))
    C.conv_dgrad(desc, w_dg, gz_d, dsts, bwd_act, weight16=w_dg16,
                 gout16=gz_d.to(torch.bfloat16) if twins else None)
    out['fam'].append(C.KERNEL_NAMES[C.last_kernel(1)[0]])
    out['modes'].append(C.last_kernel(1)[1])
    out['dx'] = [buf if lay == 'nchw' else from_nhwc(buf) for buf, _, lay in bufs]
    out['dx16'] = [(from_nhwc(b16) if b16 is not None else None) for _, b16, _ in bufs]
    ctot = sum(c for c, _ in case['src'])
    dw = torch.full((Cout, o['k'], o['k'], ctot), float('nan'), device='cuda')
    db = torch.full((Cout,), float('nan'), device='cuda')
    C.conv_wgrad(desc, gz_d, dw, db, gz_d.to(torch.bfloat16) if twins else None)
    out['fam'].append(C.KERNEL_NAMES[C.last_kernel(2)[0]])
    out['modes'].append(C.last_kernel(2)[1])
    out['dw'], out['db'] = dw.permute(0, 3, 1, 2), db
    torch.cuda.synchronize()
    return out


def reference64(case, xs, w, b, res, gz, device='cuda'):
    """float64 forward / data / weight / bias gradient of the layer (ATen autograd)."""
    o = layer_geometry(case)
    xs64 = [x.double().to(device).requires_grad_(True) for x in xs]
    w64 = w.double().to(device).requires_grad_(True)
    b64 = b.double().to(device).requires_grad_(True)
    inp = torch.cat(xs64, 1)
    if o['up']:
        inp = F.interpolate(inp, scale_factor=2, mode='nearest')
    z = F.conv2d(inp, w64, b64, stride=o['stride'], padding=o['pad'])
    if res is not None:
        z = z + res.double().to(device)
    z.backward(gz.double().to(device))
    act = case.get('act', 'relu')
    zd = z.detach()
    y = F.relu(zd) if act == 'relu' else F.mish(zd) if act == 'mish' else zd
    return dict(y=y, z=zd, dx=[x.grad for x in xs64], dw=w64.grad, db=b64.grad)
