// The convolution stack's dispatch: conv_classify turns a dvsof_conv_desc_t into the form of
// each of the layer's three passes, once per entry point; dvsof_conv2d_fwd / _dgrad / _wgrad
// fill the kernels' parameters for that form and call its launcher; the planning queries
// answer from the same classification.  (Weight forms: conv_weights.hip; head: conv_head.hip.)
#include "conv_host.h"

// family | mode << 8 of what the calling thread's last fwd (0) / dgrad (1) / wgrad (2) launched
// (dvsof_conv2d_last_kernel; dvsof_conv2d_last_patch is derived from it), noted by the launcher
// that ran; t_kind = the entry point in progress
static thread_local int t_last_kernel[3] = {0, 0, 0};
static thread_local int t_kind = 0;
void conv_note_kernel(int family, int mode) { t_last_kernel[t_kind] = family | mode << 8; }
static void conv_begin(int kind)
{
    t_kind = kind;
    t_last_kernel[kind] = DVSOF_KERNEL_NONE;
}
// the layer-level family of a launch that ran on the general kernels (the phase forms), in the
// mode the kernel noted
static int conv_retag(int rc, int family)
{
    if (rc == DVSOF_OK && t_last_kernel[t_kind]) conv_note_kernel(family, t_last_kernel[t_kind] >> 8);
    return rc;
}

namespace {

GSrc make_src(const float *p, int C, int layout, int H, int W, const void *p16 = nullptr)
{
    GSrc s;
    s.p = p;
    s.p16 = layout == DVSOF_NHWC ? (const unsigned short *)p16 : nullptr;
    s.C = C;
    if (layout == DVSOF_NCHW) {
        s.sb = (long long)C * H * W;
        s.sy = W;
        s.sx = 1;
        s.sc = H * W;
        s.flat = 1;
    } else {
        s.sb = (long long)H * W * C;
        s.sy = W * C;
        s.sx = C;
        s.sc = 1;
        s.flat = ((C & 3) || C < BK) ? 1 : 0;
    }
    return s;
}

bool desc_ok(const dvsof_conv_desc_t *d, int &Ctot, int &Ho, int &Wo)
{
    if (!d || d->nsrc < 1 || d->nsrc > 3 || d->B < 1 || d->H < 1 || d->W < 1) return false;
    if (d->ksize != 1 && d->ksize != 3 && d->ksize != 5) return false;
    if (d->stride != 1 && d->stride != 2) return false;
    if (d->upsample < 0 || d->upsample > 2) return false;
    if (d->upsample && d->stride != 1) return false;
    // upsample = 2: zero insertion (transposed convolution).  One NHWC source of
    // whole 16-channel K slices, 3x3 taps, pad 1: the phased MFMA form below
    if (d->upsample == 2 &&
        !(d->ksize == 3 && d->pad == 1 && d->nsrc == 1 && d->src[0].layout == DVSOF_NHWC &&
          d->src[0].C % BK == 0 && d->mfma != 3))
        return false;
    if (d->Cout < 1 || d->pad < 0 || d->pad >= d->ksize) return false;
    Ctot = 0;
    for (int i = 0; i < d->nsrc; ++i) {
        if (!d->src[i].p || d->src[i].C < 1) return false;
        Ctot += d->src[i].C;
    }
    const int up = d->upsample ? 2 : 1;
    Ho = (d->H * up + 2 * d->pad - d->ksize) / d->stride + 1;
    Wo = (d->W * up + 2 * d->pad - d->ksize) / d->stride + 1;
    if (Ho < 1 || Wo < 1) return false;
    if ((long long)d->B * Ho * Wo > 0x7fffffffLL) return false;
    if ((long long)d->B * d->H * up * d->W * up > 0x7fffffffLL) return false;
    return true;
}

// the operand mode the general kernels take (GConvParams.mfma_bf16)
int operand_mode(const dvsof_conv_desc_t *d) { return (d->mfma >= 1 && d->mfma <= 3) ? d->mfma : 0; }

// The layer's own geometry, shared by the forward, the weight gradient and its flat members:
// rows = output pixels, input = the (up-sampled) frame
template <class Params>
void layer_geometry(Params &P, const dvsof_conv_desc_t *d, const ConvClass &c)
{
    const int up = d->upsample ? 2 : 1;
    P.B = d->B;
    P.Hv = d->H * up;
    P.Wv = d->W * up;
    P.up = d->upsample ? UP_NEAREST : UP_NONE;
    P.Ho = c.Ho;
    P.Wo = c.Wo;
    P.stride = d->stride;
    P.pad = d->pad;
    P.ks = d->ksize;
    P.M = d->B * c.Ho * c.Wo;
}

// Four phase problems of 2x2 taps over the low-resolution grid h x w (blockIdx.z = 2 py + px):
// the sub-pixel forward and weight gradient (pad 1, less ph_pad = 1 per phase bit), the
// transposed forward and the phased stride-2 data gradient (pad 0; the caller sets ph_exact)
template <class Params>
void four_phases(Params &P, int h, int w, int pad, int ph_pad)
{
    P.up = UP_NONE;
    P.Hv = P.Ho = h;
    P.Wv = P.Wo = w;
    P.ks = 2;
    P.stride = 1;
    P.pad = pad;
    P.M = P.B * h * w;
    P.nph = 4;
    P.ph_pad = ph_pad;
}
// ... and the full-resolution tensor the phases interleave in: phase (py, px) starts py rows
// and px pixels in and steps twice as far
void phase_strides(int &sy, int &sx, int &ph_y, int &ph_x)
{
    ph_y = sy;
    ph_x = sx;
    sy *= 2;
    sx *= 2;
}

void fill_wgrad(const dvsof_conv_desc_t *d, const ConvClass &c, WGradParams &P)
{
    P.mfma_bf16 = d->mfma == 3 ? 1 : operand_mode(d);   // twins: f32 tensors, rounded operands
    P.nsrc = d->nsrc;
    for (int i = 0; i < d->nsrc; ++i)
        P.src[i] = make_src(d->src[i].p, d->src[i].C, d->src[i].layout, d->H, d->W,
                            d->mfma == 3 ? d->src[i].p16 : nullptr);
    // bf16 twins (mode 3): gout and every vector member streamed from their bf16
    // copies when all of them exist and channel runs are whole 16-byte loads
    P.gout16 = d->mfma == 3 ? (const unsigned short *)d->gout16 : nullptr;
    P.twins = P.gout16 != nullptr && (d->Cout % 8) == 0;
    for (int i = 0; i < d->nsrc; ++i)
        if (!P.src[i].flat && (!P.src[i].p16 || (P.src[i].C % 8))) P.twins = 0;
    layer_geometry(P, d, c);
    P.Cout = d->Cout;
    P.Cin_tot = c.Ctot;
    P.nph = 1;
    P.S = 1;
    P.g_sb = (long long)c.Ho * c.Wo * d->Cout;
    P.g_sy = c.Wo * d->Cout;
    P.g_sx = d->Cout;
    if (c.wgrad == WG_SUBPIXEL) {   // rows = low-res pixels, gout read at its four phases
        four_phases(P, d->H, d->W, d->pad, 1);
        phase_strides(P.g_sy, P.g_sx, P.g_py, P.g_px);
    }
}

int fill_flat(const dvsof_conv_desc_t *d, const ConvClass &c, const float *gout, FlatWG *F)
{
    int n = 0, coff = 0;
    for (int i = 0; i < d->nsrc; ++i) {
        const GSrc g = make_src(d->src[i].p, d->src[i].C, d->src[i].layout, d->H, d->W);
        if (g.flat) {
            FlatWG &f = F[n++];
            f.S = g;
            f.gout = gout;
            layer_geometry(f, d, c);
            f.Cout = d->Cout;
            f.ncol = d->ksize * d->ksize * g.C;
            f.coff = coff;
            f.Cin_tot = c.Ctot;
        }
        coff += d->src[i].C;
    }
    return n;
}

// per-channel sum of an NHWC tensor, fixed order: partial sums per workgroup
// (64 pixels per pass and lane group), then one wave per channel
__global__ __launch_bounds__(256) void channel_sum_partial_kernel(const float *__restrict__ g,
                                                                  long long npix, int C,
                                                                  float *__restrict__ part)
{
    // thread t owns channel c = t % C of pixel rows t / C, t / C + 256 / C, ... (C <= 256)
    const int per = 256 / C, c = threadIdx.x % C, r = threadIdx.x / C;
    float a = 0.f;
    if (r < per)
        for (long long p = (long long)blockIdx.x * per + r; p < npix; p += (long long)gridDim.x * per)
            a += g[p * C + c];
    __shared__ float sm[256];
    sm[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x < C) {
        float t = 0.f;
        for (int j = 0; j < per; ++j) t += sm[j * C + threadIdx.x];
        part[(size_t)blockIdx.x * C + threadIdx.x] = t;
    }
}
__global__ __launch_bounds__(256) void channel_sum_final_kernel(const float *__restrict__ part,
                                                                int nblocks, int C,
                                                                float *__restrict__ out)
{
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= C) return;
    double a = 0;
    for (int b = lane; b < nblocks; b += 64) a += (double)part[(size_t)b * C + c];
    a = wave_sum(a);
    if (lane == 0) out[c] = (float)a;
}

}  // namespace

ConvClass conv_classify(const dvsof_conv_desc_t *d)
{
    ConvClass c = {};
    c.ok = desc_ok(d, c.Ctot, c.Ho, c.Wo);
    if (!c.ok) return c;
    // ---- what the shape allows
    // up2 + 3x3/pad1/stride1 == four 2x2 phase convolutions on the low-res input
    const bool subpixel = d->upsample == 1 && d->ksize == 3 && d->pad == 1 && d->stride == 1;
    // zero-insertion 2x + 3x3/pad 1 = transposed convolution with stride 2:
    // y[Y][X] = sum_k W[ky][kx] xz[Y+ky-1][X+kx-1], xz[2i][2j] = x[i][j], else 0
    // (torch: conv_transpose2d(x, W.flip(2,3).transpose(0,1), stride 2, padding 1,
    // output_padding 1)).  Evaluated as four output-parity phases of (1+py)(1+px)
    // taps on the low-resolution input -- the adjoint of the phased stride-2 layer.
    const bool transposed = d->upsample == 2;
    const bool phased2 = !d->upsample && d->stride == 2 && d->ksize == 3 && d->pad == 1 &&
                         (d->H % 2 == 0) && (d->W % 2 == 0);
    // the first encoder layer's own kernels (first.hip); not with the border bias of a folded
    // flow member, which only the general kernels' epilogue adds
    const bool first = first_layer_shape(d->nsrc, d->src[0].layout == DVSOF_NCHW, d->src[0].C, d->Cout, d->H,
                                         d->W, d->ksize, d->stride, d->pad, d->upsample) && !d->bias_cls;
    // wide 3x3 stride-1 layer evaluated as Winograd F(2x2,3x3) / F(4x4,3x3) (winograd.hip)
    const bool wino = d->nsrc == 1 &&
                      wino_eligible_shape(d->nsrc, d->src[0].layout == DVSOF_NHWC, d->src[0].C, d->Cout, d->B,
                                          d->H, d->W, d->ksize, d->stride, d->pad, d->upsample, d->mfma);
    c.wino_mode = d->mfma == 2 ? 2 : 0;
    // ... and its weight gradient too: the tile count is the K dimension of the K-major kernel,
    // which loads whole 16-element groups
    const int wg_tile = wino ? wino_wgrad_tile(d->B, d->H, d->W, c.wino_mode) : 0;
    // sub-pixel layers whose forward (fwd_min.hip) / data gradient (dgrad_min.hip) runs the
    // nine-product minimal algorithm
    bool min9 = false, min9_dgrad = false;
    if (subpixel) {
        int C[3] = {0, 0, 0}, nhwc[3] = {0, 0, 0};
        for (int i = 0; i < d->nsrc; ++i) {
            C[i] = d->src[i].C;
            nhwc[i] = d->src[i].layout == DVSOF_NHWC;
        }
        min9 = min9_shape_ok(d->mfma, d->nsrc, C, nhwc, d->Cout, d->H, d->W);
        min9_dgrad = min9 && min9_dgrad_shape_ok(C, d->Cout, d->H);
    }
    // ---- the precedence between the forms (conv_host.h)
    c.fwd = first ? FWD_FIRST : wino ? FWD_WINO : min9 ? FWD_MIN9 : subpixel ? FWD_SUBPIXEL
          : transposed ? FWD_TRANSPOSED : FWD_GENERAL;
    c.dgrad = min9_dgrad ? DG_MIN9 : wino ? DG_WINO : subpixel ? DG_SUBPIXEL : phased2 ? DG_PHASED2
            : transposed ? DG_TRANSPOSED : d->upsample ? DG_QUAD : d->stride == 2 ? DG_ZERO2 : DG_PLAIN;
    c.wgrad = transposed ? WG_TRANSPOSED : wg_tile ? WG_WINO : first ? WG_FIRST : subpixel ? WG_SUBPIXEL
            : WG_GENERAL;
    // ---- derived facts
    if (wino) {
        c.wino_tile[0] = c.wino_tile[1] = wino_tile(d->B, d->H, d->W, c.wino_mode);
        c.wino_tile[2] = wg_tile;
        c.wino_chain[0] = wino_chain_ok(d->B, d->H, d->W, d->Cout, c.wino_mode);
        c.wino_chain[1] = wino_chain_ok(d->B, d->H, d->W, c.Ctot, c.wino_mode);
    }
    // a head folds into the nine-product data gradient (dgrad_min.hip) and into the sub-pixel
    // layers' 4x4 stride-2 form on the general kernels (conv_epilogue), member 0 (NHWC) only
    c.head_folds = min9_dgrad || (subpixel && d->src[0].layout == DVSOF_NHWC);
    return c;
}

extern "C" {

int dvsof_conv2d_fwd(const dvsof_conv_desc_t *d, const float *weight, const float *bias,
                     const float *residual, float *y, float *z, void *stream)
{
    conv_begin(0);
    const ConvClass c = conv_classify(d);
    if (!c.ok || !weight || !y) return DVSOF_EINVAL;
    hipStream_t st = as_stream(stream);
    unsigned short *y16 = d->mfma == 3 ? (unsigned short *)d->y16 : nullptr;
    if (c.fwd == FWD_FIRST && !residual)     // exact f32 in every operand mode; no residual epilogue
        return first_fwd_launch(d->src[0].p, d->B, c.Ctot, d->H, d->W, weight, bias, d->act, y, z, y16, st);
    // the forms shared along a chain of Winograd layers are a Winograd forward's options
    if (d->winograd_next_gout || (c.fwd != FWD_WINO && (d->winograd_pre || d->winograd_next)))
        return DVSOF_EINVAL;
    const int Cout = d->Cout;
    GConvParams P = {};
    P.nsrc = d->nsrc;
    for (int i = 0; i < d->nsrc; ++i)
        P.src[i] = make_src(d->src[i].p, d->src[i].C, d->src[i].layout, d->H, d->W, d->src[i].p16);
    P.ndst = 1;
    P.dst[0] = {y, residual, nullptr, nullptr, (long long)c.Ho * c.Wo * Cout, c.Wo * Cout, Cout, 1, Cout, 0, 0, y16};
    P.W = weight;
    P.W16 = d->mfma == 3 ? (const unsigned short *)d->w16 : nullptr;
    P.bias = bias;
    P.bias_cls = d->bias_cls;
    P.out_H = c.Ho;
    P.out_W = c.Wo;
    P.zout = z;
    layer_geometry(P, d, c);
    P.N = Cout;
    P.Cin_tot = c.Ctot;
    P.act = d->act;
    P.mfma_bf16 = operand_mode(d);
    P.bwd_act = ACT_NONE;
    P.nph = 1;
    switch (c.fwd) {
    case FWD_WINO: {    // `weight` is the prepared U[16 | 36][Cout][Ctot]
        const WinoChain ch = {d->winograd_pre, d->winograd_next, nullptr};
        return wino_launch(P, (float *)d->scratch, d->scratch_bytes / sizeof(float), ch, st);
    }
    case FWD_MIN9:      // `weight` is the prepared Wt[9][Cout][Ctot]
    case FWD_SUBPIXEL:  // `weight` is the prepared Wf[4][Cout][2][2][Ctot]
        four_phases(P, d->H, d->W, d->pad, 1);
        break;
    case FWD_TRANSPOSED:    // `weight` is the prepared Wt[4][Cout][2][2][Ctot]; rows = low-res positions
        four_phases(P, d->H, d->W, 0, 0);
        P.ph_exact = 1;
        break;
    default: break;     // FWD_GENERAL, FWD_FIRST with a residual
    }
    if (P.nph == 4) {
        P.w_phase_stride = (long long)Cout * 4 * c.Ctot;
        phase_strides(P.dst[0].sy, P.dst[0].sx, P.dst[0].ph_y, P.dst[0].ph_x);
    }
    if (c.fwd == FWD_MIN9) return fwd_min_launch(P, st);
    if (c.fwd == FWD_SUBPIXEL && fwd_patch_eligible(P))    // finest decoder stage: fwd_patch.hip
        return fwd_patch_launch(P, st);
    const int rc = gconv_launch(P, 0, st);
    return c.fwd == FWD_TRANSPOSED ? conv_retag(rc, DVSOF_KERNEL_TRANSPOSED) : rc;
}

int dvsof_conv2d_dgrad_fuses_head(const dvsof_conv_desc_t *d)
{
    const ConvClass c = conv_classify(d);
    return c.ok && c.head_folds ? 1 : 0;
}

int dvsof_conv2d_dgrad_head_rows(const dvsof_conv_desc_t *d)
{
    const ConvClass c = conv_classify(d);
    if (!c.ok || c.dgrad != DG_MIN9) return 0;
    return d->B * (d->H / 8) * (d->W / 16);     // dgrad_min.hip's pixel blocks
}

int dvsof_conv2d_dgrad(const dvsof_conv_desc_t *d, const float *weight_t, const float *gout,
                       const dvsof_grad_dst_t *dst, int bwd_act, void *stream)
{
    conv_begin(1);
    const ConvClass c = conv_classify(d);
    if (!c.ok || !weight_t || !gout || !dst) return DVSOF_EINVAL;
    hipStream_t st = as_stream(stream);
    GConvParams P = {};
    P.nsrc = 1;
    P.src[0] = make_src(gout, d->Cout, DVSOF_NHWC, c.Ho, c.Wo, d->mfma == 3 ? d->gout16 : nullptr);
    P.ndst = d->nsrc;
    for (int i = 0; i < d->nsrc; ++i) {
        if (!dst[i].p) return DVSOF_EINVAL;
        const GSrc g = make_src(nullptr, d->src[i].C, d->src[i].layout, d->H, d->W);
        P.dst[i] = {dst[i].p, dst[i].addend, dst[i].addend2, dst[i].actsrc, g.sb, g.sy, g.sx, g.sc, g.C, 0, 0,
                    (d->mfma == 3 && d->src[i].layout == DVSOF_NHWC) ? (unsigned short *)dst[i].p16 : nullptr,
                    dst[i].head_w, dst[i].head_gflow, dst[i].head_x, dst[i].head_part};
        if ((dst[i].head_w != nullptr) != (dst[i].head_gflow != nullptr)) return DVSOF_EINVAL;
        if ((dst[i].head_x != nullptr) != (dst[i].head_part != nullptr)) return DVSOF_EINVAL;
        if (dst[i].head_part && (!dst[i].head_w || i != 0)) return DVSOF_EINVAL;
        // a folded head: member 0 of a layer whose data gradient folds one; its weight-gradient
        // partials (head_part) are the nine-product kernel's
        if (dst[i].head_w && (i != 0 || !c.head_folds)) return DVSOF_EINVAL;
        if (dst[i].head_part && c.dgrad != DG_MIN9) return DVSOF_EINVAL;
    }
    P.W = weight_t;
    P.W16 = d->mfma == 3 ? (const unsigned short *)d->w16 : nullptr;
    P.B = d->B;
    P.N = c.Ctot;
    P.Cin_tot = d->Cout;
    P.act = ACT_NONE;
    P.mfma_bf16 = operand_mode(d);
    P.bwd_act = bwd_act;
    P.nph = 1;
    // the adjoint: a stride-1 convolution of gout (c.Ho x c.Wo) with the flipped taps, rows =
    // the layer's input pixels -- and what each form changes of that
    P.up = UP_NONE;
    P.Hv = c.Ho;
    P.Wv = c.Wo;
    P.Ho = d->H;
    P.Wo = d->W;
    P.ks = d->ksize;
    P.stride = 1;
    P.pad = d->ksize - 1 - d->pad;
    switch (c.dgrad) {
    case DG_MIN9:       // weight_t is the prepared W'[9][Ctot][Cout]
    case DG_SUBPIXEL:
        // transpose of (up2 + 3x3) = 4x4 stride-2 convolution of gout with
        // the prepared Wd[Ctot][4][4][Cout]; rows = low-res input pixels
        P.ks = 4;
        P.stride = 2;
        P.pad = 1;
        break;
    case DG_PHASED2:
        // four input-parity phases, each a 2x2-tap stride-1 conv of gout
        // (weights prepared as Wp[4][Ctot][2][2][Cout]); rows = (H/2 x W/2)
        four_phases(P, d->H / 2, d->W / 2, 0, 0);
        P.ph_exact = 1;
        P.w_phase_stride = (long long)c.Ctot * 4 * d->Cout;
        for (int i = 0; i < d->nsrc; ++i) phase_strides(P.dst[i].sy, P.dst[i].sx, P.dst[i].ph_y, P.dst[i].ph_x);
        break;
    case DG_TRANSPOSED:
        // adjoint of the zero insertion: a plain stride-2 3x3/pad-1 convolution
        // of gout (2H x 2W) with the flip-transposed weights
        P.stride = 2;
        P.pad = 1;
        break;
    case DG_QUAD:       // rows = upsampled pixels, quad-summed to H x W
        P.Ho = 2 * d->H;
        P.Wo = 2 * d->W;
        P.quad = 1;
        break;
    case DG_ZERO2:      // zero-inserted gout
        P.up = UP_ZERO;
        P.Hv = 2 * c.Ho;
        P.Wv = 2 * c.Wo;
        break;
    default: break;     // DG_PLAIN, DG_WINO (weight_t is the prepared U'[16 | 36][Ctot][Cout])
    }
    P.M = d->B * P.Ho * P.Wo;
    if (c.dgrad == DG_MIN9) return dgrad_min_launch(P, st);
    if (c.dgrad == DG_WINO) {
        const WinoChain ch = {d->winograd_pre, d->winograd_next, d->winograd_next_gout};
        return wino_launch(P, (float *)d->scratch, d->scratch_bytes / sizeof(float), ch, st);
    }
    // the forms shared along a chain of Winograd layers are a Winograd data gradient's options
    if (d->winograd_pre || d->winograd_next || d->winograd_next_gout) return DVSOF_EINVAL;
    const int rc = gconv_launch(P, 0, st);
    return c.dgrad == DG_PHASED2 ? conv_retag(rc, DVSOF_KERNEL_STRIDE2_PHASED) : rc;
}

size_t dvsof_conv2d_scratch_bytes(const dvsof_conv_desc_t *d)
{
    const ConvClass c = conv_classify(d);
    if (!c.ok || c.fwd != FWD_WINO) return 0;
    return wino_scratch_floats(d->B, d->H, d->W, c.Ctot, d->Cout, c.wino_mode) * sizeof(float);
}

// Transposed layer T: [B,H,W,Ctot] -> [B,2H,2W,Cout].  Its weight gradient is
// the weight gradient of the adjoint stride-2 layer S: [B,2H,2W,Cout] ->
// [B,H,W,Ctot] with the roles swapped (S's input = T's output gradient, S's
// output gradient = T's input), flip-transposed:
//   dW_T[co][ky][kx][ci] = dW_S[ci][2-ky][2-kx][co].
static dvsof_conv_desc_t adjoint_of_transposed(const dvsof_conv_desc_t *d, int Ctot, const float *gy)
{
    dvsof_conv_desc_t a = *d;
    a.nsrc = 1;
    a.src[0].p = gy;
    a.src[0].C = d->Cout;
    a.src[0].layout = DVSOF_NHWC;
    a.src[0].p16 = nullptr;
    a.H = 2 * d->H;
    a.W = 2 * d->W;
    a.upsample = 0;
    a.stride = 2;
    a.Cout = Ctot;
    a.scratch = nullptr;
    a.scratch_bytes = 0;
    a.winograd_input = nullptr;
    return a;
}
static int channel_sum_blocks(long long npix, int C)
{
    const long long per = 256 / C, want = (npix + per * 8 - 1) / (per * 8);
    return (int)(want < 1 ? 1 : want > 1024 ? 1024 : want);
}

size_t dvsof_conv2d_wgrad_workspace_bytes(const dvsof_conv_desc_t *d)
{
    const ConvClass c = conv_classify(d);
    if (!c.ok) return 0;
    switch (c.wgrad) {
    case WG_TRANSPOSED: {
        static const float dummy = 0.f;
        const dvsof_conv_desc_t a = adjoint_of_transposed(d, c.Ctot, &dummy);
        size_t n = dvsof_conv2d_wgrad_workspace_bytes(&a);
        n = (n + 255) & ~(size_t)255;
        n += (size_t)c.Ctot * 9 * d->Cout * sizeof(float);                       // dW of the adjoint
        if (d->Cout <= 256)
            n += (size_t)channel_sum_blocks((long long)d->B * c.Ho * c.Wo, d->Cout) * d->Cout * sizeof(float);
        return n + 256;
    }
    case WG_WINO:
        return wino_wgrad_workspace_floats(d->B, d->H, d->W, c.Ctot, d->Cout, c.wino_mode) * sizeof(float) + 16;
    default: break;     // (WG_FIRST: the larger of the first-layer kernel's and the general one's, below)
    }
    WGradParams P = {};     // (unused member slots are zeros, not stack residue: _audit.audit_exchange reads these words)
    fill_wgrad(d, c, P);
    FlatWG F[3] = {};
    const int nflat = fill_flat(d, c, nullptr, F);
    size_t n = wgrad_plan(P, F, nflat, true, true).total;
    if (c.wgrad == WG_FIRST) {
        const size_t nf = first_wgrad_workspace_floats(d->B, c.Ctot, d->H, d->W);
        if (nf > n) n = nf;
    }
    return n * sizeof(float) + 16;
}

int dvsof_conv2d_wgrad(const dvsof_conv_desc_t *d, const float *gout, float *dweight, float *dbias,
                       void *ws, size_t ws_bytes, void *stream)
{
    conv_begin(2);
    const ConvClass c = conv_classify(d);
    if (!c.ok || !gout || !dweight) return DVSOF_EINVAL;
    hipStream_t st = as_stream(stream);
    // DVSOF_CONV_WGRAD_SKIP_FLAT: the flat members' columns are the caller's
    // (dvsof_flow_fold_grads); the vector members' columns are written as usual
    const bool skip_flat = (d->flags & DVSOF_CONV_WGRAD_SKIP_FLAT) != 0;
    switch (c.wgrad) {
    case WG_TRANSPOSED: {
        if (dbias && d->Cout > 256) return DVSOF_EINVAL;
        const dvsof_conv_desc_t a = adjoint_of_transposed(d, c.Ctot, gout);
        size_t wsa = dvsof_conv2d_wgrad_workspace_bytes(&a);
        wsa = (wsa + 255) & ~(size_t)255;
        const size_t need = dvsof_conv2d_wgrad_workspace_bytes(d);
        if (!ws || ws_bytes < need) return DVSOF_ENOSPACE;
        float *dw_adj = (float *)((char *)ws + wsa);
        float *part = dw_adj + (size_t)c.Ctot * 9 * d->Cout;
        int rc = dvsof_conv2d_wgrad(&a, d->src[0].p, dw_adj, nullptr, ws, wsa, stream);
        if (rc) return rc;
        // [Ctot][tap][Cout] -> [Cout][8 - tap][Ctot]
        rc = dvsof_weight_flip_transpose(dw_adj, dweight, c.Ctot, 3, d->Cout, stream);
        if (rc) return rc;
        if (dbias) {
            const long long npix = (long long)d->B * c.Ho * c.Wo;
            const int nb = channel_sum_blocks(npix, d->Cout);
            hipLaunchKernelGGL(channel_sum_partial_kernel, dim3(nb), dim3(256), 0, st, gout, npix, d->Cout, part);
            DVSOF_LAUNCH_CHECK();
            hipLaunchKernelGGL(channel_sum_final_kernel, dim3((d->Cout + 3) / 4), dim3(256), 0, st,
                               (const float *)part, nb, d->Cout, dbias);
            DVSOF_LAUNCH_CHECK();
        }
        return DVSOF_OK;
    }
    case WG_WINO: {
        // the forward's transformed input, when the caller kept it and both use the same form
        const float *v_in = c.wino_tile[0] == c.wino_tile[2] ? d->winograd_input : nullptr;
        // ... and the gradient form of gout, when the data gradient that produced gout made it
        const float *z_in = c.wino_tile[2] == 4 ? d->winograd_gout : nullptr;
        return wino_wgrad_launch(make_src(d->src[0].p, d->src[0].C, d->src[0].layout, d->H, d->W), v_in, z_in,
                                 gout, dweight, dbias, d->B, d->H, d->W, c.Ctot, d->Cout, c.wino_mode, (float *)ws,
                                 ws_bytes / sizeof(float), st);
    }
    case WG_FIRST:
        if (!skip_flat)
            return first_wgrad_launch(d->src[0].p, d->B, c.Ctot, d->H, d->W, gout, dweight, dbias, (float *)ws,
                                      ws_bytes / sizeof(float), st);
        break;
    default: break;
    }
    WGradParams P = {};     // (unused member slots are zeros, not stack residue: _audit.audit_exchange reads these words)
    fill_wgrad(d, c, P);
    P.gout = gout;
    FlatWG F[3] = {};
    const int nflat = skip_flat ? 0 : fill_flat(d, c, gout, F);
    // (a workspace that is missing or too small for this call's plan: DVSOF_ENOSPACE)
    return wgrad_launch(P, dweight, dbias, (float *)ws, ws_bytes / sizeof(float), F, nflat, st);
}

// elements of the prepared forward / data-gradient form (conv_weights.hip makes them)
size_t dvsof_conv2d_fwd_weight_elems(const dvsof_conv_desc_t *d)
{
    const ConvClass c = conv_classify(d);
    if (!c.ok) return 0;
    const bool phases = c.fwd == FWD_MIN9 || c.fwd == FWD_SUBPIXEL || c.fwd == FWD_TRANSPOSED;
    return (size_t)d->Cout * c.Ctot * (c.fwd == FWD_WINO ? wino_components(d->B, d->H, d->W, c.wino_mode)
                                       : phases ? 16 : d->ksize * d->ksize);
}

size_t dvsof_conv2d_dgrad_weight_elems(const dvsof_conv_desc_t *d)
{
    const ConvClass c = conv_classify(d);
    if (!c.ok) return 0;
    const bool taps16 = c.dgrad == DG_MIN9 || c.dgrad == DG_SUBPIXEL || c.dgrad == DG_PHASED2;
    return (size_t)d->Cout * c.Ctot * (c.dgrad == DG_WINO ? wino_components(d->B, d->H, d->W, c.wino_mode)
                                       : taps16 ? 16 : d->ksize * d->ksize);
}

// 0: direct implicit GEMM; 2 | 4: Winograd F(2x2,3x3) | F(4x4,3x3) (kind 0 fwd, 1 dgrad, 2 wgrad)
int dvsof_conv2d_winograd_tile(const dvsof_conv_desc_t *d, int kind)
{
    const ConvClass c = conv_classify(d);
    return c.ok ? c.wino_tile[kind == 2 ? 2 : 0] : 0;
}

// 1: this layer's forward (kind 0) / data gradient (kind 1) is a Winograd evaluation whose output
// transform can also write the consumer's forms (winograd_next / winograd_next_gout)
int dvsof_conv2d_winograd_chain(const dvsof_conv_desc_t *d, int kind)
{
    const ConvClass c = conv_classify(d);
    return c.ok && (kind == 0 || kind == 1) && c.wino_chain[kind] ? 1 : 0;
}

// 2 when the LDS-DMA (v2) kernel serves this problem's vector members, else 1;
// 3: the first-layer kernels (first.hip); 0: flat members only on the VALU kernel
// (a property of the shape: a forward's residual is not known here)
// kind 2 keeps a formula of its own, not the weight gradient's plan (wgrad_plan): the recorded
// answers speak of the full-resolution frame of a sub-pixel layer (16 | 2 W, where the plan runs
// v2 on its phases when 16 | W), answer 0 for every flat-only layer whether or not its members
// take the flat kernels, and ignore what a call's pointers decide (patch-resident kernels)
int dvsof_conv2d_kernel_generation(const dvsof_conv_desc_t *d, int kind)
{
    const ConvClass c = conv_classify(d);
    if (!c.ok) return DVSOF_EINVAL;
    if (kind != 1 && c.fwd == FWD_FIRST) return 3;
    if (kind == 2) {
        for (int i = 0; i < d->nsrc; ++i) {
            const GSrc g = make_src(d->src[i].p, d->src[i].C, d->src[i].layout, d->H, d->W);
            if (!g.flat) return (c.Wo % BK == 0 && (!d->upsample || c.wgrad == WG_SUBPIXEL)) ? 2 : 1;
        }
        return 0;   // flat members only: VALU kernel
    }
    if (kind == 1) return (d->Cout % BK == 0) ? 2 : 1;
    for (int i = 0; i < d->nsrc; ++i) {
        const GSrc g = make_src(d->src[i].p, d->src[i].C, d->src[i].layout, d->H, d->W);
        if (!g.flat) return (g.C % BK == 0) ? 2 : 1;
    }
    return 1;
}

int dvsof_conv2d_last_kernel(int kind)
{
    return (kind >= 0 && kind <= 2) ? t_last_kernel[kind] : 0;
}

int dvsof_conv2d_last_patch(int kind)
{
    switch (dvsof_conv2d_last_kernel(kind) & 255) {
    case DVSOF_KERNEL_FWD_MIN4:
    case DVSOF_KERNEL_FWD_MIN8:
    case DVSOF_KERNEL_DGRAD_MIN0:
    case DVSOF_KERNEL_DGRAD_MIN1:
    case DVSOF_KERNEL_DGRAD_MIN2:
    case DVSOF_KERNEL_WGRAD_MIN: return 2;
    case DVSOF_KERNEL_FWD_PATCH:
    case DVSOF_KERNEL_WGRAD_PATCH: return 1;
    default: return 0;
    }
}

int dvsof_conv2d_tile_id(const dvsof_conv_desc_t *d, int kind)
{
    const ConvClass c = conv_classify(d);
    if (!c.ok) return DVSOF_EINVAL;
    if (kind == 0) return gconv_pick_tile((long long)d->B * c.Ho * c.Wo, d->Cout);
    if (kind == 1) {
        const int up = (c.dgrad == DG_QUAD || c.dgrad == DG_TRANSPOSED) ? 2 : 1;    // rows on the up-sampled grid
        int n = c.Ctot, trail = 0;   // narrow planar members are peeled off (gconv.hip)
        for (int i = d->nsrc - 1; i > 0; --i) {
            const GSrc g = make_src(d->src[i].p, d->src[i].C, d->src[i].layout, d->H, d->W);
            if (!g.flat || trail + g.C > 4) break;
            trail += g.C;
        }
        if (up == 1 && c.dgrad != DG_PHASED2 && n - trail >= 32) n -= trail;
        return gconv_pick_tile((long long)d->B * d->H * up * d->W * up, n);  // phases included
    }
    if (kind == 2) {
        WGradParams P = {};     // (unused member slots are zeros, not stack residue: _audit.audit_exchange reads these words)
        fill_wgrad(d, c, P);
        return wgrad_plan(P, nullptr, 0, false, true).tile;
    }
    return DVSOF_EINVAL;
}

}  // extern "C"
