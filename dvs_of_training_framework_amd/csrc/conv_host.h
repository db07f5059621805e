// Host side of the convolution stack: what a layer's three passes run as (conv_classify) and
// every launcher, shape test and size query that one file of the stack calls in another.  A
// prototype lives here and nowhere else: the library is linked with --no-undefined, so one
// that drifts from its definition fails the build, not the load.
#pragma once
#include "conv_common.h"

// ---- the form of a layer, decided once per entry point --------------------------------------
// Forward.  Precedence: first layer > Winograd > nine-product > sub-pixel phases / transposed
// > general.  (FWD_SUBPIXEL runs fwd_patch.hip where the call's pointers allow it:
// fwd_patch_eligible; FWD_FIRST falls to the general kernel when the call has a residual.)
enum ConvFwdForm { FWD_GENERAL, FWD_FIRST, FWD_WINO, FWD_MIN9, FWD_SUBPIXEL, FWD_TRANSPOSED };
// Data gradient.  Precedence: nine-product > Winograd > the general kernels, in the geometry of
// the layer: 4x4 stride-2 (sub-pixel layers), four input-parity phases (3x3 stride 2 on an
// even frame), plain stride 2 (transposed layers), quad-summed rows (other nearest-up
// layers), zero-inserted gout (other stride-2 layers), plain.
enum ConvDgradForm { DG_PLAIN, DG_MIN9, DG_WINO, DG_SUBPIXEL, DG_PHASED2, DG_TRANSPOSED, DG_QUAD, DG_ZERO2 };
// Weight gradient.  Precedence: transposed (through its adjoint) > Winograd > first layer >
// general, as four phases for a sub-pixel layer.  What the general form launches is a WGradPlan
// (below): wgrad_plan decides it once, wgrad_launch and the size queries read it.
enum ConvWgradForm { WG_GENERAL, WG_TRANSPOSED, WG_WINO, WG_FIRST, WG_SUBPIXEL };

struct ConvClass {
    bool ok;            // the descriptor is valid; nothing else is set when it is not
    int Ctot, Ho, Wo;   // channels of the concatenation, output frame
    ConvFwdForm fwd;
    ConvDgradForm dgrad;
    ConvWgradForm wgrad;
    int wino_mode;      // operand mode of the Winograd kernels: 2 (bf16x3) or 0 (exact f32)
    int wino_tile[3];   // Winograd output tile of forward / data / weight gradient: 0 | 2 | 4
    bool wino_chain[2]; // the forward's / data gradient's output transform can write its consumer's forms
    bool head_folds;    // a flow head on member 0 folds into the data gradient's epilogue
};
// conv_api.hip: a pure function of the descriptor's shape fields and bias_cls
ConvClass conv_classify(const dvsof_conv_desc_t *d);

// conv_api.hip: the calling thread's record of what its current dvsof_conv2d_fwd / _dgrad /
// _wgrad launched (dvsof_conv2d_last_kernel): a launcher notes its DVSOF_KERNEL_* family and
// the operand mode it ran in, after every fallback, once its kernel is enqueued
void conv_note_kernel(int family, int mode);

// gconv.hip / gconv2.hip: the general forward / data-gradient kernels
int gconv_launch(const GConvParams &P, int tile_hint, hipStream_t st);
int gconv_pick_tile(long long m, long long n);
bool gconv2_eligible(const GConvParams &P, long long max_src_bytes, long long w_bytes);
int gconv2_launch(const GConvParams &P, int tile, hipStream_t st);

// ---- the general weight gradient: one plan per launch (wgrad_plan.hip) -----------------------
enum WGVec { WGV_NONE, WGV_V1, WGV_V2, WGV_PATCH_TWINS, WGV_PATCH_F32, WGV_MIN9 };     // the vector members' kernel
enum WGFlat { WGF_NONE, WGF_V1, WGF_OWN };     // the flat members: on the v1 tiles / kernels of their own (VALU or matrix cores)
enum WGBias { WGB_NONE, WGB_VECTOR, WGB_COLSUM, WGB_FLAT };    // in the vector kernel (v2, patch, nine-product) /
                                                               // column-sum pass / extra column of flat member 0
enum WGReduce { WGR_NONE, WGR_SLABS, WGR_SUBPIXEL, WGR_PATCH };    // direct / slab sum / 2x2 phases -> 3x3 / 3x3 slabs
constexpr int WG_COLSUM_BLOCKS = 512;   // most partial sums of the column-sum pass
constexpr int WG_FLAT_BLOCKS = 512;     // ... and of a flat member's kernel
constexpr int WG_MIN_CT = 64;           // input channels per workgroup of the nine-product kernel
struct WGradPlan {
    int rc;             // DVSOF_EINVAL: a vector member the kernels cannot read (the layout below is set all the same)
    WGVec vec;
    int tile, bn;       // v1 / v2: tile id (1..5) and its column width; the patch kernels: bn = their channel tile
    int ntiles;         // column tiles of the vector members
    int S, klen;        // K splits, pixels per split (multiple of BK)
    WGFlat flat;
    bool flat_mfma[3];  // WGF_OWN: flat member i takes the matrix-core kernel, else the VALU kernel
    WGBias bias;
    bool bias_tail;     // the vector kernel's per-slab bias partials ride on the reduce
    WGReduce reduce;
    int zg;             // WGR_SUBPIXEL: threads that share an output quad
    // workspace, in floats: [slabs | bias or column-sum partials | flat member 0, 1, 2 partials]
    size_t bias_off, flat_off[3], total;
    int family, mode;   // what dvsof_conv2d_last_kernel reports
};
// Call mode (sizing = false) reads the call's pointers (twins bound, 16-byte alignment of gout and
// the sources) and plans the launch.  Sizing mode knows the shape only: vec / flat / bias / reduce
// stay unset, S is the largest any call of this shape can take, and total covers every such call.
WGradPlan wgrad_plan(const WGradParams &P, const FlatWG *flat, int nflat, bool with_bias, bool sizing);
// P.tile_begin = the column tiles, `width` columns each, of the chosen members (vector and / or
// flat), cols_per_channel columns per channel; returns their number
int wgrad_enumerate_tiles(WGradParams &P, int cols_per_channel, int width, bool vec, bool flat);
bool wgrad2_eligible(const WGradParams &P);      // what wgrad2_launch requires of its caller
// wgrad.hip: runs the plan
int wgrad_launch(WGradParams P, float *dW, float *dbias, float *ws, size_t ws_floats,
                 const FlatWG *flat, int nflat, hipStream_t st);
// wgrad2.hip (also winograd.hip's component GEMMs, with their own split rule)
int wgrad2_launch(const WGradParams &P, int tile, int ntiles, hipStream_t st);
// wgrad_patch.hip: the decoder stages, input patch resident in LDS (twins or exact f32);
// wgrad_min.hip: the nine-product form of the same gradient (exact f32)
int wgrad_patch_launch(const WGradParams &P, bool f32, int ct, hipStream_t st);
int wgrad_min_launch(const WGradParams &P, hipStream_t st);
// the launch both share: KERNEL over (channel tiles of CT, Cout / 32, K splits)
template <void (*KERNEL)(const WGradParams), int CT, int NT, int LDS>
int wgrad_resident_launch(const WGradParams &P0, hipStream_t st)
{
    WGradParams P = P0;
    const int nt = wgrad_enumerate_tiles(P, 1, CT, true, false);
    static bool attr_set = false;
    if (!attr_set) {
        DVSOF_HIP_TRY(hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
        attr_set = true;
    }
    P.xcd = 1;      // XCD-aware workgroup order
    hipLaunchKernelGGL(KERNEL, dim3(nt, P.Cout / 32, P.S), dim3(NT), LDS, st, P);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

// winograd.hip: wide 3x3 stride-1 layers as F(2x2,3x3) / F(4x4,3x3)
bool wino_eligible_shape(int nsrc, int layout_nhwc, int C, int N, int B, int H, int W, int ksize,
                         int stride, int pad, int upsample, int mfma);
int wino_tile(int B, int H, int W, int mfma);
int wino_components(int B, int H, int W, int mfma);
bool wino_chain_ok(int B, int H, int W, int N, int mfma);
size_t wino_scratch_floats(int B, int H, int W, int C, int N, int mfma);
int wino_prepare(const float *weight, float *U, float *Ut, int N, int C, int B, int H, int W, int mfma,
                 hipStream_t st);
int wino_launch(const GConvParams &P, float *scratch, size_t scratch_floats, const WinoChain &ch, hipStream_t st);
int wino_wgrad_tile(int B, int H, int W, int mfma);
size_t wino_wgrad_workspace_floats(int B, int H, int W, int C, int N, int mfma);
int wino_wgrad_launch(const GSrc &X, const float *V_in, const float *Z_in, const float *gout, float *dW, float *dbias, int B,
                      int H, int W, int C, int N, int mfma_bf16, float *ws, size_t ws_floats,
                      hipStream_t st);

// first.hip: the first encoder layer (planar voxel input, K = 9 C) as kernels of its own
bool first_layer_shape(int nsrc, int planar, int C, int Cout, int H, int W, int ksize, int stride,
                       int pad, int upsample);
int first_fwd_launch(const float *x, int B, int C, int H, int W, const float *w, const float *bias,
                     int act, float *y, float *z, unsigned short *y16, hipStream_t st);
size_t first_wgrad_workspace_floats(int B, int C, int H, int W);
int first_wgrad_launch(const float *x, int B, int C, int H, int W, const float *gout, float *dW,
                       float *dbias, float *ws, size_t ws_floats, hipStream_t st);

// fwd_patch.hip: forward of the finest decoder stage (patch in LDS, weights in registers)
bool fwd_patch_eligible(const GConvParams &P);
int fwd_patch_launch(const GConvParams &P, hipStream_t st);
// fwd_min.hip: the nine-product form of `nearest-up2 -> conv3x3` (exact f32; prepared
// forward form Wt[9][Cout][Ctot] = G w G^T)
bool min9_shape_ok(int mfma, int nsrc, const int *C, const int *nhwc, int Cout, int H, int W);
int min9_prepare_fwd(const float *w, float *wt, int Cout, int Ctot, hipStream_t st);
int fwd_min_launch(const GConvParams &P, hipStream_t st);
// dgrad_min.hip: its data gradient, nine products too (prepared form W'[9][Ctot][Cout])
bool min9_dgrad_shape_ok(const int *C, int Cout, int H);
int min9_prepare_dgrad(const float *w, float *wq, int Cout, int Ctot, hipStream_t st);
int dgrad_min_launch(const GConvParams &P, hipStream_t st);
