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
// general (wgrad_launch picks the kernel), as four phases for a sub-pixel layer.
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

// wgrad.hip / wgrad2.hip: the general weight gradient
int wgrad_launch(WGradParams P, float *dW, float *dbias, float *ws, size_t ws_floats,
                 const FlatWG *flat, int nflat, hipStream_t st);
size_t wgrad_flat_workspace_floats(const FlatWG *flat, int nflat);
size_t wgrad_workspace_floats(const WGradParams &P, bool with_bias);
int wgrad_splits(const WGradParams &P0, int *tile_out);
bool wgrad2_eligible(const WGradParams &P);
int wgrad2_launch(const WGradParams &P, int tile, int ntiles, hipStream_t st);
// wgrad_patch.hip: the decoder stages, input patch resident in LDS
bool wgrad_patch_shape_ok(const WGradParams &P);
bool wgrad_patch_eligible(const WGradParams &P);
int wgrad_patch_splits(const WGradParams &P);
int wgrad_patch_launch(const WGradParams &P, hipStream_t st);
// wgrad_min.hip: the nine-product form of the same gradient (exact f32)
bool wgrad_min_ok(const WGradParams &P);
int wgrad_min_splits(const WGradParams &P);
int wgrad_min_launch(WGradParams &P, hipStream_t st);

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
