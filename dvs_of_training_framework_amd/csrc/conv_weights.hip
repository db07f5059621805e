// Weight forms of the convolution stack: the kernels that turn a layer's raw weights
// w[Cout][k][k][Ctot] into the form each pass reads, their bf16 twins, and the entry points
// that make them.  Which form a layer takes is conv_classify's decision (conv_api.hip); the
// Winograd and nine-product forms are made by winograd.hip, fwd_min.hip and dgrad_min.hip.
#include "conv_host.h"

namespace {

// Wf[ph][co][a][b][ci] = sum_{ky in S(py,a)} sum_{kx in S(px,b)} W[co][ky][kx][ci]
// S(0,0)={0} S(0,1)={1,2} S(1,0)={0,1} S(1,1)={2}; ph = 2*py + px.
// (every weight-form kernel below takes an optional bf16 destination: the twin
// of the form it writes, for compute_dtype 'bf16s' -- a separate conversion
// launch per form was 23 launches and 165 us of a 1.94 ms step at batch 8)
__global__ __launch_bounds__(256) void subpixel_fwd_weights_kernel(const float *__restrict__ w,
                                                                   float *__restrict__ wf, int Cout,
                                                                   int Ctot,
                                                                   unsigned short *__restrict__ wf16)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Cout * Ctot) return;
    const int ci = (int)(i % Ctot), co = (int)(i / Ctot);
    float k[3][3];
#pragma unroll
    for (int t = 0; t < 9; ++t) k[t / 3][t % 3] = w[((size_t)co * 9 + t) * Ctot + ci];
    // row/column partial sums for (p, a): {0},{1,2},{0,1},{2}
    float r[4][3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        r[0][x] = k[0][x];
        r[1][x] = k[1][x] + k[2][x];
        r[2][x] = k[0][x] + k[1][x];
        r[3][x] = k[2][x];
    }
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int px = 0; px < 2; ++px)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const float *rr = r[2 * py + a];
                    const int q = 2 * px + b;
                    const float v = q == 0 ? rr[0] : q == 1 ? rr[1] + rr[2] : q == 2 ? rr[0] + rr[1] : rr[2];
                    const size_t o = ((((size_t)(2 * py + px) * Cout + co) * 2 + a) * 2 + b) * Ctot + ci;
                    wf[o] = v;
                    if (wf16) wf16[o] = bf16_bits(v);
                }
}

// Wd[ci][ty][tx][co] = Wf[ph][co][a][b][ci], ty -> (py,a): 0->(1,1) 1->(0,1) 2->(1,0) 3->(0,0)
__global__ __launch_bounds__(256) void subpixel_dgrad_weights_kernel(const float *__restrict__ wf,
                                                                     float *__restrict__ wd,
                                                                     int Cout, int Ctot,
                                                                     unsigned short *__restrict__ wd16)
{
    __shared__ float tile[32][33];
    const int z = blockIdx.z, ty = z >> 2, tx = z & 3;
    const int py = (ty == 0 || ty == 2) ? 1 : 0, a = ty < 2 ? 1 : 0;
    const int px = (tx == 0 || tx == 2) ? 1 : 0, b = tx < 2 ? 1 : 0;
    const float *in = wf + ((size_t)(2 * py + px) * Cout * 4 + (a * 2 + b)) * Ctot;
    const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (int r = ly; r < 32; r += 8) {
        const int co = co0 + r, ci = ci0 + lx;
        tile[r][lx] = (co < Cout && ci < Ctot) ? in[(size_t)co * 4 * Ctot + ci] : 0.f;
    }
    __syncthreads();
    for (int r = ly; r < 32; r += 8) {
        const int ci = ci0 + r, co = co0 + lx;
        if (ci < Ctot && co < Cout) {
            const size_t o = ((size_t)ci * 16 + z) * Cout + co;
            wd[o] = tile[lx][r];
            if (wd16) wd16[o] = bf16_bits(tile[lx][r]);
        }
    }
}

// The same Wd straight from the RAW weights w[co][3][3][ci] (a caller that no longer holds
// the phase kernels, or whose forward form is another one: fwd_min.hip): per axis tap t of
// the 4x4 kernel sums the raw taps {2}, {1,2}, {0,1}, {0} -- the same additions in the same
// order as subpixel_fwd_weights_kernel, so both routes give the same bits.
__global__ __launch_bounds__(256) void subpixel_dgrad_weights_raw_kernel(const float *__restrict__ w,
                                                                         float *__restrict__ wd,
                                                                         int Cout, int Ctot,
                                                                         unsigned short *__restrict__ wd16)
{
    __shared__ float tile[32][33];
    const int z = blockIdx.z, ty = z >> 2, tx = z & 3;
    const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (int r = ly; r < 32; r += 8) {
        const int co = co0 + r, ci = ci0 + lx;
        float v = 0.f;
        if (co < Cout && ci < Ctot) {
            const float *k = w + (size_t)co * 9 * Ctot + ci;
            // (rows are summed FIRST in subpixel_fwd_weights_kernel, then columns)
            auto col = [&](int kx) -> float {
                const float *kc = k + (size_t)kx * Ctot;
                return ty == 0 ? kc[6 * Ctot] : ty == 1 ? kc[3 * Ctot] + kc[6 * Ctot]
                     : ty == 2 ? kc[0] + kc[3 * Ctot] : kc[0];
            };
            v = tx == 0 ? col(2) : tx == 1 ? col(1) + col(2) : tx == 2 ? col(0) + col(1) : col(0);
        }
        tile[r][lx] = v;
    }
    __syncthreads();
    for (int r = ly; r < 32; r += 8) {
        const int ci = ci0 + r, co = co0 + lx;
        if (ci < Ctot && co < Cout) {
            const size_t o = ((size_t)ci * 16 + z) * Cout + co;
            wd[o] = tile[lx][r];
            if (wd16) wd16[o] = bf16_bits(tile[lx][r]);
        }
    }
}

// Stride-2 3x3/pad-1 data gradient as four input-parity phases of 2x2 taps:
// Wp[ph][ci][a][b][co] = W[co][ky(py,a)][kx(px,b)][ci], ky(0,0)=1, ky(0,1)=none,
// ky(1,0)=2, ky(1,1)=0 (unused taps are zero).  ph = 2*py + px.
// w16: bf16 twin of the RAW weights (each raw tap is read by exactly one z)
__global__ __launch_bounds__(256) void stride2_dgrad_weights_kernel(const float *__restrict__ w,
                                                                    float *__restrict__ wp,
                                                                    int Cout, int Ctot,
                                                                    unsigned short *__restrict__ wp16,
                                                                    unsigned short *__restrict__ w16)
{
    __shared__ float tile[32][33];
    const int z = blockIdx.z;            // ph*4 + a*2 + b
    const int ph = z >> 2, a = (z >> 1) & 1, b = z & 1, py = ph >> 1, px = ph & 1;
    const int ky = py ? (a ? 0 : 2) : (a ? -1 : 1), kx = px ? (b ? 0 : 2) : (b ? -1 : 1);
    const bool used = ky >= 0 && kx >= 0;
    const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    for (int r = ly; r < 32; r += 8) {
        const int co = co0 + r, ci = ci0 + lx;
        float v = 0.f;
        if (used && co < Cout && ci < Ctot) {
            const size_t o = ((size_t)co * 9 + ky * 3 + kx) * Ctot + ci;
            v = w[o];
            if (w16) w16[o] = bf16_bits(v);
        }
        tile[r][lx] = v;
    }
    __syncthreads();
    for (int r = ly; r < 32; r += 8) {
        const int ci = ci0 + r, co = co0 + lx;
        if (ci < Ctot && co < Cout) {
            const size_t o = (((size_t)ph * Ctot + ci) * 4 + a * 2 + b) * Cout + co;
            wp[o] = tile[lx][r];
            if (wp16) wp16[o] = bf16_bits(tile[lx][r]);
        }
    }
}

// Transposed-convolution forward as four output-parity phases of 2x2 taps:
// Wt[ph][co][a][b][ci] = W[co][ky(py,a)][kx(px,b)][ci], ky(0,0)=1, ky(0,1)=none,
// ky(1,0)=0, ky(1,1)=2 (unused taps are zero).  ph = 2*py + px.
__global__ __launch_bounds__(256) void transposed_fwd_weights_kernel(const float *__restrict__ w,
                                                                     float *__restrict__ wt,
                                                                     int Cout, int Ctot,
                                                                     unsigned short *__restrict__ wt16)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Cout * Ctot) return;
    const int ci = (int)(i % Ctot), co = (int)(i / Ctot);
#pragma unroll
    for (int z = 0; z < 16; ++z) {
        const int ph = z >> 2, a = (z >> 1) & 1, b = z & 1, py = ph >> 1, px = ph & 1;
        const int ky = py ? (a ? 2 : 0) : (a ? -1 : 1), kx = px ? (b ? 2 : 0) : (b ? -1 : 1);
        const float v = (ky >= 0 && kx >= 0) ? w[((size_t)co * 9 + ky * 3 + kx) * Ctot + ci] : 0.f;
        const size_t o = ((((size_t)ph * Cout + co) * 2 + a) * 2 + b) * Ctot + ci;
        wt[o] = v;
        if (wt16) wt16[o] = bf16_bits(v);
    }
}

__global__ __launch_bounds__(256) void flip_transpose_kernel(const float *__restrict__ w,
                                                             float *__restrict__ wt, int Cout,
                                                             int taps, int Ctot,
                                                             unsigned short *__restrict__ wt16,
                                                             unsigned short *__restrict__ w16)
{
    __shared__ float tile[32][33];
    const int tap = blockIdx.z;
    const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int co = co0 + r, ci = ci0 + tx;
        float v = 0.f;
        if (co < Cout && ci < Ctot) {
            const size_t o = ((size_t)co * taps + tap) * Ctot + ci;
            v = w[o];
            if (w16) w16[o] = bf16_bits(v);
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int ci = ci0 + r, co = co0 + tx;
        if (ci < Ctot && co < Cout) {
            const size_t o = ((size_t)ci * taps + (taps - 1 - tap)) * Cout + co;
            wt[o] = tile[tx][r];
            if (wt16) wt16[o] = bf16_bits(tile[tx][r]);
        }
    }
}

// bf16 twins of prepared weights: 8 elements per thread and iteration
__global__ __launch_bounds__(256) void to_bf16_kernel(const float *__restrict__ src,
                                                      unsigned short *__restrict__ dst, size_t n)
{
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8), aligned(4)));
    const size_t stride = (size_t)gridDim.x * 256 * 8;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += stride) {
        if (i + 7 < n) {
            const f32x4 a = *(const f32x4u *)(src + i), b = *(const f32x4u *)(src + i + 4);
            const u16x8 h = {bf16_bits(a[0]), bf16_bits(a[1]), bf16_bits(a[2]), bf16_bits(a[3]),
                             bf16_bits(b[0]), bf16_bits(b[1]), bf16_bits(b[2]), bf16_bits(b[3])};
            *(u16x8 *)(dst + i) = h;
        } else {
            for (size_t j = i; j < n; ++j) dst[j] = bf16_bits(src[j]);
        }
    }
}

// several tensors in one launch (the raw-weight twins of a step): a workgroup
// converts 2048 elements of the tensor its index falls into
constexpr int BF16_MANY_MAX = 16;
struct Bf16Many {
    const float *src[BF16_MANY_MAX];
    unsigned short *dst[BF16_MANY_MAX];
    size_t n[BF16_MANY_MAX];
    unsigned block_begin[BF16_MANY_MAX + 1];
    int count;
};
__global__ __launch_bounds__(256) void to_bf16_many_kernel(const Bf16Many J)
{
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8), aligned(4)));
    int t = 0;
#pragma unroll
    for (int i = 1; i < BF16_MANY_MAX; ++i)
        if (i < J.count && blockIdx.x >= J.block_begin[i]) t = i;
    const float *src = J.src[t];
    unsigned short *dst = J.dst[t];
    const size_t n = J.n[t];
    const size_t i = ((size_t)(blockIdx.x - J.block_begin[t]) * 256 + threadIdx.x) * 8;
    if (i + 7 < n) {
        const f32x4 a = *(const f32x4u *)(src + i), b = *(const f32x4u *)(src + i + 4);
        const u16x8 h = {bf16_bits(a[0]), bf16_bits(a[1]), bf16_bits(a[2]), bf16_bits(a[3]),
                         bf16_bits(b[0]), bf16_bits(b[1]), bf16_bits(b[2]), bf16_bits(b[3])};
        *(u16x8 *)(dst + i) = h;
    } else {
        for (size_t j = i; j < n; ++j) dst[j] = bf16_bits(src[j]);
    }
}

}  // namespace

extern "C" {

static int flip_transpose16(const float *w, float *wt, int Cout, int ksize, int Ctot,
                            unsigned short *wt16, unsigned short *w16, void *stream)
{
    if (!w || !wt || Cout < 1 || ksize < 1 || Ctot < 1) return DVSOF_EINVAL;
    const int taps = ksize * ksize;
    dim3 grid((Ctot + 31) / 32, (Cout + 31) / 32, taps);
    hipLaunchKernelGGL(flip_transpose_kernel, grid, dim3(256), 0, as_stream(stream), w, wt, Cout,
                       taps, Ctot, wt16, w16);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_weight_flip_transpose(const float *w, float *wt, int Cout, int ksize, int Ctot,
                                void *stream)
{
    return flip_transpose16(w, wt, Cout, ksize, Ctot, nullptr, nullptr, stream);
}

int dvsof_to_bf16(const float *src, void *dst, size_t n, void *stream)
{
    if (n == 0) return DVSOF_OK;      // an empty tensor may have NULL storage
    if (!src || !dst) return DVSOF_EINVAL;
    size_t nb = (n + 2047) / 2048;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(to_bf16_kernel, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), src,
                       (unsigned short *)dst, n);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_to_bf16_many(const float *const *src, void *const *dst, const size_t *n, int count,
                       void *stream)
{
    if (count < 0 || count > BF16_MANY_MAX || (count && (!src || !dst || !n))) return DVSOF_EINVAL;
    if (count == 0) return DVSOF_OK;
    Bf16Many J = {};
    size_t blocks = 0;
    for (int i = 0; i < count; ++i) {
        if (n[i] && (!src[i] || !dst[i])) return DVSOF_EINVAL;
        J.src[i] = src[i];
        J.dst[i] = (unsigned short *)dst[i];
        J.n[i] = n[i];
        J.block_begin[i] = (unsigned)blocks;
        blocks += (n[i] + 2047) / 2048;
    }
    J.count = count;
    J.block_begin[count] = (unsigned)blocks;
    if (blocks == 0) return DVSOF_OK;
    if (blocks > 0x7fffffffu) return DVSOF_EINVAL;
    hipLaunchKernelGGL(to_bf16_many_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), J);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

// The prepared forms of a layer's weights (include/dvsof.h: dvsof_conv2d_prepare), one per form
// conv_classify gives the forward and the data gradient.
// w_fwd16 / w_dgrad16 (optional): bf16 twins of the two forms, written by the kernels that
// make the forms.  For a layer whose forward form is the raw weight, w_fwd16 is the raw
// weight's twin (emitted by the data-gradient form kernel, which reads every raw element
// once; a conversion launch if no data-gradient form is asked for).
int dvsof_conv2d_prepare16(const dvsof_conv_desc_t *d, const float *weight, float *w_fwd,
                           float *w_dgrad, void *w_fwd16_, void *w_dgrad16_, void *stream)
{
    const ConvClass c = conv_classify(d);
    if (!c.ok) return DVSOF_EINVAL;
    hipStream_t st = as_stream(stream);
    unsigned short *w_fwd16 = (unsigned short *)w_fwd16_, *w_dgrad16 = (unsigned short *)w_dgrad16_;
    const int Cout = d->Cout, Ctot = c.Ctot;

    // ---- argument rules (include/dvsof.h); a call that breaks one returns DVSOF_EINVAL and
    // launches nothing.  Every form: a data-gradient twin goes with its form
    const bool some = w_fwd || w_dgrad;
    bool bad = w_dgrad16 && !w_dgrad;
    switch (c.fwd) {
    case FWD_MIN9:          // from the raw weights, at least one form; exact f32 only: no twins
        bad |= !weight || !some || (w_fwd && w_fwd16) || (c.dgrad == DG_MIN9 && w_dgrad16);
        break;
    case FWD_SUBPIXEL:      // from the raw weights, at least one form; or (weight == NULL) w_dgrad
        bad |= weight ? !some : (!w_fwd || !w_dgrad);   // from the phase kernels an earlier call left in w_fwd
        break;
    case FWD_TRANSPOSED:    // from the raw weights, at least one form, never in place
        bad |= !weight || !some || w_fwd == weight;
        break;
    case FWD_WINO:          // from the raw weights, at least one form; no twins (mode 3 runs these layers direct)
        bad |= !weight || !some || w_fwd16 || w_dgrad16;
        break;
    default:                // the forward form is the raw weight (or a copy of it); every output is optional
        bad |= !weight;
    }
    if (bad) return DVSOF_EINVAL;

    const unsigned ew_blocks = (unsigned)(((size_t)Cout * Ctot + 255) / 256);   // one thread per (co, ci)
    const dim3 tr_grid((Ctot + 31) / 32, (Cout + 31) / 32, 16);                  // 32 x 32 transposes of 16 taps
    const bool raw_fwd = c.fwd == FWD_FIRST || c.fwd == FWD_GENERAL;
    unsigned short *raw16 = raw_fwd ? w_fwd16 : nullptr;    // twin of the raw weight

    // ---- the forward form
    int rc = DVSOF_OK;
    switch (c.fwd) {
    case FWD_WINO:      // either form (or both) in one call
        return wino_prepare(weight, w_fwd, w_dgrad, Cout, Ctot, d->B, d->H, d->W, c.wino_mode, st);
    case FWD_MIN9:
        if (w_fwd) rc = min9_prepare_fwd(weight, w_fwd, Cout, Ctot, st);
        break;
    case FWD_SUBPIXEL:
        if (weight && w_fwd) {
            hipLaunchKernelGGL(subpixel_fwd_weights_kernel, dim3(ew_blocks), dim3(256), 0, st, weight, w_fwd,
                               Cout, Ctot, w_fwd16);
            DVSOF_LAUNCH_CHECK();
        } else if (!weight && w_fwd16) {
            rc = dvsof_to_bf16(w_fwd, w_fwd16, dvsof_conv2d_fwd_weight_elems(d), stream);
        }
        break;
    case FWD_TRANSPOSED:
        if (w_fwd) {
            hipLaunchKernelGGL(transposed_fwd_weights_kernel, dim3(ew_blocks), dim3(256), 0, st, weight, w_fwd,
                               Cout, Ctot, w_fwd16);
            DVSOF_LAUNCH_CHECK();
        }
        break;
    default:
        if (w_fwd && w_fwd != weight)
            DVSOF_HIP_TRY(hipMemcpyAsync(w_fwd, weight, dvsof_conv2d_fwd_weight_elems(d) * sizeof(float),
                                         hipMemcpyDeviceToDevice, st));
    }
    if (rc) return rc;

    // ---- the data-gradient form
    if (!w_dgrad) return raw16 ? dvsof_to_bf16(weight, raw16, dvsof_conv2d_fwd_weight_elems(d), stream) : DVSOF_OK;
    switch (c.dgrad) {
    case DG_MIN9:
        return min9_prepare_dgrad(weight, w_dgrad, Cout, Ctot, st);
    case DG_SUBPIXEL:
        // from the phase kernels where w_fwd holds them, else from the raw weights (same bits)
        if (c.fwd == FWD_SUBPIXEL && w_fwd)
            hipLaunchKernelGGL(subpixel_dgrad_weights_kernel, tr_grid, dim3(256), 0, st, (const float *)w_fwd,
                               w_dgrad, Cout, Ctot, w_dgrad16);
        else
            hipLaunchKernelGGL(subpixel_dgrad_weights_raw_kernel, tr_grid, dim3(256), 0, st, weight, w_dgrad,
                               Cout, Ctot, w_dgrad16);
        break;
    case DG_PHASED2:
        hipLaunchKernelGGL(stride2_dgrad_weights_kernel, tr_grid, dim3(256), 0, st, weight, w_dgrad, Cout,
                           Ctot, w_dgrad16, raw16);
        break;
    default:    // DG_PLAIN, DG_ZERO2, DG_QUAD, DG_TRANSPOSED (DG_WINO returned above)
        return flip_transpose16(weight, w_dgrad, Cout, d->ksize, Ctot, w_dgrad16, raw16, stream);
    }
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_conv2d_prepare(const dvsof_conv_desc_t *d, const float *weight, float *w_fwd,
                         float *w_dgrad, void *stream)
{
    return dvsof_conv2d_prepare16(d, weight, w_fwd, w_dgrad, nullptr, nullptr, stream);
}

}  // extern "C"
