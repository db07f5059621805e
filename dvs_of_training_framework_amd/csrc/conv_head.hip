// The 1x1 flow head (forward of one head or of up to four in one launch; backward fused with
// the activation backward of the tensor it reads, weight / bias gradient from per-workgroup
// partials in a fixed order) and the elementwise activation backward, with their entry
// points (dvsof_flow_head_*, dvsof_flow_heads_fwd, dvsof_act_bwd).
#include "conv_common.h"

namespace {

// ---- flow head ------------------------------------------------------------
// LPP = C/4 lanes share one pixel (one float4 of channels each).

template <int LPP>
__device__ __forceinline__ void head_fwd_body(const float *__restrict__ x, const float *__restrict__ w,
                                              const float *__restrict__ bias, float *__restrict__ flow,
                                              int B, int HW, int vblock, int nblocks)
{
    constexpr int C = LPP * 4, PPW = 64 / LPP;
    const int lane = threadIdx.x & 63, sub = lane % LPP, pw = lane / LPP;
    const f32x4 w0 = *(const f32x4u *)(w + 4 * sub), w1 = *(const f32x4u *)(w + C + 4 * sub);
    const float b0 = bias ? bias[0] : 0.f, b1 = bias ? bias[1] : 0.f;
    const long long total = (long long)B * HW;
    const long long wave_id = (long long)vblock * 4 + (threadIdx.x >> 6);
    const long long nwaves = (long long)nblocks * 4;
    for (long long base = wave_id * PPW; base < total; base += nwaves * PPW) {
        const long long pix = base + pw;
        float p0 = 0.f, p1 = 0.f;
        if (pix < total) {
            const f32x4 v = *(const f32x4u *)(x + pix * C + 4 * sub);
            p0 = v[0] * w0[0] + v[1] * w0[1] + v[2] * w0[2] + v[3] * w0[3];
            p1 = v[0] * w1[0] + v[1] * w1[1] + v[2] * w1[2] + v[3] * w1[3];
        }
#pragma unroll
        for (int off = LPP / 2; off > 0; off >>= 1) {
            p0 += __shfl_xor(p0, off, 64);
            p1 += __shfl_xor(p1, off, 64);
        }
        if (sub == 0 && pix < total) {
            const long long b = pix / HW, r = pix - b * HW;
            flow[(b * 2) * HW + r] = p0 + b0;
            flow[(b * 2 + 1) * HW + r] = p1 + b1;
        }
    }
}

template <int LPP>
__global__ __launch_bounds__(256) void head_fwd_kernel(const float *__restrict__ x,
                                                       const float *__restrict__ w,
                                                       const float *__restrict__ bias,
                                                       float *__restrict__ flow, int B, int HW)
{
    head_fwd_body<LPP>(x, w, bias, flow, B, HW, blockIdx.x, gridDim.x);
}

// Up to 4 heads in ONE launch (the training forward with the flow member folded:
// nothing between the decoder stages reads a flow, so all of them are computed
// ahead of the loss; a launch of this size is mostly its ~4.5 us of dispatch)
constexpr int HEADS_MAX = 4;
struct HeadsFwd {
    const float *x[HEADS_MAX], *w[HEADS_MAX], *bias[HEADS_MAX];
    float *flow[HEADS_MAX];
    int HW[HEADS_MAX], C[HEADS_MAX], block_begin[HEADS_MAX + 1];
    int B, n;
};
__global__ __launch_bounds__(256) void heads_fwd_kernel(const HeadsFwd A)
{
    int h = 0;
#pragma unroll
    for (int i = 1; i < HEADS_MAX; ++i)
        if (i < A.n && (int)blockIdx.x >= A.block_begin[i]) h = i;
    const int vb = blockIdx.x - A.block_begin[h], nb = A.block_begin[h + 1] - A.block_begin[h];
    switch (A.C[h] / 4) {
    case 4: head_fwd_body<4>(A.x[h], A.w[h], A.bias[h], A.flow[h], A.B, A.HW[h], vb, nb); break;
    case 8: head_fwd_body<8>(A.x[h], A.w[h], A.bias[h], A.flow[h], A.B, A.HW[h], vb, nb); break;
    case 16: head_fwd_body<16>(A.x[h], A.w[h], A.bias[h], A.flow[h], A.B, A.HW[h], vb, nb); break;
    case 32: head_fwd_body<32>(A.x[h], A.w[h], A.bias[h], A.flow[h], A.B, A.HW[h], vb, nb); break;
    default: head_fwd_body<64>(A.x[h], A.w[h], A.bias[h], A.flow[h], A.B, A.HW[h], vb, nb); break;
    }
}

template <int LPP>
__global__ __launch_bounds__(256) void head_bwd_kernel(
    const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ gflow,
    const float *gx_in, const float *__restrict__ actsrc, int act, float *gx,
    float *__restrict__ part, int B, int HW, unsigned short *__restrict__ gx16)
{
    constexpr int C = LPP * 4, PPW = 64 / LPP;
    __shared__ float red[4][2 * C + 2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane % LPP, pw = lane / LPP;
    const f32x4 w0 = *(const f32x4u *)(w + 4 * sub), w1 = *(const f32x4u *)(w + C + 4 * sub);
    const long long total = (long long)B * HW;
    const long long wave_id = (long long)blockIdx.x * 4 + wave;
    const long long nwaves = (long long)gridDim.x * 4;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    float s0 = 0.f, s1 = 0.f;
    for (long long base = wave_id * PPW; base < total; base += nwaves * PPW) {
        const long long pix = base + pw;
        if (pix < total) {
            const long long b = pix / HW, r = pix - b * HW;
            const float g0 = gflow[(b * 2) * HW + r], g1 = gflow[(b * 2 + 1) * HW + r];
            const size_t o = (size_t)pix * C + 4 * sub;
            const f32x4 v = *(const f32x4u *)(x + o);
            a0 += g0 * v;
            a1 += g1 * v;
            if (sub == 0) {
                s0 += g0;
                s1 += g1;
            }
            if (!gx) continue;      // weight / bias gradient only (wave-uniform)
            f32x4 g = g0 * w0 + g1 * w1;
            if (gx_in) g += *(const f32x4u *)(gx_in + o);
            if (actsrc) {
                const f32x4 sv = *(const f32x4u *)(actsrc + o);
#pragma unroll
                for (int i = 0; i < 4; ++i) g[i] *= act_bwd(sv[i], act);
            }
            *(f32x4u *)(gx + o) = g;
            if (gx16) {     // bf16 twin for the data gradient that reads it next
                typedef unsigned short u16x4 __attribute__((ext_vector_type(4), aligned(2)));
                const u16x4 h = {bf16_bits(g[0]), bf16_bits(g[1]), bf16_bits(g[2]), bf16_bits(g[3])};
                *(u16x4 *)(gx16 + o) = h;
            }
        }
    }
    // lanes with equal `sub` hold partial sums of the same channels
#pragma unroll
    for (int off = LPP; off < 64; off <<= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a0[i] += __shfl_xor(a0[i], off, 64);
            a1[i] += __shfl_xor(a1[i], off, 64);
        }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (pw == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            red[wave][4 * sub + i] = a0[i];
            red[wave][C + 4 * sub + i] = a1[i];
        }
    }
    if (lane == 0) {
        red[wave][2 * C] = s0;
        red[wave][2 * C + 1] = s1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C + 2; i += 256)
        part[(size_t)blockIdx.x * (2 * C + 2) + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// dw[2*C], dbias[2] from the per-workgroup partials, fixed order: one wave
// per output column, lanes stride over the workgroups, shuffle tree.
__global__ __launch_bounds__(256) void head_bwd_reduce_kernel(const float *__restrict__ part,
                                                              int nblocks, int C, float *dw,
                                                              float *dbias)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= 2 * C + 2) return;
    double a = 0;
    for (int b = lane; b < nblocks; b += 64) a += (double)part[(size_t)b * (2 * C + 2) + i];
    a = wave_sum(a);
    if (lane == 0) {
        if (i < 2 * C) dw[i] = (float)a;
        else if (dbias) dbias[i - 2 * C] = (float)a;
    }
}

__global__ __launch_bounds__(256) void act_bwd_kernel(const float *dy,
                                                      const float *__restrict__ actsrc, int act,
                                                      float *dz, size_t n)
{
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 3 < n) {
            f32x4 g = *(const f32x4u *)(dy + i);
            const f32x4 s = *(const f32x4u *)(actsrc + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] *= act_bwd(s[j], act);
            *(f32x4u *)(dz + i) = g;
        } else {
            for (size_t j = i; j < n; ++j) dz[j] = dy[j] * act_bwd(actsrc[j], act);
        }
    }
}

// workgroups of the head backward = partial rows of its weight-gradient reduce
int head_blocks(long long total, int lpp)
{
    constexpr int cap = 512;
    const long long per_block = 4LL * (64 / lpp);
    long long nb = (total + per_block - 1) / per_block;
    return (int)(nb < cap ? (nb < 1 ? 1 : nb) : cap);
}

}  // namespace

extern "C" {

#define HEAD_DISPATCH(KERNEL, nb, ...)                                                         \
    switch (C / 4) {                                                                           \
    case 4: hipLaunchKernelGGL((KERNEL<4>), dim3(nb), dim3(256), 0, st, __VA_ARGS__); break;   \
    case 8: hipLaunchKernelGGL((KERNEL<8>), dim3(nb), dim3(256), 0, st, __VA_ARGS__); break;   \
    case 16: hipLaunchKernelGGL((KERNEL<16>), dim3(nb), dim3(256), 0, st, __VA_ARGS__); break; \
    case 32: hipLaunchKernelGGL((KERNEL<32>), dim3(nb), dim3(256), 0, st, __VA_ARGS__); break; \
    case 64: hipLaunchKernelGGL((KERNEL<64>), dim3(nb), dim3(256), 0, st, __VA_ARGS__); break; \
    default: return DVSOF_EINVAL;                                                              \
    }

constexpr int HEAD_FWD_ITERS = 4;   // pixels per lane group of the forward heads, see dvsof_flow_head_fwd
static bool head_c_ok(int C) { return C == 16 || C == 32 || C == 64 || C == 128 || C == 256; }

int dvsof_flow_head_fwd(const float *x, const float *w, const float *bias, float *flow, int B,
                        int H, int W, int C, void *stream)
{
    if (!x || !w || !flow || B < 1 || H < 1 || W < 1 || !head_c_ok(C)) return DVSOF_EINVAL;
    hipStream_t st = as_stream(stream);
    // no partial sums here, so the grid is free: ~4 pixels per lane group keeps enough
    // waves in flight (512 workgroups walked 32 dependent iterations: 22 us for 67 MB)
    const long long per_block = 4LL * (64 / (C / 4)) * HEAD_FWD_ITERS;
    long long nbl = ((long long)B * H * W + per_block - 1) / per_block;
    const int nb = (int)(nbl < 1 ? 1 : nbl > 65535 ? 65535 : nbl);
    HEAD_DISPATCH(head_fwd_kernel, nb, x, w, bias, flow, B, H * W);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_flow_heads_fwd(int n, const float *const *x, const float *const *w, const float *const *bias,
                         float *const *flow, int B, const int *H, const int *W, const int *C,
                         void *stream)
{
    if (n < 1 || n > HEADS_MAX || !x || !w || !flow || !H || !W || !C || B < 1) return DVSOF_EINVAL;
    HeadsFwd A = {};
    long long blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (!x[i] || !w[i] || !flow[i] || H[i] < 1 || W[i] < 1 || !head_c_ok(C[i])) return DVSOF_EINVAL;
        A.x[i] = x[i];
        A.w[i] = w[i];
        A.bias[i] = bias ? bias[i] : nullptr;
        A.flow[i] = flow[i];
        A.HW[i] = H[i] * W[i];
        A.C[i] = C[i];
        const long long per_block = 4LL * (64 / (C[i] / 4)) * HEAD_FWD_ITERS;
        long long nbl = ((long long)B * H[i] * W[i] + per_block - 1) / per_block;
        nbl = nbl < 1 ? 1 : nbl > 65535 ? 65535 : nbl;
        A.block_begin[i] = (int)blocks;
        blocks += nbl;
    }
    A.block_begin[n] = (int)blocks;
    A.B = B;
    A.n = n;
    hipLaunchKernelGGL(heads_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), A);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

size_t dvsof_flow_head_bwd_workspace_bytes(int B, int H, int W, int C)
{
    if (B < 1 || H < 1 || W < 1 || !head_c_ok(C)) return 0;
    return (size_t)head_blocks((long long)B * H * W, C / 4) * (2 * C + 2) * sizeof(float);
}

int dvsof_flow_head_bwd(const float *x, const float *w, const float *gflow, const float *gx_in,
                        const float *actsrc, int act, float *gx, float *dw, float *dbias, int B,
                        int H, int W, int C, void *ws, size_t ws_bytes, void *gx16, void *stream)
{
    // gx == NULL: the head's own weight / bias gradient only (its data part was folded into the
    // data gradient that produced gx_in's tensor: dvsof_grad_dst_t.head_w)
    if (!x || !w || !gflow || !dw || !ws || B < 1 || H < 1 || W < 1 || !head_c_ok(C))
        return DVSOF_EINVAL;
    if (ws_bytes < dvsof_flow_head_bwd_workspace_bytes(B, H, W, C)) return DVSOF_ENOSPACE;
    hipStream_t st = as_stream(stream);
    const int nb = head_blocks((long long)B * H * W, C / 4);
    float *part = (float *)ws;
    HEAD_DISPATCH(head_bwd_kernel, nb, x, w, gflow, gx_in, actsrc, act, gx, part, B, H * W,
                  (unsigned short *)gx16);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_bwd_reduce_kernel, dim3((2 * C + 2 + 3) / 4), dim3(256), 0, st,
                       (const float *)part, nb, C, dw, dbias);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_flow_head_reduce(const float *part, int rows, int C, float *dw, float *dbias, void *stream)
{
    if (!part || !dw || rows < 1 || C < 1) return DVSOF_EINVAL;
    hipLaunchKernelGGL(head_bwd_reduce_kernel, dim3((2 * C + 2 + 3) / 4), dim3(256), 0, as_stream(stream), part,
                       rows, C, dw, dbias);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_act_bwd(const float *dy, const float *actsrc, int act, float *dz, size_t n, void *stream)
{
    if (!dy || !actsrc || !dz) return DVSOF_EINVAL;
    if (n == 0) return DVSOF_OK;
    size_t nb = (n + 1023) / 1024;
    if (nb > 2048) nb = 2048;
    hipLaunchKernelGGL(act_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), dy,
                       actsrc, act, dz, n);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
