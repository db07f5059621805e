// Learnable event representation (docs/LEARNED_VOXEL_SPEC.md): the voxel grid
// of docs/VOXEL_SPEC.md with the triangle kernel replaced by a piecewise-linear
// lookup table theta[K], K = 2 R S + 1 knots (R = radius in bins, S = knots per
// bin) -- the form Gehrig et al. (ICCV 2019) deploy their learned temporal
// kernel in.  Forward and the gradient with respect to theta.
//
// Forward: one thread per event, coalesced reads of the event columns (the
// int64 wire columns or the 9 B/event encoded ones: ONE kernel body, templated
// on the column loader), the table in LDS, up to 2 R memory-side float atomics
// per event into the grid that a fill KERNEL zeroed on the same stream.
//
// Backward: no float atomics at all.  Every thread owns a private row of K
// accumulators in LDS (row pitch K is odd: threads that hit the same knot sit in
// different banks) and adds its events in ascending order; a knot's rows are
// then summed per wave by a shuffle tree, the waves of a block in order, and the
// block's K sums go to part[block][K]; a closing kernel adds the partials in
// block order in float64 and rounds once.  Same inputs, same bits.
//
// This file relies on -ffp-contract=off: u, j and g are the float32 operations
// of the spec, one rounding each.
#include "common.h"

namespace {

constexpr int NT = 256;             // forward: threads per block
constexpr int BNT = 128;            // backward: threads per block (<= 128 * 97 * 4 B of LDS)
constexpr int B_EPT = 8;            // backward: events per thread until the block count saturates
constexpr int B_MAX_BLOCKS = 512;
constexpr int MAX_R = 3, MAX_S = 16;
constexpr int MAX_K = 2 * MAX_R * MAX_S + 1;

struct Event {
    int64_t b, x, y;
    float s;        // sign of the polarity: -1, 0 or +1
};

// the reference's wire format (utils/dataset.py:961-1020)
struct WireCols {
    const int64_t *x, *y, *pol, *sample;
    __device__ __forceinline__ Event load(int64_t i) const
    {
        const int64_t pv = pol[i];
        return Event{sample[i], x[i], y[i], pv > 0 ? 1.f : (pv < 0 ? -1.f : 0.f)};
    }
};

// the encoded columns (utils/dataset.py:286-289) + the first event of every sample
struct EncodedCols {
    const int16_t *x, *y;
    const uint8_t *pol;
    const int64_t *ev_off;      // [B + 1]
    int B;
    __device__ __forceinline__ Event load(int64_t i) const
    {
        int lo = 0, hi = B;     // last sample with ev_off <= i
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (ev_off[mid] <= i) lo = mid; else hi = mid;
        }
        return Event{(int64_t)lo, (int64_t)x[i], (int64_t)y[i], pol[i] ? 1.f : -1.f};
    }
};

struct LvP {
    const float *t, *t0, *t1, *theta;
    int64_t n;
    int B, C, H, W, R, S;
};

// Drop rule and tn of VOXEL_SPEC (same float32 operations, same order).
// -> false: the event is dropped.
__device__ __forceinline__ bool normalised_time(const LvP &P, const Event &e, int64_t i, float &tn)
{
    if (!(e.b >= 0 && e.b < P.B && e.x >= 0 && e.x < P.W && e.y >= 0 && e.y < P.H)) return false;
    const float ts = P.t[i], lo = P.t0[e.b], hi = P.t1[e.b];
    if (!(ts >= lo && ts <= hi)) return false;
    const float dt = hi - lo;
    tn = dt > 0.f ? ((ts - lo) / dt) * (float)(P.C - 1) : 0.f;
    return true;
}

// bins an event can touch: |floor(tn) - c| <= R covers every c with -R <= tn - c < R
__device__ __forceinline__ void bin_range(const LvP &P, float tn, int &c_lo, int &c_hi)
{
    const int c0 = (int)floorf(tn);
    c_lo = max(c0 - P.R, 0);
    c_hi = min(c0 + P.R, P.C - 1);
}

// knot j and fraction g of (event, bin c); false: outside the kernel's support
__device__ __forceinline__ bool knot(const LvP &P, float tn, int c, int &j, float &g)
{
    const float u = ((tn - (float)c) + (float)P.R) * (float)P.S;
    if (!(u >= 0.f && u < (float)(2 * P.R * P.S))) return false;
    j = (int)floorf(u);
    g = u - (float)j;
    return true;
}

template <class Cols>
__global__ __launch_bounds__(NT) void lv_fwd_kernel(const Cols cols, const LvP P, float *__restrict__ out)
{
    __shared__ float th[MAX_K];
    const int K = 2 * P.R * P.S + 1;
    for (int k = threadIdx.x; k < K; k += NT) th[k] = P.theta[k];
    __syncthreads();
    const size_t plane = (size_t)P.H * P.W;
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < P.n; i += stride) {
        const Event e = cols.load(i);
        float tn;
        if (e.s == 0.f || !normalised_time(P, e, i, tn)) continue;     // s = 0 adds s * w = 0
        int c_lo, c_hi;
        bin_range(P, tn, c_lo, c_hi);
        float *o = out + ((size_t)e.b * P.C * P.H + (size_t)e.y) * P.W + (size_t)e.x;
        for (int c = c_lo; c <= c_hi; ++c) {
            int j;
            float g;
            if (!knot(P, tn, c, j, g)) continue;
            const float w = th[j] * (1.f - g) + th[j + 1] * g;
            atomicAdd(o + (size_t)c * plane, e.s * w);
        }
    }
}

template <class Cols>
__global__ __launch_bounds__(BNT) void lv_bwd_kernel(const Cols cols, const LvP P,
                                                     const float *__restrict__ gV,
                                                     float *__restrict__ part)
{
    extern __shared__ float rows[];         // [BNT][K]
    __shared__ float wsum[BNT / kWave][MAX_K];
    const int K = 2 * P.R * P.S + 1;
    float *mine = rows + (size_t)threadIdx.x * K;
    for (int k = 0; k < K; ++k) mine[k] = 0.f;
    const size_t plane = (size_t)P.H * P.W;
    const int64_t stride = (int64_t)gridDim.x * BNT;
    for (int64_t i = (int64_t)blockIdx.x * BNT + threadIdx.x; i < P.n; i += stride) {
        const Event e = cols.load(i);
        float tn;
        if (e.s == 0.f || !normalised_time(P, e, i, tn)) continue;
        int c_lo, c_hi;
        bin_range(P, tn, c_lo, c_hi);
        const float *gp = gV + ((size_t)e.b * P.C * P.H + (size_t)e.y) * P.W + (size_t)e.x;
        for (int c = c_lo; c <= c_hi; ++c) {
            int j;
            float g;
            if (!knot(P, tn, c, j, g)) continue;
            const float sg = e.s * gp[(size_t)c * plane];       // exact: s = +-1
            mine[j] += sg * (1.f - g);
            mine[j + 1] += sg * g;
        }
    }
    __syncthreads();
    // knot k: the 64 rows of a wave by a shuffle tree, then the waves in order
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int k = 0; k < K; ++k) {
        float v = mine[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
        if (lane == 0) wsum[wave][k] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += BNT) {
        float v = wsum[0][k];
#pragma unroll
        for (int w = 1; w < BNT / kWave; ++w) v += wsum[w][k];
        part[(size_t)blockIdx.x * K + k] = v;
    }
}

// the partials of knot k added in block order in float64, rounded once: the closing sum of
// BOTH exports (their bitwise equality is this one function)
__device__ __forceinline__ float block_order_sum(const float *__restrict__ part, int G, int K, int k)
{
    double s = 0.0;
    int g = 0;
    for (; g + 8 <= G; g += 8) {        // eight loads in flight, added in order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(g + u) * K + k];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)v[u];
    }
    for (; g < G; ++g) s += (double)part[(size_t)g * K + k];
    return (float)s;
}

__global__ __launch_bounds__(kWave) void lv_bwd_final_kernel(const float *__restrict__ part, int G,
                                                             int K, float *__restrict__ gtheta)
{
    const int k = blockIdx.x * kWave + threadIdx.x;
    if (k >= K) return;
    gtheta[k] = block_order_sum(part, G, K, k);
}

// The closing kernel of the RESIDENT gradient slot (dvsof_learned_voxelize_bwd_into): the same
// sum s, WRITTEN (accumulate = 0) or added to what the slot holds (accumulate = 1: one float32
// add, the rounding of autograd's `grad += g`).  G = 0 (no events) writes zeros; the accumulating
// call with no events is not launched at all, so that a slot holding -0.0 keeps its bits.
__global__ __launch_bounds__(kWave) void lv_bwd_final_into_kernel(const float *__restrict__ part,
                                                                  int G, int K, float *gtheta,
                                                                  int accumulate)
{
    const int k = blockIdx.x * kWave + threadIdx.x;
    if (k >= K) return;
    const float r = block_order_sum(part, G, K, k);
    gtheta[k] = accumulate ? gtheta[k] + r : r;
}

int fwd_blocks(int64_t n) { return (int)((n + NT - 1) / NT < 2048 ? (n + NT - 1) / NT : 2048); }

int bwd_blocks(int64_t n)
{
    const int64_t g = (n + (int64_t)BNT * B_EPT - 1) / ((int64_t)BNT * B_EPT);
    return (int)(g < 1 ? 1 : (g > B_MAX_BLOCKS ? B_MAX_BLOCKS : g));
}

bool bad_shape(int64_t n, int B, int C, int H, int W, int R, int S)
{
    return n < 0 || B < 1 || C < 1 || H < 1 || W < 1 || R < 1 || R > MAX_R || S < 1 || S > MAX_S;
}

LvP params(const float *t, int64_t n, const float *t0, const float *t1, const float *theta, int B,
           int C, int H, int W, int R, int S)
{
    return LvP{t, t0, t1, theta, n, B, C, H, W, R, S};
}

template <class Cols>
int launch_fwd(const Cols &cols, const LvP &P, float *out, hipStream_t st)
{
    DVSOF_HIP_TRY((hipError_t)fill_u32(out, 0u, sizeof(float) * (size_t)P.B * P.C * P.H * P.W, st));
    if (P.n == 0) return DVSOF_OK;
    hipLaunchKernelGGL(lv_fwd_kernel<Cols>, dim3(fwd_blocks(P.n)), dim3(NT), 0, st, cols, P, out);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

template <class Cols>
int launch_bwd(const Cols &cols, const LvP &P, const float *gV, float *gtheta, void *workspace,
               size_t workspace_bytes, hipStream_t st)
{
    const int K = 2 * P.R * P.S + 1;
    if (P.n == 0) return fill_u32(gtheta, 0u, sizeof(float) * K, st);
    if (!workspace || workspace_bytes < dvsof_learned_voxelize_bwd_workspace_bytes(P.n, P.R, P.S))
        return DVSOF_ENOSPACE;
    const int G = bwd_blocks(P.n);
    float *part = (float *)workspace;
    hipLaunchKernelGGL(lv_bwd_kernel<Cols>, dim3(G), dim3(BNT), sizeof(float) * BNT * K, st, cols, P,
                       gV, part);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(lv_bwd_final_kernel, dim3((K + kWave - 1) / kWave), dim3(kWave), 0, st,
                       (const float *)part, G, K, gtheta);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

// Kernels only (no fill, no memset, no copy): what a stream capture may hold.
template <class Cols>
int launch_bwd_into(const Cols &cols, const LvP &P, const float *gV, float *gtheta, int accumulate,
                    void *workspace, size_t workspace_bytes, hipStream_t st)
{
    const int K = 2 * P.R * P.S + 1;
    if (P.n == 0 && accumulate) return DVSOF_OK;       // gtheta + 0 would turn -0.0 into +0.0
    int G = 0;
    float *part = (float *)workspace;
    if (P.n > 0) {
        if (!workspace || workspace_bytes < dvsof_learned_voxelize_bwd_workspace_bytes(P.n, P.R, P.S))
            return DVSOF_ENOSPACE;
        G = bwd_blocks(P.n);
        hipLaunchKernelGGL(lv_bwd_kernel<Cols>, dim3(G), dim3(BNT), sizeof(float) * BNT * K, st, cols,
                           P, gV, part);
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lv_bwd_final_into_kernel, dim3((K + kWave - 1) / kWave), dim3(kWave), 0, st,
                       (const float *)part, G, K, gtheta, accumulate ? 1 : 0);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // namespace

extern "C" {

int dvsof_learned_voxelize_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *pol,
                               const int64_t *sample, int64_t n, const float *t0, const float *t1,
                               const float *theta, int R, int S, int B, int C, int H, int W,
                               float *out, void *stream)
{
    if (!out || !t0 || !t1 || !theta || bad_shape(n, B, C, H, W, R, S)) return DVSOF_EINVAL;
    if (n > 0 && (!x || !y || !t || !pol || !sample)) return DVSOF_EINVAL;
    return launch_fwd(WireCols{x, y, pol, sample}, params(t, n, t0, t1, theta, B, C, H, W, R, S), out,
                      as_stream(stream));
}

int dvsof_learned_voxelize_encoded(const int16_t *x, const int16_t *y, const float *t,
                                   const uint8_t *pol, const int64_t *sample_event_offsets, int64_t n,
                                   const float *t0, const float *t1, const float *theta, int R, int S,
                                   int B, int C, int H, int W, float *out, void *stream)
{
    if (!out || !t0 || !t1 || !theta || bad_shape(n, B, C, H, W, R, S)) return DVSOF_EINVAL;
    if (n > 0 && (!x || !y || !t || !pol || !sample_event_offsets)) return DVSOF_EINVAL;
    return launch_fwd(EncodedCols{x, y, pol, sample_event_offsets, B},
                      params(t, n, t0, t1, theta, B, C, H, W, R, S), out, as_stream(stream));
}

size_t dvsof_learned_voxelize_bwd_workspace_bytes(int64_t n_events, int R, int S)
{
    if (n_events < 0 || R < 1 || R > MAX_R || S < 1 || S > MAX_S) return 0;
    return sizeof(float) * (size_t)bwd_blocks(n_events) * (2 * R * S + 1);
}

int dvsof_learned_voxelize_bwd_blocks(int64_t n_events) { return n_events < 0 ? 0 : bwd_blocks(n_events); }

int dvsof_learned_voxelize_bwd(const void *x, const void *y, const float *t, const void *pol,
                               const int64_t *sample, int encoded, int64_t n, const float *t0,
                               const float *t1, int R, int S, int B, int C, int H, int W,
                               const float *gV, float *gtheta, void *workspace, size_t workspace_bytes,
                               void *stream)
{
    if (!gV || !gtheta || !t0 || !t1 || bad_shape(n, B, C, H, W, R, S)) return DVSOF_EINVAL;
    if (n > 0 && (!x || !y || !t || !pol || !sample)) return DVSOF_EINVAL;
    const LvP P = params(t, n, t0, t1, nullptr, B, C, H, W, R, S);
    if (encoded)
        return launch_bwd(EncodedCols{(const int16_t *)x, (const int16_t *)y, (const uint8_t *)pol, sample, B},
                          P, gV, gtheta, workspace, workspace_bytes, as_stream(stream));
    return launch_bwd(WireCols{(const int64_t *)x, (const int64_t *)y, (const int64_t *)pol, sample}, P, gV,
                      gtheta, workspace, workspace_bytes, as_stream(stream));
}

int dvsof_learned_voxelize_bwd_into(const void *x, const void *y, const float *t, const void *pol,
                                    const int64_t *sample, int encoded, int64_t n, const float *t0,
                                    const float *t1, int R, int S, int B, int C, int H, int W,
                                    const float *gV, float *gtheta, int accumulate, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    if (!gV || !gtheta || !t0 || !t1 || bad_shape(n, B, C, H, W, R, S)) return DVSOF_EINVAL;
    if (accumulate != 0 && accumulate != 1) return DVSOF_EINVAL;
    if (n > 0 && (!x || !y || !t || !pol || !sample)) return DVSOF_EINVAL;
    const LvP P = params(t, n, t0, t1, nullptr, B, C, H, W, R, S);
    if (encoded)
        return launch_bwd_into(EncodedCols{(const int16_t *)x, (const int16_t *)y, (const uint8_t *)pol, sample, B},
                               P, gV, gtheta, accumulate, workspace, workspace_bytes, as_stream(stream));
    return launch_bwd_into(WireCols{(const int64_t *)x, (const int64_t *)y, (const int64_t *)pol, sample}, P,
                           gV, gtheta, accumulate, workspace, workspace_bytes, as_stream(stream));
}

}  // extern "C"
