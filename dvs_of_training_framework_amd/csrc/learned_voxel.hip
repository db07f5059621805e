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
// Order-independent forward (dvsof_learned_voxelize_tiled, opt-in): the structure
// of the tiled fixed voxeliser (voxel.hip) with the table lookup inside the tile
// pass.  A bucket pass sorts 8-byte records {local pixel | sign, bits of tn} by
// tile; one workgroup per tile adds Q = trunc(s * w * 2^32) to [C][tile] 64-bit
// integer accumulators in LDS and converts every voxel once.  Integer sums do
// not depend on the order of their addends: same inputs, same bits, whatever the
// arrival order.  Where the tiled plan does not apply, one thread per event adds
// the same Q with 64-bit integer global atomics into an int64 scratch grid that
// a closing kernel converts: the same bits by construction.
//
// This file relies on -ffp-contract=off: u, j and g are the float32 operations
// of the spec, one rounding each.
#include "common.h"
#include "voxel_tiles.h"

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

// ---------------------------------------------------------------------------
// order-independent forward
// ---------------------------------------------------------------------------
constexpr double kTwo32 = 4294967296.0, kTwoM32 = 2.3283064365386963e-10;

// s * w in 2^-32 fixed point, truncated toward zero (s * w is exact, so Q(-w) = -Q(w));
// defined while |w| < 2^31
__device__ __forceinline__ unsigned long long fixed_q(float sw)
{
    return (unsigned long long)(long long)((double)sw * kTwo32);
}

// One kept event (its tn, its sign) into 64-bit accumulators `acc` with bin pitch `pitch`:
// the bins, the knot test and w of the Forward section, then one integer atomic per kept bin
// (LDS in the tile pass, global memory in the fallback).  floor(tn) is clamped to the grid
// (a no-op for the tn of a kept event, 0 <= tn <= C - 1): no index leaves the accumulators
// whatever the windows hold.
__device__ __forceinline__ void lv_add(unsigned long long *acc, size_t pitch, const float *th,
                                       const LvP &P, float tn, bool neg)
{
    const int c0 = min(max((int)floorf(tn), 0), P.C - 1);
    const int c_lo = max(c0 - P.R, 0), c_hi = min(c0 + P.R, P.C - 1);
    for (int c = c_lo; c <= c_hi; ++c) {
        int j;
        float g;
        if (!knot(P, tn, c, j, g)) continue;
        const float w = th[j] * (1.f - g) + th[j + 1] * g;
        atomicAdd(acc + (size_t)c * pitch, fixed_q(neg ? -w : w));
    }
}

// Bucket pass: vox_bucket_kernel (voxel.hip) with another record -- the key carries the local
// pixel and the sign, the payload the bits of tn -- over the column loaders of this file.
// Same tiles, cursors, overflow list and self-cleaning control words (voxel_tiles.h).
template <class Cols, int EPT>
__global__ __launch_bounds__(NT) void lv_bucket_kernel(const Cols cols, const LvP P, const VoxV2 T)
{
    extern __shared__ int sh[];          // hist[ntile], base[ntile]
    __shared__ int s_lo, s_hi;
    int *hist = sh, *base = sh + T.ntile;
    if (threadIdx.x == 0) {
        s_lo = T.ntile;
        s_hi = -1;
    }
    __syncthreads();
    const int64_t e0 = ((int64_t)blockIdx.x * NT) * EPT + threadIdx.x;
    int tile[EPT], rank[EPT];
    unsigned key[EPT];
    float tnv[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int64_t i = e0 + (int64_t)k * NT;   // coalesced across the workgroup
        tile[k] = -1;
        if (i < P.n) {
            const Event e = cols.load(i);
            float tn;
            if (e.s != 0.f && normalised_time(P, e, i, tn)) {     // s = 0 reaches no bucket
                const int yi = (int)e.y, xi = (int)e.x;
                const int ty = yi >> (T.lp - T.lx), tx = xi >> T.lx;
                tile[k] = ((int)e.b * T.TY + ty) * T.TX + tx;
                key[k] = (unsigned)(((yi - (ty << (T.lp - T.lx))) << T.lx) + (xi - (tx << T.lx))) |
                         (e.s < 0.f ? 0x80000000u : 0u);
                tnv[k] = tn;
            }
        }
    }
    // tile range of this workgroup's events
    {
        int lo = T.ntile, hi = -1;
#pragma unroll
        for (int k = 0; k < EPT; ++k)
            if (tile[k] >= 0) {
                lo = min(lo, tile[k]);
                hi = max(hi, tile[k]);
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = min(lo, __shfl_xor(lo, off, kWave));
            hi = max(hi, __shfl_xor(hi, off, kWave));
        }
        if ((threadIdx.x & (kWave - 1)) == 0 && hi >= 0) {
            atomicMin(&s_lo, lo);
            atomicMax(&s_hi, hi);
        }
    }
    __syncthreads();
    const int t_lo = s_lo, t_hi = s_hi;
    for (int i = t_lo + (int)threadIdx.x; i <= t_hi; i += NT) hist[i] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPT; ++k)
        if (tile[k] >= 0) rank[k] = atomicAdd(&hist[tile[k]], 1);
    __syncthreads();
    for (int i = t_lo + (int)threadIdx.x; i <= t_hi; i += NT) {
        const int c = hist[i];
        base[i] = c ? atomicAdd(&T.cursor[i], c) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        if (tile[k] < 0) continue;
        const int pos = base[tile[k]] + rank[k];
        if (pos < T.cap) {
            T.records[(size_t)tile[k] * T.cap + pos] = make_uint2(key[k], __float_as_uint(tnv[k]));
        } else {
            if (pos == T.cap) atomicAdd(T.ovf_tiles, 1);     // exactly one event per full bucket
            const int o = atomicAdd(T.ovf_count, 1);
            if (o < T.ovf_cap) T.ovf[o] = make_int4(tile[k], (int)key[k], __float_as_int(tnv[k]), 0);
        }
    }
}

// Tile pass: vox_tile_kernel (voxel.hip) with the table in LDS next to the accumulators and
// lv_add in place of the two triangle weights -- at most 2 R integer LDS atomics per record.
__global__ __launch_bounds__(NT) void lv_tile_kernel(const LvP P, const VoxV2 T)
{
    // [C][2^lp] fixed-point accumulators, behind the static table: aligned for the 16-byte clears
    extern __shared__ __attribute__((aligned(16))) unsigned long long tl[];
    __shared__ float th[MAX_K];
    const int tile = blockIdx.x;
    const int tx = tile % T.TX, ty = (tile / T.TX) % T.TY, b = tile / (T.TX * T.TY);
    const int nel = P.C << T.lp;
    const size_t pitch = (size_t)1 << T.lp;
    // the first 4*NT records are fetched speculatively together with the count, while the
    // table is staged and the LDS tile zeroed
    const uint2 *rec = T.records + (size_t)tile * T.cap;
    const int reserved = T.cursor[tile];
    uint2 r0[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = u * NT + (int)threadIdx.x;
        r0[u] = i < T.cap ? rec[i] : make_uint2(0u, 0u);
    }
    const int K = 2 * P.R * P.S + 1;
    for (int k = threadIdx.x; k < K; k += NT) th[k] = P.theta[k];
    for (int i = threadIdx.x * 2; i < nel; i += NT * 2) *(ulonglong2 *)(tl + i) = make_ulonglong2(0ull, 0ull);
    const int cnt = min(reserved, T.cap);
    __syncthreads();
    if (threadIdx.x == 0) T.cursor[tile] = 0;       // self-cleaning control words
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (u * NT + (int)threadIdx.x < cnt)
            lv_add(tl + (r0[u].x & 0x3ff), pitch, th, P, __uint_as_float(r0[u].y), r0[u].x >> 31);
    for (int i0 = 4 * NT; i0 < cnt; i0 += 4 * NT) {
        uint2 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * NT + (int)threadIdx.x;
            r[u] = i < cnt ? rec[i] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * NT + (int)threadIdx.x < cnt)
                lv_add(tl + (r[u].x & 0x3ff), pitch, th, P, __uint_as_float(r[u].y), r[u].x >> 31);
    }
    // events that did not fit this tile's bucket: on the overflow list among those of the
    // other full buckets
    const bool spilled = reserved > T.cap;
    if (spilled) {
        const int64_t novf = min((int64_t)*T.ovf_count, T.ovf_cap);
        for (int64_t i = threadIdx.x; i < novf; i += NT) {
            const int4 r = T.ovf[i];
            if (r.x == tile)
                lv_add(tl + ((unsigned)r.y & 0x3ff), pitch, th, P, __int_as_float(r.z), (unsigned)r.y >> 31);
        }
    }
    __syncthreads();
    // 16 bytes per lane along a tile row
    const int y0 = ty << (T.lp - T.lx), x0 = tx << T.lx;
    const bool vec = (P.W & 3) == 0 && ((uintptr_t)T.out & 15) == 0;
    for (int i = threadIdx.x * 4; i < nel; i += NT * 4) {
        const int c = i >> T.lp, r = i - (c << T.lp), ly = r >> T.lx, lx = r - (ly << T.lx);
        const int y = y0 + ly, x = x0 + lx;
        if (y >= P.H || x >= P.W) continue;
        float *o = T.out + (((size_t)b * P.C + c) * P.H + y) * P.W + x;
        float4 v;
        // signed 2^-32 fixed point -> the correctly rounded float of the integer sum
        v.x = (float)((double)(long long)tl[i] * kTwoM32);
        v.y = (float)((double)(long long)tl[i + 1] * kTwoM32);
        v.z = (float)((double)(long long)tl[i + 2] * kTwoM32);
        v.w = (float)((double)(long long)tl[i + 3] * kTwoM32);
        if (vec) {          // W % 4 == 0 and x % 4 == 0: the quad is inside the row
            *(float4 *)o = v;
        } else {
            o[0] = v.x;
            if (x + 1 < P.W) o[1] = v.y;
            if (x + 2 < P.W) o[2] = v.z;
            if (x + 3 < P.W) o[3] = v.w;
        }
    }
    // the last spilled tile to finish clears the overflow words
    if (spilled && threadIdx.x == 0 && atomicAdd(T.done, 1) == *T.ovf_tiles - 1) {
        *T.ovf_count = 0;
        *T.ovf_tiles = 0;
        *T.done = 0;
    }
}

// Fallback where the tiled plan does not apply: one thread per event, the same Q with 64-bit
// integer memory-side atomics into the int64 scratch grid acc[B,C,H,W] (zeroed by a fill
// kernel), then one conversion per voxel.
template <class Cols>
__global__ __launch_bounds__(NT) void lv_global_kernel(const Cols cols, const LvP P,
                                                       unsigned long long *__restrict__ acc)
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
        if (e.s == 0.f || !normalised_time(P, e, i, tn)) continue;
        lv_add(acc + ((size_t)e.b * P.C * P.H + (size_t)e.y) * P.W + (size_t)e.x, plane, th, P, tn,
               e.s < 0.f);
    }
}

__global__ __launch_bounds__(NT) void lv_convert_kernel(const unsigned long long *__restrict__ acc,
                                                        size_t total, float *__restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * NT;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += stride)
        out[i] = (float)((double)(long long)acc[i] * kTwoM32);
}

constexpr int LV_FLAGS = DVSOF_VOX_WS_CLEAN | DVSOF_LV_GLOBAL | DVSOF_LV_EPT8 | DVSOF_LV_EPT16;

bool bad_flags(int flags)
{
    return (flags & ~LV_FLAGS) || ((flags & DVSOF_LV_EPT8) && (flags & DVSOF_LV_EPT16));
}

// the tiled path serves this size: the fixed voxeliser's predicate
bool lv_tiled(int64_t n, int B, int C, int H, int W, int flags, VoxV2 &T)
{
    return !(flags & DVSOF_LV_GLOBAL) && n >= 4096 && v2_plan(n, B, C, H, W, T);
}

template <class Cols, int EPT>
void launch_bucket(const Cols &cols, const LvP &P, const VoxV2 &T, hipStream_t st)
{
    hipLaunchKernelGGL((lv_bucket_kernel<Cols, EPT>), dim3((unsigned)((P.n + NT * EPT - 1) / (NT * EPT))),
                       dim3(NT), (size_t)T.ntile * 8, st, cols, P, T);
}

// lv_tile_kernel's own dynamic-LDS limit (v2_launch's guard belongs to vox_tile_kernel).  The
// table is static LDS next to the dynamic accumulators: 64 KiB of them (C = 16) is already past
// the default limit of the two together; 388 B + 150 KiB stays within the 160 KiB of a workgroup.
int raise_tile_lds(size_t tile_lds)
{
    static bool attr_set = false;
    if (tile_lds + sizeof(float) * MAX_K > 64 * 1024 && !attr_set) {
        DVSOF_HIP_TRY(hipFuncSetAttribute((const void *)lv_tile_kernel,
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        attr_set = true;
    }
    return DVSOF_OK;
}

template <class Cols>
int launch_tiled(const Cols &cols, const LvP &P, const VoxV2 &T, int flags, hipStream_t st)
{
    if (!(flags & DVSOF_VOX_WS_CLEAN))
        DVSOF_HIP_TRY((hipError_t)fill_u32(T.cursor, 0u, v2_control_bytes(T), st));
    if ((flags & DVSOF_LV_EPT16) || (!(flags & DVSOF_LV_EPT8) && P.n >= EPT16_FROM))
        launch_bucket<Cols, 16>(cols, P, T, st);
    else if ((flags & DVSOF_LV_EPT8) || P.n >= EPT8_FROM)
        launch_bucket<Cols, 8>(cols, P, T, st);
    else
        launch_bucket<Cols, 4>(cols, P, T, st);
    DVSOF_LAUNCH_CHECK();
    const size_t tile_lds = ((size_t)P.C << T.lp) * 8;
    DVSOF_HIP_TRY((hipError_t)raise_tile_lds(tile_lds));
    hipLaunchKernelGGL(lv_tile_kernel, dim3(T.ntile), dim3(NT), tile_lds, st, P, T);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

template <class Cols>
int launch_global(const Cols &cols, const LvP &P, float *out, void *workspace, hipStream_t st)
{
    const size_t total = (size_t)P.B * P.C * P.H * P.W;
    unsigned long long *acc = (unsigned long long *)workspace;
    DVSOF_HIP_TRY((hipError_t)fill_u32(acc, 0u, total * 8, st));
    hipLaunchKernelGGL(lv_global_kernel<Cols>, dim3(fwd_blocks(P.n)), dim3(NT), 0, st, cols, P, acc);
    DVSOF_LAUNCH_CHECK();
    const size_t blocks = (total + NT - 1) / NT;
    hipLaunchKernelGGL(lv_convert_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(NT), 0, st,
                       (const unsigned long long *)acc, total, out);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

template <class Cols>
int launch_exact(const Cols &cols, const LvP &P, float *out, void *workspace, size_t workspace_bytes,
                 int flags, hipStream_t st)
{
    if (P.n == 0) return fill_u32(out, 0u, sizeof(float) * (size_t)P.B * P.C * P.H * P.W, st);
    if (!workspace ||
        workspace_bytes < dvsof_learned_voxelize_tiled_workspace_bytes(P.n, P.B, P.C, P.H, P.W, flags))
        return DVSOF_ENOSPACE;
    if ((uintptr_t)workspace & 15) return DVSOF_EINVAL;
    VoxV2 T = {};
    if (!lv_tiled(P.n, P.B, P.C, P.H, P.W, flags, T)) return launch_global(cols, P, out, workspace, st);
    v2_bind(T, workspace);
    T.n = P.n; T.B = P.B; T.C = P.C; T.H = P.H; T.W = P.W;
    T.out = out;
    return launch_tiled(cols, P, T, flags, st);
}

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

size_t dvsof_learned_voxelize_tiled_workspace_bytes(int64_t n, int B, int C, int H, int W, int flags)
{
    if (n < 0 || B < 1 || C < 1 || H < 1 || W < 1 || bad_flags(flags)) return 0;
    VoxV2 T = {};
    if (lv_tiled(n, B, C, H, W, flags, T)) return v2_bytes(T, n);
    return (size_t)B * C * H * W * 8;       // the int64 scratch grid
}

size_t dvsof_learned_voxelize_tiled_control_bytes(int64_t n, int B, int C, int H, int W, int flags)
{
    if (n < 0 || B < 1 || C < 1 || H < 1 || W < 1 || bad_flags(flags)) return 0;
    VoxV2 T = {};
    return lv_tiled(n, B, C, H, W, flags, T) ? v2_control_bytes(T) : 0;
}

int dvsof_learned_voxelize_tiled(const void *x, const void *y, const float *t, const void *pol,
                                 const void *sample, int encoded, int64_t n, const float *t0,
                                 const float *t1, const float *theta, int R, int S, int B, int C, int H,
                                 int W, float *out, void *workspace, size_t workspace_bytes, int flags,
                                 void *stream)
{
    if (!out || !t0 || !t1 || !theta || bad_shape(n, B, C, H, W, R, S) || bad_flags(flags))
        return DVSOF_EINVAL;
    if (encoded != 0 && encoded != 1) return DVSOF_EINVAL;
    if (n > 0 && (!x || !y || !t || !pol || !sample)) return DVSOF_EINVAL;
    const LvP P = params(t, n, t0, t1, theta, B, C, H, W, R, S);
    if (encoded)
        return launch_exact(EncodedCols{(const int16_t *)x, (const int16_t *)y, (const uint8_t *)pol,
                                        (const int64_t *)sample, B},
                            P, out, workspace, workspace_bytes, flags, as_stream(stream));
    return launch_exact(WireCols{(const int64_t *)x, (const int64_t *)y, (const int64_t *)pol,
                                 (const int64_t *)sample},
                        P, out, workspace, workspace_bytes, flags, as_stream(stream));
}

}  // extern "C"
