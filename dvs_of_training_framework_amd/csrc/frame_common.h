// Device helpers shared by the per-frame evaluation kernels (eval.hip,
// iwe.hip, eval_panels.hip, render.hip, contrast.hip; iwe.hip and contrast.hip
// reach the warp and the splat through event_images.h), so that what the specs
// call the same arithmetic is the same code:
//   - the fixed-order reduction of docs/EVAL_SPEC.md section 3 and
//     docs/IWE_SPEC.md section 3: thread (strided pixels, ascending) -> wave
//     (shuffle tree) -> block (waves 0..3) -> frame (partials ascending per
//     lane, shuffle tree); eval.kernel_order_sum restates it;
//   - the frame of an event, docs/EVAL_SPEC.md section 4 and
//     docs/IWE_SPEC.md section 2;
//   - the warp and the 2x2 splat of docs/IWE_SPEC.md section 2, which
//     docs/CONTRAST_SPEC.md section 2 reuses forward and backward;
//   - the counted-pixel predicate and the endpoint error of
//     docs/EVAL_SPEC.md section 3, which docs/EVAL_PANELS_SPEC.md draws.
// Everything here relies on -ffp-contract=off.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr int kFrameNT = 256;
constexpr int kMaxPartials = 128;     // per frame: two per lane of the closing wave
constexpr int kMaxEventBlocks = 2048;
constexpr int kMaxSide = 32767;       // beyond it an int16-saturated coordinate could be inside the map
constexpr int kMaxFrames = 65535;     // frames ride in gridDim.y
constexpr float kOne = 4294967296.f;  // 2^32: the fixed-point unit of q

inline bool bad_frame_sizes(int F, int h, int w)
{
    return F > kMaxFrames || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide;
}

// ---------------------------------------------------------------------------
// Fixed-order reduction.  Ops names the accumulator Ops::Row (any trivially
// copyable struct of 32-bit words; a result row of the C ABI where that is
// what is summed), its identity Ops::zero() and Ops::add(a, b).
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T shfl_down_words(const T &a, int off)
{
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "shuffled word by word");
    uint32_t word[sizeof(T) / 4];
    __builtin_memcpy(word, &a, sizeof(T));
#pragma unroll
    for (size_t i = 0; i < sizeof(T) / 4; ++i) word[i] = __shfl_down(word[i], off, kWave);
    T b;
    __builtin_memcpy(&b, word, sizeof(T));
    return b;
}

// valid in lane 0
template <typename Ops>
__device__ __forceinline__ typename Ops::Row wave_tree(typename Ops::Row a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a = Ops::add(a, shfl_down_words(a, off));
    return a;
}

// valid in thread 0 of a block of kFrameNT: the waves' sums through LDS, added in the order of the waves
template <typename Ops>
__device__ __forceinline__ typename Ops::Row block_tree(typename Ops::Row a)
{
    a = wave_tree<Ops>(a);
    __shared__ typename Ops::Row sh[kFrameNT / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = sh[0];
#pragma unroll
        for (int k = 1; k < kFrameNT / kWave; ++k) a = Ops::add(a, sh[k]);
    }
    return a;
}

// Launch 1, grid (nb, F): pixel(a, p) adds pixel p of frame blockIdx.y to a; block b of the
// frame takes pixels b * kFrameNT + thread + k * nb * kFrameNT and stores partial [f][b].
template <typename Ops, typename Pixel>
__device__ __forceinline__ void frame_partial(int n, int nb, typename Ops::Row *__restrict__ part, Pixel pixel)
{
    const int f = blockIdx.y, b = blockIdx.x;
    typename Ops::Row a = Ops::zero();
    for (int p = b * kFrameNT + threadIdx.x; p < n; p += nb * kFrameNT) pixel(a, p);
    a = block_tree<Ops>(a);
    if (threadIdx.x == 0) part[(size_t)f * nb + b] = a;
}

// Launch 2, one wave per frame: lane k adds partials k, k + 64, then the tree.
template <typename Ops>
__global__ __launch_bounds__(kWave) void frame_final_kernel(const typename Ops::Row *__restrict__ part, int nb,
                                                            typename Ops::Row *__restrict__ result)
{
    const int f = blockIdx.x;
    typename Ops::Row a = Ops::zero();
    for (int k = threadIdx.x; k < nb; k += kWave) {
        const typename Ops::Row r = part[(size_t)f * nb + k];  // the whole row in flight before the first use
        a = Ops::add(a, r);
    }
    a = wave_tree<Ops>(a);
    if (threadIdx.x == 0) result[f] = a;
}

inline int partial_blocks(int h, int w)
{
    const long long n = (long long)h * w;
    const long long nb = (n + 4 * kFrameNT - 1) / (4 * kFrameNT);  // ~4 pixels per thread
    return (int)(nb < 1 ? 1 : (nb > kMaxPartials ? kMaxPartials : nb));
}

// ---------------------------------------------------------------------------
// Events of a batch of frames.  One thread per event, grid-stride; the frame
// of event e is the last f with begin[f] <= e, and an event before begin[0] or
// from begin[F] on belongs to no frame (a test, not a clamp).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int frame_of_event(const int64_t *__restrict__ begin, int F, int64_t e)
{
    int lo = 0, hi = F;  // begin[lo] <= e < begin[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (begin[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// body(e, f) for every event e of this thread that belongs to a frame f
template <typename Body>
__device__ __forceinline__ void for_each_frame_event(int64_t n, const int64_t *__restrict__ begin, int F, Body body)
{
    const int64_t stride = (int64_t)gridDim.x * kFrameNT;
    const int64_t first = begin[0], last = begin[F];
    for (int64_t e = (int64_t)blockIdx.x * kFrameNT + threadIdx.x; e < n; e += stride) {
        if (e < first || e >= last) continue;
        body(e, frame_of_event(begin, F, e));
    }
}

inline unsigned event_blocks(int64_t n)
{
    const int64_t blocks = (n + kFrameNT - 1) / kFrameNT;
    return (unsigned)(blocks < kMaxEventBlocks ? blocks : kMaxEventBlocks);
}

// ---------------------------------------------------------------------------
// Warp and splat, IWE_SPEC section 2.
// ---------------------------------------------------------------------------
struct Warp {
    int cx, cy;  // the corner floor(xw), floor(yw)
    float wx[2], wy[2];
    float tau;
};

// Step 1 alone: the time of an event within its window, in [0, 1]
__device__ __forceinline__ float event_tau(float te, float t0, float t1)
{
    const float d = t1 - t0;
    return d > 0.f ? fminf(fmaxf((te - t0) / d, 0.f), 1.f) : 0.f;
}

// Steps 2-6 for an event that takes part in a frame, carried to the reference
// time rho in [0, 1] of the window (docs/CONTRAST_SPEC.md section 11) over
// sig = tau - rho; rho = 0 is the start of the window of IWE_SPEC section 2,
// where sig has the bits of tau (tau - 0.f, -0 included).  o.tau holds sig.
// u, v: the flow at the event's own pixel, read by the caller once for all
// references.  false: dropped by the inside test.  Every splat and the backward
// call this, so they see the same bits.
__device__ __forceinline__ bool warp_event_to(float tau, float rho, float u, float v, int64_t xi, int64_t yi,
                                              int h, int w, Warp &o)
{
    o.tau = tau - rho;
    const float xw = (float)xi - o.tau * u, yw = (float)yi - o.tau * v;
    // in float, before any conversion: false for a NaN, an infinity, 1e30
    if (!(xw > -1.f && xw < (float)w && yw > -1.f && yw < (float)h)) return false;
    const float flx = floorf(xw), fly = floorf(yw);  // in [-1, side - 1]
    const float fx = xw - flx, fy = yw - fly;
    o.wx[0] = 1.f - fx;
    o.wx[1] = fx;
    o.wy[0] = 1.f - fy;
    o.wy[1] = fy;
    o.cx = (int)flx;
    o.cy = (int)fly;
    return true;
}

// Steps 7-8: the four corners inside the h x w image img, in units of 2^-32
__device__ __forceinline__ void splat_corners(const Warp &p, int h, int w, unsigned long long *__restrict__ img)
{
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int xx = p.cx + i, yy = p.cy + j;
            if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
            const int64_t Q = (int64_t)(p.wy[j] * p.wx[i] * kOne);  // truncates; 0 <= Q <= 2^32
            if (Q > 0) atomicAdd(img + (size_t)yy * w + (size_t)xx, (unsigned long long)Q);
        }
    }
}

// ---------------------------------------------------------------------------
// Counted pixels, EVAL_SPEC: the ground-truth side of the predicate (the caller
// adds max_row and the events), and the endpoint error, one rounding a step.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool gt_counts(float tu, float tv)
{
    return !isinf(tu) && !isinf(tv) && sqrtf(tu * tu + tv * tv) > 0.f;
}
__device__ __forceinline__ float endpoint_error(float tu, float tv, float qu, float qv)
{
    const float du = tu - qu, dv = tv - qv;
    return sqrtf(du * du + dv * dv);
}

}  // namespace
