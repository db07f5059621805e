// What the two users of the average-timestamp images share (avg_timestamp.hip:
// the training term, docs/AVG_TIMESTAMP_SPEC.md; iwe.hip: the validation
// metric, docs/IWE_SPEC.md sections 14-21): what one event does to q, s, base
// and count of the images of its frame (AVG_TIMESTAMP_SPEC section 2), the
// per-pixel quantities and the 32-byte statistics row of an image (section 3).
// Which events belong to a frame is each user's own rule.  Everything here
// relies on -ffp-contract=off.
#pragma once
#include "event_images.h"

namespace {

constexpr double kEps = 0x1p-10;  // T = A / (I + kEps): 1 / (I + kEps) <= 1024

// the accumulator of the statistics
struct StatRow {
    double S, S0, peak;
    uint32_t n, n0;  // at most h w < 2^30
};
static_assert(sizeof(StatRow) == 32, "a statistics row is 32 bytes");

// ---------------------------------------------------------------------------
// An event at (xi, yi) = pixel pix inside an h x w frame, of channel c, at tau
// of the window of its frame f, with the flow (u, v) at its own pixel (read
// once for all references): per reference the count and the distance at the
// event's own pixel, and at the corners inside the image the weight and the
// weight times the distance.  plane: h w; q, s, base and count start at the
// images of this shape.
// ---------------------------------------------------------------------------
template <int R, bool POL>
__device__ __forceinline__ void avgts_splat_event(const Refs &refs, int f, int c, float tau, float u, float v,
                                                  int64_t xi, int64_t yi, size_t pix, size_t plane, int h, int w,
                                                  unsigned long long *__restrict__ q,
                                                  unsigned long long *__restrict__ s,
                                                  unsigned long long *__restrict__ base,
                                                  uint32_t *__restrict__ count)
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t m = image_of<R, POL>(f, r, c);
        Warp p;
        const bool inside = warp_event_to(tau, refs.rho[r], u, v, xi, yi, h, w, p);
        const float a = fabsf(p.tau);  // p.tau holds sig, set before the inside test; 0 <= a <= 1
        atomicAdd(count + m * plane + pix, 1u);
        const int64_t B = (int64_t)(a * kOne);  // exact; 0 <= B <= 2^32
        if (B > 0) atomicAdd(base + m * plane + pix, (unsigned long long)B);
        if (!inside) continue;
        unsigned long long *qm = q + m * plane, *sm = s + m * plane;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int xx = p.cx + i, yy = p.cy + j;
                if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
                const float wgt = p.wy[j] * p.wx[i];
                const int64_t Q = (int64_t)(wgt * kOne);         // the addend of splat_corners
                const int64_t QA = (int64_t)((wgt * a) * kOne);  // one float32 product, then exact; QA <= Q
                const size_t at = (size_t)yy * w + (size_t)xx;
                if (Q > 0) atomicAdd(qm + at, (unsigned long long)Q);
                if (QA > 0) atomicAdd(sm + at, (unsigned long long)QA);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// A pixel of an image, in float64: the average distance T of the events that
// landed on it, D = 1 / (I + kEps), and the average distance T0 at zero flow.
// ---------------------------------------------------------------------------
struct AvgPixel {
    double T, D, T0;
};
__device__ __forceinline__ AvgPixel avgts_pixel(int64_t Q, int64_t S, int64_t B, uint32_t c)
{
    const double den = (double)Q * 0x1p-32 + kEps;
    AvgPixel o;
    o.T = (double)S * 0x1p-32 / den;
    o.D = 1.0 / den;
    o.T0 = (double)B * 0x1p-32 / ((double)c + kEps);
    return o;
}

// ---------------------------------------------------------------------------
// Statistics, by the fixed-order reduction of frame_common.h.
// ---------------------------------------------------------------------------
struct AvgSum {
    using Row = StatRow;
    static __device__ __forceinline__ Row zero() { return Row{0.0, 0.0, 0.0, 0u, 0u}; }
    static __device__ __forceinline__ Row add(const Row &a, const Row &b)
    {
        return Row{a.S + b.S, a.S0 + b.S0, a.peak > b.peak ? a.peak : b.peak, a.n + b.n, a.n0 + b.n0};
    }
};

__global__ __launch_bounds__(kFrameNT) void avgts_stats_partial_kernel(
    const int64_t *__restrict__ q, const int64_t *__restrict__ s, const int64_t *__restrict__ base,
    const uint32_t *__restrict__ count, int h, int w, int nb, StatRow *__restrict__ part)
{
    const int m = blockIdx.y;
    const int n = h * w;
    const int64_t *qm = q + (size_t)m * n, *sm = s + (size_t)m * n, *bm = base + (size_t)m * n;
    const uint32_t *cm = count + (size_t)m * n;
    frame_partial<AvgSum>(n, nb, part, [=](StatRow &a, int p) {
        const int64_t Q = qm[p];
        const uint32_t c = cm[p];
        const AvgPixel px = avgts_pixel(Q, sm[p], bm[p], c);
        const double pk = 2.0 * px.T * px.D;
        a.S += px.T * px.T;
        a.S0 += px.T0 * px.T0;
        a.peak = a.peak > pk ? a.peak : pk;
        a.n += Q > 0;
        a.n0 += c > 0;
    });
}

}  // namespace
