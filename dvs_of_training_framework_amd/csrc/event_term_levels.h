// What the two events-only training terms (contrast.hip, avg_timestamp.hip) and
// the tiled schedule of their splat (tiled_splat.h) say about levels, once:
// the level table of include/dvsof_contrast_pyramid.h and its refusals, the two
// views through which one kernel serves a call on one flow and a call over a
// table, the closing kernel of the backward, and the four-corner tail of the
// backward over events.  Everything here relies on -ffp-contract=off.
#pragma once
#include "event_columns.h"
#include "../../include/dvsof_contrast_pyramid.h"

namespace {

using Levels = dvsof_contrast_levels_t;
using Level = dvsof_contrast_level_t;
constexpr int kMaxLevels = 8;
constexpr int kMaxShift = 15;
static_assert(sizeof(Levels::level) / sizeof(Level) == kMaxLevels, "the table holds eight levels");

// The sum of the levels' pixels; 0: a table the calls refuse (K outside [1, 8], sizes the frame
// rule refuses, a shift outside [0, 15], a level that is not ceil(side / 2^shift)).  packed_M > 0:
// the offsets are also those of levels packed one behind the other at packed_M images a level.
inline size_t level_table_pixels(int F, int h, int w, const Levels &lv, int packed_M)
{
    if (lv.K < 1 || lv.K > kMaxLevels || bad_frame_sizes(F, h, w)) return 0;
    size_t pixels = 0;
    for (int k = 0; k < lv.K; ++k) {
        const Level &L = lv.level[k];
        if (bad_frame_sizes(F, L.h, L.w) || L.shift < 0 || L.shift > kMaxShift) return 0;
        const int round = (1 << L.shift) - 1;
        if (L.h != (h + round) >> L.shift || L.w != (w + round) >> L.shift) return 0;
        if (packed_M > 0 && (L.image_offset != (size_t)packed_M * pixels || L.row_offset != (size_t)k * packed_M ||
                             L.sums_offset != 2 * (size_t)F * pixels))
            return 0;
        pixels += (size_t)L.h * L.w;
    }
    return pixels;
}

// ---------------------------------------------------------------------------
// The two views of a call's levels.  A kernel takes one by value, walks
// k < levels() and reads at(k); a lambda inside it captures the view by
// reference.  kTable: the call has per-level terms and a weighted value.
// ---------------------------------------------------------------------------
// a level table as the calls over every flow scale take it, K at run time
struct TableView {
    Levels lv;
    static constexpr bool kTable = true;
    __host__ __device__ __forceinline__ int levels() const { return lv.K; }
    __host__ __device__ __forceinline__ const Level &at(int k) const { return lv.level[k]; }
    const Levels &table() const { return lv; }
};

// One flow of the frame's own size.  The level count, the shift and the three offsets are
// constants, so the level loop, the shifts and the offset adds of a kernel fold away.
struct OneLevel {
    int h, w;
    const float *flow;
    float weight;      // read by the backward only
    float *grad_flow;  // likewise
    static constexpr bool kTable = false;
    __host__ __device__ __forceinline__ constexpr int levels() const { return 1; }
    __host__ __device__ __forceinline__ Level at(int) const { return Level{flow, grad_flow, h, w, 0, weight, 0, 0, 0}; }
    // the table of one level that states the same call: what the host checks and lays out
    Levels table() const
    {
        Levels t{};
        t.K = 1;
        t.level[0] = at(0);
        return t;
    }
};

// ---------------------------------------------------------------------------
// The backward's closing kernel.  One thread per element of every level's
// grad_flow, the level found from the element's place in the sums: convert,
// clear the sum for the next backward of the same forward, store.  unit: one
// per level and frame, M: the images of a level.
// ---------------------------------------------------------------------------
template <class View>
__global__ __launch_bounds__(kFrameNT) void event_term_bwd_close_kernel(long long *__restrict__ acc,
                                                                        const double *__restrict__ unit,
                                                                        const float *__restrict__ seed, int F, int M,
                                                                        const View view, size_t total)
{
    const size_t stride = (size_t)gridDim.x * kFrameNT;
    const float s0 = seed[0];
    for (size_t i = (size_t)blockIdx.x * kFrameNT + threadIdx.x; i < total; i += stride) {
        int k = 0;
        while (k + 1 < view.levels() && i >= view.at(k + 1).sums_offset) ++k;
        const Level &L = view.at(k);
        const size_t local = i - L.sums_offset, per_frame = 2 * (size_t)L.h * L.w;
        const float sw = s0 * L.weight;
        const long long a = acc[i];
        acc[i] = 0;
        const double value = (double)a / unit[(size_t)k * F + local / per_frame] / (double)M;  // the first division is exact
        L.grad_flow[local] = sw * (float)value;
    }
}

// ---------------------------------------------------------------------------
// The tail of the backward over events, for one reference of one event warped
// to p on an h x w level: G at the four corners (G_at(pixel index) inside the
// image, 0 outside), the derivative of the bilinear weights, -sig of it to the
// event's own pixel of the flow, in float64, truncated to the frame's unit un
// and added to su, sv (integers: no order).
// ---------------------------------------------------------------------------
template <class GAt>
__device__ __forceinline__ void corner_addends(const Warp &p, int h, int w, double un, GAt G_at, long long &su,
                                               long long &sv)
{
    double G[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int xx = p.cx + i, yy = p.cy + j;
            const bool in = xx >= 0 && xx < w && yy >= 0 && yy < h;
            G[j][i] = in ? G_at((size_t)yy * w + (size_t)xx) : 0.0;
        }
    }
    const double gx = (double)p.wy[0] * (G[0][1] - G[0][0]) + (double)p.wy[1] * (G[1][1] - G[1][0]);
    const double gy = (double)p.wx[0] * (G[1][0] - G[0][0]) + (double)p.wx[1] * (G[1][1] - G[0][1]);
    const double ms = -(double)p.tau;  // p.tau holds sig; d xw / d u = -sig
    su += (long long)(ms * gx * un);
    sv += (long long)(ms * gy * un);
}

}  // namespace
