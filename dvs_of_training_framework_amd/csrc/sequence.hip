// Event windows of a device-resident sequence -> one wire-format batch
// (docs/SEQUENCE_SPEC.md).
//
// Replaces (reference paths): the per-frame slicing of frame_generator
// utils/data.py:139-152 and EventCrop utils/data.py:24-42 as driven by
// utils/testing.py:64-66, the collation of DummyNet/of.py:76-115, and the
// event side of DatasetImpl.__getitem__ / collate_wrapper
// utils/dataset.py:714-751, 961-1020 (stack the elements of every sample,
// subtract the first image timestamp in float64, cast to float32).
//
// One gather kernel, HBM-bound: 13 B/event in (int16 x, int16 y, float64 t,
// int8 p), 44 B/event out (five int64 columns and one float32 column).  A
// thread owns V consecutive output slots and writes every column of them with
// one vector store (V = 2: 16 B per int64 column, 8 B for the timestamp), so
// every output element below `capacity` is written exactly once: window
// events, then the padding.  No atomics, no fill launch in front.
//
// The arithmetic is pinned bit for bit by the spec: one float64 subtraction,
// one rounding to float32.
#include "common.h"

namespace {

constexpr int NT = 256;

struct Slot {
    int64_t x, y, p, s, e;
    float t;
};

// the window of output slot `slot` (< win_out[W]): the LAST k with win_out[k] <= slot, which
// skips the empty windows that share their first slot with the window behind them
__device__ __forceinline__ int find_window(const int64_t *__restrict__ win_out, int W, int64_t slot)
{
    int lo = 0, hi = W;  // win_out[lo] <= slot < win_out[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (win_out[mid] <= slot) lo = mid; else hi = mid;
    }
    return lo;
}

template <int V>
__global__ __launch_bounds__(NT) void event_windows_kernel(
    const int16_t *__restrict__ x, const int16_t *__restrict__ y, const double *__restrict__ t,
    const int8_t *__restrict__ p, int64_t n_events, const int64_t *__restrict__ win_begin,
    const int64_t *__restrict__ win_end, const int64_t *__restrict__ win_out,
    const double *__restrict__ win_origin, const int32_t *__restrict__ win_sample,
    const int32_t *__restrict__ win_element, int W, int y0, int x0, int h, int w,
    int64_t *__restrict__ x_out, int64_t *__restrict__ y_out, float *__restrict__ t_out,
    int64_t *__restrict__ p_out, int64_t *__restrict__ s_out, int64_t *__restrict__ e_out,
    int64_t n_out, int64_t capacity)
{
    const int64_t first = ((int64_t)blockIdx.x * NT + threadIdx.x) * V;
    if (first >= capacity) return;

    Slot r[V];
    int k = -1;
    int64_t k_end = 0;  // first slot behind window k
    double origin = 0.0;
    int64_t src0 = 0, src1 = 0, dst0 = 0;
    int64_t sample = 0, element = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int64_t slot = first + v;
        r[v] = Slot{-1, -1, 0, 0, 0, 0.f};  // padding, and what a malformed table leaves
        if (slot >= n_out || W < 1) continue;
        if (k < 0 || slot >= k_end) {
            // a neighbour slot is in the same window or in one of the next few: walk, do not search
            if (k < 0) k = find_window(win_out, W, slot);
            else while (k + 1 < W && win_out[k + 1] <= slot) ++k;
            dst0 = win_out[k];
            k_end = win_out[k + 1];
            src0 = win_begin[k];
            src1 = win_end[k];
            origin = win_origin[k];
            sample = win_sample[k];
            element = win_element[k];
        }
        const int64_t i = src0 + (slot - dst0);
        // the wrapper validates the table on the host; a table that is wrong all the same reads
        // nothing outside the sequence
        if (slot < dst0 || i < 0 || i >= n_events || i >= src1) continue;
        int64_t xi = x[i], yi = y[i];
        if (h > 0) {
            xi -= x0;
            yi -= y0;
            if (xi < 0 || xi >= w || yi < 0 || yi >= h) xi = yi = -1;
        }
        r[v].x = xi;
        r[v].y = yi;
        r[v].t = (float)(t[i] - origin);
        r[v].p = p[i];
        r[v].s = sample;
        r[v].e = element;
    }

    if (V == 2 && first + 1 < capacity) {
        typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
        typedef float f32x2v __attribute__((ext_vector_type(2)));
        const i64x2 vx = {r[0].x, r[V - 1].x}, vy = {r[0].y, r[V - 1].y}, vp = {r[0].p, r[V - 1].p},
                    vs = {r[0].s, r[V - 1].s}, ve = {r[0].e, r[V - 1].e};
        const f32x2v vt = {r[0].t, r[V - 1].t};
        *(i64x2 *)(x_out + first) = vx;
        *(i64x2 *)(y_out + first) = vy;
        *(f32x2v *)(t_out + first) = vt;
        *(i64x2 *)(p_out + first) = vp;
        *(i64x2 *)(s_out + first) = vs;
        *(i64x2 *)(e_out + first) = ve;
    } else {  // V == 1, or the odd last slot
        x_out[first] = r[0].x;
        y_out[first] = r[0].y;
        t_out[first] = r[0].t;
        p_out[first] = r[0].p;
        s_out[first] = r[0].s;
        e_out[first] = r[0].e;
    }
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int dvsof_event_windows(const int16_t *x, const int16_t *y, const double *t, const int8_t *p,
                                   int64_t n_events, const int64_t *win_begin, const int64_t *win_end,
                                   const int64_t *win_out, const double *win_origin,
                                   const int32_t *win_sample, const int32_t *win_element, int W, int y0,
                                   int x0, int h, int w, int64_t *x_out, int64_t *y_out, float *t_out,
                                   int64_t *polarity_out, int64_t *sample_out, int64_t *element_out,
                                   int64_t n_out, int64_t capacity, void *stream)
{
    if (n_events < 0 || W < 0 || n_out < 0 || capacity < n_out) return DVSOF_EINVAL;
    if (h < 0 || w < 0 || (h == 0) != (w == 0) || y0 < 0 || x0 < 0) return DVSOF_EINVAL;
    // int16 coordinates: a box that reaches beyond them holds no further event
    if ((long long)y0 + h > 32768 || (long long)x0 + w > 32768) return DVSOF_EINVAL;
    if (W == 0 && n_out != 0) return DVSOF_EINVAL;
    if (capacity == 0) return DVSOF_OK;
    if (!x_out || !y_out || !t_out || !polarity_out || !sample_out || !element_out) return DVSOF_EINVAL;
    if (n_out > 0 && (!win_begin || !win_end || !win_out || !win_origin || !win_sample || !win_element))
        return DVSOF_EINVAL;
    if (n_out > 0 && (n_events == 0 || !x || !y || !t || !p)) return DVSOF_EINVAL;
    if (n_out == 0) W = 0;  // padding only: the table is not read

    const bool wide = aligned(x_out, 16) && aligned(y_out, 16) && aligned(polarity_out, 16) &&
                      aligned(sample_out, 16) && aligned(element_out, 16) && aligned(t_out, 8);
    const int V = wide ? 2 : 1;
    const int64_t blocks = (capacity + (int64_t)NT * V - 1) / ((int64_t)NT * V);
    if (blocks > 0x7fffffffLL) return DVSOF_EINVAL;
    const dim3 grid((unsigned)blocks), block(NT);
    if (wide)
        hipLaunchKernelGGL(event_windows_kernel<2>, grid, block, 0, as_stream(stream), x, y, t, p, n_events,
                           win_begin, win_end, win_out, win_origin, win_sample, win_element, W, y0, x0, h,
                           w, x_out, y_out, t_out, polarity_out, sample_out, element_out, n_out, capacity);
    else
        hipLaunchKernelGGL(event_windows_kernel<1>, grid, block, 0, as_stream(stream), x, y, t, p, n_events,
                           win_begin, win_end, win_out, win_origin, win_sample, win_element, W, y0, x0, h,
                           w, x_out, y_out, t_out, polarity_out, sample_out, element_out, n_out, capacity);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}
