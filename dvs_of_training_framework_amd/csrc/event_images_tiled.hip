// The splat into the images of warped events (event_images.h) by a second
// schedule, for dense frames (include/dvsof_event_images_tiled.h,
// docs/IWE_SPEC.md section 22): the same images, the same bytes.
//
// The kernels of iwe.hip and contrast.hip issue up to four 64-bit integer
// atomics per (event, reference) straight into global memory, where almost
// every pixel collides.  Here the collisions are met in LDS:
//
//   pass 1, bucket   one thread per event, by the frame rule of the caller
//                    (a template parameter: position in the columns for the
//                    metric, sample and time window for the term, in either
//                    form of the columns).  Per (event, frame) the channel,
//                    tau, one read of the flow and the count atomics, exactly
//                    as splat_event; per reference warp_event_to, and for a
//                    survivor ONE 32-bit atomic on the cursor of the tile that
//                    holds (max(cx, 0), max(cy, 0)) and a 12-byte record: the
//                    corner relative to the tile and the bits of fx and fy.
//                    A reservation past the bucket's capacity writes nothing:
//                    the thread calls splat_corners itself.
//   pass 2, tile     one workgroup per tile; (kTileW + 1) x (kTileH + 1)
//                    64-bit sums in LDS, the extra column and row for the
//                    right and bottom corners of footprints on the seam.  It
//                    streams its records (three coalesced word columns),
//                    rebuilds the weights and the units by corner_weights and
//                    corner_units of frame_common.h -- the code warp_event_to
//                    and splat_corners run -- and adds with LDS atomics; then
//                    every nonzero sum inside the image goes to q by one
//                    global atomic add (the halo belongs to a neighbour's
//                    pixels, and overflowed records are already in q).
//
// All sums are integers, so neither the order of the records nor which path a
// record took can be seen in the bytes.  This file relies on -ffp-contract=off.
#include "event_columns.h"
#include "event_images_tiled.h"
#include "../../include/dvsof_event_images_tiled.h"

namespace {

constexpr int NT = kFrameNT;
constexpr int kAccW = kTileW + 1, kAccH = kTileH + 1;
static_assert(kTileW <= 0x7fff && kTileH <= 0x7fff, "a record's corner is two 16-bit fields");

struct Buckets {
    uint32_t *cursor;  // [tiles * kCursorStride], the first word of every line
    uint32_t *rec;     // [tiles][3][cap]
    int TX, TY, cap;
};

Buckets bind(const TilePlan &tp, void *workspace)
{
    return Buckets{(uint32_t *)workspace, (uint32_t *)((char *)workspace + tile_cursor_bytes(tp)), tp.TX, tp.TY,
                   tp.cap};
}

// splat_event with the corners put off: the counts as there, per surviving reference a record
// in the bucket of its tile, or the corners themselves where the bucket is full
template <int R, bool POL>
__device__ __forceinline__ void bucket_event(const Buckets &bk, const Refs &refs, int f, int c, float tau, float u,
                                             float v, int64_t xi, int64_t yi, size_t pix, size_t plane, int h, int w,
                                             unsigned long long *__restrict__ q, uint32_t *__restrict__ count)
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t m = image_of<R, POL>(f, r, c);
        atomicAdd(count + m * plane + pix, 1u);
        Warp p;
        if (!warp_event_to(tau, refs.rho[r], u, v, xi, yi, h, w, p)) continue;
        const int tx = max(p.cx, 0) / kTileW, ty = max(p.cy, 0) / kTileH;  // cx <= w - 1: tx < TX
        const size_t tile = (m * bk.TY + ty) * bk.TX + tx;
        const uint32_t slot = atomicAdd(bk.cursor + tile * kCursorStride, 1u);
        if (slot < (uint32_t)bk.cap) {
            uint32_t *rec = bk.rec + tile * 3 * bk.cap + slot;
            // the corner relative to the tile, + 1: -1 at the image's left and top edge
            rec[0] = (uint32_t)(p.cx - tx * kTileW + 1) | (uint32_t)(p.cy - ty * kTileH + 1) << 16;
            rec[bk.cap] = __float_as_uint(p.wx[1]);
            rec[2 * bk.cap] = __float_as_uint(p.wy[1]);
        } else {
            splat_corners(p, h, w, q + m * plane);
        }
    }
}

// Pass 1 by the metric's frame rule: iwe_splat_kernel with bucket_event for splat_event
template <int R, bool POL>
__global__ __launch_bounds__(NT) void bucket_frames_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t,
    const int64_t *__restrict__ pol, int64_t n, const int64_t *__restrict__ begin, const float *__restrict__ ts,
    const float *__restrict__ flow, int F, int h, int w, Refs refs, Buckets bk, unsigned long long *__restrict__ q,
    uint32_t *__restrict__ count)
{
    const size_t plane = (size_t)h * w;
    for_each_frame_event(n, begin, F, [=](int64_t e, int f) {
        const int64_t xi = x[e], yi = y[e];
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) return;  // the -1 slots of cropped and padded events
        int c;
        if (!event_channel<POL>(pol, e, c)) return;
        const size_t pix = (size_t)yi * w + (size_t)xi;
        const float tau = event_tau(t[e], ts[2 * f], ts[2 * f + 1]);
        const float *fl = flow + (size_t)f * 2 * plane + pix;
        const float u = fl[0], v = fl[plane];
        bucket_event<R, POL>(bk, refs, f, c, tau, u, v, xi, yi, pix, plane, h, w, q, count);
    });
}

// Pass 1 by the term's frame rule: contrast_splat_kernel with bucket_event for splat_event
template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void bucket_windows_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts, const int64_t *__restrict__ frame_sample,
    const float *__restrict__ flow, int F, int h, int w, Refs refs, Buckets bk, unsigned long long *__restrict__ q,
    uint32_t *__restrict__ count)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    const size_t plane = (size_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const EventRow ev = cols.template load<POL>(e);
        const int64_t xi = ev.x, yi = ev.y;
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;  // the -1 slots of cropped and padded events
        int c;
        if (!event_channel<POL>(ev.sign, c)) continue;
        const float te = ev.t;
        const int64_t s = ev.sample;
        const size_t pix = (size_t)yi * w + (size_t)xi;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != s) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;  // a test, not a clamp; false for a NaN
            const float tau = event_tau(te, t0, t1);
            const float *fl = flow + (size_t)f * 2 * plane + pix;
            const float u = fl[0], v = fl[plane];
            bucket_event<R, POL>(bk, refs, f, c, tau, u, v, xi, yi, pix, plane, h, w, q, count);
        }
    }
}

// Pass 2: workgroup = tile
__global__ __launch_bounds__(NT) void tile_sum_kernel(Buckets bk, int h, int w, unsigned long long *__restrict__ q)
{
    const size_t tile = blockIdx.x;
    const uint32_t n = min(bk.cursor[tile * kCursorStride], (uint32_t)bk.cap);
    if (n == 0) return;
    __shared__ unsigned long long acc[kAccH * kAccW];
    for (int k = threadIdx.x; k < kAccH * kAccW; k += NT) acc[k] = 0;
    __syncthreads();
    const int per_image = bk.TX * bk.TY, in_image = (int)(tile % per_image);
    const int x0 = in_image % bk.TX * kTileW, y0 = in_image / bk.TX * kTileH;
    const uint32_t *rec = bk.rec + tile * 3 * bk.cap;
    for (uint32_t k = threadIdx.x; k < n; k += NT) {
        const uint32_t corner = rec[k];
        const float fx = __uint_as_float(rec[bk.cap + k]), fy = __uint_as_float(rec[2 * bk.cap + k]);
        const int lx = (int)(corner & 0xffffu) - 1, ly = (int)(corner >> 16) - 1;  // in [-1, side - 1]
        float wx[2], wy[2];
        corner_weights(fx, fy, wx, wy);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ax = lx + i, ay = ly + j;  // in [-1, side]; -1 only outside the image
                const int xx = x0 + ax, yy = y0 + ay;
                if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
                const int64_t Q = corner_units(wy[j], wx[i]);
                if (Q > 0) atomicAdd(acc + ay * kAccW + ax, (unsigned long long)Q);
            }
        }
    }
    __syncthreads();
    unsigned long long *img = q + tile / per_image * ((size_t)h * w);
    for (int k = threadIdx.x; k < kAccH * kAccW; k += NT) {
        const int xx = x0 + k % kAccW, yy = y0 + k / kAccW;
        const unsigned long long a = acc[k];
        if (a != 0 && xx < w && yy < h) atomicAdd(img + (size_t)yy * w + (size_t)xx, a);
    }
}

int tile_pass(const Buckets &bk, const TilePlan &tp, int h, int w, int64_t *q, hipStream_t st)
{
    hipLaunchKernelGGL(tile_sum_kernel, dim3((unsigned)tp.tiles), dim3(NT), 0, st, bk, h, w,
                       (unsigned long long *)q);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

// both passes of the term's splat on one form of the columns
template <class Cols>
int term_splat(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
               const float *flow, int F, int h, int w, const Plan &pl, const TilePlan &tp, int64_t *q,
               uint32_t *count, void *tile_workspace, hipStream_t st)
{
    const Buckets bk = bind(tp, tile_workspace);
    DVSOF_HIP_TRY((hipError_t)fill_u32(bk.cursor, 0u, tile_cursor_bytes(tp), st));
    DVSOF_REFS_POL_DISPATCH(bucket_windows_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols, n_events,
                            frame_ts, frame_sample, flow, F, h, w, pl.refs, bk, (unsigned long long *)q, count);
    DVSOF_LAUNCH_CHECK();
    return tile_pass(bk, tp, h, w, q, st);
}

}  // namespace

int event_images_tiled_term_splat(const TiledTermColumns &c, int64_t n_events, const float *frame_ts,
                                  const int64_t *frame_sample, const float *flow, int F, int h, int w,
                                  int reference_mask, int polarity, const TilePlan &tp, int64_t *q, uint32_t *count,
                                  void *tile_workspace, hipStream_t stream)
{
    Plan pl;
    if (!plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (c.encoded)
        return term_splat(EncodedColumns{(const int16_t *)c.x, (const int16_t *)c.y, c.t, (const uint8_t *)c.pol,
                                         c.sample, c.B},
                          n_events, frame_ts, frame_sample, flow, F, h, w, pl, tp, q, count, tile_workspace, stream);
    return term_splat(WireColumns{(const int64_t *)c.x, (const int64_t *)c.y, c.t, (const int64_t *)c.pol, c.sample},
                      n_events, frame_ts, frame_sample, flow, F, h, w, pl, tp, q, count, tile_workspace, stream);
}

extern "C" {

int dvsof_event_images_tiled_plan(int F, int reference_mask, int polarity, int h, int w, int64_t n_events,
                                  int32_t *out)
{
    TilePlan tp;
    if (!out || !tile_plan(F, reference_mask, polarity, h, w, n_events, tp)) return 0;
    out[0] = kTileW;
    out[1] = kTileH;
    out[2] = tp.tiles;
    out[3] = tp.cap;
    return 1;
}

size_t dvsof_event_images_tiled_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                int64_t n_events)
{
    TilePlan tp;
    return tile_plan(F, reference_mask, polarity, h, w, n_events, tp) ? tile_workspace_bytes(tp) : 0;
}

int dvsof_iwe_splat_multi_tiled(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                int64_t n_events, const int64_t *frame_event_begin, const float *frame_ts,
                                const float *flow, int F, int h, int w, int reference_mask, int polarity, int64_t *q,
                                uint32_t *count, void *stream, void *tile_workspace, size_t tile_workspace_bytes,
                                int mode)
{
    if (mode != 0 && mode != 1) return DVSOF_EINVAL;
    // the twin's refusals, in the twin's order
    Plan pl;
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !count || !frame_event_begin || !frame_ts || !flow) return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || !t || (polarity && !p))) return DVSOF_EINVAL;
    TilePlan tp;
    const int tiled = tile_decide(mode, F, reference_mask, polarity, h, w, n_events, tile_workspace,
                                  tile_workspace_bytes, tp);
    if (tiled == 1)
        return dvsof_iwe_splat_multi(x, y, t, p, n_events, frame_event_begin, frame_ts, flow, F, h, w,
                                     reference_mask, polarity, q, count, stream);
    if (tiled != DVSOF_OK) return tiled;
    hipStream_t st = as_stream(stream);
    const size_t pixels = (size_t)pl.M * h * w;
    const Buckets bk = bind(tp, tile_workspace);
    DVSOF_HIP_TRY((hipError_t)fill_u32(q, 0u, sizeof(int64_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(count, 0u, sizeof(uint32_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(bk.cursor, 0u, tile_cursor_bytes(tp), st));
    DVSOF_REFS_POL_DISPATCH(bucket_frames_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, x, y, t, p,
                            n_events, frame_event_begin, frame_ts, flow, F, h, w, pl.refs, bk,
                            (unsigned long long *)q, count);
    DVSOF_LAUNCH_CHECK();
    return tile_pass(bk, tp, h, w, q, st);
}

}  // extern "C"
