// The splat into the average-timestamp images (avg_timestamp_images.h) by a
// second schedule, for dense frames (include/dvsof_avg_timestamp_tiled.h,
// docs/AVG_TIMESTAMP_SPEC.md section 17, docs/IWE_SPEC.md section 23): the same
// images, the same bytes.
//
// avgts_splat_event issues per (event, reference) one 32-bit and up to nine
// 64-bit integer atomics into global memory; eight of the nine are the corner
// adds into q and, at the same pixel right behind it, into s, where almost
// every pixel collides.  Here those eight are met in LDS:
//
//   pass 1, bucket   one thread per event, by the frame rule of the caller
//                    (position in the columns for the metric; sample and time
//                    window for the term, in either form of the columns).  Per
//                    (event, frame) the channel, tau and one read of the flow;
//                    per reference warp_event_to and, at the event's own pixel,
//                    the count and base atomics exactly as avgts_splat_event
//                    (global: unwarped pixels, about a fifth of the traffic).
//                    A survivor takes ONE 32-bit atomic on the cursor of the
//                    tile that holds (max(cx, 0), max(cy, 0)) and writes a
//                    16-byte record: the corner relative to the tile and the
//                    bits of fx, fy and a = |sig|.  A reservation past the
//                    bucket's capacity writes nothing: the thread calls
//                    avgts_splat_corners itself.
//   pass 2, tile     one workgroup per tile; (kTileW + 1) x (kTileH + 1) PAIRS
//                    of 64-bit sums in LDS, {q, s} of a pixel side by side in
//                    16 bytes: the two adds of a corner share one address
//                    register (the second is the first at offset:8), the
//                    zeroing is one ds_write_b128 and the flush one
//                    ds_read_b128 per pixel.  It streams its records (four
//                    coalesced word columns), rebuilds the weights by
//                    corner_weights and the units by avgts_corner_units -- the
//                    code avgts_splat_corners runs -- and adds with LDS
//                    atomics; then every pixel inside the image with a nonzero
//                    q sum adds it to q by one global atomic, and its s sum
//                    where that is nonzero (QA <= Q: s is only nonzero where q
//                    is).  The halo belongs to a neighbour's pixels, and
//                    overflowed records are already in q and s.
//
// All sums are integers, so neither the order of the records nor which path a
// record took can be seen in the bytes.  Not here: bucketing count and base by
// the event's own tile, an LDS histogram for the reservations, the pyramid
// splats, the captured step.  This file relies on -ffp-contract=off.
#include "event_columns.h"
#include "avg_timestamp_images.h"
#include "avg_timestamp_tiled.h"
#include "../../include/dvsof_avg_timestamp_tiled.h"

namespace {

constexpr int NT = kFrameNT;
constexpr int kAccW = kTileW + 1, kAccH = kTileH + 1;
constexpr int kCols = kAvgtsRecordBytes / 4;
static_assert(kTileW <= 0x7fff && kTileH <= 0x7fff, "a record's corner is two 16-bit fields");
static_assert(kAccW * kAccH * 16 <= 18 * 1024, "two planes of sums: 17.3 KiB, occupancy stays bound by waves");

struct Buckets {
    uint32_t *cursor;  // [tiles * kCursorStride], the first word of every line
    uint32_t *rec;     // [tiles][kCols][cap]
    int TX, TY, cap;
};

Buckets bind(const TilePlan &tp, void *workspace)
{
    return Buckets{(uint32_t *)workspace, (uint32_t *)((char *)workspace + tile_cursor_bytes(tp)), tp.TX, tp.TY,
                   tp.cap};
}

struct Images {
    unsigned long long *q, *s, *base;
    uint32_t *count;
};

Images unsigned_of(const AvgtsImages &i)
{
    return Images{(unsigned long long *)i.q, (unsigned long long *)i.s, (unsigned long long *)i.base, i.count};
}

// avgts_splat_event with the corners put off: count and base as there, per surviving reference
// a record in the bucket of its tile, or the corners themselves where the bucket is full
template <int R, bool POL>
__device__ __forceinline__ void bucket_event(const Buckets &bk, const Refs &refs, int f, int c, float tau, float u,
                                             float v, int64_t xi, int64_t yi, size_t pix, size_t plane, int h, int w,
                                             const Images &im)
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t m = image_of<R, POL>(f, r, c);
        Warp p;
        const bool inside = warp_event_to(tau, refs.rho[r], u, v, xi, yi, h, w, p);
        const float a = fabsf(p.tau);  // p.tau holds sig, set before the inside test; 0 <= a <= 1
        atomicAdd(im.count + m * plane + pix, 1u);
        const int64_t B = (int64_t)(a * kOne);  // exact; 0 <= B <= 2^32
        if (B > 0) atomicAdd(im.base + m * plane + pix, (unsigned long long)B);
        if (!inside) continue;
        const int tx = max(p.cx, 0) / kTileW, ty = max(p.cy, 0) / kTileH;  // cx <= w - 1: tx < TX
        const size_t tile = (m * bk.TY + ty) * bk.TX + tx;
        const uint32_t slot = atomicAdd(bk.cursor + tile * kCursorStride, 1u);
        if (slot < (uint32_t)bk.cap) {
            uint32_t *rec = bk.rec + tile * kCols * bk.cap + slot;
            // the corner relative to the tile, + 1: -1 at the image's left and top edge
            rec[0] = (uint32_t)(p.cx - tx * kTileW + 1) | (uint32_t)(p.cy - ty * kTileH + 1) << 16;
            rec[bk.cap] = __float_as_uint(p.wx[1]);
            rec[2 * bk.cap] = __float_as_uint(p.wy[1]);
            rec[3 * bk.cap] = __float_as_uint(a);
        } else {
            avgts_splat_corners(p, a, h, w, im.q + m * plane, im.s + m * plane);
        }
    }
}

// Pass 1 by the metric's frame rule: iwe_avgts_splat_kernel with bucket_event for avgts_splat_event
template <int R, bool POL>
__global__ __launch_bounds__(NT) void avgts_bucket_frames_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t,
    const int64_t *__restrict__ pol, int64_t n, const int64_t *__restrict__ begin, const float *__restrict__ ts,
    const float *__restrict__ flow, int F, int h, int w, Refs refs, Buckets bk, Images im)
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
        bucket_event<R, POL>(bk, refs, f, c, tau, u, v, xi, yi, pix, plane, h, w, im);
    });
}

// Pass 1 by the term's frame rule: avgts_splat_kernel with bucket_event for avgts_splat_event
template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void avgts_bucket_windows_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts, const int64_t *__restrict__ frame_sample,
    const float *__restrict__ flow, int F, int h, int w, Refs refs, Buckets bk, Images im)
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
        const int64_t smp = ev.sample;
        const size_t pix = (size_t)yi * w + (size_t)xi;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != smp) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;  // a test, not a clamp; false for a NaN
            const float tau = event_tau(te, t0, t1);
            const float *fl = flow + (size_t)f * 2 * plane + pix;
            const float u = fl[0], v = fl[plane];
            bucket_event<R, POL>(bk, refs, f, c, tau, u, v, xi, yi, pix, plane, h, w, im);
        }
    }
}

// Pass 2: workgroup = tile; acc[k].x the q sum, acc[k].y the s sum of accumulator pixel k
__global__ __launch_bounds__(NT) void avgts_tile_sum_kernel(Buckets bk, int h, int w,
                                                            unsigned long long *__restrict__ q,
                                                            unsigned long long *__restrict__ s)
{
    const size_t tile = blockIdx.x;
    const uint32_t n = min(bk.cursor[tile * kCursorStride], (uint32_t)bk.cap);
    if (n == 0) return;
    __shared__ ulonglong2 acc[kAccH * kAccW];
    for (int k = threadIdx.x; k < kAccH * kAccW; k += NT) acc[k] = make_ulonglong2(0, 0);
    __syncthreads();
    const int per_image = bk.TX * bk.TY, in_image = (int)(tile % per_image);
    const int x0 = in_image % bk.TX * kTileW, y0 = in_image / bk.TX * kTileH;
    const uint32_t *rec = bk.rec + tile * kCols * bk.cap;
    for (uint32_t k = threadIdx.x; k < n; k += NT) {
        const uint32_t corner = rec[k];
        const float fx = __uint_as_float(rec[bk.cap + k]), fy = __uint_as_float(rec[2 * bk.cap + k]);
        const float a = __uint_as_float(rec[3 * bk.cap + k]);
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
                int64_t Q, QA;
                avgts_corner_units(wy[j], wx[i], a, Q, QA);
                ulonglong2 *at = acc + ay * kAccW + ax;
                if (Q > 0) atomicAdd(&at->x, (unsigned long long)Q);
                if (QA > 0) atomicAdd(&at->y, (unsigned long long)QA);
            }
        }
    }
    __syncthreads();
    const size_t image = tile / per_image * ((size_t)h * w);
    for (int k = threadIdx.x; k < kAccH * kAccW; k += NT) {
        const int xx = x0 + k % kAccW, yy = y0 + k / kAccW;
        const ulonglong2 sum = acc[k];
        if (sum.x == 0 || xx >= w || yy >= h) continue;
        const size_t at = image + (size_t)yy * w + (size_t)xx;
        atomicAdd(q + at, sum.x);
        if (sum.y != 0) atomicAdd(s + at, sum.y);
    }
}

// the cursors cleared, then pass 1 by `bucket` and pass 2
template <class Bucket>
int both_passes(const TilePlan &tp, void *tile_workspace, int h, int w, const Images &im, hipStream_t st,
                Bucket bucket)
{
    const Buckets bk = bind(tp, tile_workspace);
    DVSOF_HIP_TRY((hipError_t)fill_u32(bk.cursor, 0u, tile_cursor_bytes(tp), st));
    bucket(bk);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(avgts_tile_sum_kernel, dim3((unsigned)tp.tiles), dim3(NT), 0, st, bk, h, w, im.q, im.s);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

template <class Cols>
int term_splat(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
               const float *flow, int F, int h, int w, const Plan &pl, const TilePlan &tp, const Images &im,
               void *tile_workspace, hipStream_t st)
{
    return both_passes(tp, tile_workspace, h, w, im, st, [&](const Buckets &bk) {
        DVSOF_REFS_POL_DISPATCH(avgts_bucket_windows_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, flow, F, h, w, pl.refs, bk, im);
    });
}

}  // namespace

int avg_timestamp_tiled_term_splat(const TiledTermColumns &c, int64_t n_events, const float *frame_ts,
                                   const int64_t *frame_sample, const float *flow, int F, int h, int w,
                                   int reference_mask, int polarity, const TilePlan &tp, const AvgtsImages &img,
                                   void *tile_workspace, hipStream_t stream)
{
    Plan pl;
    if (!plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    const Images im = unsigned_of(img);
    if (c.encoded)
        return term_splat(EncodedColumns{(const int16_t *)c.x, (const int16_t *)c.y, c.t, (const uint8_t *)c.pol,
                                         c.sample, c.B},
                          n_events, frame_ts, frame_sample, flow, F, h, w, pl, tp, im, tile_workspace, stream);
    return term_splat(WireColumns{(const int64_t *)c.x, (const int64_t *)c.y, c.t, (const int64_t *)c.pol, c.sample},
                      n_events, frame_ts, frame_sample, flow, F, h, w, pl, tp, im, tile_workspace, stream);
}

int avg_timestamp_tiled_frames_splat(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                     int64_t n_events, const int64_t *frame_event_begin, const float *frame_ts,
                                     const float *flow, int F, int h, int w, int reference_mask, int polarity,
                                     const TilePlan &tp, const AvgtsImages &img, void *tile_workspace,
                                     hipStream_t stream)
{
    Plan pl;
    if (!plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    const Images im = unsigned_of(img);
    return both_passes(tp, tile_workspace, h, w, im, stream, [&](const Buckets &bk) {
        DVSOF_REFS_POL_DISPATCH(avgts_bucket_frames_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, stream, x,
                                y, t, p, n_events, frame_event_begin, frame_ts, flow, F, h, w, pl.refs, bk, im);
    });
}

extern "C" {

size_t dvsof_avg_timestamp_tiled_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                 int64_t n_events)
{
    TilePlan tp;
    return tile_plan(F, reference_mask, polarity, h, w, n_events, tp) ? tile_workspace_bytes(tp, kAvgtsRecordBytes)
                                                                      : 0;
}

}  // extern "C"
