// The splat into the images of warped events (event_images.h) and into the
// average-timestamp images (avg_timestamp_images.h) by a second schedule, for
// dense frames (include/dvsof_event_images_tiled.h,
// include/dvsof_avg_timestamp_tiled.h; docs/IWE_SPEC.md sections 22-23,
// docs/AVG_TIMESTAMP_SPEC.md section 17): the same images, the same bytes.
//
// The one-thread-per-event kernels of iwe.hip, contrast.hip and
// avg_timestamp.hip issue their corner adds straight into global memory, where
// almost every pixel collides: up to four 64-bit integer atomics per (event,
// reference) into q, and for the average-timestamp images four more into s at
// the same pixel right behind it.  Here those collisions are met in LDS:
//
//   pass 1, bucket   one thread per event, by the frame rule of the caller
//                    (position in the columns for the metric; sample and time
//                    window for the term, in either form of the columns).  Per
//                    (event, frame) the channel, tau and one read of the flow;
//                    per reference warp_event_to and, at the event's own pixel,
//                    the family's atomics exactly as splat_event (count) or
//                    avgts_splat_event (count and base; global: unwarped
//                    pixels, about a fifth of that family's traffic).  A
//                    survivor takes ONE 32-bit atomic on the cursor of the tile
//                    that holds (max(cx, 0), max(cy, 0)) and writes a record:
//                    the corner relative to the tile and the bits of fx and fy
//                    (12 bytes), for the average-timestamp images those of
//                    a = |sig| too (16 bytes).  A reservation past the bucket's
//                    capacity writes nothing: the thread calls splat_corners or
//                    avgts_splat_corners itself.
//   pass 2, tile     one workgroup per tile; (kTileW + 1) x (kTileH + 1)
//                    accumulators in LDS, the extra column and row for the
//                    right and bottom corners of footprints on the seam.  An
//                    accumulator is a 64-bit sum, or for the average-timestamp
//                    images a PAIR, {q, s} of a pixel side by side in 16 bytes:
//                    the two adds of a corner share one address register (the
//                    second is the first at offset:8), the zeroing is one
//                    ds_write_b128 and the flush one ds_read_b128 per pixel.
//                    It streams its records (coalesced word columns), rebuilds
//                    the weights by corner_weights and the units by
//                    corner_units or avgts_corner_units -- the code
//                    splat_corners and avgts_splat_corners run -- and adds with
//                    LDS atomics; then every pixel inside the image with a
//                    nonzero q sum adds it to q by one global atomic, and its s
//                    sum where that is nonzero (QA <= Q: s is only nonzero
//                    where q is).  The halo belongs to a neighbour's pixels,
//                    and overflowed records are already in the images.
//
// All sums are integers, so neither the order of the records nor which path a
// record took can be seen in the bytes.  The schedule is written once; a family
// of images (Family below) supplies what an event adds at its own pixel, its
// record's last column, its accumulator and its flush, all resolved at compile
// time.  Not here: bucketing count and base by the event's own tile, an LDS
// histogram for the reservations, the pyramid splats, the captured step.  This
// file relies on -ffp-contract=off.
#include "avg_timestamp_images.h"
#include "tiled_splat.h"
#include "../../include/dvsof_event_images_tiled.h"
#include "../../include/dvsof_avg_timestamp_tiled.h"

namespace {

constexpr int NT = kFrameNT;
constexpr int kAccW = kTileW + 1, kAccH = kTileH + 1;
static_assert(kTileW <= 0x7fff && kTileH <= 0x7fff, "a record's corner is two 16-bit fields");

// ---------------------------------------------------------------------------
// The two families.  kCols: the word columns of a record; own_pixel: the adds
// of an event at its own pixel `at` of its image (a = |sig|); overflowed: the
// corners of a record past the bucket's capacity, into the image at `image`; Acc,
// zero, add: an accumulator of LDS and what a corner of weights wy, wx adds to
// it; flush: an accumulator's sums to pixel `at` of the images.
// ---------------------------------------------------------------------------
template <class Images>
struct Family;

template <>
struct Family<EventImages> {
    static constexpr int kCols = EventImages::kRecordBytes / 4;
    unsigned long long *q;
    uint32_t *count;
    explicit Family(const EventImages &i) : q((unsigned long long *)i.q), count(i.count) {}

    __device__ __forceinline__ void own_pixel(size_t at, float) const { atomicAdd(count + at, 1u); }
    __device__ __forceinline__ void overflowed(const Warp &p, float, int h, int w, size_t image) const
    {
        splat_corners(p, h, w, q + image);
    }

    using Acc = unsigned long long;
    static __device__ __forceinline__ Acc zero() { return 0; }
    static __device__ __forceinline__ void add(Acc *at, float wy, float wx, float)
    {
        const int64_t Q = corner_units(wy, wx);
        if (Q > 0) atomicAdd(at, (unsigned long long)Q);
    }
    __device__ __forceinline__ void flush(const Acc &sum, size_t at) const
    {
        if (sum != 0) atomicAdd(q + at, sum);
    }
};

template <>
struct Family<AvgtsImages> {
    static constexpr int kCols = AvgtsImages::kRecordBytes / 4;
    unsigned long long *q, *s, *base;
    uint32_t *count;
    explicit Family(const AvgtsImages &i)
        : q((unsigned long long *)i.q), s((unsigned long long *)i.s), base((unsigned long long *)i.base),
          count(i.count)
    {
    }

    __device__ __forceinline__ void own_pixel(size_t at, float a) const
    {
        atomicAdd(count + at, 1u);
        const int64_t B = (int64_t)(a * kOne);  // exact; 0 <= B <= 2^32
        if (B > 0) atomicAdd(base + at, (unsigned long long)B);
    }
    __device__ __forceinline__ void overflowed(const Warp &p, float a, int h, int w, size_t image) const
    {
        avgts_splat_corners(p, a, h, w, q + image, s + image);
    }

    using Acc = ulonglong2;  // .x the q sum, .y the s sum of an accumulator pixel
    static __device__ __forceinline__ Acc zero() { return make_ulonglong2(0, 0); }
    static __device__ __forceinline__ void add(Acc *at, float wy, float wx, float a)
    {
        int64_t Q, QA;
        avgts_corner_units(wy, wx, a, Q, QA);
        if (Q > 0) atomicAdd(&at->x, (unsigned long long)Q);
        if (QA > 0) atomicAdd(&at->y, (unsigned long long)QA);
    }
    __device__ __forceinline__ void flush(const Acc &sum, size_t at) const
    {
        if (sum.x == 0) return;
        atomicAdd(q + at, sum.x);
        if (sum.y != 0) atomicAdd(s + at, sum.y);
    }
};
static_assert(kAccW * kAccH * sizeof(Family<AvgtsImages>::Acc) <= 18 * 1024,
              "two planes of sums: 17.3 KiB, occupancy stays bound by waves");

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

// splat_event / avgts_splat_event with the corners put off: the adds at the event's own pixel as
// there, per surviving reference a record in the bucket of its tile, or the corners themselves
// where the bucket is full
template <int R, bool POL, class Fam>
__device__ __forceinline__ void bucket_event(const Buckets &bk, const Fam &fam, const Refs &refs, int f, int c,
                                             float tau, float u, float v, int64_t xi, int64_t yi, size_t pix,
                                             size_t plane, int h, int w)
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t m = image_of<R, POL>(f, r, c);
        // the bits of |p.tau| below: p.tau holds sig = tau - rho; 0 <= a <= 1.  The adds at the event's
        // own pixel go out before the warp, so that the wait for the slot does not wait for them too
        const float a = fabsf(tau - refs.rho[r]);
        fam.own_pixel(m * plane + pix, a);
        Warp p;
        if (!warp_event_to(tau, refs.rho[r], u, v, xi, yi, h, w, p)) continue;
        const int tx = max(p.cx, 0) / kTileW, ty = max(p.cy, 0) / kTileH;  // cx <= w - 1: tx < TX
        const size_t tile = (m * bk.TY + ty) * bk.TX + tx;
        const uint32_t slot = atomicAdd(bk.cursor + tile * kCursorStride, 1u);
        if (slot < (uint32_t)bk.cap) {
            uint32_t *rec = bk.rec + tile * Fam::kCols * bk.cap + slot;
            // the corner relative to the tile, + 1: -1 at the image's left and top edge
            rec[0] = (uint32_t)(p.cx - tx * kTileW + 1) | (uint32_t)(p.cy - ty * kTileH + 1) << 16;
            rec[bk.cap] = __float_as_uint(p.wx[1]);
            rec[2 * bk.cap] = __float_as_uint(p.wy[1]);
            if constexpr (Fam::kCols == 4) rec[3 * bk.cap] = __float_as_uint(a);
        } else {
            fam.overflowed(p, a, h, w, m * plane);
        }
    }
}

// Pass 1 by the metric's frame rule: iwe_splat_kernel / iwe_avgts_splat_kernel with bucket_event
// for the splat of an event
template <int R, bool POL, class Fam>
__global__ __launch_bounds__(NT) void bucket_frames_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t,
    const int64_t *__restrict__ pol, int64_t n, const int64_t *__restrict__ begin, const float *__restrict__ ts,
    const float *__restrict__ flow, int F, int h, int w, Refs refs, Buckets bk, Fam fam)
{
    const size_t plane = (size_t)h * w;
    const auto bucket = [=](int64_t xi, int64_t yi, int c, int f, float tau) {
        const size_t pix = (size_t)yi * w + (size_t)xi;
        float u, v;
        flow_at(flow, f, plane, pix, u, v);
        bucket_event<R, POL>(bk, fam, refs, f, c, tau, u, v, xi, yi, pix, plane, h, w);
    };
    for_each_position_event<POL>(x, y, t, pol, n, begin, ts, F, h, w, bucket);
}

// Pass 1 by the terms' frame rule: contrast_splat_kernel / avgts_splat_kernel likewise
template <int R, bool POL, class Fam, class Cols>
__global__ __launch_bounds__(NT) void bucket_windows_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts, const int64_t *__restrict__ frame_sample,
    const float *__restrict__ flow, int F, int h, int w, Refs refs, Buckets bk, Fam fam)
{
    const size_t plane = (size_t)h * w;
    const auto bucket = [=](int64_t xi, int64_t yi, int c, int f, float tau) {
        const size_t pix = (size_t)yi * w + (size_t)xi;
        float u, v;
        flow_at(flow, f, plane, pix, u, v);
        bucket_event<R, POL>(bk, fam, refs, f, c, tau, u, v, xi, yi, pix, plane, h, w);
    };
    for_each_window_event<POL>(cols, n, ts, frame_sample, F, h, w, bucket);
}

// Pass 2: workgroup = tile
template <class Fam>
__global__ __launch_bounds__(NT) void tile_sum_kernel(Buckets bk, int h, int w, Fam fam)
{
    using Acc = typename Fam::Acc;
    const size_t tile = blockIdx.x;
    const uint32_t n = min(bk.cursor[tile * kCursorStride], (uint32_t)bk.cap);
    if (n == 0) return;
    __shared__ Acc acc[kAccH * kAccW];
    for (int k = threadIdx.x; k < kAccH * kAccW; k += NT) acc[k] = Fam::zero();
    __syncthreads();
    const int per_image = bk.TX * bk.TY, in_image = (int)(tile % per_image);
    const int x0 = in_image % bk.TX * kTileW, y0 = in_image / bk.TX * kTileH;
    const uint32_t *rec = bk.rec + tile * Fam::kCols * bk.cap;
    for (uint32_t k = threadIdx.x; k < n; k += NT) {
        const uint32_t corner = rec[k];
        const float fx = __uint_as_float(rec[bk.cap + k]), fy = __uint_as_float(rec[2 * bk.cap + k]);
        float a = 0.f;
        if constexpr (Fam::kCols == 4) a = __uint_as_float(rec[3 * bk.cap + k]);
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
                Fam::add(acc + ay * kAccW + ax, wy[j], wx[i], a);
            }
        }
    }
    __syncthreads();
    const size_t image = tile / per_image * ((size_t)h * w);
    for (int k = threadIdx.x; k < kAccH * kAccW; k += NT) {
        const int xx = x0 + k % kAccW, yy = y0 + k / kAccW;
        if (xx < w && yy < h) fam.flush(acc[k], image + (size_t)yy * w + (size_t)xx);
    }
}

// the cursors cleared, then pass 1 by `bucket` and pass 2
template <class Fam, class Bucket>
int both_passes(const TilePlan &tp, void *tile_workspace, int h, int w, const Fam &fam, hipStream_t st, Bucket bucket)
{
    const Buckets bk = bind(tp, tile_workspace);
    DVSOF_HIP_TRY((hipError_t)fill_u32(bk.cursor, 0u, tile_cursor_bytes(tp), st));
    bucket(bk);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(tile_sum_kernel<Fam>, dim3((unsigned)tp.tiles), dim3(NT), 0, st, bk, h, w, fam);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

// both passes of a term's splat on one form of the columns
template <class Fam, class Cols>
int term_splat(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
               const float *flow, int F, int h, int w, const Plan &pl, const TilePlan &tp, const Fam &fam,
               void *tile_workspace, hipStream_t st)
{
    return both_passes(tp, tile_workspace, h, w, fam, st, [&](const Buckets &bk) {
        DVSOF_REFS_POL_DISPATCH(bucket_windows_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, flow, F, h, w, pl.refs, bk, fam);
    });
}

}  // namespace

template <class Images>
int TiledLaunch<Images>::term(const TiledTermColumns &c, int64_t n_events, const float *frame_ts,
                              const int64_t *frame_sample, const float *flow, int F, int h, int w,
                              int reference_mask, int polarity, const TilePlan &tp, const Images &img,
                              void *tile_workspace, hipStream_t stream)
{
    Plan pl;
    if (!plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    const Family<Images> fam(img);
    if (c.encoded)
        return term_splat(EncodedColumns{(const int16_t *)c.x, (const int16_t *)c.y, c.t, (const uint8_t *)c.pol,
                                         c.sample, c.B},
                          n_events, frame_ts, frame_sample, flow, F, h, w, pl, tp, fam, tile_workspace, stream);
    return term_splat(WireColumns{(const int64_t *)c.x, (const int64_t *)c.y, c.t, (const int64_t *)c.pol, c.sample},
                      n_events, frame_ts, frame_sample, flow, F, h, w, pl, tp, fam, tile_workspace, stream);
}

template <class Images>
int TiledLaunch<Images>::frames(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                int64_t n_events, const int64_t *frame_event_begin, const float *frame_ts,
                                const float *flow, int F, int h, int w, int reference_mask, int polarity,
                                const TilePlan &tp, const Images &img, void *tile_workspace, hipStream_t stream)
{
    Plan pl;
    if (!plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    const Family<Images> fam(img);
    return both_passes(tp, tile_workspace, h, w, fam, stream, [&](const Buckets &bk) {
        DVSOF_REFS_POL_DISPATCH(bucket_frames_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, stream, x, y, t,
                                p, n_events, frame_event_begin, frame_ts, flow, F, h, w, pl.refs, bk, fam);
    });
}

// the four launchers: family by frame rule
template struct TiledLaunch<EventImages>;
template struct TiledLaunch<AvgtsImages>;

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
    return tile_plan(F, reference_mask, polarity, h, w, n_events, tp) ? tile_workspace_bytes<EventImages>(tp) : 0;
}

size_t dvsof_avg_timestamp_tiled_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                 int64_t n_events)
{
    TilePlan tp;
    return tile_plan(F, reference_mask, polarity, h, w, n_events, tp) ? tile_workspace_bytes<AvgtsImages>(tp) : 0;
}

}  // extern "C"
