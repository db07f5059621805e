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
// time.  Behind the one-level passes: the same schedule over the level table of
// the terms on every flow scale (include/dvsof_event_pyramids_tiled.h), with
// tiles summed in slices, reservations agreed within a wave and the own-pixel
// sums folded from the finest level.  Not here: bucketing count and base by the
// event's own tile at one level, an LDS histogram for the reservations, the
// captured step.  This file relies on -ffp-contract=off.
#include "avg_timestamp_images.h"
#include "tiled_splat.h"
#include "../../include/dvsof_event_images_tiled.h"
#include "../../include/dvsof_avg_timestamp_tiled.h"
#include "../../include/dvsof_event_pyramids_tiled.h"

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

// ---------------------------------------------------------------------------
// The schedule over a level table (the terms on every flow scale).  Three
// things differ from the one-level passes above.  A coarse level has few
// tiles and huge buckets, so pass 2 sums a tile in slices of kSlice records,
// one workgroup each; integer sums let any number of workgroups flush the same
// pixel.  Almost every lane of a wave reserves in the same one or two tiles
// there, so the lanes that are active together agree on one cursor atomic per
// distinct tile.  And the sums at the events' own pixels, which collide at a
// coarse level as the corners did, are taken at the table's finest level
// alone: which events take part and a = |tau - rho| do not depend on the level,
// so count and base of level k at (Y, X) are the sums of the source level's
// over the block (Y << d .., X << d ..), d = shift_k - shift_source, clipped at
// the source's edge -- integers, exact, count modulo 2^32 either way.
// ---------------------------------------------------------------------------
struct PyramidBuckets {
    uint32_t *cursor;  // [tiles of all levels * kCursorStride]
    uint32_t *rec;     // per level [tiles_k][kCols][cap_k], level k at record rec_base[k]
    PyramidTilePlan tp;
};

// One slot per calling lane in the bucket behind `cursor`, which is the same word for all lanes
// with the same `tile`.  The lanes that are active here together take one atomic per distinct
// tile: the first of them names its tile, those with that tile count themselves, the lowest adds
// their number and the others stand behind it by rank.  Called under divergence (the frame walk,
// a dropped warp), so every step is over the active lanes only.
__device__ __forceinline__ uint32_t reserve_agreed(uint32_t *cursor, int tile)
{
    const unsigned lane = __lane_id();
    uint32_t slot = 0;
    for (bool done = false; !done;) {
        if (tile == __builtin_amdgcn_readfirstlane(tile)) {
            const unsigned long long peers = __ballot(1);
            const unsigned rank = __popcll(peers & ((1ull << lane) - 1ull));
            uint32_t first = 0;
            if (rank == 0) first = atomicAdd(cursor, (uint32_t)__popcll(peers));
            slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)first) + rank;  // the first active lane has rank 0
            done = true;
        }
    }
    return slot;
}

// bucket_event at level k of the table: the own-pixel adds at the source level only, the record
// into the bucket of the level's destination tile
template <int R, bool POL, class Fam>
__device__ __forceinline__ void bucket_level_event(const PyramidBuckets &bk, int k, const Level &L, const Fam &fam,
                                                   const Refs &refs, int f, int c, float tau, int64_t xi, int64_t yi)
{
    const int64_t xs = xi >> L.shift, ys = yi >> L.shift;  // xs <= (w - 1) >> s <= L.w - 1
    const size_t plane = (size_t)L.h * L.w;
    const size_t pix = (size_t)ys * L.w + (size_t)xs;
    float u, v;
    flow_at(L.flow, f, plane, pix, u, v);
    const int TX = bk.tp.TX[k], TY = bk.tp.TY[k], cap = bk.tp.cap[k];
    const bool agree = TX * TY <= kAggregateTiles;  // the same for the whole wave
    const bool own = k == bk.tp.source;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t m = image_of<R, POL>(f, r, c);
        const float a = fabsf(tau - refs.rho[r]);
        if (own) fam.own_pixel(L.image_offset + m * plane + pix, a);
        Warp p;
        if (!warp_event_to(tau, refs.rho[r], u, v, xs, ys, L.h, L.w, p)) continue;
        const int tx = max(p.cx, 0) / kTileW, ty = max(p.cy, 0) / kTileH;
        const int in_level = ((int)m * TY + ty) * TX + tx;  // below tiles[k] <= 8192
        const int tile = bk.tp.tile_base[k] + in_level;
        uint32_t *cursor = bk.cursor + (size_t)tile * kCursorStride;
        const uint32_t slot = agree ? reserve_agreed(cursor, tile) : atomicAdd(cursor, 1u);
        if (slot < (uint32_t)cap) {
            uint32_t *rec = bk.rec + (bk.tp.rec_base[k] + (size_t)in_level * cap) * Fam::kCols + slot;
            rec[0] = (uint32_t)(p.cx - tx * kTileW + 1) | (uint32_t)(p.cy - ty * kTileH + 1) << 16;
            rec[cap] = __float_as_uint(p.wx[1]);
            rec[2 * cap] = __float_as_uint(p.wy[1]);
            if constexpr (Fam::kCols == 4) rec[3 * cap] = __float_as_uint(a);
        } else {
            fam.overflowed(p, a, L.h, L.w, L.image_offset + m * plane);
        }
    }
}

// Pass 1 over the table: one walk by the terms' frame rule, the levels a loop inside it
template <int R, bool POL, class Fam, class Cols>
__global__ __launch_bounds__(NT) void bucket_pyramid_kernel(const Cols cols, int64_t n, const float *__restrict__ ts,
                                                            const int64_t *__restrict__ frame_sample, int F, int h,
                                                            int w, Refs refs, const Levels lv,
                                                            const PyramidBuckets bk, Fam fam)
{
    const auto bucket = [=, &lv, &bk](int64_t xi, int64_t yi, int c, int f, float tau) {
#pragma unroll 1
        for (int k = 0; k < lv.K; ++k) bucket_level_event<R, POL>(bk, k, lv.level[k], fam, refs, f, c, tau, xi, yi);
    };
    for_each_window_event<POL>(cols, n, ts, frame_sample, F, h, w, bucket);
}

// Pass 2 over the table: workgroup = (level, tile, slice of kSlice records), tile_sum_kernel on
// its slice.  A slice past the cursor has nothing to do.
template <class Fam>
__global__ __launch_bounds__(NT) void slice_sum_kernel(const PyramidBuckets bk, const Levels lv, Fam fam)
{
    using Acc = typename Fam::Acc;
    int k = 0;
    while (k + 1 < bk.tp.K && (int)blockIdx.x >= bk.tp.block_base[k + 1]) ++k;
    const int slices = bk.tp.slices[k], cap = bk.tp.cap[k], TX = bk.tp.TX[k], TY = bk.tp.TY[k];
    const int local = (int)blockIdx.x - bk.tp.block_base[k];
    const int in_level = local / slices;
    const uint32_t n = min(bk.cursor[(size_t)(bk.tp.tile_base[k] + in_level) * kCursorStride], (uint32_t)cap);
    const uint32_t from = (uint32_t)(local % slices) * kSlice;
    if (from >= n) return;
    const uint32_t to = min(n, from + kSlice);
    const Level &L = lv.level[k];
    const int h = L.h, w = L.w;
    __shared__ Acc acc[kAccH * kAccW];
    for (int i = threadIdx.x; i < kAccH * kAccW; i += NT) acc[i] = Fam::zero();
    __syncthreads();
    const int per_image = TX * TY, in_image = in_level % per_image;
    const int x0 = in_image % TX * kTileW, y0 = in_image / TX * kTileH;
    const uint32_t *rec = bk.rec + (bk.tp.rec_base[k] + (size_t)in_level * cap) * Fam::kCols;
    for (uint32_t e = from + threadIdx.x; e < to; e += NT) {
        const uint32_t corner = rec[e];
        const float fx = __uint_as_float(rec[cap + e]), fy = __uint_as_float(rec[2 * cap + e]);
        float a = 0.f;
        if constexpr (Fam::kCols == 4) a = __uint_as_float(rec[3 * cap + e]);
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
    const size_t image = L.image_offset + (size_t)(in_level / per_image) * ((size_t)h * w);
    for (int i = threadIdx.x; i < kAccH * kAccW; i += NT) {
        const int xx = x0 + i % kAccW, yy = y0 + i / kAccW;
        if (xx < w && yy < h) fam.flush(acc[i], image + (size_t)yy * w + (size_t)xx);
    }
}

// The fold: one thread per pixel of every image of every level but the source, which sums the
// source level's count (and base) over its block.  No atomics: nothing else writes these pixels.
template <class Fam>
__global__ __launch_bounds__(NT) void fold_own_pixels_kernel(const Levels lv, int source, size_t M, size_t total,
                                                             Fam fam)
{
    const size_t stride = (size_t)gridDim.x * NT;
    const Level &S = lv.level[source];
    const size_t src_plane = (size_t)S.h * S.w;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += stride) {
        int k = 0;
        while (k + 1 < lv.K && i >= lv.level[k + 1].image_offset) ++k;
        if (k == source) continue;
        const Level &L = lv.level[k];
        const size_t local = i - L.image_offset, plane = (size_t)L.h * L.w;
        const size_t m = local / plane, pix = local % plane;
        const int Y = (int)(pix / L.w), X = (int)(pix % L.w), d = L.shift - S.shift;
        const int y1 = min((Y + 1) << d, S.h), x1 = min((X + 1) << d, S.w);
        const size_t from = S.image_offset + m * src_plane;
        uint32_t n = 0;
        unsigned long long b = 0;
        for (int y = Y << d; y < y1; ++y) {
            for (int x = X << d; x < x1; ++x) {
                const size_t at = from + (size_t)y * S.w + (size_t)x;
                n += fam.count[at];
                if constexpr (Fam::kCols == 4) b += fam.base[at];
            }
        }
        fam.count[i] = n;
        if constexpr (Fam::kCols == 4) fam.base[i] = b;
    }
}

// the cursors cleared, pass 1, the fold and pass 2 of a term over a level table
template <class Fam, class Cols>
int pyramid_splat(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F, int h,
                  int w, const Plan &pl, const Levels &lv, const PyramidTilePlan &tp, const Fam &fam,
                  void *tile_workspace, hipStream_t st)
{
    const PyramidBuckets bk{(uint32_t *)tile_workspace,
                            (uint32_t *)((char *)tile_workspace + pyramid_cursor_bytes(tp)), tp};
    DVSOF_HIP_TRY((hipError_t)fill_u32(bk.cursor, 0u, pyramid_cursor_bytes(tp), st));
    DVSOF_REFS_POL_DISPATCH(bucket_pyramid_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols, n_events,
                            frame_ts, frame_sample, F, h, w, pl.refs, lv, bk, fam);
    DVSOF_LAUNCH_CHECK();
    if (lv.K > 1) {
        const Level &last = lv.level[lv.K - 1];
        const size_t total = last.image_offset + (size_t)pl.M * last.h * last.w;
        hipLaunchKernelGGL(fold_own_pixels_kernel<Fam>, dim3(event_blocks((int64_t)total)), dim3(NT), 0, st, lv,
                           tp.source, (size_t)pl.M, total, fam);
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(slice_sum_kernel<Fam>, dim3((unsigned)tp.block_base[tp.K]), dim3(NT), 0, st, bk, lv, fam);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // namespace

template <class Images>
int TiledLaunch<Images>::pyramid(const TiledTermColumns &c, int64_t n_events, const float *frame_ts,
                                 const int64_t *frame_sample, int F, int h, int w, int reference_mask, int polarity,
                                 const dvsof_contrast_levels_t &levels, const PyramidTilePlan &tp, const Images &img,
                                 void *tile_workspace, hipStream_t stream)
{
    Plan pl;
    if (!plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    const Family<Images> fam(img);
    if (c.encoded)
        return pyramid_splat(EncodedColumns{(const int16_t *)c.x, (const int16_t *)c.y, c.t, (const uint8_t *)c.pol,
                                            c.sample, c.B},
                             n_events, frame_ts, frame_sample, F, h, w, pl, levels, tp, fam, tile_workspace, stream);
    return pyramid_splat(WireColumns{(const int64_t *)c.x, (const int64_t *)c.y, c.t, (const int64_t *)c.pol,
                                     c.sample},
                         n_events, frame_ts, frame_sample, F, h, w, pl, levels, tp, fam, tile_workspace, stream);
}

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

// include/dvsof_event_pyramids_tiled.h: the plan over a level table
int dvsof_event_pyramids_tiled_plan(int F, int reference_mask, int polarity, int h, int w,
                                    dvsof_contrast_levels_t levels, int64_t n_events, int32_t *out)
{
    PyramidTilePlan tp;
    if (!out || !pyramid_tile_plan(F, reference_mask, polarity, h, w, levels, n_events, tp)) return 0;
    out[0] = kTileW;
    out[1] = kTileH;
    out[2] = tp.tile_base[tp.K];
    out[3] = kSlice;
    out[4] = kAggregateTiles;
    out[5] = tp.source;
    for (int k = 0; k < tp.K; ++k) {
        out[6 + 3 * k] = tp.tiles[k];
        out[7 + 3 * k] = tp.cap[k];
        out[8 + 3 * k] = tp.slices[k];
    }
    return 1;
}

size_t dvsof_contrast_pyramid_tiled_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                    dvsof_contrast_levels_t levels, int64_t n_events)
{
    PyramidTilePlan tp;
    return pyramid_tile_plan(F, reference_mask, polarity, h, w, levels, n_events, tp)
               ? pyramid_tile_workspace_bytes<EventImages>(tp)
               : 0;
}

size_t dvsof_avg_timestamp_pyramid_tiled_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                         dvsof_contrast_levels_t levels, int64_t n_events)
{
    PyramidTilePlan tp;
    return pyramid_tile_plan(F, reference_mask, polarity, h, w, levels, n_events, tp)
               ? pyramid_tile_workspace_bytes<AvgtsImages>(tp)
               : 0;
}

}  // extern "C"
