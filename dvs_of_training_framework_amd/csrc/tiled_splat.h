// The tiled schedule of the splat (tiled_splat.hip) into the two families of
// images: those of warped events of event_images.h
// (include/dvsof_event_images_tiled.h) and the average-timestamp images of
// avg_timestamp_images.h (include/dvsof_avg_timestamp_tiled.h).  What the
// entry points share that run it: contrast.hip and avg_timestamp.hip (the
// training terms, whose forwards run around the splat) and iwe.hip (the
// validation metrics, likewise).  Host side only: the plan, the workspace
// layout, the decision between the two schedules, and the launchers of the
// splat, which live in tiled_splat.hip and take the term's event columns as
// plain pointers (the loaders of event_columns.h are per translation unit).
//
// The plan follows voxel_tiles.h: events bucketed by destination tile, one
// workgroup per tile with its sums in LDS, the 8192-tile ceiling, the bucket
// capacity 2 * (records / tiles) + 256 rounded to 64 and its 2^24 limit.  A
// tile is a kTileW x kTileH rectangle of ONE image m = (f R + r) C + c, so
// tiles = M * TX * TY.  A bucket that overflows loses nothing: the thread whose
// reservation lands past the capacity splats its record into global memory
// itself, and integer sums have no order.
//
// The same schedule over the level table of a term on every flow scale
// (include/dvsof_event_pyramids_tiled.h; PyramidTilePlan below): every level has
// its own tiles, capacity and record region, a tile is summed in slices of
// kSlice records, and the sums at the events' own pixels are taken at the
// finest level of the table alone and folded into the others.
#pragma once
#include "event_term_levels.h"
#include "voxel_tiles.h"

// 64 x 16: a row of the tile's accumulators is one 520-byte run of LDS, a row of its flush 64
// contiguous pixels of q; 65 x 17 x 8 bytes = 8.6 KiB of LDS, so the workgroups of a CU are
// bounded by waves, not by LDS.  Measured at this size only (8 frames of 256 x 256, whole
// call, per-event kernel -> tiled: 57.7 -> 40.4 us at 240 k events and one image a frame,
// 608.6 -> 291.8 us at 960 k events and six; profiles/event_images_tiled/README.md); other
// sizes are untried.
constexpr int kTileW = 64, kTileH = 16;
// one cursor per 128-byte line: the reservations of different tiles go to different L2 lines
constexpr int kCursorStride = 32;
// mode 0 runs the tiled schedule from this many events on: the smallest measured count at which
// every row of profiles/event_images_tiled/README.md wins by more than the spread of its block
// means (0.48-0.77 of the per-event kernel's time; at 64 k events one row is within the spread,
// at 16 k the tiled schedule loses)
constexpr int64_t kTiledFromEvents = 240000;
// the same for the average-timestamp images: the smallest measured count at which
// every row of profiles/avg_timestamp_tiled/README.md wins by more than the spread of its block
// means: 8 frames of 8 000 events (0.78-0.80 of the per-event call's time in all four rows, the
// spreads below 1 us; 0.37-0.45 at the benchmark batch and above).  At 8 x 2 000 events all four
// rows lose by 1-3 %.  Measured at 8 frames of 256 x 256 only.
constexpr int64_t kAvgtsTiledFromEvents = 64000;
// The level table: a workgroup of pass 2 sums at most this many records of a tile, so that the two
// tiles of a 32 x 32 level still spread over the device.  Of 4096, 8192 and 16384 the best at the
// benchmark batch (whole forward call, 8192 -> 4096: 1-3 % less, 16384: 4-8 % more;
// profiles/event_pyramids_tiled/README.md)
constexpr int kSlice = 4096;
// pass 1 agrees within a wave on the reservations of a level whose images have at most this many
// tiles each (one cursor atomic per distinct tile among the active lanes); above it a wave touches
// too many tiles for the agreement loop to pay.  Without it (0) the whole forward call of the
// benchmark batch takes 2.5-6 times as long: almost every lane then hits one of two words
constexpr int kAggregateTiles = 4;
// mode 0 of the level-table calls runs the tiled schedule from this many events on, per family:
// the smallest measured count at which every row of profiles/event_pyramids_tiled/README.md wins
// by more than the spread of its block means.  The images of warped events: 8 frames of 8 000
// events (0.96 and 0.71 of the per-event call's time, spreads below 0.5 us; 0.30-0.53 at the
// benchmark batch); at 8 x 2 000 both rows lose by 29-37 %.
constexpr int64_t kPyramidTiledFromEvents = 64000;
// The average-timestamp images: the same count (0.73 and 0.52; 0.20-0.31 at the benchmark batch);
// at 8 x 2 000 both rows lose by 7-18 %.  Measured at 8 frames of 256 x 256 and four levels only.
constexpr int64_t kAvgtsPyramidTiledFromEvents = 64000;

// A family: the images of one call, each [M, h, w], with the bytes of its record (coalesced word
// columns per tile) and the event count from which its mode 0 tiles.
// The images of warped events; a record: the corner, the bits of fx, of fy
struct EventImages {
    int64_t *q;
    uint32_t *count;
    static constexpr int kRecordBytes = 12;
    static constexpr int64_t kTiledFrom = kTiledFromEvents;
    static constexpr int64_t kPyramidTiledFrom = kPyramidTiledFromEvents;
};
// The average-timestamp images; a record: the corner, the bits of fx, of fy, of a = |sig|
struct AvgtsImages {
    int64_t *q, *s, *base;
    uint32_t *count;
    static constexpr int kRecordBytes = 16;
    static constexpr int64_t kTiledFrom = kAvgtsTiledFromEvents;
    static constexpr int64_t kPyramidTiledFrom = kAvgtsPyramidTiledFromEvents;
};

// the event columns of a training term in either form (event_columns.h), as plain pointers
struct TiledTermColumns {
    int encoded;
    const void *x, *y;      // int64 (wire) or int16 (encoded)
    const float *t;
    const void *pol;        // int64 (wire) or uint8 (encoded); may be null without polarity channels
    const int64_t *sample;  // wire: the sample of every event; encoded: the first event of every sample [B + 1]
    int B;
};

struct TilePlan {
    int TX, TY, tiles, cap;
};

// The plan over a level table, passed to the kernels by value like the table.  Level k has
// tiles[k] = M TX[k] TY[k] tiles of cap[k] records, summed by slices[k] workgroups each; its
// cursors start at tile tile_base[k], its records at record rec_base[k], its workgroups of pass 2
// at block_base[k].  source: the level with the smallest shift (the first of them), the one whose
// own-pixel sums pass 1 takes.
struct PyramidTilePlan {
    int K, source;
    int TX[kMaxLevels], TY[kMaxLevels], tiles[kMaxLevels], cap[kMaxLevels], slices[kMaxLevels];
    int tile_base[kMaxLevels + 1], block_base[kMaxLevels + 1];
    size_t rec_base[kMaxLevels + 1];
};

namespace {

inline TiledTermColumns plain(const WireColumns &c) { return TiledTermColumns{0, c.x, c.y, c.t, c.pol, c.sample, 0}; }
inline TiledTermColumns plain(const EncodedColumns &c)
{
    return TiledTermColumns{1, c.x, c.y, c.t, c.pol, c.ev_off, c.B};
}

// the tiled twins' three arguments; mode < 0: the calls that have none
struct TiledSplat {
    void *workspace;
    size_t bytes;
    int mode;
};

// false: refused (arguments the calls refuse, more than 8192 tiles, a bucket past 2^24 records)
inline bool tile_plan(int F, int reference_mask, int polarity, int h, int w, int64_t n_events, TilePlan &o)
{
    Plan pl;
    if (F < 1 || n_events < 0 || bad_frame_sizes(F, h, w) || !plan_of(F, reference_mask, polarity, pl)) return false;
    o.TX = (w + kTileW - 1) / kTileW;
    o.TY = (h + kTileH - 1) / kTileH;
    const int64_t nt = (int64_t)pl.M * o.TX * o.TY;
    if (nt > V2_MAX_TILES) return false;
    o.tiles = (int)nt;
    // an event takes part in the R images of its channel (the term: per frame that holds it)
    int64_t cap = 2 * (n_events * pl.R / nt) + 256;
    cap = (cap + 63) / 64 * 64;
    if (cap > (1 << 24)) return false;
    o.cap = (int)cap;
    return true;
}

inline size_t tile_cursor_bytes(const TilePlan &p) { return (size_t)p.tiles * kCursorStride * 4; }

// the cursors, then per tile the record's columns of cap words
template <class Images>
inline size_t tile_workspace_bytes(const TilePlan &p)
{
    return tile_cursor_bytes(p) + (size_t)p.tiles * p.cap * Images::kRecordBytes;
}

// Which schedule a call of the family Images runs.  DVSOF_OK: tiled (plan filled in); 1: the
// one-thread-per-event kernel (no events, mode 0 below the threshold, or a refused plan); else
// the error to return.  tiled.mode is 0 or 1, or below 0 for a call that has no tiled twin.
template <class Images>
inline int tile_decide(const TiledSplat &tiled, int F, int reference_mask, int polarity, int h, int w,
                       int64_t n_events, TilePlan &tp)
{
    if (tiled.mode < 0) return 1;
    if (tiled.mode != 0 && tiled.mode != 1) return DVSOF_EINVAL;
    if (n_events == 0 || (tiled.mode == 0 && n_events < Images::kTiledFrom)) return 1;
    if (!tile_plan(F, reference_mask, polarity, h, w, n_events, tp)) return 1;
    if (!tiled.workspace || tiled.bytes < tile_workspace_bytes<Images>(tp)) return DVSOF_ENOSPACE;
    return DVSOF_OK;
}

// tile_plan over the levels of a table.  false: refused (arguments or a table the calls refuse,
// more than 8192 tiles in all, a bucket past 2^24 records)
inline bool pyramid_tile_plan(int F, int reference_mask, int polarity, int h, int w, const dvsof_contrast_levels_t &lv,
                              int64_t n_events, PyramidTilePlan &o)
{
    Plan pl;
    if (F < 1 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return false;
    if (level_table_pixels(F, h, w, lv, 0) == 0) return false;
    o.K = lv.K;
    o.source = 0;
    o.tile_base[0] = o.block_base[0] = 0;
    o.rec_base[0] = 0;
    int64_t total = 0, blocks = 0;
    for (int k = 0; k < lv.K; ++k) {
        const Level &L = lv.level[k];
        if (L.shift < lv.level[o.source].shift) o.source = k;
        o.TX[k] = (L.w + kTileW - 1) / kTileW;
        o.TY[k] = (L.h + kTileH - 1) / kTileH;
        const int64_t nt = (int64_t)pl.M * o.TX[k] * o.TY[k];
        total += nt;
        if (total > V2_MAX_TILES) return false;
        int64_t cap = 2 * (n_events * pl.R / nt) + 256;
        cap = (cap + 63) / 64 * 64;
        if (cap > (1 << 24)) return false;
        o.tiles[k] = (int)nt;
        o.cap[k] = (int)cap;
        o.slices[k] = (int)((cap + kSlice - 1) / kSlice);
        blocks += nt * o.slices[k];  // at most 8192 * 2048
        o.tile_base[k + 1] = (int)total;
        o.block_base[k + 1] = (int)blocks;
        o.rec_base[k + 1] = o.rec_base[k] + (size_t)nt * (size_t)cap;
    }
    return true;
}

inline size_t pyramid_cursor_bytes(const PyramidTilePlan &p) { return (size_t)p.tile_base[p.K] * kCursorStride * 4; }

// the cursors of all levels, then level by level the tiles' record columns
template <class Images>
inline size_t pyramid_tile_workspace_bytes(const PyramidTilePlan &p)
{
    return pyramid_cursor_bytes(p) + p.rec_base[p.K] * Images::kRecordBytes;
}

// tile_decide for a call over a level table
template <class Images>
inline int pyramid_tile_decide(const TiledSplat &tiled, int F, int reference_mask, int polarity, int h, int w,
                               const dvsof_contrast_levels_t &lv, int64_t n_events, PyramidTilePlan &tp)
{
    if (tiled.mode < 0) return 1;
    if (tiled.mode != 0 && tiled.mode != 1) return DVSOF_EINVAL;
    if (n_events == 0 || (tiled.mode == 0 && n_events < Images::kPyramidTiledFrom)) return 1;
    if (!pyramid_tile_plan(F, reference_mask, polarity, h, w, lv, n_events, tp)) return 1;
    if (!tiled.workspace || tiled.bytes < pyramid_tile_workspace_bytes<Images>(tp)) return DVSOF_ENOSPACE;
    return DVSOF_OK;
}

}  // namespace

// The launchers of the family Images (EventImages or AvgtsImages), defined in tiled_splat.hip.
// term: the splat of the term's one-thread-per-event kernel on one flow (contrast_splat_kernel,
// avgts_splat_kernel: sample and time window, either form of the columns) by the tiled schedule;
// frames: that of the metric's (iwe_splat_kernel, iwe_avgts_splat_kernel: position in the
// columns).  The same bytes in the images, all zeroed by the caller; tp: the plan of these
// arguments, tile_workspace: tile_workspace_bytes<Images>(tp) bytes.
template <class Images>
struct __attribute__((visibility("hidden"))) TiledLaunch {
    static int term(const TiledTermColumns &cols, int64_t n_events, const float *frame_ts,
                    const int64_t *frame_sample, const float *flow, int F, int h, int w, int reference_mask,
                    int polarity, const TilePlan &tp, const Images &img, void *tile_workspace, hipStream_t stream);
    static int frames(const int64_t *x, const int64_t *y, const float *t, const int64_t *p, int64_t n_events,
                      const int64_t *frame_event_begin, const float *frame_ts, const float *flow, int F, int h,
                      int w, int reference_mask, int polarity, const TilePlan &tp, const Images &img,
                      void *tile_workspace, hipStream_t stream);
    // pyramid: the splat of the same kernels over a level table (their TableView instances);
    // img: the images of all levels, a level's at its image_offset
    static int pyramid(const TiledTermColumns &cols, int64_t n_events, const float *frame_ts,
                       const int64_t *frame_sample, int F, int h, int w, int reference_mask, int polarity,
                       const dvsof_contrast_levels_t &levels, const PyramidTilePlan &tp, const Images &img,
                       void *tile_workspace, hipStream_t stream);
};
