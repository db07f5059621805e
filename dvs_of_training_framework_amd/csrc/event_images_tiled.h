// The tiled schedule of the splat into the images of event_images.h
// (event_images_tiled.hip; include/dvsof_event_images_tiled.h): what its entry
// points in event_images_tiled.hip (the validation metric) and contrast.hip (the
// training term, whose forward runs around the splat) share.  Host side only:
// the plan, the workspace layout, the decision between the two schedules, and
// the launcher of the term's splat, which lives in event_images_tiled.hip and
// takes the event columns as plain pointers (the loaders of event_columns.h are
// per translation unit).
//
// The plan follows voxel_tiles.h: events bucketed by destination tile, one
// workgroup per tile with its sums in LDS, the 8192-tile ceiling, the bucket
// capacity 2 * (records / tiles) + 256 rounded to 64 and its 2^24 limit.  A
// tile is a kTileW x kTileH rectangle of ONE image m = (f R + r) C + c, so
// tiles = M * TX * TY.  A bucket that overflows loses nothing: the thread whose
// reservation lands past the capacity splats its record into global memory
// itself, and integer sums have no order.
#pragma once
#include "event_images.h"
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

// the event columns of the training term in either form (event_columns.h), as plain pointers
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

namespace {

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

// the cursors, then per tile three columns of cap words: the corner, the bits of fx, of fy
// (record_bytes = 16 for the average-timestamp splat of avg_timestamp_tiled.h: a fourth column)
constexpr int kTileRecordBytes = 12;
inline size_t tile_workspace_bytes(const TilePlan &p, int record_bytes = kTileRecordBytes)
{
    return tile_cursor_bytes(p) + (size_t)p.tiles * p.cap * record_bytes;
}

// Which schedule a call runs.  DVSOF_OK: tiled (plan filled in); 1: the one-thread-per-event
// kernel (no events, mode 0 below the threshold, or a refused plan); else the error to return.
// record_bytes, from_events: those of the splat that asks (the defaults: the images of event_images.h).
inline int tile_decide(int mode, int F, int reference_mask, int polarity, int h, int w, int64_t n_events,
                       const void *tile_workspace, size_t tile_workspace_bytes_, TilePlan &tp,
                       int record_bytes = kTileRecordBytes, int64_t from_events = kTiledFromEvents)
{
    if (mode != 0 && mode != 1) return DVSOF_EINVAL;
    if (n_events == 0 || (mode == 0 && n_events < from_events)) return 1;
    if (!tile_plan(F, reference_mask, polarity, h, w, n_events, tp)) return 1;
    if (!tile_workspace || tile_workspace_bytes_ < tile_workspace_bytes(tp, record_bytes)) return DVSOF_ENOSPACE;
    return DVSOF_OK;
}

}  // namespace

// The splat of contrast_splat_kernel by the tiled schedule (the same events by the same frame
// rule, the same bytes in q and count, both zeroed by the caller); tp: the plan of these
// arguments, tile_workspace: tile_workspace_bytes(tp) bytes.
__attribute__((visibility("hidden"))) int event_images_tiled_term_splat(
    const TiledTermColumns &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
    const float *flow, int F, int h, int w, int reference_mask, int polarity, const TilePlan &tp, int64_t *q,
    uint32_t *count, void *tile_workspace, hipStream_t stream);
