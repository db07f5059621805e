// The tiled schedule of the splat into the average-timestamp images of
// avg_timestamp_images.h (avg_timestamp_tiled.hip;
// include/dvsof_avg_timestamp_tiled.h): what its entry points in
// avg_timestamp.hip (the training term, whose forward runs around the splat)
// and iwe.hip (the validation metric, likewise) share.  Host side only.  The
// plan is tile_plan of event_images_tiled.h unchanged; a record is 16 bytes,
// not 12, and the event count from which mode 0 tiles is this splat's own.
#pragma once
#include "event_images_tiled.h"

// four coalesced word columns per tile: the corner, the bits of fx, of fy, of a = |sig|
constexpr int kAvgtsRecordBytes = 16;
// mode 0 runs the tiled schedule from this many events on: the smallest measured count at which
// every row of profiles/avg_timestamp_tiled/README.md wins by more than the spread of its block
// means: 8 frames of 8 000 events (0.78-0.80 of the per-event call's time in all four rows, the
// spreads below 1 us; 0.37-0.45 at the benchmark batch and above).  At 8 x 2 000 events all four
// rows lose by 1-3 %.  Measured at 8 frames of 256 x 256 only.
constexpr int64_t kAvgtsTiledFromEvents = 64000;

// the four images of one call, each [M, h, w]
struct AvgtsImages {
    int64_t *q, *s, *base;
    uint32_t *count;
};

namespace {

inline int avgts_tile_decide(int mode, int F, int reference_mask, int polarity, int h, int w, int64_t n_events,
                             const void *tile_workspace, size_t tile_workspace_bytes_, TilePlan &tp)
{
    return tile_decide(mode, F, reference_mask, polarity, h, w, n_events, tile_workspace, tile_workspace_bytes_, tp,
                       kAvgtsRecordBytes, kAvgtsTiledFromEvents);
}

}  // namespace

// The splat of avgts_splat_kernel (the term's frame rule: sample and time window, either form of
// the columns) by the tiled schedule: the same bytes in the four images, all zeroed by the
// caller; tp: the plan of these arguments, tile_workspace: tile_workspace_bytes(tp, 16) bytes.
__attribute__((visibility("hidden"))) int avg_timestamp_tiled_term_splat(
    const TiledTermColumns &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
    const float *flow, int F, int h, int w, int reference_mask, int polarity, const TilePlan &tp,
    const AvgtsImages &img, void *tile_workspace, hipStream_t stream);

// The same for iwe_avgts_splat_kernel (the metric's frame rule: position in the columns)
__attribute__((visibility("hidden"))) int avg_timestamp_tiled_frames_splat(
    const int64_t *x, const int64_t *y, const float *t, const int64_t *p, int64_t n_events,
    const int64_t *frame_event_begin, const float *frame_ts, const float *flow, int F, int h, int w,
    int reference_mask, int polarity, const TilePlan &tp, const AvgtsImages &img, void *tile_workspace,
    hipStream_t stream);
