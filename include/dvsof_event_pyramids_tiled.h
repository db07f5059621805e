/*
 * dvsof_event_pyramids_tiled.h -- extension of the C ABI of libdvsof_hip.so
 * (dvsof.h, whose conventions hold here): the forward splat of the two
 * events-only terms on every flow scale (dvsof_contrast_pyramid.h,
 * dvsof_avg_timestamp_pyramid.h and their encoded twins of
 * dvsof_event_terms_encoded.h) by the tiled schedule of
 * dvsof_event_images_tiled.h, over the level table (csrc/tiled_splat.hip,
 * docs/CONTRAST_SPEC.md section 25, docs/AVG_TIMESTAMP_SPEC.md section 18).
 *
 * A schedule, not a definition.  Every forward here is the twin of the call
 * whose name it carries: the twin's argument list and, behind it,
 *   void *tile_workspace, size_t tile_workspace_bytes, int mode
 * It writes, in every output and in every region of the workspace its twin
 * documents, the bytes the twin writes, and returns what the twin returns, in
 * the twin's order; the twin's _bwd runs on the result unchanged.
 *
 *   mode            0: the call decides by the event count, from a threshold
 *                   per family that was measured
 *                   (profiles/event_pyramids_tiled/); 1: the tiled schedule
 *                   wherever its plan applies.  Anything else: DVSOF_EINVAL.
 *   the plan        per level k of the table tiles of tile_w x tile_h pixels of
 *                   ONE image of that level, tiles_k = M ceil(w_k / tile_w)
 *                   ceil(h_k / tile_h), each with room for cap_k records and
 *                   summed by slices_k = ceil(cap_k / slice) workgroups.
 *                   Refused with more than 8192 tiles over the whole table or a
 *                   bucket of more than 2^24 records.  A refused plan is no
 *                   error: the call runs the twin's kernel.  So does a call
 *                   with n_events = 0 or F = 0.
 *   own pixels      count (and base) are summed per event at the table's level
 *                   of the smallest shift only (the first such level) and
 *                   folded from there into every other level: the sum over the
 *                   2^d x 2^d block, d the difference of the shifts, clipped at
 *                   the edge.  Integers: the same bytes.
 *   tile_workspace  device memory of the family's *_tiled_workspace_bytes for
 *                   the same arguments; looked at only where the tiled schedule
 *                   runs (DVSOF_ENOSPACE there if null or too small, before any
 *                   launch); its contents on entry do not matter.  A bucket
 *                   that overflows loses nothing.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_event_pyramids_tiled.json) and no struct of its
 * own: the level table is that of dvsof_contrast_pyramid.h.
 */
#ifndef DVSOF_EVENT_PYRAMIDS_TILED_H
#define DVSOF_EVENT_PYRAMIDS_TILED_H

#include "dvsof_contrast_pyramid.h"
#include "dvsof_avg_timestamp_pyramid.h"
#include "dvsof_event_terms_encoded.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 and out = {tile_w, tile_h, tiles of all levels, slice, the tiles per image up to which a wave
 * agrees on its reservations, the level the own-pixel sums are taken at}, then {tiles_k, cap_k,
 * slices_k} per level (6 + 3 K values); 0 and out untouched where the plan is refused */
int dvsof_event_pyramids_tiled_plan(int F, int reference_mask, int polarity, int h, int w,
                                    dvsof_contrast_levels_t levels, int64_t n_events, int32_t *out);

/* 0 where the plan is refused; the offsets and pointers of the table are not looked at */
size_t dvsof_contrast_pyramid_tiled_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                    dvsof_contrast_levels_t levels, int64_t n_events);
size_t dvsof_avg_timestamp_pyramid_tiled_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                         dvsof_contrast_levels_t levels, int64_t n_events);

/* twin: dvsof_contrast_pyramid_fwd; dvsof_contrast_pyramid_bwd takes its workspace */
int dvsof_contrast_pyramid_fwd_tiled(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                     const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                     const int64_t *frame_sample, int F, int h, int w, int reference_mask,
                                     int polarity, dvsof_contrast_levels_t levels, dvsof_iwe_result_t *result,
                                     float *terms, float *value, void *workspace, size_t workspace_bytes,
                                     void *stream, void *tile_workspace, size_t tile_workspace_bytes, int mode);

/* twin: dvsof_contrast_pyramid_fwd_encoded */
int dvsof_contrast_pyramid_fwd_encoded_tiled(const int16_t *x, const int16_t *y, const float *t,
                                             const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                             int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                             int F, int h, int w, int reference_mask, int polarity_channels,
                                             dvsof_contrast_levels_t levels, dvsof_iwe_result_t *result,
                                             float *terms, float *value, void *workspace, size_t workspace_bytes,
                                             void *stream, void *tile_workspace, size_t tile_workspace_bytes,
                                             int mode);

/* twin: dvsof_avg_timestamp_pyramid_fwd; dvsof_avg_timestamp_pyramid_bwd takes its workspace */
int dvsof_avg_timestamp_pyramid_fwd_tiled(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                          const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                          const int64_t *frame_sample, int F, int h, int w, int reference_mask,
                                          int polarity, dvsof_contrast_levels_t levels, float *terms, float *value,
                                          void *workspace, size_t workspace_bytes, void *stream,
                                          void *tile_workspace, size_t tile_workspace_bytes, int mode);

/* twin: dvsof_avg_timestamp_pyramid_fwd_encoded */
int dvsof_avg_timestamp_pyramid_fwd_encoded_tiled(const int16_t *x, const int16_t *y, const float *t,
                                                  const uint8_t *polarity, const int64_t *sample_event_offsets,
                                                  int B, int64_t n_events, const float *frame_ts,
                                                  const int64_t *frame_sample, int F, int h, int w,
                                                  int reference_mask, int polarity_channels,
                                                  dvsof_contrast_levels_t levels, float *terms, float *value,
                                                  void *workspace, size_t workspace_bytes, void *stream,
                                                  void *tile_workspace, size_t tile_workspace_bytes, int mode);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_EVENT_PYRAMIDS_TILED_H */
