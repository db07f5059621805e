/*
 * dvsof_event_images_tiled.h -- extension of the C ABI of libdvsof_hip.so
 * (dvsof.h, whose conventions hold here): the splat into the images of warped
 * events of dvsof_iwe_multi.h and dvsof_contrast_multi.h by a second schedule,
 * for dense frames (csrc/tiled_splat.hip, docs/IWE_SPEC.md section 22).
 * Events are bucketed by the tile of the image they land in, every tile is
 * summed in LDS by one workgroup, and a touched pixel costs one global atomic
 * per tile in place of one per corner per event.
 *
 * A schedule, not a definition.  Every call here is the twin of the call whose
 * name it carries: the twin's argument list and, behind it,
 *   void *tile_workspace, size_t tile_workspace_bytes, int mode
 * It writes, in every output and in every region of the workspace its twin
 * documents, the bytes the twin writes -- all sums are 64-bit integers, which
 * have no order -- and returns what the twin returns, in the twin's order.
 *
 *   mode            0: the call decides: the tiled schedule from an event
 *                   count on that was measured (profiles/event_images_tiled/),
 *                   the twin's kernel below it; 1: the tiled schedule wherever
 *                   its plan applies.  Anything else: DVSOF_EINVAL.
 *   the plan        tiles of tile_w x tile_h pixels of ONE image; refused with
 *                   more than 8192 tiles (M images x tiles per image) or a
 *                   bucket of more than 2^24 records.  A refused plan is no
 *                   error: the call runs the twin's kernel.  So does a call
 *                   with n_events = 0.
 *   tile_workspace  device memory of dvsof_event_images_tiled_workspace_bytes
 *                   for the same arguments; looked at only where the tiled
 *                   schedule runs (DVSOF_ENOSPACE there if null or too small,
 *                   before any launch); its contents on entry do not matter.
 *                   A bucket that overflows loses nothing.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_event_images_tiled.json) and no struct of its
 * own; dvsof.h, the older extension headers and their tables stay as they are.
 */
#ifndef DVSOF_EVENT_IMAGES_TILED_H
#define DVSOF_EVENT_IMAGES_TILED_H

#include "dvsof_iwe_multi.h"
#include "dvsof_contrast_multi.h"
#include "dvsof_event_terms_encoded.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[4]: tile width, tile height, number of tiles, records a bucket holds.  1: the plan
 * applies; 0: refused (out is left alone), also for what the calls refuse and for F = 0. */
int dvsof_event_images_tiled_plan(int F, int reference_mask, int polarity, int h, int w, int64_t n_events,
                                  int32_t *out);

/* 0 where the plan is refused */
size_t dvsof_event_images_tiled_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                int64_t n_events);

/* twin: dvsof_iwe_splat_multi */
int dvsof_iwe_splat_multi_tiled(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                int64_t n_events, const int64_t *frame_event_begin, const float *frame_ts,
                                const float *flow, int F, int h, int w, int reference_mask, int polarity, int64_t *q,
                                uint32_t *count, void *stream, void *tile_workspace, size_t tile_workspace_bytes,
                                int mode);

/* twin: dvsof_contrast_multi_fwd; dvsof_contrast_multi_bwd takes its q and workspace */
int dvsof_contrast_multi_fwd_tiled(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                   const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                   const int64_t *frame_sample, const float *flow, int F, int h, int w,
                                   int reference_mask, int polarity, int64_t *q, uint32_t *count,
                                   dvsof_iwe_result_t *result, float *term, void *workspace, size_t workspace_bytes,
                                   void *stream, void *tile_workspace, size_t tile_workspace_bytes, int mode);

/* twin: dvsof_contrast_multi_fwd_encoded; dvsof_contrast_multi_bwd_encoded takes its q and workspace */
int dvsof_contrast_multi_fwd_encoded_tiled(const int16_t *x, const int16_t *y, const float *t,
                                           const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                           int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                           const float *flow, int F, int h, int w, int reference_mask,
                                           int polarity_channels, int64_t *q, uint32_t *count,
                                           dvsof_iwe_result_t *result, float *term, void *workspace,
                                           size_t workspace_bytes, void *stream, void *tile_workspace,
                                           size_t tile_workspace_bytes, int mode);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_EVENT_IMAGES_TILED_H */
