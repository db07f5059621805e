/*
 * dvsof_event_terms_encoded.h -- extension of the C ABI of libdvsof_hip.so
 * (dvsof.h, whose conventions hold here): the two events-only training terms,
 * the contrast term (dvsof_contrast_multi.h, dvsof_contrast_pyramid.h) and the
 * average-timestamp term (dvsof_avg_timestamp.h, dvsof_avg_timestamp_pyramid.h),
 * fed from the encoded event columns of a preprocessed dataset as they are
 * stored, 9 bytes an event, in place of the 36 bytes of the wire columns
 * (csrc/event_columns.h, docs/CONTRAST_SPEC.md section 24,
 * docs/AVG_TIMESTAMP_SPEC.md section 16).
 *
 * Every call here is the twin of the call whose name it carries: the twin's
 * argument list, with the five event columns
 *   const int64_t *x, *y, const float *t, const int64_t *p, const int64_t *sample_index
 * replaced by
 *   const int16_t *x, *y, const float *t, const uint8_t *polarity,
 *   const int64_t *sample_event_offsets (B + 1 entries), int B
 * and everything else in the twin's meaning and order.  The workspace is the
 * twin's, sized by the twin's *_workspace_bytes.
 *
 * The bytes.  An encoded call gives, in every output and in every region of
 * the workspace its twin documents, the bytes the twin gives on the decoded
 * columns:
 *   x, y             widened to int64;
 *   p                polarity ? +1 : -1;
 *   sample_index[i]  the largest b in [0, B) with sample_event_offsets[b] <= i,
 *                    the rule of dvsof_voxelize_encoded.  Empty samples are
 *                    repeated offsets.
 * An event at or past sample_event_offsets[B] falls to sample B - 1, so it has
 * to be a padded slot, x = y = -1, as the captured step pads the columns to
 * their capacity.  All sums of the terms are 64-bit integer atomics, which
 * have no order: the equality is exact.
 *
 * Error returns: the twin's, in the twin's order; where the twin refuses a
 * null event column (n_events > 0), a null sample_event_offsets and B < 1 are
 * refused as well.  polarity may be null when the polarity option is 0, as p
 * may be.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_event_terms_encoded.json) and no struct of its
 * own; dvsof.h, the older extension headers and their tables stay as they are.
 */
#ifndef DVSOF_EVENT_TERMS_ENCODED_H
#define DVSOF_EVENT_TERMS_ENCODED_H

#include "dvsof_contrast_multi.h"
#include "dvsof_contrast_pyramid.h"
#include "dvsof_avg_timestamp.h"
#include "dvsof_avg_timestamp_pyramid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* twin: dvsof_contrast_multi_fwd; workspace: dvsof_contrast_multi_workspace_bytes */
int dvsof_contrast_multi_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                     const int64_t *sample_event_offsets /* [B + 1] */, int B, int64_t n_events,
                                     const float *frame_ts, const int64_t *frame_sample, const float *flow, int F,
                                     int h, int w, int reference_mask, int polarity_channels, int64_t *q,
                                     uint32_t *count, dvsof_iwe_result_t *result, float *term, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* twin: dvsof_contrast_multi_bwd */
int dvsof_contrast_multi_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                     const int64_t *sample_event_offsets, int B, int64_t n_events,
                                     const float *frame_ts, const int64_t *frame_sample, const float *flow, int F,
                                     int h, int w, int reference_mask, int polarity_channels, const int64_t *q,
                                     void *workspace, size_t workspace_bytes, const float *seed, float weight,
                                     float *grad_flow, void *stream);

/* twin: dvsof_contrast_pyramid_fwd; workspace: dvsof_contrast_pyramid_workspace_bytes */
int dvsof_contrast_pyramid_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                       const int64_t *sample_event_offsets, int B, int64_t n_events,
                                       const float *frame_ts, const int64_t *frame_sample, int F, int h, int w,
                                       int reference_mask, int polarity_channels, dvsof_contrast_levels_t levels,
                                       dvsof_iwe_result_t *result, float *terms, float *value, void *workspace,
                                       size_t workspace_bytes, void *stream);

/* twin: dvsof_contrast_pyramid_bwd */
int dvsof_contrast_pyramid_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                       const int64_t *sample_event_offsets, int B, int64_t n_events,
                                       const float *frame_ts, const int64_t *frame_sample, int F, int h, int w,
                                       int reference_mask, int polarity_channels, dvsof_contrast_levels_t levels,
                                       void *workspace, size_t workspace_bytes, const float *seed, void *stream);

/* twin: dvsof_avg_timestamp_fwd; workspace: dvsof_avg_timestamp_workspace_bytes */
int dvsof_avg_timestamp_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                    const int64_t *sample_event_offsets, int B, int64_t n_events,
                                    const float *frame_ts, const int64_t *frame_sample, const float *flow, int F,
                                    int h, int w, int reference_mask, int polarity_channels, float *term,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* twin: dvsof_avg_timestamp_bwd */
int dvsof_avg_timestamp_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                    const int64_t *sample_event_offsets, int B, int64_t n_events,
                                    const float *frame_ts, const int64_t *frame_sample, const float *flow, int F,
                                    int h, int w, int reference_mask, int polarity_channels, void *workspace,
                                    size_t workspace_bytes, const float *seed, float weight, float *grad_flow,
                                    void *stream);

/* twin: dvsof_avg_timestamp_pyramid_fwd; workspace: dvsof_avg_timestamp_pyramid_workspace_bytes */
int dvsof_avg_timestamp_pyramid_fwd_encoded(const int16_t *x, const int16_t *y, const float *t,
                                            const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                            int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                            int F, int h, int w, int reference_mask, int polarity_channels,
                                            dvsof_contrast_levels_t levels, float *terms, float *value,
                                            void *workspace, size_t workspace_bytes, void *stream);

/* twin: dvsof_avg_timestamp_pyramid_bwd */
int dvsof_avg_timestamp_pyramid_bwd_encoded(const int16_t *x, const int16_t *y, const float *t,
                                            const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                            int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                            int F, int h, int w, int reference_mask, int polarity_channels,
                                            dvsof_contrast_levels_t levels, void *workspace, size_t workspace_bytes,
                                            const float *seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_EVENT_TERMS_ENCODED_H */
