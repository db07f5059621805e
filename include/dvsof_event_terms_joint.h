/*
 * dvsof_event_terms_joint.h -- extension of the C ABI of libdvsof_hip.so
 * (dvsof.h, whose conventions hold here): the two events-only training terms
 * on every flow scale, the contrast term of dvsof_contrast_pyramid.h and the
 * average-timestamp term of dvsof_avg_timestamp_pyramid.h, from one splat, one
 * statistics pass and one backward (csrc/avg_timestamp.hip, its last section;
 * docs/CONTRAST_SPEC.md section 26, docs/AVG_TIMESTAMP_SPEC.md section 19).
 *
 * A schedule, not a definition.  The average-timestamp images q and count of
 * frame f, reference time rho and channel c are the bytes of the contrast
 * term's image of the same (f, rho, c), so a run that takes both terms needs
 * the contrast term's fill, event walk and splat no second time, and both
 * backwards walk the same events to the same corners.  Every output of the
 * calls below is, byte for byte, what the two existing calls write on the same
 * inputs: contrast_result, contrast_terms and contrast_value those of
 * dvsof_contrast_pyramid_fwd with (contrast_mask, contrast_levels),
 * avg_timestamp_terms and avg_timestamp_value those of
 * dvsof_avg_timestamp_pyramid_fwd with (avg_timestamp_mask,
 * avg_timestamp_levels), each table's grad_flow that of the term's _bwd.  The
 * gradients stay apart, one set per term.  The workspace is the calls' own
 * and has a layout of its own.
 *
 *   the masks      contrast_mask must be a non-empty subset of
 *                  avg_timestamp_mask; one `polarity` holds for both terms.
 *   the tables     two level tables by value, each with its own term's packed
 *                  offsets (M differs where the masks differ), weights and
 *                  grad_flow.  They must agree in K, in every level's h, w
 *                  and shift, and in flow.  K = 1 with shift 0 is the
 *                  finest-scale form: the bytes of dvsof_contrast_multi_fwd /
 *                  _bwd and dvsof_avg_timestamp_fwd / _bwd.
 *   mode           -1: the splat of one thread per event; 0 and 1: as in
 *                  dvsof_avg_timestamp_pyramid_fwd_tiled
 *                  (dvsof_event_pyramids_tiled.h), with tile_workspace that of
 *                  dvsof_avg_timestamp_pyramid_tiled_workspace_bytes for
 *                  avg_timestamp_mask and avg_timestamp_levels.  Anything else:
 *                  DVSOF_EINVAL.
 *
 * Returns, before any launch and in this order: DVSOF_EINVAL for a mode that
 * is none of the three; those of dvsof_contrast_pyramid_fwd / _bwd on the
 * contrast term's arguments, then those of dvsof_avg_timestamp_pyramid_fwd /
 * _bwd on the other's, each in its own order up to its workspace test (F == 0
 * is DVSOF_OK and nothing to do once the options and both K are accepted);
 * DVSOF_EINVAL for a contrast_mask that is no subset of avg_timestamp_mask and
 * for tables that disagree; DVSOF_ENOSPACE where the workspace or, where the
 * tiled schedule runs, the tile workspace is missing or short.  n_events == 0:
 * the event columns may be null; the images stay zero and everything else
 * runs, as in the two calls.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_event_terms_joint.json) and no struct of its
 * own: the level table is that of dvsof_contrast_pyramid.h.
 */
#ifndef DVSOF_EVENT_TERMS_JOINT_H
#define DVSOF_EVENT_TERMS_JOINT_H

#include "dvsof_contrast_pyramid.h"
#include "dvsof_avg_timestamp_pyramid.h"
#include "dvsof_event_terms_encoded.h"
#include "dvsof_event_pyramids_tiled.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of the workspace both calls share.  With Ma = F Ra C images per level
 * of the average-timestamp term and Mc = F Rc C of the contrast term,
 * P = Ma * sum_k h_k w_k and S = 2 F * sum_k h_k w_k, at these byte offsets:
 *   0             q      int64[P]    the images of weights of all levels, in units of 2^-32
 *   8 P           s      int64[P]    the images of weight times distance
 *   16 P          base   int64[P]    the sums of the distances at the events' own level pixels
 *   24 P          sums   int64[S]    the average-timestamp term's fixed-point gradient sums
 *   24 P + 8 S    sums   int64[S]    the contrast term's
 *   24 P + 16 S   count  uint32[P]   the count images, then padding to a multiple of 8 bytes
 * (one contiguous region, zeroed by one fill; the average-timestamp table's
 * image_offset indexes q, s, base and count, either table's sums_offset the
 * sums), and behind it
 *   T, D   float64[P] each: per pixel the average distance and 1 / (I + eps)
 *          of dvsof_avg_timestamp.h, stored by the statistics for the backward
 *   one 64-byte record per level and average-timestamp image, K Ma of them
 *   one float64 unit per level and frame, K F of them: the average-timestamp term's
 *   one 32-byte record per level and contrast image, K Mc of them
 *   one float64 unit per level and frame, K F of them: the contrast term's
 *   one 80-byte statistics row per level and average-timestamp image, K Ma of
 *     them (the 32-byte row of dvsof_avg_timestamp.h, then the 48-byte
 *     dvsof_iwe_result_t of the same image), then nb of them per image for Ma
 *     images, the partials, sized for the largest level.
 * Only F, the options, (h, w), K and the levels' h, w and shift are read; 0
 * for arguments the calls refuse.
 */
size_t dvsof_event_terms_joint_workspace_bytes(int F, int contrast_mask, int avg_timestamp_mask, int polarity, int h,
                                               int w, dvsof_contrast_levels_t contrast_levels,
                                               dvsof_contrast_levels_t avg_timestamp_levels);

/*
 * Launches, kernels only: one fill, one splat for all levels (n_events > 0;
 * per event or by tiles), two of the statistics per level (the partials of
 * both terms' rows from one read of q, s, base and count, which also stores
 * T and D; the closing reduction), one closing wave for both terms.
 */
int dvsof_event_terms_joint_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                const int64_t *sample_index, int64_t n_events,
                                const float *frame_ts /* [2F]: start, stop */,
                                const int64_t *frame_sample /* [F] */, int F, int h, int w, int contrast_mask,
                                int avg_timestamp_mask, int polarity, dvsof_contrast_levels_t contrast_levels,
                                dvsof_contrast_levels_t avg_timestamp_levels, dvsof_iwe_result_t *contrast_result,
                                float *contrast_terms, float *contrast_value, float *avg_timestamp_terms,
                                float *avg_timestamp_value, void *workspace, size_t workspace_bytes, void *stream,
                                void *tile_workspace, size_t tile_workspace_bytes, int mode);

/*
 * Every element of both tables' grad_flow, contrast_levels' from
 * contrast_seed[0] and avg_timestamp_levels' from avg_timestamp_seed[0].  One
 * launch over the events (one walk, one flow read and one warp per event,
 * frame, level and reference for both terms; up to four integer atomics at the
 * event's own level pixel), one over the elements of all levels, which
 * converts, clears both sums and stores.  Same columns, tables, options,
 * level tables and workspace as the dvsof_event_terms_joint_fwd call before it.
 */
int dvsof_event_terms_joint_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                const int64_t *frame_sample, int F, int h, int w, int contrast_mask,
                                int avg_timestamp_mask, int polarity, dvsof_contrast_levels_t contrast_levels,
                                dvsof_contrast_levels_t avg_timestamp_levels, void *workspace,
                                size_t workspace_bytes, const float *contrast_seed, const float *avg_timestamp_seed,
                                void *stream);

/* The twins on the encoded event columns of dvsof_event_terms_encoded.h */
int dvsof_event_terms_joint_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                        const int64_t *sample_event_offsets, int B, int64_t n_events,
                                        const float *frame_ts, const int64_t *frame_sample, int F, int h, int w,
                                        int contrast_mask, int avg_timestamp_mask, int polarity_channels,
                                        dvsof_contrast_levels_t contrast_levels,
                                        dvsof_contrast_levels_t avg_timestamp_levels,
                                        dvsof_iwe_result_t *contrast_result, float *contrast_terms,
                                        float *contrast_value, float *avg_timestamp_terms,
                                        float *avg_timestamp_value, void *workspace, size_t workspace_bytes,
                                        void *stream, void *tile_workspace, size_t tile_workspace_bytes, int mode);

int dvsof_event_terms_joint_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                        const int64_t *sample_event_offsets, int B, int64_t n_events,
                                        const float *frame_ts, const int64_t *frame_sample, int F, int h, int w,
                                        int contrast_mask, int avg_timestamp_mask, int polarity_channels,
                                        dvsof_contrast_levels_t contrast_levels,
                                        dvsof_contrast_levels_t avg_timestamp_levels, void *workspace,
                                        size_t workspace_bytes, const float *contrast_seed,
                                        const float *avg_timestamp_seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_EVENT_TERMS_JOINT_H */
