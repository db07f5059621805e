/*
 * dvsof_avg_timestamp_pyramid.h -- extension of the C ABI of libdvsof_hip.so
 * (dvsof.h, whose conventions hold here): the average-timestamp term of
 * dvsof_avg_timestamp.h on every flow scale of the network at once
 * (csrc/avg_timestamp.hip, docs/AVG_TIMESTAMP_SPEC.md sections 11-15).
 *
 * (h, w) is the frame the event coordinates live in.  Level k has a shape
 * (h_k, w_k) and a shift s in [0, 15] with h_k == ceil(h / 2^s) and
 * w_k == ceil(w / 2^s): the level table of dvsof_contrast_pyramid.h, passed by
 * value, with its packed offsets.  Which events take part in frame f is
 * decided at full resolution, by dvsof_avg_timestamp_fwd's rule on (h, w);
 * such an event sits at level pixel (y >> s, x >> s), which is also its own
 * pixel for base and count, reads flow_k there and is splatted into the
 * level's images.  Per level q, s, base, count, the statistics rows, the image
 * records, the units, the sums and the flow gradient are the bytes that
 * dvsof_avg_timestamp_fwd / _bwd give at shape (h_k, w_k) on the columns
 * x >> s, y >> s (-1 for an event outside the full-resolution frame; the
 * inside test comes before the shift), with weight = the level's.  With one
 * level of shift 0 the calls give the bytes of dvsof_avg_timestamp_fwd / _bwd.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_avg_timestamp_pyramid.json) and no struct of
 * its own; dvsof.h, the older extension headers and their tables stay as they
 * are.
 */
#ifndef DVSOF_AVG_TIMESTAMP_PYRAMID_H
#define DVSOF_AVG_TIMESTAMP_PYRAMID_H

#include "dvsof_contrast_pyramid.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of the workspace both calls share.  With M = F R C images per level,
 * P_k = h_k w_k, P = M * sum_k P_k and S = 2 F * sum_k P_k, at these byte
 * offsets:
 *   0            q      int64[P]   the images of weights of all levels, in units of 2^-32
 *   8 P          s      int64[P]   the images of weight times distance, in units of 2^-32
 *   16 P         base   int64[P]   the sums of the distances at the events' own level pixels, 2^-32
 *   24 P         sums   int64[S]   the fixed-point gradient sums
 *   24 P + 8 S   count  uint32[P]  the count images, then padding to a multiple of 8 bytes
 * (one contiguous region, zeroed by one fill; a level's image_offset indexes
 * q, s, base and count alike, its sums_offset the sums), and behind it
 *   one 64-byte record per level and image, K M of them, level k's at
 *     row_offset: the eight float64 of dvsof_avg_timestamp.h
 *   one float64 unit per level and frame, K F of them
 *   one 32-byte statistics row per level and image, K M of them, level k's at
 *     row_offset, then nb of them per image for M images, the partials of the
 *     fixed-order reduction, sized for the largest level
 *     (nb = max_k min(max(ceil(h_k w_k / 1024), 1), 128)).
 * Only F, the options, (h, w), K and the levels' h, w and shift are read; 0
 * for arguments the calls refuse.
 */
size_t dvsof_avg_timestamp_pyramid_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                   dvsof_contrast_levels_t levels);

/*
 *   terms   float32[K]: level k's (1/M) sum_m value_m, added in m order in
 *           float64, unweighted
 *   value   one float32: (float) sum_k (double)weight_k * that float64 mean,
 *           added in k order
 * Launches, kernels only: one fill, one splat for all levels (n_events > 0),
 * the two of the statistics per level, one closing wave.  DVSOF_EINVAL before
 * any launch, in this order: those of dvsof_avg_timestamp_fwd on (F, n_events,
 * options), K outside [1, 8], (h, w) or a level's shape outside [1, 32767], a
 * level whose shift is outside [0, 15] or does not give its shape, offsets
 * other than the packed ones, null pointers (the event columns may be null
 * when n_events = 0, p also when polarity = 0; grad_flow is not looked at);
 * DVSOF_ENOSPACE: the workspace is missing or short.  F == 0: nothing to do.
 */
int dvsof_avg_timestamp_pyramid_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                    const int64_t *sample_index, int64_t n_events,
                                    const float *frame_ts /* [2F]: start, stop */,
                                    const int64_t *frame_sample /* [F] */, int F, int h, int w,
                                    int reference_mask, int polarity, dvsof_contrast_levels_t levels,
                                    float *terms, float *value, void *workspace, size_t workspace_bytes,
                                    void *stream);

/*
 * Every level's grad_flow = seed[0] * weight_k * d term_k / d flow_k, every
 * element written.  One launch over the events, one over the elements of all
 * levels, which converts, clears the sums and stores.  Same columns, tables,
 * options, level table and workspace as the dvsof_avg_timestamp_pyramid_fwd
 * call before it.  Error returns as above, with a null grad_flow refused.
 */
int dvsof_avg_timestamp_pyramid_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                    const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                    const int64_t *frame_sample, int F, int h, int w, int reference_mask,
                                    int polarity, dvsof_contrast_levels_t levels, void *workspace,
                                    size_t workspace_bytes, const float *seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_AVG_TIMESTAMP_PYRAMID_H */
