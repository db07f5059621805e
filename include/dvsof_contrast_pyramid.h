/*
 * dvsof_contrast_pyramid.h -- extension of the C ABI of libdvsof_hip.so
 * (dvsof.h, whose conventions hold here): the contrast-maximisation term of
 * dvsof_contrast_multi.h on every flow scale of the network at once
 * (csrc/contrast.hip, docs/CONTRAST_SPEC.md sections 19-23).
 *
 * (h, w) is the frame the event coordinates live in.  Level k has a shape
 * (h_k, w_k) and a shift s in [0, 15] with h_k == ceil(h / 2^s) and
 * w_k == ceil(w / 2^s).  Which events take part in frame f is decided at
 * full resolution, by dvsof_contrast_multi_fwd's rule on (h, w); such an
 * event sits at level pixel (y >> s, x >> s), reads flow_k there and is
 * splatted into the level's images.  Per level the images, counts, rows,
 * records, units, sums and flow gradient are the bytes that
 * dvsof_contrast_multi_fwd / _bwd give at shape (h_k, w_k) on the columns
 * x >> s, y >> s (-1 for an event outside the full-resolution frame), with
 * weight = the level's.  With one level of shift 0 the calls give the bytes
 * of dvsof_contrast_multi_fwd / _bwd.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_contrast_pyramid.json) and the two structs
 * below; dvsof.h, the older extension headers and their tables stay as they
 * are.
 */
#ifndef DVSOF_CONTRAST_PYRAMID_H
#define DVSOF_CONTRAST_PYRAMID_H

#include "dvsof.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * One level.  With M = F R C images per level and P_k = h_k w_k, the offsets
 * are those of the packed layout, in elements, and are checked:
 *   image_offset  M * (P_0 + ... + P_{k-1}), into q and into count
 *   row_offset    k * M, into result and into the image records
 *   sums_offset   2 F * (P_0 + ... + P_{k-1}), into the fixed-point sums
 */
typedef struct {
    const float *flow;   /* [F,2,h_k,w_k] */
    float *grad_flow;    /* [F,2,h_k,w_k]; read by dvsof_contrast_pyramid_bwd only */
    int h, w;
    int shift;
    float weight;
    size_t image_offset;
    size_t row_offset;
    size_t sums_offset;
} dvsof_contrast_level_t;

/* The level table, passed by value: the first K of the eight entries are read, 1 <= K <= 8 */
typedef struct {
    int K;
    dvsof_contrast_level_t level[8];
} dvsof_contrast_levels_t;

/*
 * Bytes of the workspace both calls share, in this order, with
 * P = M * sum_k P_k and S = 2 F * sum_k P_k:
 *   q      int64[P]    the images of all levels in units of 2^-32
 *   sums   int64[S]    the fixed-point gradient sums
 *   count  uint32[P]   the count images, then padding to a multiple of 8 bytes
 *   one 32-byte record {mean, coef, gmax, term} (four float64) per image, K M of them
 *   one float64 unit per level and frame, K F of them
 *   the partials of dvsof_iwe_stats for M frames of the largest level
 * q, sums and count are one contiguous region, zeroed by one fill.  Only F,
 * the options, (h, w), K and the levels' h, w and shift are read; 0 for
 * arguments the calls refuse.
 */
size_t dvsof_contrast_pyramid_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                              dvsof_contrast_levels_t levels);

/*
 *   result  K M statistics rows, level k's at row_offset
 *   terms   float32[K]: level k's (1/M) sum_m term_m, added in m order in
 *           float64, unweighted
 *   value   one float32: (float) sum_k (double)weight_k * that float64 mean,
 *           added in k order
 * Launches: one fill, one splat for all levels (n_events > 0), the two of
 * dvsof_iwe_stats per level, one closing wave.  DVSOF_EINVAL before any
 * launch, in this order: those of dvsof_contrast_multi_fwd on (F, n_events,
 * options), K outside [1, 8], (h, w) or a level's shape outside [1, 32767], a
 * level whose shift is outside [0, 15] or does not give its shape, offsets
 * other than the packed ones, null pointers (the event columns may be null
 * when n_events = 0, p also when polarity = 0; grad_flow is not looked at);
 * DVSOF_ENOSPACE: the workspace is missing or short.  F == 0: nothing to do.
 */
int dvsof_contrast_pyramid_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                               const int64_t *sample_index, int64_t n_events,
                               const float *frame_ts /* [2F]: start, stop */,
                               const int64_t *frame_sample /* [F] */, int F, int h, int w,
                               int reference_mask, int polarity, dvsof_contrast_levels_t levels,
                               dvsof_iwe_result_t *result, float *terms, float *value, void *workspace,
                               size_t workspace_bytes, void *stream);

/*
 * Every level's grad_flow = seed[0] * weight_k * d term_k / d flow_k, every
 * element written.  One launch over the events, one over the elements of all
 * levels, which converts, clears the sums and stores.  Same columns, tables,
 * options, level table and workspace as the dvsof_contrast_pyramid_fwd call
 * before it.  Error returns as above, with a null grad_flow refused.
 */
int dvsof_contrast_pyramid_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                               const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                               const int64_t *frame_sample, int F, int h, int w, int reference_mask,
                               int polarity, dvsof_contrast_levels_t levels, void *workspace,
                               size_t workspace_bytes, const float *seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_CONTRAST_PYRAMID_H */
