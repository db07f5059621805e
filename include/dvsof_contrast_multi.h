/*
 * dvsof_contrast_multi.h -- extension of the C ABI of libdvsof_hip.so (dvsof.h,
 * whose conventions hold here): the contrast-maximisation term of
 * dvsof_contrast.h with several reference times and with ON and OFF events
 * accumulated apart (csrc/contrast.hip, docs/CONTRAST_SPEC.md sections
 * 11-15; Zhu et al., CVPR 2019; Shiba et al., ECCV 2022).
 *
 *   reference_mask  bit 0: the window's start (rho = 0), bit 1: its middle
 *                   (rho = 1/2), bit 2: its end (rho = 1); R = the bits set
 *   polarity        0: one image per (frame, reference), p is not read (C = 1);
 *                   1: channel 0 takes the events with p > 0, channel 1 those
 *                   with p < 0, an event with p == 0 takes no part (C = 2)
 *   image           m = (f R + r) C + c, r counting the set bits upwards;
 *                   M = F R C of them
 *
 * An event is carried over sig = tau - rho (one float32 subtraction) instead
 * of tau; everything else is dvsof_contrast_fwd / _bwd.  With reference_mask =
 * 1 and polarity = 0 the calls give the bytes of dvsof_contrast_fwd / _bwd.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_contrast_multi.json); dvsof.h and
 * dvsof_contrast.h and their tables stay as they are.
 */
#ifndef DVSOF_CONTRAST_MULTI_H
#define DVSOF_CONTRAST_MULTI_H

#include "dvsof.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of the workspace both calls share, in this order: the fixed-point
 * gradient sums int64[F,2,h,w]; one 32-byte record {mean, coef, gmax, term}
 * (four float64) per image; one float64 unit per frame; the partials of
 * dvsof_iwe_stats for M frames.  0 for arguments the calls refuse.
 */
size_t dvsof_contrast_multi_workspace_bytes(int F, int reference_mask, int polarity, int h, int w);

/*
 * Which events take part in frame f is dvsof_contrast_fwd's rule; with
 * polarity = 1 an event takes part in the images of its own channel only.
 *   p       int64[n_events], the wire column; may be null with polarity = 0
 *   q       int64[M,h,w]   the images in units of 2^-32, zeroed by the call
 *   count   uint32[M,h,w]  the count image of channel c of frame f, the same
 *           bytes for every reference; zeroed by the call
 *   result  one statistics row per image (dvsof_iwe_stats on M frames)
 *   term    one float32: (1/M) sum_m (1 - var(I_m)/var(c_m)), images with
 *           var(c_m) = 0 contributing 0
 * Launches: three fills, the splat (n_events > 0), the two of dvsof_iwe_stats,
 * one closing wave.  DVSOF_EINVAL before any launch: F < 0 or > 65535,
 * n_events < 0, h or w outside [1, 32767], reference_mask outside [1, 7],
 * polarity outside {0, 1}, M > 65535, null pointers (the event columns may be
 * null when n_events = 0, p also when polarity = 0); DVSOF_ENOSPACE: the
 * workspace is missing or short.  F == 0: nothing to do.
 */
int dvsof_contrast_multi_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                             const int64_t *sample_index, int64_t n_events,
                             const float *frame_ts /* [2F]: start, stop */,
                             const int64_t *frame_sample /* [F] */, const float *flow /* [F,2,h,w] */,
                             int F, int h, int w, int reference_mask, int polarity, int64_t *q,
                             uint32_t *count, dvsof_iwe_result_t *result, float *term, void *workspace,
                             size_t workspace_bytes, void *stream);

/*
 * grad_flow float32[F,2,h,w] = seed[0] * weight * d term / d flow, every
 * element written.  All R C images of a frame add into the same fixed-point
 * sums with one unit per frame; one thread per element converts, clears the
 * sum and stores.  Same columns, tables, flow, options, q and workspace as
 * the dvsof_contrast_multi_fwd call before it.  Error returns as above.
 */
int dvsof_contrast_multi_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                             const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                             const int64_t *frame_sample, const float *flow, int F, int h, int w,
                             int reference_mask, int polarity, const int64_t *q, void *workspace,
                             size_t workspace_bytes, const float *seed, float weight,
                             float *grad_flow /* [F,2,h,w] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_CONTRAST_MULTI_H */
