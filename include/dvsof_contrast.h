/*
 * dvsof_contrast.h -- extension of the C ABI of libdvsof_hip.so (dvsof.h, whose
 * conventions hold here): the contrast-maximisation term of the training loss
 * (csrc/contrast.hip, docs/CONTRAST_SPEC.md): term = mean over frames of
 * 1 - var(I_f)/var(c_f), I_f the image of warped events of frame f, c_f its
 * count image, and the gradient of that term with respect to the flow.
 *
 * An extension header of its own: the entry points of dvsof.h are a recorded
 * table (tests/golden/abi_signatures.json) that stays as it is; this header has
 * its own (tests/golden/abi_signatures_contrast.json).  The binding reads both
 * (_abi.py) and the library exports both.
 */
#ifndef DVSOF_CONTRAST_H
#define DVSOF_CONTRAST_H

#include "dvsof.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of the workspace both calls share: the fixed-point gradient sums
 * int64[F,2,h,w], one 32-byte record {mean, coef, gmax, term} per frame, one
 * float64 unit per frame and the partials of dvsof_iwe_stats: what
 * dvsof_contrast_multi_workspace_bytes(F, 1, 0, h, w) of dvsof_contrast_multi.h
 * returns, whose kernels these calls run (8 F bytes more than while the unit
 * was the record's third field).  0 for sizes the calls refuse.
 */
size_t dvsof_contrast_workspace_bytes(int F, int h, int w);

/*
 * An event of the wire columns x, y, t, sample_index (n_events entries) takes
 * part in frame f iff sample_index == frame_sample[f], 0 <= x < w, 0 <= y < h
 * and frame_ts[2f] <= t <= frame_ts[2f+1] (a test, not a clamp; an event may
 * take part in several frames).  Its warp and corner weights are steps 1-8 of
 * dvsof_iwe_splat.
 *   q       int64[F,h,w]   the images in units of 2^-32, zeroed by the call
 *   count   uint32[F,h,w]  the events that take part per pixel, zeroed by the call
 *   result  one statistics row per frame (dvsof_iwe_stats of q and count)
 *   term    one float32: (1/F) sum_f (1 - var(I_f)/var(c_f)), frames with
 *           var(c_f) = 0 contributing 0; evaluated on the device in float64
 * The workspace is left ready for dvsof_contrast_bwd.  Launches: three fills,
 * the splat (n_events > 0), the two of dvsof_iwe_stats, one closing wave.
 * DVSOF_EINVAL before any launch: F < 0 or > 65535, n_events < 0, h or w
 * outside [1, 32767], null pointers; DVSOF_ENOSPACE: the workspace is missing
 * or short.  F == 0: nothing to do.
 */
int dvsof_contrast_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *sample_index,
                       int64_t n_events, const float *frame_ts /* [2F]: start, stop */,
                       const int64_t *frame_sample /* [F] */, const float *flow /* [F,2,h,w] */, int F,
                       int h, int w, int64_t *q, uint32_t *count, dvsof_iwe_result_t *result, float *term,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * grad_flow float32[F,2,h,w] = seed[0] * weight * d term / d flow, every
 * element written (no memset, no floating-point atomics): one thread per
 * event recomputes the forward's warp, reads q at its four corners and adds
 * two 64-bit fixed-point integers at its own pixel of the workspace; one
 * thread per element converts, clears the sum and stores.  Same columns,
 * tables, flow, q and workspace as the dvsof_contrast_fwd call before it.
 *   seed    device scalar: the gradient arriving at weight * term
 * Error returns as above.
 */
int dvsof_contrast_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *sample_index,
                       int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                       const float *flow, int F, int h, int w, const int64_t *q, void *workspace,
                       size_t workspace_bytes, const float *seed, float weight,
                       float *grad_flow /* [F,2,h,w] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_CONTRAST_H */
