/*
 * dvsof_avg_timestamp.h -- extension of the C ABI of libdvsof_hip.so (dvsof.h,
 * whose conventions hold here): the average-timestamp term of a training from
 * events alone and its gradient with respect to the flow
 * (csrc/avg_timestamp.hip, docs/AVG_TIMESTAMP_SPEC.md; Zhu et al., CVPR 2019;
 * Hagenaars et al., NeurIPS 2021).
 *
 * The options, the images m = (f R + r) C + c and the events that take part in
 * an image are those of dvsof_contrast_multi.h.  Beside its weight an event
 * splats its distance in time from the reference, a = |tau - rho| in [0, 1];
 * per pixel T = A / (I + 2^-10) is the average distance of the events that
 * landed there, T0 the same at zero flow, and
 *   value_m = (sum_p T^2 / n) / (sum_p T0^2 / n0),
 * n and n0 the pixels that hold weight; term = (1/M) sum_m value_m.  At zero
 * flow every image that has events gives exactly 1.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_avg_timestamp.json); dvsof.h, the older
 * extension headers and their tables stay as they are.
 */
#ifndef DVSOF_AVG_TIMESTAMP_H
#define DVSOF_AVG_TIMESTAMP_H

#include "dvsof.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of the workspace both calls share.  With M = F R C images, P = M h w
 * and S = 2 F h w, at these byte offsets:
 *   0            q      int64[P]   the images of weights, in units of 2^-32
 *   8 P          s      int64[P]   the images of weight times distance, in units of 2^-32
 *   16 P         base   int64[P]   the sums of the distances at the events' own pixels, 2^-32
 *   24 P         sums   int64[S]   the fixed-point gradient sums
 *   24 P + 8 S   count  uint32[P]  the count images, then padding to a multiple of 8 bytes
 * (one contiguous region, zeroed by one fill), and behind it
 *   one 64-byte record per image, eight float64:
 *     {S, S0, n, n0, peak = max_p 2 T D, value, 2 k, gmax = k peak}, k = n0 / (n S0),
 *     D = 1 / (I + 2^-10); k = 0 where the image has no gradient
 *   one float64 unit per frame
 *   one 32-byte statistics row per image {float64 S, S0, peak; uint32 n, n0},
 *   then nb of them per image, the partials of the fixed-order reduction
 *   (nb = min(max(ceil(h w / 1024), 1), 128), that of dvsof_iwe_stats).
 * 0 for arguments the calls refuse.
 */
size_t dvsof_avg_timestamp_workspace_bytes(int F, int reference_mask, int polarity, int h, int w);

/*
 * Which events take part in image m is dvsof_contrast_multi_fwd's rule, and q
 * and count are its bytes.
 *   p       int64[n_events], the wire column; may be null with polarity = 0
 *   term    one float32: (float)((1/M) sum_m value_m), added in image order in
 *           float64; value_m = 0 for an image without events, 1 (and no
 *           gradient) for an image whose events all left it
 * Launches, kernels only: one fill, the splat (n_events > 0), two of the
 * statistics, one closing wave.  DVSOF_EINVAL before any launch: F < 0 or
 * > 65535, n_events < 0, reference_mask outside [1, 7], polarity outside
 * {0, 1}, M > 65535, h or w outside [1, 32767], null pointers (the event
 * columns may be null when n_events = 0, p also when polarity = 0);
 * DVSOF_ENOSPACE: the workspace is missing or short.  F == 0: nothing to do.
 */
int dvsof_avg_timestamp_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                            const int64_t *sample_index, int64_t n_events,
                            const float *frame_ts /* [2F]: start, stop */,
                            const int64_t *frame_sample /* [F] */, const float *flow /* [F,2,h,w] */,
                            int F, int h, int w, int reference_mask, int polarity, float *term,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * grad_flow float32[F,2,h,w] = seed[0] * weight * d term / d flow, every
 * element written.  All R C images of a frame add into the same fixed-point
 * sums with one unit per frame; one thread per element converts, clears the
 * sum and stores: two launches.  Same columns, tables, flow, options and
 * workspace as the dvsof_avg_timestamp_fwd call before it.  Error returns as
 * above.
 */
int dvsof_avg_timestamp_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                            const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                            const int64_t *frame_sample, const float *flow, int F, int h, int w,
                            int reference_mask, int polarity, void *workspace, size_t workspace_bytes,
                            const float *seed, float weight, float *grad_flow /* [F,2,h,w] */,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_AVG_TIMESTAMP_H */
