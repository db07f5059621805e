/*
 * dvsof_contrast_gradient.h -- extension of the C ABI of libdvsof_hip.so
 * (dvsof.h, whose conventions hold here): the contrast term with the second
 * focus function of the contrast-maximisation literature, the mean squared
 * gradient magnitude of the image of warped events (csrc/contrast.hip,
 * docs/CONTRAST_SPEC.md sections 27-31; Gallego, Gehrig and Scaramuzza, CVPR
 * 2019), on the images of dvsof_contrast_multi.h: the same events, frame rule,
 * reference_mask, polarity, image m = (f R + r) C + c, q and count.
 *
 *   GM(A)   the sum over every horizontally or vertically adjacent pair of
 *           pixels of the squared difference, each pair once
 *   term_m  GM(c_m) > 0 ? 1 - GM(I_m)/GM(c_m) : 0;  term = (1/M) sum_m term_m
 *   Lap_m   at a pixel, the sum over its neighbours inside the image of
 *           I_m(pixel) - I_m(neighbour); d term_m / d I_m = -2/GM(c_m) Lap_m
 *
 * The argument lists are those of dvsof_contrast_multi_fwd / _bwd without the
 * result rows: what the calls compute per image is a record in the workspace,
 * whose layout is part of this interface.  The refusals and their order are
 * those of dvsof_contrast_multi.h.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_contrast_gradient.json).
 */
#ifndef DVSOF_CONTRAST_GRADIENT_H
#define DVSOF_CONTRAST_GRADIENT_H

#include "dvsof.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of the workspace both calls share, in this order: the fixed-point
 * gradient sums int64[F,2,h,w]; the Laplacian plane int64[M,h,w] in units of
 * 2^-32; one 48-byte record per image {float64 coef, gmax, term, GM(I); uint64
 * GM(c); int64 max |Lap|}; one float64 unit per frame; one 24-byte row {float64
 * GM(I); uint64 GM(c); int64 max |Lap|} per image and then one per (image,
 * 64x16 tile).  0 for arguments the calls refuse.
 */
size_t dvsof_contrast_gradient_workspace_bytes(int F, int reference_mask, int polarity, int h, int w);

/*
 * q, count: the images of dvsof_contrast_multi_fwd, the same bytes.
 *   term    one float32: the mean over the images of 1 - GM(I_m)/GM(c_m),
 *           images with GM(c_m) = 0 contributing 0
 * Launches: three fills, the splat (n_events > 0), the stencil statistics (one
 * workgroup per tile and image), their closing reduction, one closing wave.
 * Every byte of the workspace the backward reads is written.  Error returns:
 * those of dvsof_contrast_multi_fwd, without the result pointer.
 */
int dvsof_contrast_gradient_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                const int64_t *sample_index, int64_t n_events,
                                const float *frame_ts /* [2F]: start, stop */,
                                const int64_t *frame_sample /* [F] */, const float *flow /* [F,2,h,w] */,
                                int F, int h, int w, int reference_mask, int polarity, int64_t *q,
                                uint32_t *count, float *term, void *workspace, size_t workspace_bytes,
                                void *stream);

/*
 * grad_flow float32[F,2,h,w] = seed[0] * weight * d term / d flow, every
 * element written, by the sums, the unit per frame and the closing kernel of
 * dvsof_contrast_multi_bwd.  Same columns, tables, flow, options, q and
 * workspace as the dvsof_contrast_gradient_fwd call before it; q is checked
 * and not read (the backward gathers the Laplacian plane of the workspace).
 * Error returns as dvsof_contrast_multi_bwd.
 */
int dvsof_contrast_gradient_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                const int64_t *frame_sample, const float *flow, int F, int h, int w,
                                int reference_mask, int polarity, const int64_t *q, void *workspace,
                                size_t workspace_bytes, const float *seed, float weight,
                                float *grad_flow /* [F,2,h,w] */, void *stream);

/*
 * The twins on the encoded event columns of dvsof_event_terms_encoded.h (int16
 * x, y, float32 t, uint8 polarity, the B + 1 offsets of the samples): the same
 * bytes as the calls above on the columns they stand for.
 */
int dvsof_contrast_gradient_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                        const int64_t *sample_event_offsets, int B, int64_t n_events,
                                        const float *frame_ts, const int64_t *frame_sample, const float *flow,
                                        int F, int h, int w, int reference_mask, int polarity_channels, int64_t *q,
                                        uint32_t *count, float *term, void *workspace, size_t workspace_bytes,
                                        void *stream);

int dvsof_contrast_gradient_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                        const int64_t *sample_event_offsets, int B, int64_t n_events,
                                        const float *frame_ts, const int64_t *frame_sample, const float *flow,
                                        int F, int h, int w, int reference_mask, int polarity_channels,
                                        const int64_t *q, void *workspace, size_t workspace_bytes,
                                        const float *seed, float weight, float *grad_flow, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_CONTRAST_GRADIENT_H */
