/*
 * dvsof_loss_frameless.h -- extension of the C ABI of libdvsof_hip.so (dvsof.h,
 * whose conventions hold here): the two terms of the multi-scale loss that
 * read no frame -- Charbonnier smoothness and the out-of-border regulariser of
 * utils/loss.py:76-119 -- and the gradient of
 *
 *   loss = (w_s sum_k smooth_k + w_o sum_k border_k) / K * loss_scale
 *
 * into every grad_flow, for a training run from an event-only recording
 * (csrc/loss_frameless.hip, docs/FRAMELESS_SPEC.md).  The arithmetic is that of
 * dvsof_loss_fused for these two terms; no pyramid is built, no frame is read
 * and nothing is gathered.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_loss_frameless.json); dvsof.h, dvsof_contrast.h,
 * dvsof_contrast_multi.h and dvsof_iwe_multi.h and their tables stay as they
 * are.
 */
#ifndef DVSOF_LOSS_FRAMELESS_H
#define DVSOF_LOSS_FRAMELESS_H

#include "dvsof.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of workspace dvsof_loss_frameless needs for these scales; 0 for what
 * that call refuses with DVSOF_EINVAL.  host_scales[k].frames is not read. */
size_t dvsof_loss_frameless_workspace_bytes(const dvsof_loss_scale_t *host_scales, int num_scales,
                                            int N);

/*
 *   host_scales   .flow [N,2,h,w] and .grad_flow [N,2,h,w] (written in full)
 *                 of every scale; .frames is not read and may be NULL
 *   host_weights  host float[2]: smoothness, out-of-border
 *   terms         device float[3*num_scales], rows as dvsof_loss_fused writes
 *                 them: smoothness_k, photometric_k, outborder_k; the
 *                 photometric row is written as +0
 *   loss_out      device float[1]
 *   oob_count     device int32[num_scales*N]: out-of-border pixels per
 *                 (scale, sample) (utils/loss.py:101)
 * Launches, kernels only (nothing is zeroed by a memset or a copy): the
 * out-of-border count, one sweep over all scales, one closing workgroup.
 * Workgroup sums are added in 64-bit fixed point (2^-20) with integer atomics:
 * same input, same bits.
 * DVSOF_EINVAL before any launch: num_scales outside 1..DVSOF_MAX_SCALES,
 * N < 1, a null host_scales, host_weights, flow, grad_flow, terms, loss_out or
 * oob_count, a side below 1, a scale of more than 2^28 - 1 pixels, more than
 * 2^30 - 1 tiles.  DVSOF_ENOSPACE, also
 * before any launch: a null workspace or fewer than
 * dvsof_loss_frameless_workspace_bytes bytes of it.
 */
int dvsof_loss_frameless(const dvsof_loss_scale_t *host_scales, int num_scales, int N,
                         const float *host_weights, float loss_scale, float *terms,
                         float *loss_out, int32_t *oob_count, void *workspace,
                         size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_LOSS_FRAMELESS_H */
