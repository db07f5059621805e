/*
 * dvsof_census.h -- extension of the C ABI of libdvsof_hip.so (dvsof.h, whose
 * conventions hold here): the ternary census term of the framed loss
 * (csrc/census.hip, docs/CENSUS_SPEC.md; Meister, Hur and Roth, AAAI 2018),
 * on the level table of dvsof_loss_fwd: host_scales[k] = {frames [D,h,w], flow
 * [N,2,h,w], grad_flow [N,2,h,w] or NULL, h, w}, start_idx / stop_idx int32[N]
 * the first and second frame of prediction n.  Per level, with A the first
 * frame and Bw the second sampled bilinearly (zeros outside) at (x + u, y + v):
 *
 *   t_I(p,d)  D / sqrt(0.81 + D D), D = I(p + d) - I(p), d over the 7x7 patch
 *             without its centre
 *   dist(p)   sum_d s / (0.1 + s), s = (t_A(p,d) - t_Bw(p,d))^2
 *   counted   3 <= x < w - 3, 3 <= y < h - 3 and the sample position of p
 *             inside [0, w-1] x [0, h-1]
 *   term_k    sum over the counted p of (dist(p)^2 + 1e-6)^0.45, over their
 *             number (1 where there is none)
 *   value     weight * (1/K) sum_k term_k
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_census.json).
 */
#ifndef DVSOF_CENSUS_H
#define DVSOF_CENSUS_H

#include "dvsof.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Bytes of the workspace both calls share, in this order: 16 uint64 (per level
 * the sum of rho in units of 2^-20 and the number of counted pixels); 8 float32
 * (per level weight / (K * max(count, 1)), written by the forward's closing
 * wave); then per level two float32 planes [N,h,w]: Bw, and r = d rho / d dist
 * at the counted pixels, 0 elsewhere.  0 for arguments the calls refuse.
 */
size_t dvsof_census_workspace_bytes(const dvsof_loss_scale_t *host_scales, int num_scales, int N);

/*
 * terms float32[num_scales], value float32[1].  grad_flow is not looked at.
 * Launches: one fill of the 40 header words, the tile sweep over all levels,
 * one closing wave.  Every byte of the workspace the backward reads is written.
 * DVSOF_EINVAL before any launch: null pointers, num_scales outside
 * 1..DVSOF_MAX_SCALES, N < 1, a side < 1 or h * w >= 2^30, more than 2^31 - 1
 * tiles; DVSOF_ENOSPACE: the workspace is missing or too small.
 */
int dvsof_census_fwd(const dvsof_loss_scale_t *host_scales, int num_scales, int N, const int32_t *start_idx,
                     const int32_t *stop_idx, float weight, float *terms, float *value, void *workspace,
                     size_t workspace_bytes, void *stream);

/*
 * host_scales[k].grad_flow = seed[0] * d value / d flow_k, every element
 * written, by one launch without atomics: the same input gives the same bytes.
 * seed: one device float.  Same table, indices and workspace as the
 * dvsof_census_fwd call before it, whose weight the workspace holds.  Error
 * returns as above, and DVSOF_EINVAL for a level without grad_flow.
 */
int dvsof_census_bwd(const dvsof_loss_scale_t *host_scales, int num_scales, int N, const int32_t *start_idx,
                     const int32_t *stop_idx, const float *seed, void *workspace, size_t workspace_bytes,
                     void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_CENSUS_H */
