/*
 * dvsof_iwe_multi.h -- extension of the C ABI of libdvsof_hip.so (dvsof.h,
 * whose conventions hold here): the image of warped events of dvsof_iwe_splat
 * at several reference times of the window and with ON and OFF events
 * accumulated apart (csrc/iwe.hip, docs/IWE_SPEC.md sections 8-13).  The
 * options and the images are those of dvsof_contrast_multi.h, so that the
 * validation metric and the training term look at the same image:
 *
 *   reference_mask  bit 0: the window's start (rho = 0), bit 1: its middle
 *                   (rho = 1/2), bit 2: its end (rho = 1); R = the bits set
 *   polarity        0: one image per (frame, reference), p is not read (C = 1);
 *                   1: channel 0 takes the events with p > 0, channel 1 those
 *                   with p < 0, an event with p == 0 takes no part (C = 2)
 *   image           m = (f R + r) C + c, r counting the set bits upwards;
 *                   M = F R C of them
 *
 * Which events belong to frame f is dvsof_iwe_splat's rule (the position in
 * the columns against frame_event_begin), not the contrast term's.  With
 * reference_mask = 1 and polarity = 0, q holds the bytes of dvsof_iwe_splat
 * and count those of dvsof_count_image_batched over the box (0, 0, h, w).
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_iwe_multi.json); dvsof.h, dvsof_contrast.h and
 * dvsof_contrast_multi.h and their tables stay as they are.
 */
#ifndef DVSOF_IWE_MULTI_H
#define DVSOF_IWE_MULTI_H

#include "dvsof.h"

#ifdef __cplusplus
extern "C" {
#endif

/* M = F R C, the images dvsof_iwe_splat_multi writes; 0 for what that call
 * refuses (and for F = 0). */
int dvsof_iwe_multi_images(int F, int reference_mask, int polarity);

/*
 *   x, y, t, frame_event_begin, frame_ts, flow: as dvsof_iwe_splat takes them
 *   p       int64[n_events], the wire column; may be null with polarity = 0
 *   q       int64[M,h,w]   the images in units of 2^-32, zeroed by the call
 *   count   uint32[M,h,w]  the count image of channel c of frame f, the same
 *           bytes for every reference; zeroed by the call.  dvsof_iwe_stats
 *           and dvsof_iwe_render take q and count as M frames.
 * Launches: two fills and, with n_events > 0, the splat.  DVSOF_EINVAL before
 * any launch: F < 0 or > 65535, n_events < 0, h or w outside [1, 32767],
 * reference_mask outside [1, 7], polarity outside {0, 1}, M > 65535, a null
 * q, count, frame_event_begin, frame_ts or flow, a null x, y or t with
 * n_events > 0, a null p with polarity = 1 and n_events > 0.  F == 0: nothing
 * to do.  n_events == 0: the outputs are zeroed.
 */
int dvsof_iwe_splat_multi(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                          int64_t n_events, const int64_t *frame_event_begin /* [F+1] */,
                          const float *frame_ts /* [2F]: start, stop */, const float *flow /* [F,2,h,w] */,
                          int F, int h, int w, int reference_mask, int polarity, int64_t *q,
                          uint32_t *count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_IWE_MULTI_H */
