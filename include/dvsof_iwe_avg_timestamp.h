/*
 * dvsof_iwe_avg_timestamp.h -- extension of the C ABI of libdvsof_hip.so
 * (dvsof.h, whose conventions hold here): the average-timestamp images of the
 * warped events of a batch of validation frames and their statistics, from
 * which the ratio of squared average timestamps (RSAT; Hagenaars et al.,
 * NeurIPS 2021) is derived beside the flow warp loss (csrc/iwe.hip,
 * docs/IWE_SPEC.md sections 14-21).
 *
 * The options and the images are those of dvsof_iwe_multi.h:
 *
 *   reference_mask  bit 0: the window's start, bit 1: its middle, bit 2: its
 *                   end; R = the bits set
 *   polarity        0: one image per (frame, reference), p is not read (C = 1);
 *                   1: ON and OFF events apart, p == 0 takes no part (C = 2)
 *   image           m = (f R + r) C + c; M = F R C <= 65535 of them
 *
 * Which events belong to frame f is dvsof_iwe_splat's rule (the position in
 * the columns against frame_event_begin; tau clamped, no time test), not the
 * training term's.  What an event does to the images is the term's
 * (docs/AVG_TIMESTAMP_SPEC.md section 2), and so are the statistics of an
 * image (section 3): q and count hold the bytes of dvsof_iwe_splat_multi, and
 * where both rules pick the same events all four images and the rows hold the
 * bytes of dvsof_avg_timestamp_fwd's workspace.
 *
 * An extension header of its own, with its own recorded table
 * (tests/golden/abi_signatures_iwe_avg_timestamp.json); dvsof.h and the older
 * extension headers and their tables stay as they are.
 */
#ifndef DVSOF_IWE_AVG_TIMESTAMP_H
#define DVSOF_IWE_AVG_TIMESTAMP_H

#include "dvsof.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The bytes of the caller-provided region of images.  With P = M h w:
 *   q      int64[P]   at 0      the images of warped events, units of 2^-32
 *   s      int64[P]   at 8 P    weight times distance in time, units of 2^-32
 *   base   int64[P]   at 16 P   the distances at the events' own pixels
 *   count  uint32[P]  at 24 P   the count image of the image's channel
 * padded to a multiple of 8.  0 for what dvsof_iwe_avg_timestamp refuses and
 * for F = 0.
 */
size_t dvsof_iwe_avg_timestamp_image_bytes(int F, int h, int w, int reference_mask, int polarity);

/* Room for M nb partial rows of 32 bytes, nb the partials of an h x w image
 * (dvsof_iwe_stats_workspace_bytes's); 0 as above. */
size_t dvsof_iwe_avg_timestamp_workspace_bytes(int F, int h, int w, int reference_mask, int polarity);

/*
 *   x, y, t, p, frame_event_begin, frame_ts, flow: as dvsof_iwe_splat_multi
 *           takes them
 *   images  the region above, image_bytes of it; zeroed by the call
 *   rows    M rows of 32 bytes, one per image:
 *           { double S, S0, peak; uint32_t n, n0; }
 *           S = sum_p T^2, S0 = sum_p T0^2 in the fixed order of dvsof_iwe_stats,
 *           peak = max_p 2 T / (I + 2^-10), n the pixels with q > 0, n0 those
 *           with count > 0
 *   workspace  dvsof_iwe_avg_timestamp_workspace_bytes of scratch
 * Launches, kernels only: one fill of the whole region, the splat with
 * n_events > 0, two for the statistics.  Before any launch DVSOF_EINVAL: F < 0
 * or > 65535, n_events < 0, reference_mask outside [1, 7], polarity outside
 * {0, 1}, M > 65535, h or w outside [1, 32767], a null images, rows,
 * frame_event_begin, frame_ts or flow, a null x, y or t with n_events > 0, a
 * null p with polarity = 1 and n_events > 0; then DVSOF_ENOSPACE: image_bytes
 * or workspace_bytes too small, a null workspace.  F == 0: nothing to do.
 * n_events == 0: the images are zeroed and the rows are those of empty images.
 */
int dvsof_iwe_avg_timestamp(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                            int64_t n_events, const int64_t *frame_event_begin /* [F+1] */,
                            const float *frame_ts /* [2F]: start, stop */, const float *flow /* [F,2,h,w] */,
                            int F, int h, int w, int reference_mask, int polarity, void *images,
                            size_t image_bytes, void *rows, void *workspace, size_t workspace_bytes,
                            void *stream);

/*
 * canvas uint8[M,h,2w,3]: per image the average distance in time at zero flow
 * T0 on the left, the average distance T after the warp on the right, grey on
 * the fixed scale [0, 1): g = min(255, (int)(T * 255.f + 0.5f)) of the float64
 * T converted once to float32.  images: the region dvsof_iwe_avg_timestamp
 * filled for the same F, h, w, reference_mask and polarity.  DVSOF_EINVAL: the
 * sizes and options above, a null images or canvas.  F == 0: nothing to do.
 */
int dvsof_iwe_avg_timestamp_render(const void *images, int F, int h, int w, int reference_mask, int polarity,
                                   uint8_t *canvas, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_IWE_AVG_TIMESTAMP_H */
