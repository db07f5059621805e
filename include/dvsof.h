/*
 * dvsof.h -- C ABI of libdvsof_hip.so, the MI355X (gfx950) implementation of
 * the optical-flow training hot path of e-sha/dvs_of_training_framework.
 *
 * Conventions
 *   - every entry point returns int: 0 = ok, >0 = hipError_t of the failing
 *     HIP call, <0 = DVSOF_E* argument error.  No exceptions cross the ABI.
 *   - all pointers are DEVICE pointers unless a parameter is named host_*.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     Calls only enqueue work: no allocation, no synchronisation, no
 *     host<->device copies, so a caller may capture them into a hipGraph.
 *   - scratch memory is provided by the caller (sizes from *_workspace_bytes);
 *     the library retains no pointer after a call returns.
 *   - tensors are dense, row-major, float32 unless stated.  "NCHW"/"NHWC"
 *     name the memory order.
 *
 * Each entry point cites the reference interface it replaces
 * (paths relative to the reference repository root).
 */
#ifndef DVSOF_H
#define DVSOF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVSOF_VERSION 100 /* 0.1.0 */
#define DVSOF_MAX_SCALES 8

enum {
    DVSOF_OK = 0,
    DVSOF_EINVAL = -1,  /* bad shape / null pointer / unsupported size */
    DVSOF_ENOSPACE = -2, /* workspace too small */
    DVSOF_ECOMM = -3     /* RCCL missing or a collective / communicator call failed */
};

int dvsof_version(void);
/* static string for a code returned by any entry point */
const char *dvsof_error_string(int code);

/* ------------------------------------------------------------------ *
 * Event stream  ->  images / voxel grids
 * ------------------------------------------------------------------ */

/*
 * Per-pixel event count (integer histogram, idx = y*W + x).
 * Replaces get_count_image, utils/data.py:120-136 (numpy add.at, uint64).
 * out[H*W] uint32 is zeroed by the call.  Events outside the frame are
 * ignored (the reference raises; the Python wrapper checks and raises).
 */
int dvsof_count_image(const int64_t *x, const int64_t *y, int64_t n_events,
                      int H, int W, uint32_t *out, void *stream);

/*
 * Event batch -> polarity-signed, time-bilinear voxel grid out[B,C,H,W]
 * (NCHW, zeroed by the call), docs/VOXEL_SPEC.md.
 * Replaces EV_FlowNet Model.quantize / quantization_layer as called at
 * utils/training.py:59-64 and scripts/quantize_preprocessed.py:87-91; output
 * contract utils/dataset.py:436-448.  Event columns are the reference's wire
 * format (utils/dataset.py:961-1020): int64 x,y,polarity,sample_index and
 * float32 window-relative timestamp.  t0[b], t1[b] are the window of sample b.
 * n_events may be 0 (utils/loss.py:217-240 probes the model that way).
 * polarity is a SIGN: > 0 adds, < 0 subtracts, 0 contributes nothing.
 * bin0 (int32[n]) / lin0 (int64[n]) are optional debug outputs: the lower
 * temporal bin and the linear index of (b,bin0,y,x), -1 for dropped events.
 */
int dvsof_voxelize_fwd(const int64_t *x, const int64_t *y, const float *t,
                       const int64_t *polarity, const int64_t *sample_index,
                       int64_t n_events, const float *t0, const float *t1,
                       int B, int C, int H, int W, float *out, int32_t *bin0,
                       int64_t *lin0, void *stream);

/*
 * Same result through LDS-staged voxel tiles, two launches: events are
 * bucketed per 32x32 tile in one coalesced pass, each tile is accumulated in
 * LDS and stored with plain coalesced writes (no zero-fill pass, no global
 * float atomics).  Falls back to dvsof_voxelize_fwd for tiny inputs or when
 * the workspace is missing/too small.  Integer parts are identical; float
 * sums differ only in accumulation order.
 *
 * Workspace contract: the first dvsof_voxelize_control_bytes() bytes are
 * control words (bucket cursors, counters).  They must be ZERO when the call
 * starts executing and the call leaves them zero again (the kernels clean up
 * after themselves).  flags:
 *   0                   the call zero-fills the control words first (a fill
 *                       KERNEL: no entry point of this library enqueues
 *                       hipMemsetAsync, so a stream capture of it holds kernel
 *                       nodes only)
 *   DVSOF_VOX_WS_CLEAN  the caller guarantees they are zero (zero-filled once,
 *                       then only used by calls of this family, one at a time
 *                       in stream order): no fill is enqueued
 */
#define DVSOF_VOX_WS_CLEAN 1
size_t dvsof_voxelize_workspace_bytes(int64_t n_events, int B, int C, int H,
                                      int W);
/* 0 when the thread-per-event kernel serves this size (no control words) */
size_t dvsof_voxelize_control_bytes(int64_t n_events, int B, int C, int H,
                                    int W);
int dvsof_voxelize_tiled(const int64_t *x, const int64_t *y, const float *t,
                         const int64_t *polarity, const int64_t *sample_index,
                         int64_t n_events, const float *t0, const float *t1,
                         int B, int C, int H, int W, float *out, int32_t *bin0,
                         int64_t *lin0, void *workspace,
                         size_t workspace_bytes, int flags, void *stream);

/*
 * The same grid from the reference's ENCODED event columns (encode_batch,
 * utils/dataset.py:240-305: int16 x, int16 y, float32 timestamp, bool
 * polarity = 9 bytes/event instead of 44).  sample_event_offsets[B+1] = index
 * of the first event of every sample (from events_per_element /
 * elements_per_sample).  Workspace and flags: as dvsof_voxelize_tiled.
 */
int dvsof_voxelize_encoded(const int16_t *x, const int16_t *y, const float *t,
                           const uint8_t *polarity,
                           const int64_t *sample_event_offsets,
                           int64_t n_events, const float *t0, const float *t1,
                           int B, int C, int H, int W, float *out,
                           int32_t *bin0, int64_t *lin0, void *workspace,
                           size_t workspace_bytes, int flags, void *stream);

/*
 * LEARNABLE event representation (csrc/learned_voxel.hip,
 * docs/LEARNED_VOXEL_SPEC.md): the grid above with the triangle kernel replaced
 * by a piecewise-linear lookup table theta[K], K = 2*R*S + 1 float32 knots
 * (R = radius in bins, 1..3; S = knots per bin, 1..16; knot j at offset
 * j/S - R bins).  Drop rule, windows, tn and the polarity sign are those of
 * dvsof_voxelize_fwd; an event adds sign * (theta[j]*(1-g) + theta[j+1]*g) to
 * every bin c with 0 <= u = ((tn - c) + R) * S < 2*R*S, j = floor(u), g = u - j.
 * With theta[j] = max(0, 1 - |j/S - R|) that is the grid of dvsof_voxelize_fwd.
 * Upstream's learnable quantization layer lives in the absent EV_FlowNet
 * submodule (train_flownet.py:50-54,79-99 only splits its parameter group and
 * schedules its learning rate): parity unpinned, the spec is this build's.
 *
 * out[B,C,H,W] is zeroed by the call (a fill kernel: a stream capture holds
 * kernel nodes only), then one thread per event adds with memory-side float
 * atomics: the sum of a voxel depends on the order of its addends, inside the
 * bound the spec derives.  n_events may be 0 (zeros).  No workspace.
 */
int dvsof_learned_voxelize_fwd(const int64_t *x, const int64_t *y,
                               const float *t, const int64_t *polarity,
                               const int64_t *sample_index, int64_t n_events,
                               const float *t0, const float *t1,
                               const float *theta, int R, int S, int B, int C,
                               int H, int W, float *out, void *stream);

/* The same kernel body over the 9 B/event ENCODED columns and
 * sample_event_offsets[B+1] (see dvsof_voxelize_encoded). */
int dvsof_learned_voxelize_encoded(const int16_t *x, const int16_t *y,
                                   const float *t, const uint8_t *polarity,
                                   const int64_t *sample_event_offsets,
                                   int64_t n_events, const float *t0,
                                   const float *t1, const float *theta, int R,
                                   int S, int B, int C, int H, int W,
                                   float *out, void *stream);

/*
 * Gradient with respect to the table: for every kept (event, bin)
 *   gtheta[j]   += sign * gV[b,c,y,x] * (1-g)
 *   gtheta[j+1] += sign * gV[b,c,y,x] * g
 * gV[B,C,H,W] is the gradient of the grid; gtheta[K] is WRITTEN (zeros for
 * n_events = 0).  There is no gradient to events or timestamps.
 * encoded = 0: x, y, polarity are the int64 wire columns and `sample` is
 * sample_index[n]; encoded = 1: int16 x, int16 y, uint8 polarity and `sample`
 * is sample_event_offsets[B+1].
 * Fixed-order reduction, no float atomics, bitwise reproducible: a thread adds
 * its events in ascending order, a wave's threads are combined by a shuffle
 * tree, a block's waves in order into part[block][K] (the workspace), and a
 * closing kernel adds the partials in block order in float64 and rounds once.
 * dvsof_learned_voxelize_bwd_blocks(n) is the number of blocks (128 threads
 * each) the call uses for n events: with it the longest chain of float32
 * additions a term passes through is known to the caller (the spec's `m`).
 */
size_t dvsof_learned_voxelize_bwd_workspace_bytes(int64_t n_events, int R,
                                                  int S);
int dvsof_learned_voxelize_bwd_blocks(int64_t n_events);
int dvsof_learned_voxelize_bwd(const void *x, const void *y, const float *t,
                               const void *polarity, const int64_t *sample,
                               int encoded, int64_t n_events, const float *t0,
                               const float *t1, int R, int S, int B, int C,
                               int H, int W, const float *gV, float *gtheta,
                               void *workspace, size_t workspace_bytes,
                               void *stream);

/*
 * The same gradient into a RESIDENT slot gtheta[K] the caller keeps for the
 * whole run (net.LearnedVoxelGrid.make_resident: the captured step and the
 * gradient exchange need a gradient with a stable address).  The reduction is
 * that of dvsof_learned_voxelize_bwd up to s = (float)(float64 block-order
 * sum); the closing kernel then stores
 *   accumulate = 0:  gtheta[j] = s            (the bits of ..._bwd)
 *   accumulate = 1:  gtheta[j] = gtheta[j] + s   (ONE float32 add: the rounding
 *                    of autograd's `grad += g` over micro-batches)
 * Kernel launches only -- no memset, no copy, no float atomics -- so a stream
 * capture holds nothing else.  n_events = 0: accumulate = 0 writes zeros,
 * accumulate = 1 enqueues nothing (gtheta keeps its bits, -0.0 included).
 * The workspace may be larger than needed (sized for a capacity with
 * dvsof_learned_voxelize_bwd_workspace_bytes(capacity, R, S)): the number of
 * blocks, and with it the order of the sum, follows n_events alone.
 */
int dvsof_learned_voxelize_bwd_into(const void *x, const void *y,
                                    const float *t, const void *polarity,
                                    const int64_t *sample, int encoded,
                                    int64_t n_events, const float *t0,
                                    const float *t1, int R, int S, int B,
                                    int C, int H, int W, const float *gV,
                                    float *gtheta, int accumulate,
                                    void *workspace, size_t workspace_bytes,
                                    void *stream);

/*
 * ORDER-INDEPENDENT forward of the learnable representation (opt-in:
 * learned_voxel.voxelize(..., deterministic=True)).  Drop rule, tn, u, j, g and
 * w are those of dvsof_learned_voxelize_fwd; from w on
 *   Q = (int64) trunc((double)(s*w) * 2^32)         toward zero
 *   A[b,c,y,x] = sum of Q                            64-bit integers, any order
 *   out[b,c,y,x] = (float)((double)A * 2^-32)        once per voxel
 * so the same events give the same bits in whatever order they arrive
 * (docs/LEARNED_VOXEL_SPEC.md, "Order-independent forward").  Defined while the
 * sum of |w| of every voxel stays below 2^31; outside that range the result is
 * unspecified (nothing is checked on the host, nothing faults).
 * Where the plan of dvsof_voxelize_tiled applies (n_events >= 4096, at most 8192
 * tiles, at most 37 bins) the call is its two launches -- bucket pass, tile pass
 * with the table and the accumulators in LDS -- on a workspace of the same
 * layout and contract (control words first, self-cleaning, DVSOF_VOX_WS_CLEAN).
 * Elsewhere it is three kernels: zero an int64 scratch grid [B,C,H,W] in the
 * workspace, one thread per event adding Q with 64-bit integer atomics, one
 * conversion per voxel; the same bits.  Kernel launches only, no memset, no
 * copy.  n_events = 0 zero-fills out and needs no workspace.
 * Columns and `encoded`: as dvsof_learned_voxelize_bwd.  flags:
 *   DVSOF_VOX_WS_CLEAN  as dvsof_voxelize_tiled (ignored where there are no
 *                       control words)
 *   DVSOF_LV_GLOBAL     take the three-kernel path whatever the size
 *   DVSOF_LV_EPT8 / DVSOF_LV_EPT16  8 / 16 events per thread in the bucket pass
 *                       whatever n_events (default: 4, 8 from 2 Mi, 16 from
 *                       3 Mi events); not both
 * The two size queries take the flags of the call they size.  DVSOF_ENOSPACE:
 * workspace missing or too small (nothing is enqueued); DVSOF_EINVAL: bad
 * shape, null pointer, unknown flag, workspace not 16-byte aligned.
 */
#define DVSOF_LV_GLOBAL 2
#define DVSOF_LV_EPT8 4
#define DVSOF_LV_EPT16 8
size_t dvsof_learned_voxelize_tiled_workspace_bytes(int64_t n_events, int B,
                                                    int C, int H, int W,
                                                    int flags);
/* 0 where the three-kernel path serves the call (no control words) */
size_t dvsof_learned_voxelize_tiled_control_bytes(int64_t n_events, int B,
                                                  int C, int H, int W,
                                                  int flags);
int dvsof_learned_voxelize_tiled(const void *x, const void *y, const float *t,
                                 const void *polarity,
                                 const void *sample_or_offsets, int encoded,
                                 int64_t n_events, const float *t0,
                                 const float *t1, const float *theta, int R,
                                 int S, int B, int C, int H, int W, float *out,
                                 void *workspace, size_t workspace_bytes,
                                 int flags, void *stream);

/*
 * Data gradient of the first encoder layer (enc.0: 3x3, stride 2, pad 1, C
 * planar input channels, 1..16, 64 NHWC output channels; csrc/first.hip) --
 * what a learnable representation needs below the predictor:
 *   gV[b,c,iy,ix] = sum gz[b,oy,ox,co] * weight[co][ky][kx][c]
 *   over 2*oy - 1 + ky = iy, 2*ox - 1 + kx = ix, co in [0,64).
 * gz[B,H/2,W/2,64] is the gradient with respect to the layer's PRE-activation
 * (the tensor its weight gradient consumes: the activation's derivative is
 * already applied); weight is the physical [64][3][3][C] buffer; gV[B,C,H,W]
 * is written, not accumulated.  H and W even; gz 16-byte aligned.  Exact f32
 * FMAs in every operand mode, channels added in ascending order.
 */
int dvsof_first_dgrad(const float *gz, const float *weight, int B, int C,
                      int H, int W, float *gV, void *stream);

/* ------------------------------------------------------------------ *
 * Data augmentation on the device: horizontal
 * flip -> nearest-neighbour LUT rotation about the frame centre -> crop, the
 * order of utils/dataset.py:753-769.  Per-sample parameters are device
 * arrays: flip u8[B]; cos_sin f64[B][2] (cos, sin of the angle, computed on
 * the host in float64 as utils/data.py:181-186 does); box i32[B][4] =
 * (y0, x0, h, w) with one (h, w) for the whole batch.
 * ------------------------------------------------------------------ */

/* lut[b][source pixel] = rotated pixel that reads it (smallest index when
 * several do; >= H*W: none).  Replaces the (src, dst) index lists
 * RandomRotation hands to the native transformation.map, utils/data.py:199-215. */
int dvsof_augment_lut(const double *cos_sin, int B, int H, int W, int32_t *lut,
                      void *stream);

/* dst f32[D,h,w] = crop(rotate(flip(src[D,H,W]))); src is u8 or f32;
 * frame_sample i32[D] = sample of every frame, each in [0, B): the call does
 * not know B and reads flip / cos_sin / box there unchecked
 * (docs/AUGMENT_SPEC.md section 7).  utils/dataset.py:755-757,
 * utils/data.py:203-206 (rimages), utils/data.py:45-75 (crop). */
int dvsof_augment_frames(const void *src, int src_is_u8, int D, int H, int W,
                         const int32_t *frame_sample, const uint8_t *flip,
                         const double *cos_sin, const int32_t *box, int h,
                         int w, float *dst, void *stream);

/* Event coordinates through the same flip / rotation / crop
 * (utils/dataset.py:758, utils/data.py:208-213, utils/data.py:24-42).  lut
 * may be NULL (no rotation).  Removed events get x_out = y_out = -1 instead of
 * being compacted away (the voxeliser skips them). */
int dvsof_augment_events(const int64_t *x, const int64_t *y,
                         const int64_t *sample_index, int64_t n_events,
                         const uint8_t *flip, const int32_t *lut,
                         const int32_t *box, int B, int H, int W,
                         int64_t *x_out, int64_t *y_out, void *stream);

/* ------------------------------------------------------------------ *
 * Evaluation against ground-truth flow (csrc/eval.hip, docs/EVAL_SPEC.md):
 * the per-frame body of evaluate, utils/testing.py:64-93, for a BATCH of F
 * frames per launch.
 * ------------------------------------------------------------------ */

/*
 * Ground-truth flow over each frame's interval.  Replaces
 * estimate_corresponding_gt_flow / prop_flow, utils/eval.py:53-184.
 *   x_flow, y_flow     [K,H,W] displacement maps, float32 (DVSOF_EVAL_F32) or
 *                      float64 (DVSOF_EVAL_F64, what MVSEC stores); inf allowed;
 *                      H, W <= 32767
 *   frame_step_begin   int32[F+1]: steps of frame f are [begin[f], begin[f+1])
 *   step_map           int32[S]: map index of every step (0 <= index < K; a step
 *                      with another index samples 0)
 *   step_scale         double[S]: scale factor of every step
 *   frame_mode         int32[F]: 0 = propagate through the steps; 1 = direct
 *                      scale (utils/eval.py:127-128): TWO table entries naming
 *                      the same map, step_scale = {dt, gt_dt},
 *                      result = (float)((flow * dt) / gt_dt) in float64
 *   (y0, x0, h, w)     output window on the full frame: pixel (i, j) starts at
 *                      (x0 + j, y0 + i), i.e. propagate on the full frame, then
 *                      crop; DVSOF_EINVAL when it leaves the frame
 *   u, v               float32[F,h,w]
 * Per step: ix = rint(x), iy = rint(y) (ties to even; outside the map, beyond
 * the int16 range or not finite: the sample is 0), a sampled 0 clears that
 * component's mask for good, x = (float)((double)x + (double)fx * scale);
 * u = x - x_start or 0 where the mask is cleared.
 */
#define DVSOF_EVAL_F32 0
#define DVSOF_EVAL_F64 1
int dvsof_gt_flow_propagate(const void *x_flow, const void *y_flow,
                            int flow_dtype, int K, int H, int W,
                            const int32_t *frame_step_begin,
                            const int32_t *step_map, const double *step_scale,
                            const int32_t *frame_mode, int F, int S, int y0,
                            int x0, int h, int w, float *u, float *v,
                            void *stream);

/* one row per frame, 32 bytes */
typedef struct {
    double sum_ee;    /* sum of the endpoint errors of the counted pixels */
    int64_t n_points; /* counted pixels */
    int64_t n_below;  /* ... with an endpoint error < 3 */
    float pred_max;   /* max / min of the prediction over the whole [2,h,w] */
    float pred_min;   /* window (a NaN wins, as in numpy) */
} dvsof_eval_result_t;

/*
 * Masked endpoint error.  Replaces flow_error_dense, utils/eval.py:6-50.
 *   gt_u, gt_v   float32[F,h,w]
 *   pred         float32[F,2,h,w], the model's NCHW output
 *   count        uint32[F,h,w] event counts, or NULL (is_dense)
 *   max_row      rows >= max_row are not counted (is_car: min(190, h), else h)
 * A pixel counts when count > 0, neither ground-truth component is infinite
 * and sqrt(u^2 + v^2) > 0 in float32; EE = sqrt(du^2 + dv^2) in float32, summed
 * in float64 in a fixed order (per-block partials in `workspace`, then one
 * closing pass; no floating-point atomics): same input, same bits.
 */
size_t dvsof_flow_error_workspace_bytes(int F, int h, int w);
int dvsof_flow_error(const float *gt_u, const float *gt_v, const float *pred,
                     const uint32_t *count, int F, int h, int w, int max_row,
                     dvsof_eval_result_t *result, void *workspace,
                     size_t workspace_bytes, void *stream);

/*
 * dvsof_count_image for F frames at once: events [begin[f], begin[f+1]) of the
 * columns x, y (n_events entries) belong to frame f.  (y0, x0, h, w) is a crop
 * box with the semantics of EventCrop, utils/data.py:24-42: events outside it
 * are dropped, the rest shifted by (x0, y0).  out uint32[F,h,w] is zeroed by
 * the call.
 */
int dvsof_count_image_batched(const int64_t *x, const int64_t *y,
                              int64_t n_events,
                              const int64_t *frame_event_begin, int F, int y0,
                              int x0, int h, int w, uint32_t *out,
                              void *stream);

/*
 * dvsof_count_image_batched by polarity: p is the int64 wire polarity column,
 * out uint32[F,2,h,w] (zeroed by the call); plane 0 of a frame counts its
 * events with p > 0, plane 1 those with p <= 0.  The two planes add up to
 * what dvsof_count_image_batched writes for the same columns, exactly.
 */
int dvsof_count_image_polarity_batched(const int64_t *x, const int64_t *y,
                                       const int64_t *p, int64_t n_events,
                                       const int64_t *frame_event_begin,
                                       int F, int y0, int x0, int h, int w,
                                       uint32_t *out, void *stream);

/* ------------------------------------------------------------------ *
 * Rendering (csrc/render.hip, docs/RENDER_SPEC.md): predicted flow as a
 * colour image on the device.  Replaces flow2img, utils/visualization.py:5-18
 * (four numpy passes and two cv2 calls per sample on the host) and the
 * put_image / join_images layout of visualize.py:37-127.  Two launches per
 * call whatever the number of images: per-chunk min / max, then colouring.
 * ------------------------------------------------------------------ */

#define DVSOF_RENDER_FLOW 0   /* src: float32 [2,h,w], x plane then y plane */
#define DVSOF_RENDER_FRAME 1  /* src: uint8 [h,w] grey, replicated to B, G, R */
#define DVSOF_RENDER_FILL 2   /* no src: the rectangle is set to 0 */
#define DVSOF_RENDER_MAX_CHUNKS 64

/*
 * One workgroup's work: rows [row0, row0 + rows) of an h x w source, written
 * as BGR bytes at pixel (x0, y0 + row0) of a destination whose first byte is
 * canvas + dst_offset and whose rows are dst_stride bytes apart.  64 bytes.
 * The table is built on the host (visualization.py) and must be readable at
 * BOTH addresses the entry points take: `items` by the host (it is validated
 * there), `items_dev` by the kernels (the caller's one upload of the same
 * bytes).
 * Flow items come first in the table.  The chunks of one image stand together
 * in ascending order, chunk 0 first, and tile its rows exactly; an image has
 * at most DVSOF_RENDER_MAX_CHUNKS of them (dvsof_flow_render_chunk_rows keeps
 * to that).  Every image 0 .. n_images-1 occurs exactly once.  Items must not
 * overlap in the destination (not checked: the table is the caller's layout).
 */
typedef struct {
    const void *src;
    int64_t dst_offset; /* bytes from `canvas` to the destination's pixel (0,0) */
    int64_t dst_stride; /* bytes per destination row, >= 3 * (x0 + w) */
    int32_t kind;       /* DVSOF_RENDER_* */
    int32_t image;      /* flow: row of stats / max_magnitude; else ignored */
    int32_t h, w;       /* the source (flow, frame) or the rectangle (fill) */
    int32_t x0, y0;     /* where its pixel (0,0) lands in the destination */
    int32_t row0, rows; /* the rows of the source this item covers */
    int32_t chunk, chunks; /* flow: this item's place among the image's items */
} dvsof_render_item_t;

/* per image, 16 bytes: over the pixels whose two components are finite
 * (lo = +inf, hi = -inf when there is none) */
typedef struct {
    float lo, hi;       /* min / max of sqrtf(fx*fx + fy*fy) */
    int32_t nonfinite;  /* pixels with a NaN or an infinite component */
    int32_t reserved;
} dvsof_render_stats_t;

/* Rows per item for an h x w source: about 2048 pixels, and at most
 * DVSOF_RENDER_MAX_CHUNKS items per image.  0 for h or w outside [1, 32767]. */
int dvsof_flow_render_chunk_rows(int h, int w);
/* Scratch for the per-chunk partials of n_images flow images. */
size_t dvsof_flow_render_workspace_bytes(int n_images);

/*
 * Launch 1: one workgroup per flow item (the first n_flow entries of the
 * table) writes {lo, hi, nonfinite} of its rows into `workspace`.  Min and
 * max are exact in any order and the count is an integer: same input, same
 * bits.  n_flow == 0: nothing to do.
 */
int dvsof_flow_render_stats(const dvsof_render_item_t *items,
                            const dvsof_render_item_t *items_dev, int n_flow,
                            int n_images, void *workspace,
                            size_t workspace_bytes, void *stream);

/*
 * Launch 2: one workgroup per item of the whole table.  A flow item reduces
 * the partials of its image (chunk 0 also stores them to stats[image]), then
 * colours its pixels (docs/RENDER_SPEC.md section 2):
 *   V = trunc(min((mag - lo) * (hi - lo > 0 ? 255 / (hi - lo) : 0), 255))
 *   hue = trunc((atan2f(fy, fx) + pi) * 180 / pi / 2), S = 255, HSV -> BGR by
 *   OpenCV's float formula, a pixel with a non-finite component black.
 *   max_magnitude  float32[n_images] or NULL.  m > 0: lo = 0, hi = m, mag
 *                  clamped to m (one colour scale for several images);
 *                  m <= 0 or NULL: the image's own min / max.
 *   canvas         the byte range every destination lies in
 *   stats          dvsof_render_stats_t[n_images]: always the image's OWN
 *                  min / max; the caller may copy it back once
 * Stream order after dvsof_flow_render_stats is the only synchronisation.  No
 * memset: what no flow or frame item covers is the caller's to cover with
 * fill items.  DVSOF_EINVAL, before any launch: null pointers, sizes outside
 * [1, 32767], a malformed table (see dvsof_render_item_t), an item reaching
 * outside its destination row or outside the canvas; DVSOF_ENOSPACE: the
 * workspace is missing or too small.
 */
int dvsof_flow_render(const dvsof_render_item_t *items,
                      const dvsof_render_item_t *items_dev, int n_items,
                      int n_flow, int n_images, const float *max_magnitude,
                      const void *workspace, size_t workspace_bytes,
                      uint8_t *canvas, size_t canvas_bytes,
                      dvsof_render_stats_t *stats, void *stream);

/* ------------------------------------------------------------------ *
 * Evaluation panels (csrc/eval_panels.hip, docs/EVAL_PANELS_SPEC.md): per
 * frame one picture of h x 4w BGR bytes, the panels events | prediction |
 * ground truth | endpoint error side by side, prediction and ground truth
 * on one colour scale.  Two launches for any number of frames.
 * ------------------------------------------------------------------ */

/* per frame, 32 bytes: the prediction's and the ground truth's
 * dvsof_render_stats_t values, then the pixels dvsof_flow_error counts */
typedef struct {
    float pred_lo, pred_hi;
    int32_t pred_nonfinite;
    float gt_lo, gt_hi;
    int32_t gt_nonfinite;
    int32_t n_counted;  /* dvsof_eval_result_t.n_points */
    int32_t n_below;    /* ... with an endpoint error < 3 */
} dvsof_eval_panel_stats_t;

/* Scratch for the per-chunk partials of F frames (64 slots of 32 bytes each). */
size_t dvsof_eval_panels_workspace_bytes(int F);

/*
 * Launch 1: one workgroup per (frame, chunk of dvsof_flow_render_chunk_rows
 * rows) writes the partial statistics of its rows into `workspace`.
 *   pred         float32[F,2,h,w]
 *   gt_u, gt_v   float32[F,h,w]
 *   count2       uint32[F,2,h,w] (dvsof_count_image_polarity_batched) or NULL
 *   max_row      rows >= max_row are not counted, 0 <= max_row <= h
 * Integers and min / max only: same input, same bits.
 */
int dvsof_eval_panels_stats(const float *pred, const float *gt_u,
                            const float *gt_v, const uint32_t *count2, int F,
                            int h, int w, int max_row, void *workspace,
                            size_t workspace_bytes, void *stream);

/*
 * Launch 2: one workgroup per (frame, panel, chunk) reduces the partials of
 * its frame and colours its rows (docs/EVAL_PANELS_SPEC.md).  Picture f has
 * its pixel (0,0) at canvas + f * frame_stride, rows row_stride bytes apart,
 * panel k at x0 = k * w.
 *   frames       uint8[F,h,w] grey under the events, or NULL (black)
 *   flow_scale   > 0: max_magnitude of both flow panels; <= 0: the ground
 *                truth's hi when finite and > 0, else the prediction's
 *   err_max      > 0: the endpoint error drawn at full scale
 *   gain         1..255: colour per event
 *   stats        dvsof_eval_panel_stats_t[F]; the caller may copy it back once
 * Stream order after dvsof_eval_panels_stats is the only synchronisation.
 * Every byte of every picture is written exactly once, nothing else is.
 * DVSOF_EINVAL before any launch: null pointers, F < 0, h or w outside
 * [1, 32767], max_row outside [0, h], row_stride < 12 w, pictures that overlap
 * (F > 1 and frame_stride < h * row_stride) or reach past canvas_bytes,
 * err_max not > 0 or not finite, gain outside 1..255; DVSOF_ENOSPACE: the
 * workspace is missing or too small.  F == 0: nothing to do.
 */
int dvsof_eval_panels(const float *pred, const float *gt_u, const float *gt_v,
                      const uint32_t *count2, const uint8_t *frames, int F,
                      int h, int w, int max_row, float flow_scale,
                      float err_max, int gain, const void *workspace,
                      size_t workspace_bytes, uint8_t *canvas,
                      size_t canvas_bytes, int64_t frame_stride,
                      int64_t row_stride, dvsof_eval_panel_stats_t *stats,
                      void *stream);

/* ------------------------------------------------------------------ *
 * Image of warped events and flow warp loss (csrc/iwe.hip,
 * docs/IWE_SPEC.md): label-free validation.  Every event of a frame is moved
 * along the predicted flow to the start of its window and splatted
 * bilinearly; FWL = variance of that image / variance of the count image.
 * ------------------------------------------------------------------ */

typedef struct {            /* 48 bytes, one per frame */
    double  sum_sq;         /* sum over pixels of I*I, I = (double)Q * 2^-32; fixed order */
    int64_t sum_q;          /* sum over pixels of Q (exact) */
    int64_t max_q;          /* max over pixels of Q */
    int64_t count_sum;      /* sum over pixels of c (exact) */
    int64_t count_sq;       /* sum over pixels of c*c (exact) */
    int64_t count_max;
} dvsof_iwe_result_t;

/*
 * Events [begin[f], begin[f+1]) of the wire columns x, y, t (n_events entries)
 * belong to frame f; events outside [begin[0], begin[F]) and events with x or
 * y outside the image (the -1 slots of cropped and padded events) are skipped.
 *   frame_ts   float32[2F]: start and stop of every frame on the clock of t
 *   flow       float32[F,2,h,w], read at the event's own pixel
 *   q          int64[F,h,w], zeroed by the call: bilinear weights in units of
 *              2^-32, summed by integer atomics (exact in any order)
 * tau = clamp((t - start) / (stop - start), 0, 1), 0 for stop <= start; the
 * event lands at (x - tau u, y - tau v); corners outside the image and events
 * whose warped position is not inside (-1, w) x (-1, h) are dropped.
 * DVSOF_EINVAL before any launch: F < 0 or > 65535, n_events < 0, h or w
 * outside [1, 32767], null pointers.  F == 0: nothing to do.
 */
int dvsof_iwe_splat(const int64_t *x, const int64_t *y, const float *t, int64_t n_events,
                    const int64_t *frame_event_begin, const float *frame_ts /* [2F]: start, stop */,
                    const float *flow /* [F,2,h,w] */, int F, int h, int w,
                    int64_t *q /* [F,h,w] */, void *stream);

/*
 * One dvsof_iwe_result_t per frame from q and the count image of the same
 * events (dvsof_count_image_batched).  Two launches: per-block partials in
 * `workspace`, then one closing wave per frame; the order is fixed and there
 * are no floating-point atomics: same input, same bits.  DVSOF_EINVAL as
 * above; DVSOF_ENOSPACE: the workspace is missing or too small.
 */
size_t dvsof_iwe_stats_workspace_bytes(int F, int h, int w);
int dvsof_iwe_stats(const int64_t *q, const uint32_t *count /* [F,h,w] */, int F, int h, int w,
                    dvsof_iwe_result_t *result, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Per frame two grey panels side by side, the count image on the left and the
 * image of warped events on the right, each scaled to its own maximum
 * (count_max, max_q of `result`).  One launch; every byte of the canvas is
 * written exactly once.
 */
int dvsof_iwe_render(const int64_t *q, const uint32_t *count, const dvsof_iwe_result_t *result,
                     int F, int h, int w, uint8_t *canvas /* [F,h,2w,3] */, void *stream);

/* ------------------------------------------------------------------ *
 * Device-resident event sequence -> wire-format batch
 * (docs/SEQUENCE_SPEC.md)
 * ------------------------------------------------------------------ */

/*
 * W windows cut from one resident, time-sorted sequence, collated into the
 * wire format in one launch.  Replaces the per-frame slicing, cropping and
 * collation of utils/testing.py:64-66 + DummyNet/of.py:76-115 and the event
 * side of DatasetImpl.__getitem__ / collate_wrapper, utils/dataset.py:714-751,
 * 961-1020.
 *   x, y, t, p     the sequence: int16 coordinates, float64 timestamps sorted
 *                  ascending, int8 polarity; n_events entries
 *   win_begin/end  int64[W]: window k holds the events [begin[k], end[k])
 *   win_out        int64[W+1]: first output slot of every window, the prefix
 *                  sum of the lengths; win_out[W] = n_out
 *   win_origin     double[W]: subtracted from t in float64
 *   win_sample, win_element  int32[W]: sample_index / element_index of the window
 *   (y0, x0, h, w) crop box with the semantics of EventCrop,
 *                  utils/data.py:24-42; h == w == 0: no crop
 *   *_out          `capacity` >= n_out slots each
 * Slot win_out[k] + j holds event i = win_begin[k] + j:
 *   t_out = (float)(t[i] - win_origin[k]); inside the box x_out = x - x0,
 *   y_out = y - y0, outside it x_out = y_out = -1 (the slot stays: no
 *   compaction); polarity, sample and element as given.
 * Slots [n_out, capacity): x = y = -1, t = 0, polarity = sample = element = 0.
 * Windows may be empty, overlap, repeat and come in any order; W = 0 and
 * n_out = 0 are valid.  Every output element is written exactly once; one
 * kernel launch, no memset.  The window table is trusted (its Python wrapper
 * validates it on the host); a wrong one reads nothing outside the sequence.
 */
int dvsof_event_windows(const int16_t *x, const int16_t *y, const double *t,
                        const int8_t *p, int64_t n_events,
                        const int64_t *win_begin, const int64_t *win_end,
                        const int64_t *win_out, const double *win_origin,
                        const int32_t *win_sample, const int32_t *win_element,
                        int W, int y0, int x0, int h, int w, int64_t *x_out,
                        int64_t *y_out, float *t_out, int64_t *polarity_out,
                        int64_t *sample_out, int64_t *element_out,
                        int64_t n_out, int64_t capacity, void *stream);

/* ------------------------------------------------------------------ *
 * Multi-scale warp / Charbonnier / smoothness / out-of-border loss
 * ------------------------------------------------------------------ */

/*
 * Bilinear resize with align_corners=True of n single-channel images.
 * Replaces utils/loss.py:20-21 (F.interpolate) as used for the CASCADED frame
 * pyramid at utils/loss.py:207-210.
 */
int dvsof_resize_bilinear_ac(const float *src, float *dst, int n, int hin,
                             int win, int hout, int wout, void *stream);

/*
 * The whole CASCADED pyramid of utils/loss.py:207-210 (level 0 resamples
 * images [D,H,W] to (hs[0],ws[0]); level k resamples level k-1) into
 * levels[k] = float[D*hs[k]*ws[k]].  One launch when the level sizes are
 * non-decreasing (the coarse -> fine order Losses uses), otherwise one resize
 * launch per level; bitwise the same values either way.
 */
int dvsof_loss_pyramid(const float *images, int D, int H, int W,
                       float *const *levels, const int *hs, const int *ws,
                       int num_levels, void *stream);

typedef struct {
    const float *frames; /* [D,h,w] all frames of the batch at this scale */
    const float *flow;   /* [N,2,h,w] predicted flow, pixels of this scale */
    float *grad_flow;    /* [N,2,h,w] written by *_bwd / *_fused, else NULL */
    int h, w;
} dvsof_loss_scale_t;

/* bytes of workspace dvsof_loss_* need for these scales (0 on bad input) */
size_t dvsof_loss_workspace_bytes(const dvsof_loss_scale_t *host_scales,
                                  int num_scales, int N);

/*
 * Forward of Losses.__call__ / Loss.__call__, utils/loss.py:121-171,179-214,
 * for all scales in one launch sequence.
 *   start_idx/stop_idx  int32[N]: frame index of the first/second image of
 *                       prediction n (resolved on the host from timestamps,
 *                       utils/loss.py:182-206)
 *   terms               float[3*num_scales]: smoothness_k, photometric_k,
 *                       outborder_k (row order as returned at utils/loss.py:171)
 *   oob_count           int32[num_scales*N]: out-of-border pixels per sample
 *                       (utils/loss.py:101), kept for the backward pass
 */
int dvsof_loss_fwd(const dvsof_loss_scale_t *host_scales, int num_scales,
                   int N, const int32_t *start_idx, const int32_t *stop_idx,
                   float *terms, int32_t *oob_count, void *workspace,
                   size_t workspace_bytes, void *stream);

/*
 * Backward: grad_flow_k = d(sum_t seeds[t,k] * term[t,k]) / d flow_k, i.e.
 * what loss.backward() (utils/training.py:158) yields through utils/loss.py.
 * seeds: device float[3*num_scales] (upstream gradients of the 12 scalars).
 * oob_count: as produced by dvsof_loss_fwd on the same inputs.
 */
int dvsof_loss_bwd(const dvsof_loss_scale_t *host_scales, int num_scales,
                   int N, const int32_t *start_idx, const int32_t *stop_idx,
                   const float *seeds, const int32_t *oob_count, void *stream);

/*
 * Training fast path: terms AND the gradient of
 *   loss = sum_t host_weights[t] * mean_k term[t,k] * loss_scale
 * (combined_loss, utils/training.py:12-24, with the 1/accumulation_steps of
 * utils/training.py:156 folded into loss_scale) in one sweep over the inputs.
 * Also writes the scalar loss to loss_out[0].
 */
int dvsof_loss_fused(const dvsof_loss_scale_t *host_scales, int num_scales,
                     int N, const int32_t *start_idx, const int32_t *stop_idx,
                     const float *host_weights /*[3]*/, float loss_scale,
                     float *terms, float *loss_out, int32_t *oob_count,
                     void *workspace, size_t workspace_bytes, void *stream);

/*
 * dvsof_loss_fused that first builds the frame pyramid from images [D,H,W]
 * INTO host_scales[k].frames (as dvsof_loss_pyramid does), sharing a launch
 * with the out-of-border count: Losses.__call__'s interpolate cascade
 * (utils/loss.py:207-210) + terms + gradient in 4 launches.
 */
int dvsof_loss_fused_pyramid(const float *images, int D, int H, int W,
                             const dvsof_loss_scale_t *host_scales,
                             int num_scales, int N, const int32_t *start_idx,
                             const int32_t *stop_idx,
                             const float *host_weights /*[3]*/,
                             float loss_scale, float *terms, float *loss_out,
                             int32_t *oob_count, void *workspace,
                             size_t workspace_bytes, void *stream);


/* ------------------------------------------------------------------ *
 * EV_FlowNet predictor: convolution stack on the f32 matrix cores
 * (docs/MODEL_SPEC.md).  Replaces the ATen conv2d / upsample / cat /
 * activation ops and their autograd inside EV_FlowNet.net.Model.predictor as
 * called at utils/training.py:59-64 and differentiated at
 * utils/training.py:158 (source absent upstream; contract from
 * DummyNet/net.py:59-80 and tests/training/test_training.py:45-46).
 * ------------------------------------------------------------------ */

enum { DVSOF_ACT_NONE = 0, DVSOF_ACT_RELU = 1, DVSOF_ACT_MISH = 2 };
enum { DVSOF_NHWC = 0, DVSOF_NCHW = 1 };

typedef struct {
    const float *p; /* dense tensor [B,H,W,C] (NHWC) or [B,C,H,W] (NCHW) */
    int C;
    int layout; /* DVSOF_NHWC | DVSOF_NCHW */
    const void *p16; /* optional bf16 twin of an NHWC tensor (same shape, same
                        values rounded to bf16): read instead of p by the
                        matrix-core kernels in mfma mode 3 */
} dvsof_src_t;

/*
 * One conv layer y = act(conv(up(cat(src...)), W) + bias [+ residual]):
 * the input is the channel concatenation of nsrc tensors of spatial size
 * H x W, optionally 2x nearest-upsampled first; ksize x ksize taps, zero
 * padding `pad`, stride 1 or 2.  Output is NHWC [B,Ho,Wo,Cout] with
 * Ho = (H*(upsample ? 2 : 1) + 2*pad - ksize)/stride + 1.
 * Weights are [Cout][ksize][ksize][Ctot] (channels contiguous, Ctot = sum C).
 *
 * upsample = 2 makes the layer a TRANSPOSED convolution with stride 2 (the
 * north star's "strided conv / transposed-conv / Mish stack"; the reference's
 * network source is absent, docs/MODEL_SPEC.md keeps nearest up-sampling as
 * the decoder's default): zeros are inserted between the input pixels
 * (xz[2i][2j] = x[i][j]) before the 3x3 / pad-1 convolution, Ho = 2H.  With
 * W' = W flipped in both tap axes and its channel axes swapped this is
 * torch conv_transpose2d(x, W', stride 2, padding 1, output_padding 1).
 * Forward: four output-parity phases of (1+py)(1+px) taps on the
 * low-resolution input (prepared form [4][Cout][2][2][Ctot]); data gradient:
 * a stride-2 3x3 convolution of the output gradient with the flip-transposed
 * weights; weight gradient: that of the adjoint stride-2 layer, flip-
 * transposed; bias gradient: channel sums of the output gradient.
 */
typedef struct {
    dvsof_src_t src[3];
    int nsrc;
    int B, H, W;
    int upsample; /* 0 | 1 = 2x nearest | 2 = 2x zero insertion (transposed
                     convolution, stride 2: one NHWC source with C % 16 == 0,
                     ksize 3, pad 1, stride 1; see below) */
    int ksize, stride, pad;
    int Cout;
    int act; /* DVSOF_ACT_* */
    int mfma; /* 0: f32 matrix cores (exact products); 1: operands rounded to
                 bf16 in registers, v_mfma_f32_32x32x16_bf16, f32 accumulate;
                 2: operands split into bf16 hi + lo, products hi*hi + hi*lo +
                 lo*hi (the dropped lo*lo term is 2^-16 relative).
                 Every tensor stays f32 in memory in modes 0-2.
                 3: bf16 TWINS -- like 1, but the forward / data-gradient
                 kernels stream bf16 copies of their NHWC operands (src[i].p16,
                 gout16) and of the prepared weights (w16) through LDS: half
                 the LDS-DMA bytes mode 1 is bound by, no conversion in the K
                 loop.  Producers write the twin of their output next to the
                 f32 tensor (y16, dst[i].p16, dvsof_flow_head_bwd's gx16); the
                 weight gradient, the heads and the loss keep reading f32.
                 Needs every NHWC operand of the call in whole 64-byte runs of
                 bf16 -- forward: every NHWC source channel count % 32 == 0;
                 data gradient: Cout % 32 == 0 -- else the call runs as
                 mode 1.
                 Rounding contract (tests/test_gpu_conv_exact.py emulates it
                 in float64): every product a*b of a pass is
                   modes 1, 3: RNE_bf16(a) * RNE_bf16(b)
                   mode 2:     hi(a)hi(b) + hi(a)lo(b) + lo(a)hi(b),
                               hi = RNE_bf16(a), lo = RNE_bf16(a - hi)
                 of the f32 operands, accumulated in f32:
                   forward:  input (every member, planar ones included)
                             x the forward weight form -- of a sub-pixel
                             layer (up-sampling, 3x3 / pad 1) the phase sums
                             of taps, made in f32 and then rounded; any other
                             up-sampling layer rounds the raw taps;
                   data gradient: gout x the data-gradient form (the same
                             values); the gradient of a narrow planar (NCHW)
                             member (trailing, <= 4 channels in all, beside
                             >= 32 other channels) of a stride-1 layer that
                             is plain or sub-pixel is exact f32 in every mode:
                             it runs beside the matrix-core launch.  In the
                             quad-summed form (other up-sampling layers) and
                             in a stride-2 layer it stays in the matrix-core
                             problem and rounds like the rest;
                   weight gradient: gout x input on the (up-sampled) frame,
                             the raw taps' sums; the columns of a planar
                             member are exact f32; the bias gradient sums the
                             f32 gout (mode 3 with a twin-reading kernel: the
                             twin, i.e. RNE(gout)).
                 The f32-only families (dvsof_conv2d_last_kernel reports mode
                 0) and the Winograd forms, whose mode 2 rounds TRANSFORMED
                 operands, are outside this list.  Bias, residual, addends,
                 border-class bias, act / act' and the folded flow head stay
                 f32 in every mode. */
    void *scratch;        /* device scratch for layers that run as Winograd */
    size_t scratch_bytes; /* F(2x2,3x3) (dvsof_conv2d_scratch_bytes > 0); read by
                             dvsof_conv2d_fwd / _dgrad only, which return
                             DVSOF_ENOSPACE when it is missing or too small */
    const float *winograd_input; /* optional, read by dvsof_conv2d_wgrad only:
                             dvsof_conv2d_fwd leaves the transformed input of a
                             Winograd layer at the start of `scratch`; a caller
                             that kept that buffer intact passes it here and the
                             weight gradient skips its own input transform
                             (used when both run the same tile form) */
    /* mode 3 only (NULL otherwise) */
    void *y16;           /* dvsof_conv2d_fwd: bf16 twin of y, written */
    const void *w16;     /* bf16 twin of the weight argument of the call
                            (dvsof_to_bf16 of the prepared form) */
    const void *gout16;  /* dvsof_conv2d_dgrad / _wgrad: bf16 twin of gout */
    int flags;           /* DVSOF_CONV_* bits */
    const float *bias_cls; /* dvsof_conv2d_fwd, optional: [9][Cout] added to the
                            output rows of border class c = 3 * (top 1 |
                            bottom 2) + (left 1 | right 2); row 0 (interior)
                            is not read.  The position-dependent share of a
                            folded constant member (dvsof_flow_fold_weights) */
    /* Forms shared by CONSECUTIVE Winograd layers of one frame (the residual
     * chain), all optional; dvsof_conv2d_winograd_chain(desc, kind) says whether
     * this layer's forward / data gradient can write them (F(4x4) form, <= 64
     * tiles per image), DVSOF_EINVAL otherwise.  A producer then makes the
     * consumer's transforms in its own output transform (one launch and one pass
     * over the tensor instead of three; same bits):
     *   winograd_next       fwd / dgrad: also write the transformed input
     *                       [36][T][channels of the output] of the layer that
     *                       consumes this call's output (same B, H, W);
     *   winograd_pre        fwd / dgrad: this call's transformed input as a
     *                       producer wrote it -- the input transform is skipped
     *                       (fwd: it is also what winograd_input names for the
     *                       weight gradient);
     *   winograd_next_gout  dgrad: also write the gradient form [36][T][C] of
     *                       the output, for the weight gradient that takes it as
     *                       gout;
     *   winograd_gout       wgrad: that form of gout (used when the weight
     *                       gradient runs the F(4x4) form, else ignored). */
    const float *winograd_pre;
    float *winograd_next;
    float *winograd_next_gout;
    const float *winograd_gout;
} dvsof_conv_desc_t;
/* dvsof_conv2d_wgrad leaves the columns of the narrow planar members (the
 * 2-channel flow) unwritten: dvsof_flow_fold_grads fills them (below) */
#define DVSOF_CONV_WGRAD_SKIP_FLAT 1

/*
 * Bytes of scratch dvsof_conv2d_fwd / dvsof_conv2d_dgrad need for this layer:
 * non-zero for the wide 3x3 stride-1 layers (one NHWC source, channel counts
 * multiples of 64 and >= 256, even H and W, mfma != 1), which are evaluated as
 * Winograd convolutions -- F(4x4,3x3) when H and W are multiples of 4 (4x fewer
 * multiply-adds), else F(2x2,3x3) (2.25x fewer): input transform, NG = 36 | 16
 * component GEMMs on the matrix cores, output transform with the fused
 * epilogue.  Same result up to fp32 rounding of the transforms (~1e-5 | ~1e-6
 * of the output peak).  Their prepared weights are U[NG][Cout][Ctot] forward
 * and U'[NG][Ctot][Cout] backward; dvsof_conv2d_prepare makes either or both
 * from the raw weights (weight must not be NULL for these layers).  The
 * scratch holds the transformed input and the component products; it is only
 * used during the call.  The weight gradient of such a layer runs through the
 * same transforms inside its ordinary workspace.
 */
size_t dvsof_conv2d_scratch_bytes(const dvsof_conv_desc_t *desc);
/* 0: direct implicit GEMM; 2 | 4: Winograd output tile side used for this
 * problem (kind 0 forward, 1 data gradient, 2 weight gradient); for tools. */
int dvsof_conv2d_winograd_tile(const dvsof_conv_desc_t *desc, int kind);
/* 1: the forward (kind 0) / data gradient (kind 1) of this layer accepts
 * winograd_next [/ winograd_next_gout] (see dvsof_conv_desc_t) */
int dvsof_conv2d_winograd_chain(const dvsof_conv_desc_t *desc, int kind);

/*
 * Prepared weights.  An upsampled 3x3/pad-1 layer is evaluated as four 2x2
 * sub-pixel phase convolutions on the low-resolution input (16 instead of 36
 * tap-products per low-resolution pixel, same result up to fp32 summation
 * order): forward weights Wf[4][Cout][2][2][Ctot], data-gradient weights the
 * 4x4 stride-2 kernel Wd[Ctot][4][4][Cout] -- or, in exact f32 (mfma == 0)
 * with two NHWC members of 32 | C, 32 | Cout, 16 | W, 4 | H, by the minimal
 * bilinear algorithm of csrc/fwd_min.hip with NINE products: forward weights
 * Wt[9][Cout][Ctot] = G w G^T, and (64 | C, 8 | H) data-gradient weights
 * W'[9][Ctot][Cout] = G' w G'^T.  Which form a buffer holds is a function of
 * the descriptor alone (the same test picks the kernel at launch); the buffer
 * sizes are those of the sub-pixel forms either way.  Every other layer uses
 * the raw weights forward and their tap-flipped transpose backward.
 * dvsof_conv2d_prepare fills w_fwd (may be NULL when
 * dvsof_conv2d_fwd_weight_elems == Cout*k*k*Ctot: forward then takes the raw
 * weights) and w_dgrad (may be NULL) from the raw [Cout][k][k][Ctot] weights.
 * For a sub-pixel layer w_fwd == NULL with w_dgrad makes the data-gradient
 * form alone, from the raw weights (lets a caller make it later, e.g. on
 * another stream).  (Sixteen-product form only: weight == NULL means "w_fwd
 * already holds the phase kernels of an earlier call" and w_dgrad is derived
 * from them -- DVSOF_EINVAL for a layer whose forward form is Wt.)
 * Once Wt / W' are prepared the layer is bound to the nine-product kernels:
 * the pointers passed to dvsof_conv2d_fwd / _dgrad must then be 16-byte
 * aligned and the forward takes no residual (DVSOF_EINVAL otherwise, see there).
 */
size_t dvsof_conv2d_fwd_weight_elems(const dvsof_conv_desc_t *desc);
size_t dvsof_conv2d_dgrad_weight_elems(const dvsof_conv_desc_t *desc);
int dvsof_conv2d_prepare(const dvsof_conv_desc_t *desc, const float *weight,
                         float *w_fwd, float *w_dgrad, void *stream);

/* weight = prepared forward weights (see above).
 * y (and z = pre-activation, optional, for Mish backward) are NHWC.
 * Nine-product layers (forward form Wt, see above) have no other kernel to
 * fall back to once the weights are prepared: DVSOF_EINVAL, before any launch
 * and with y / z untouched, when a source, y, z, weight, bias or bias_cls is
 * not 16-byte aligned, or when a residual is given. */
int dvsof_conv2d_fwd(const dvsof_conv_desc_t *desc, const float *weight,
                     const float *bias, const float *residual, float *y,
                     float *z, void *stream);

typedef struct {
    float *p;            /* gradient w.r.t. desc->src[i], same layout/shape */
    const float *addend; /* optional: p = result + addend (may alias p) */
    const float *addend2; /* optional second addend */
    const float *actsrc; /* optional: p *= act'(actsrc), the producer's y
                            (ReLU) or z (Mish): yields its dz directly */
    void *p16;           /* optional bf16 twin of p, written (mode 3; NHWC
                            members only).  In mode 3 the vector members'
                            gradients multiply the twins of gout and of the
                            weights; a planar (NCHW or narrow) member's
                            gradient is computed from the f32 gout and f32
                            weights, as that member's forward reads f32. */
    /* optional, only where dvsof_conv2d_dgrad_fuses_head(desc) says so (the
     * nine-product data gradient, csrc/dgrad_min.hip): the flow head that hangs
     * on this source is folded into the epilogue,
     *   p = (result + addends + head_w[0][c] gflow[b][0][y][x] + head_w[1][c] gflow[b][1][y][x]) * act'(actsrc)
     * head_w [2][C] (the head's 1x1 weights), head_gflow [B][2][H][W] planar (the
     * flow's loss gradient): what dvsof_flow_head_bwd computes as gx, without
     * the pass over the tensor in between (the head's own weight gradient:
     * dvsof_flow_head_bwd with gx == NULL).  DVSOF_EINVAL on any other kernel. */
    const float *head_w;
    const float *head_gflow;
    /* ... and, optionally with them, the head's OWN weight / bias gradient from
     * the same pass: head_x = the head's input (the tensor p is the gradient of;
     * may equal actsrc), head_part = [dvsof_conv2d_dgrad_head_rows(desc)][2 C + 2]
     * floats of per-block partial sums, every element written:
     * dvsof_flow_head_reduce(head_part, rows, C, dw, dbias) adds them up in a
     * fixed order (instead of dvsof_flow_head_bwd's second pass over x). */
    const float *head_x;
    float *head_part;
} dvsof_grad_dst_t;

/*
 * Data gradient: for every source i, dst[i].p = d loss / d src[i] given
 * gout = d loss / d (pre-activation output) [B,Ho,Wo,Cout] NHWC.
 * weight_t is the prepared data-gradient weight (dvsof_conv2d_prepare; for a
 * plain layer the tap-flipped transpose [Ctot][ksize][ksize][Cout]).  dst[i].p == NULL skips nothing (all sources
 * are computed together); pass a scratch buffer if a gradient is not needed.
 */
/* 1 when the data gradient of this layer accepts dvsof_grad_dst_t.head_w /
 * head_gflow (shape test alone; see above) */
int dvsof_conv2d_dgrad_fuses_head(const dvsof_conv_desc_t *desc);
/* rows of dvsof_grad_dst_t.head_part for this layer (0: not available) */
int dvsof_conv2d_dgrad_head_rows(const dvsof_conv_desc_t *desc);
/* dw [2][C], dbias [2] (may be NULL) = column sums of part [rows][2 C + 2] */
int dvsof_flow_head_reduce(const float *part, int rows, int C, float *dw, float *dbias, void *stream);
/* Nine-product data gradient (form W', see dvsof_conv2d_prepare): DVSOF_EINVAL,
 * before any launch and with every dst untouched, when gout, weight_t or a
 * dst's p / addend / addend2 / actsrc / head_w is not 16-byte aligned. */
int dvsof_conv2d_dgrad(const dvsof_conv_desc_t *desc, const float *weight_t,
                       const float *gout, const dvsof_grad_dst_t *dst,
                       int bwd_act, void *stream);

size_t dvsof_conv2d_wgrad_workspace_bytes(const dvsof_conv_desc_t *desc);
/* dweight [Cout][k][k][Ctot], dbias [Cout] (optional); overwritten. */
int dvsof_conv2d_wgrad(const dvsof_conv_desc_t *desc, const float *gout,
                       float *dweight, float *dbias, void *workspace,
                       size_t workspace_bytes, void *stream);


/*
 * Which tile shape the library picks for this problem (for profiling tools):
 * kind 0 = forward, 1 = data gradient, 2 = weight gradient.  Returns the
 * tile id (1..5: 128x128, 128x64, 64x64, 256x32|64x128, 128x32|32x128) or <0.
 */
int dvsof_conv2d_tile_id(const dvsof_conv_desc_t *desc, int kind);
/* kernel generation serving the problem: 2 = LDS-DMA ring (gconv2/wgrad2),
 * 1 = register-staged (gconv/wgrad), 0 = VALU-only (flat members),
 * 3 = the first encoder layer's own kernels (csrc/first.hip: one planar source
 * of <= 16 channels, 3x3 stride 2 pad 1, 64 outputs, even frame sides; forward
 * and weight gradient, exact f32 in every operand mode). */
int dvsof_conv2d_kernel_generation(const dvsof_conv_desc_t *desc, int kind);
/* What the calling thread's LAST dvsof_conv2d_fwd (kind 0) / _dgrad (1) / _wgrad
 * (2) ran for a decoder stage: 0 the general kernels, 1 a patch-resident
 * sixteen-product kernel (csrc/fwd_patch.hip, csrc/wgrad_patch.hip), 2 the
 * nine-product minimal form (csrc/fwd_min.hip, dgrad_min.hip, wgrad_min.hip:
 * exact f32; 9 instead of 16 matrix products per low-resolution pixel).  The
 * choice depends on operand mode, twins and shape (profiling tools: bench.py
 * names its roofline groups and counts executed FLOPs with it).  Derived from
 * the record dvsof_conv2d_last_kernel reads. */
int dvsof_conv2d_last_patch(int kind);
/* Kernel families of the conv stack (dvsof_conv2d_last_kernel). */
enum {
    DVSOF_KERNEL_NONE = 0,          /* nothing launched (refused call) */
    DVSOF_KERNEL_GENERAL_V1 = 1,    /* csrc/gconv.hip, wgrad.hip: register-staged, exact f32 */
    DVSOF_KERNEL_GENERAL_V2 = 2,    /* csrc/gconv2.hip, wgrad2.hip: LDS-DMA ring */
    DVSOF_KERNEL_FLAT_VALU = 3,     /* weight gradient of flat (planar / narrow) members only */
    DVSOF_KERNEL_FIRST = 4,         /* csrc/first.hip */
    DVSOF_KERNEL_WINO2 = 5,         /* csrc/winograd.hip, F(2x2,3x3) */
    DVSOF_KERNEL_WINO4 = 6,         /* csrc/winograd.hip, F(4x4,3x3) */
    DVSOF_KERNEL_FWD_MIN4 = 7,      /* csrc/fwd_min.hip, 4-row blocks */
    DVSOF_KERNEL_FWD_MIN8 = 8,      /* csrc/fwd_min.hip, 8-row blocks */
    DVSOF_KERNEL_FWD_PATCH = 9,     /* csrc/fwd_patch.hip (f32 or twins) */
    DVSOF_KERNEL_DGRAD_MIN0 = 10,   /* csrc/dgrad_min.hip <0>: resident weights, persistent */
    DVSOF_KERNEL_DGRAD_MIN1 = 11,   /* <1>: one item per workgroup */
    DVSOF_KERNEL_DGRAD_MIN2 = 12,   /* <2>: two items per workgroup (a loss inside the step: never reported now) */
    DVSOF_KERNEL_WGRAD_PATCH = 13,  /* csrc/wgrad_patch.hip */
    DVSOF_KERNEL_WGRAD_MIN = 14,    /* csrc/wgrad_min.hip */
    DVSOF_KERNEL_TRANSPOSED = 15,   /* transposed layer (upsample 2): output-parity phases */
    DVSOF_KERNEL_STRIDE2_PHASED = 16 /* stride-2 data gradient as four input-parity phases */
};
/* What the calling thread's LAST dvsof_conv2d_fwd (kind 0) / _dgrad (1) / _wgrad
 * (2) launched: family | effective_mode << 8.  family is a DVSOF_KERNEL_* value
 * (DVSOF_KERNEL_NONE when the call launched nothing); effective_mode is the
 * operand mode after every fallback (0 exact f32, 1 bf16-rounded operands,
 * 2 bf16x3, 3 bf16 twins streamed).  Mode 3 silently becomes 1 where a twin is
 * missing or a channel count does not fit; this record tells the two apart.
 * The first-layer kernels compute in f32 in every mode: their mode is 3 when
 * the forward wrote y16, else 0.  A weight gradient with flat and vector
 * members records the vector members' kernel.  Set after the launch (recorded
 * by the launcher that ran, not by the planning predicates). */
int dvsof_conv2d_last_kernel(int kind);

/* wt[ci][k*k-1-tap][co] = w[co][tap][ci] */
int dvsof_weight_flip_transpose(const float *w, float *wt, int Cout, int ksize,
                                int Ctot, void *stream);

/*
 * Flow head: flow[b,j,y,x] = sum_c w[j][c] * x[b,y,x,c] + bias[j], j = 0,1.
 * x NHWC [B,H,W,C] (C % 4 == 0), flow NCHW [B,2,H,W] (the layout the loss
 * and the reference's prediction contract use, utils/training.py:59-64).
 */
int dvsof_flow_head_fwd(const float *x, const float *w, const float *bias,
                        float *flow, int B, int H, int W, int C, void *stream);
/* n <= 4 heads in one launch (host arrays of device pointers / sizes; bias may
 * be NULL or hold NULLs): the training forward computes all flows ahead of the
 * loss once nothing between the decoder stages reads them. */
int dvsof_flow_heads_fwd(int n, const float *const *host_x,
                         const float *const *host_w,
                         const float *const *host_bias, float *const *host_flow,
                         int B, const int *host_H, const int *host_W,
                         const int *host_C, void *stream);

size_t dvsof_flow_head_bwd_workspace_bytes(int B, int H, int W, int C);
/*
 * Backward of the head fused with the activation backward of the decoder
 * layer that produced x:
 *   gx = (gx_in + w^T gflow) * act'(actsrc)      (gx_in optional, may alias gx)
 *   dw[j][c] = sum gflow_j * x_c ,  dbias[j] = sum gflow_j
 */
int dvsof_flow_head_bwd(const float *x, const float *w, const float *gflow,
                        const float *gx_in, const float *actsrc, int act,
                        float *gx, float *dw, float *dbias, int B, int H, int W,
                        int C, void *workspace, size_t workspace_bytes,
                        void *gx16 /* optional bf16 twin of gx, written */,
                        void *stream);

/* dst[i] = bf16(src[i]) (round to nearest even), n elements: the bf16 twins of
 * the prepared weights for mfma mode 3.  Bit for bit torch's .to(bfloat16): ties
 * to even, finite values past the largest bf16 become +-inf, NaN stays NaN,
 * subnormals are rounded, not flushed.  n == 0 (a NULL pointer allowed) does
 * nothing; so does a tensor of n == 0 in dvsof_to_bf16_many. */
int dvsof_to_bf16(const float *src, void *dst, size_t n, void *stream);
/* up to 16 tensors in ONE launch (host arrays of device pointers / sizes) */
int dvsof_to_bf16_many(const float *const *host_src, void *const *host_dst,
                       const size_t *host_n, int count, void *stream);
/* dvsof_conv2d_prepare that also writes the bf16 twins of the forms it makes
 * (compute mode 3, "bf16 twins"), from the same kernels: w_fwd16 = twin of the
 * forward form -- of the RAW weight where that is the forward form --,
 * w_dgrad16 = twin of the data-gradient form; either may be NULL. */
int dvsof_conv2d_prepare16(const dvsof_conv_desc_t *desc, const float *weight,
                           float *w_fwd, float *w_dgrad, void *w_fwd16,
                           void *w_dgrad16, void *stream);

/* dz = dy * act'(actsrc), n elements (dz may alias dy) */
int dvsof_act_bwd(const float *dy, const float *actsrc, int act, float *dz,
                  size_t n, void *stream);


/* ------------------------------------------------------------------ *
 * Optimizer
 * ------------------------------------------------------------------ */

/* elements one workgroup of dvsof_adamw_step handles (chunk table unit) */
int dvsof_adamw_chunk_elems(void);

/*
 * Fused multi-tensor AdamW step (decoupled weight decay, optional amsgrad) for
 * one parameter group.  Replaces torch.optim.AdamW(amsgrad=True).step() as
 * built at train_flownet.py:57-75 and called at utils/training.py:164.
 *   ptrs    device uint64[5*T]: {param, grad, exp_avg, exp_avg_sq,
 *           max_exp_avg_sq} pointers of tensor t (float32, dense)
 *   sizes   device int64[T]: element counts
 *   chunks  device int32[2*num_chunks]: (tensor id, chunk index) per
 *           workgroup, chunk = dvsof_adamw_chunk_elems() elements
 *   step    1-based step count (bias correction)
 */
int dvsof_adamw_step(const uint64_t *ptrs, const int64_t *sizes,
                     const int32_t *chunks, int num_chunks, float lr,
                     float beta1, float beta2, float eps, float weight_decay,
                     int step, int amsgrad, void *stream);

/*
 * The same update for a step that is CAPTURED in a hipGraph (the train loop of
 * utils/training.py:138-167 replayed as one graph launch): kernel arguments
 * are frozen at capture, so what changes per step -- the scheduled learning
 * rate (LambdaLR, train_flownet.py:91-109) and the bias corrections -- is read
 * from `dyn`, device float[3] = {lr, lr/(1-beta1^t), sqrt(1-beta2^t)}.
 * dvsof_adamw_dynamic fills a HOST float[3] with exactly the values
 * dvsof_adamw_step would use (the caller puts it into `dyn` before each replay:
 * dvsof_adamw_set_dynamic),
 * so both entry points give bit-identical parameters.
 */
void dvsof_adamw_dynamic(float lr, float beta1, float beta2, int step,
                         float *host_out3);
/* host_values[n] -> dyn[n] (device) in stream order, the values travelling as
 * kernel arguments: no copy engine, no fence in front of the step's first
 * kernel; host_values may be reused as soon as the call returns */
int dvsof_adamw_set_dynamic(float *dyn, const float *host_values, int n,
                            void *stream);
int dvsof_adamw_step_dyn(const uint64_t *ptrs, const int64_t *sizes,
                         const int32_t *chunks, int num_chunks,
                         const float *dyn, float beta1, float beta2, float eps,
                         float weight_decay, int amsgrad, void *stream);


/*
 * Fused multi-tensor RAdam / Ranger step for one parameter group.  Replaces
 * RAdam.radam.RAdam and ranger.Ranger (train_flownet.py:62-71; un-vendored
 * submodules upstream -- arithmetic per Liu et al. 2020 and Lookahead, Zhang
 * et al. 2019; oracle/ref_optim.py).  Tables as for dvsof_adamw_step;
 * ptrs[5t+4] is the Lookahead slow buffer (Ranger) or unused (RAdam).
 *   degenerate_to_sgd  bit 0: take an un-rectified momentum step while the
 *                      variance is not tractable (both upstream defaults);
 *                      bit 1: RAdam's ">= threshold" rule instead of Ranger's ">"
 *                      Weight decay (p -= weight_decay * lr * p, before the
 *                      update) is applied only on a step that takes an update:
 *                      rectified, or un-rectified with bit 0.  Without bit 0
 *                      the un-rectified steps advance the moments and leave p
 *                      bit for bit (docs/OPTIM_SPEC.md).
 *   lookahead_now      1 on every k-th step of Ranger, else 0
 *   lookahead_alpha    slow-weight step (0 = no slow buffer: plain RAdam)
 */
int dvsof_radam_step(const uint64_t *ptrs, const int64_t *sizes,
                     const int32_t *chunks, int num_chunks, float lr,
                     float beta1, float beta2, float eps, float weight_decay,
                     int step, float nsma_threshold, int degenerate_to_sgd,
                     int lookahead_now, float lookahead_alpha, void *stream);

/*
 * The same update for a CAPTURED step (see dvsof_adamw_step_dyn): what the
 * step count and the learning-rate schedule decide is read from `dyn`, device
 * float[4] = {lr, step size, rectified (0/1), Lookahead-sync-now (0/1)}.  The
 * two decisions are uniform over the launch: a step that does not synchronise
 * neither reads nor writes the slow buffer (28 B per parameter, else 36).
 * dvsof_radam_dynamic fills a HOST float[4] with exactly the values
 * dvsof_radam_step would use (one code path for the double-precision
 * rectification term; step size -1 = "no update": un-rectified without
 * degenerate_to_sgd bit 0), the sync decision being lookahead_k > 0 &&
 * step % lookahead_k == 0; dvsof_adamw_set_dynamic puts it into `dyn`.
 */
void dvsof_radam_dynamic(float lr, float beta1, float beta2, int step,
                         float nsma_threshold, int degenerate_to_sgd,
                         int lookahead_k, float *host_out4);
int dvsof_radam_step_dyn(const uint64_t *ptrs, const int64_t *sizes,
                         const int32_t *chunks, int num_chunks,
                         const float *dyn, float beta1, float beta2, float eps,
                         float weight_decay, float lookahead_alpha,
                         void *stream);

/* Gradient centralisation (Ranger): grad[r][:] -= mean(grad[r][:]). */
int dvsof_grad_centralize(float *grad, int rows, int row_len, void *stream);
/*
 * The rows of many tensors in one launch (one workgroup per row), bit for bit
 * what dvsof_grad_centralize gives tensor by tensor.
 *   rows    device int64[2*num_rows]: {address of the row (float32, contiguous),
 *           row length}
 */
int dvsof_grad_centralize_multi(const int64_t *rows, int num_rows,
                                void *stream);

/* ------------------------------------------------------------------ *
 * Step guard (csrc/optim.hip, docs/STEP_GUARD_SPEC.md): global gradient-norm
 * clipping and the skip of a step with non-finite gradients, decided on the
 * device by kernels that are part of the (captured) step.
 *
 * The guard RECORD is DVSOF_GUARD_RECORD_BYTES of device memory, 8-byte
 * aligned, zeroed once by the caller and persistent from then on:
 *
 *   float    scale        (float)min(1, max_norm / (norm + 1e-6)), the
 *                         quotient in float64; 1.0f when max_norm <= 0
 *                         (clipping off) or when bad > 0
 *   uint32_t skip         1 iff bad > 0 and skip_nonfinite
 *   double   norm         sqrt(sum of squares); NaN when bad > 0
 *   uint32_t bad          non-finite gradient elements of this step (saturating)
 *   uint32_t skipped      steps skipped since the record was zeroed
 *   uint32_t clipped      steps with scale < 1
 *   uint32_t consecutive  skipped steps in a row (0 after a step that updated)
 *
 * dvsof_grad_guard enqueues two launches in stream order.  PARTIALS: one
 * workgroup per (tensor, chunk) work item writes {double sum of
 * (double)g * (double)g over its finite elements, uint32 count of elements
 * whose exponent field is all ones} -- per thread, then the wave, then the four
 * waves, in a fixed order, without atomics.  CLOSE: one workgroup sums the
 * partials in a fixed order in float64 and writes the record.  Nothing inside
 * a launch waits for another workgroup.
 *   grads      device uint64: grads[t * ptr_stride] is the gradient pointer of
 *              tensor t (float32, dense, 4-byte aligned).  With a pointer
 *              table of dvsof_adamw_step: ptrs + 1 and ptr_stride 5; the
 *              tables of several parameter groups concatenated (tensor ids of
 *              `chunks` offset accordingly) give ONE norm and ONE decision
 *   sizes, chunks, num_chunks   as for dvsof_adamw_step
 *   partials   device workspace, 8-byte aligned, at least num_chunks *
 *              dvsof_grad_guard_partial_bytes() (DVSOF_ENOSPACE otherwise;
 *              nothing is enqueued)
 *   max_norm   <= 0: no clipping
 * num_chunks == 0 (no gradient at all): the close alone runs, norm 0.
 * ------------------------------------------------------------------ */
#define DVSOF_GUARD_RECORD_BYTES 32
#define DVSOF_GUARD_PARTIAL_BYTES 16
int dvsof_grad_guard_record_bytes(void);
int dvsof_grad_guard_partial_bytes(void);
int dvsof_grad_guard(const uint64_t *grads, int ptr_stride,
                     const int64_t *sizes, const int32_t *chunks,
                     int num_chunks, void *partials, size_t partials_bytes,
                     double max_norm, int skip_nonfinite, void *guard,
                     void *stream);

/*
 * The update entry points above under a guard: every workgroup reads `skip`
 * and `scale` from the record.  A skipped step returns before any load or
 * store -- no parameter, moment, max_exp_avg_sq, weight decay, Lookahead slow
 * buffer or Lookahead synchronisation is written.  Otherwise each gradient is
 * multiplied by `scale` (one float32 multiply, after the gradient
 * centralisation of Ranger, which is a launch of its own and is not gated)
 * and the update is the unguarded one: with scale == 1.0f bit for bit.
 */
int dvsof_adamw_step_guarded(const uint64_t *ptrs, const int64_t *sizes,
                             const int32_t *chunks, int num_chunks, float lr,
                             float beta1, float beta2, float eps,
                             float weight_decay, int step, int amsgrad,
                             const void *guard, void *stream);
int dvsof_adamw_step_dyn_guarded(const uint64_t *ptrs, const int64_t *sizes,
                                 const int32_t *chunks, int num_chunks,
                                 const float *dyn, float beta1, float beta2,
                                 float eps, float weight_decay, int amsgrad,
                                 const void *guard, void *stream);
int dvsof_radam_step_guarded(const uint64_t *ptrs, const int64_t *sizes,
                             const int32_t *chunks, int num_chunks, float lr,
                             float beta1, float beta2, float eps,
                             float weight_decay, int step,
                             float nsma_threshold, int degenerate_to_sgd,
                             int lookahead_now, float lookahead_alpha,
                             const void *guard, void *stream);
int dvsof_radam_step_dyn_guarded(const uint64_t *ptrs, const int64_t *sizes,
                                 const int32_t *chunks, int num_chunks,
                                 const float *dyn, float beta1, float beta2,
                                 float eps, float weight_decay,
                                 float lookahead_alpha, const void *guard,
                                 void *stream);

/* ------------------------------------------------------------------ *
 * Checkpoint snapshot (csrc/snapshot.hip, docs/CHECKPOINT_SPEC.md): one
 * launch copies the storage of many float32 tensors into one device slab and
 * counts the values whose exponent field is all ones (NaN, +-Inf).
 *
 * Slab: DVSOF_SNAPSHOT_HEADER_BYTES of header, then the tensors at their
 * offsets.  Header word[parity] (uint32) holds the count of this launch;
 * word[parity ^ 1] is zeroed by this launch for the next one, which passes
 * the other parity.  The first launch into a slab needs word[parity] == 0
 * (a freshly zeroed allocation).  Nothing else of the header and no byte
 * between or behind the tensors is written.
 *
 *   srcs     device uint64[T]: address of tensor t's storage (float32,
 *            4-byte aligned; dense: counts[t] consecutive floats)
 *   counts   device int64[T]: elements
 *   offsets  device int64[T]: first float of tensor t in the slab, counted
 *            from the slab's start; a multiple of 4 (16 bytes) and at least
 *            DVSOF_SNAPSHOT_HEADER_BYTES / 4
 *   items    device int32[2*num_items]: (tensor id, chunk index), chunk =
 *            dvsof_snapshot_chunk_elems() elements
 *   slab     16-byte aligned
 * num_items == 0 enqueues nothing and returns 0.  The tables and the slab
 * bound are the caller's: the kernel cannot check them.
 * ------------------------------------------------------------------ */
#define DVSOF_SNAPSHOT_HEADER_BYTES 16
int dvsof_snapshot_chunk_elems(void);
int dvsof_snapshot_header_bytes(void);
int dvsof_snapshot_pack(const uint64_t *srcs, const int64_t *counts,
                        const int64_t *offsets, const int32_t *items,
                        int num_items, void *slab, int parity, void *stream);

/* ------------------------------------------------------------------ *
 * The flow member of a decoder stage in weight space (csrc/flowfold.hip).
 * Stage i convolves cat[x, skip, flow] with flow = Wh x + bh, the previous
 * stage's 1x1 flow head applied to the x member.  For the BACKWARD
 * (utils/training.py:158 through the network) the member is folded away:
 *   dvsof_flow_fold_weights   w_eff[Cout][9][Ctot-2] = the layer's weights
 *       without the two flow columns, x columns += Wflow . Wh: the data
 *       gradient then runs on cat[x, skip] alone and already contains the
 *       path through the flow head (the head's backward gets the flow's LOSS
 *       gradient only);
 *   dvsof_flow_fold_grads     after dvsof_conv2d_wgrad with
 *       DVSOF_CONV_WGRAD_SKIP_FLAT: writes the flow columns of dW from its x
 *       columns, Wh, bh, the bias gradient db_conv and the border sums of the
 *       output gradient g [B,H,W,Cout], and ADDS the stage's contribution to
 *       the head's gradients dwh [2][Cx], dbh [2].
 * cx_off / cf_off: first column of the x member / of the flow pair in a
 * weight row; 3x3 taps; the flow is the member convolved at the x member's
 * resolution (both up-sampled together).  ws: dvsof_flow_fold_workspace_bytes.
 * Both entries refuse, with DVSOF_EINVAL and before any launch: a negative
 * offset, an x range [cx_off, cx_off + Cx) or a flow pair [cf_off, cf_off + 2)
 * that leaves the row or that overlap each other, Ctot < 3.
 * ------------------------------------------------------------------ */
int dvsof_flow_fold_weights(const float *w, int Cout, int Ctot, int cx_off,
                            int Cx, int cf_off, const float *wh, float *w_eff,
                            void *stream);
/* The same fold for the FORWARD: y = conv(up cat[x, skip], w_eff) + bias_eff
 * + bias_cls[class of the output pixel], where the head's bias bh reaches the
 * output through the flow taps that lie inside the frame:
 *   bias_eff[co]    = bias[co] + sum_{t,f} Wflow[co][t][f] bh[f]
 *   bias_cls[c][co] = - sum_{t outside for class c, f} Wflow[co][t][f] bh[f]
 * (3x3 taps, pad 1; rows of the first / last output line lose ky = 0 / 2,
 * columns kx = 0 / 2).  bias_cls is [9][Cout], row 0 zero. */
int dvsof_flow_fold_bias(const float *w, int Cout, int Ctot, int cf_off,
                         const float *bh, const float *bias, float *bias_eff,
                         float *bias_cls, void *stream);
size_t dvsof_flow_fold_workspace_bytes(int B, int Cout);
int dvsof_flow_fold_grads(float *dW, const float *w, int Cout, int Ctot,
                          int cx_off, int Cx, int cf_off, const float *wh,
                          const float *bh, const float *db_conv,
                          const float *g, int B, int H, int W, float *dwh,
                          float *dbh, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ *
 * Data-parallel gradient exchange (RCCL over xGMI).  The reference is single
 * process (no torch.distributed / NCCL use anywhere); this
 * is the one collective of the build: the average of a gradient bucket over
 * the ranks, in place, enqueued on `stream` (the caller's exchange stream,
 * gated by an event behind the bucket's last weight gradient and joined
 * before the optimizer step: parallel.GradReducer).  One process per GPU;
 * librccl is opened on first use (DVSOF_ECOMM when it is absent).
 *   rank 0:   dvsof_comm_unique_id(id)  -> send the 128 bytes to every rank
 *   all:      dvsof_comm_create(&comm, world, rank, id)   (current HIP device)
 *   per step: dvsof_allreduce_bucket(comm, bucket, n, stream) per bucket
 * ------------------------------------------------------------------ */
#define DVSOF_COMM_ID_BYTES 128
int dvsof_comm_unique_id(void *host_id128);
int dvsof_comm_create(void **comm, int world_size, int rank,
                      const void *host_id128);
int dvsof_comm_destroy(void *comm);
int dvsof_allreduce_bucket(void *comm, float *bucket, size_t n, void *stream);
/* dvsof_comm_info: ranks = what the communicator spans (ncclCommCount for an
 * RCCL communicator -- bench.py prints it as config.rccl_ranks), loopback = 1
 * for a loopback communicator, calls / elements = dvsof_allreduce_bucket calls
 * issued on it so far and the floats they carried (any pointer may be NULL).
 *
 * dvsof_comm_create_loopback: a communicator WITHOUT peers, for the ordering
 * tests of the exchange on one GPU: the other world_size - 1 ranks are
 * imaginary and contribute all-zero buckets, the wire is a spin of delay_us on
 * `stream`.  dvsof_allreduce_bucket then leaves bucket / world_size in place,
 * delay_us late -- an exchange that is neither the identity nor instantaneous
 * (a 1-rank RCCL group launches nothing at all), so a kernel that reads or
 * rewrites a bucket on the wrong side of its collective changes the result.
 * No RCCL involved; never used by a training run. */
int dvsof_comm_info(void *comm, int *ranks, int *loopback,
                    unsigned long long *calls, unsigned long long *elements);
int dvsof_comm_create_loopback(void **comm, int world_size, int delay_us);

/* ------------------------------------------------------------------ *
 * Step executor (csrc/exec.hip): the loop body of the reference's train()
 * (utils/training.py:138-167: model, loss, backward, optimizer.step) captured
 * once per batch signature as a hipGraph and replayed as plain kernel
 * launches from ONE C call, on the streams of the eager schedule.
 *   graph         hipGraph_t of a stream capture; kernel (and empty) nodes
 *                 only, else DVSOF_EINVAL; must outlive the executor
 *   side_streams  hipStream_t of lanes 1..n_side (lane 0 = the stream given
 *                 to dvsof_exec_launch); nodes are split into at most
 *                 1 + n_side chains, one event per dependency across chains
 *   dvsof_exec_calibrate  runs the step ONCE on `stream` alone with a timing
 *                       event per kernel, waits for it and re-plans the lanes
 *                       from the measured durations.  Three plans: "paths"
 *                       (lane 0 = longest path by time, the rest on the last
 *                       lane), "list" (list scheduling by remaining path
 *                       length, which also fixes the launch order; marks keep
 *                       their capture order) and "chain" (the greedy split in
 *                       effect before calibration).  The next 6 calls of
 *                       dvsof_exec_launch are real steps under each plan in
 *                       turn, timed on the device (the host waits for the
 *                       previous step before each of them); the fastest plan
 *                       stays.
 *                       It IS a step: same kernels, same results as
 *                       dvsof_exec_launch -- under every plan
 *   dvsof_exec_plan     name of the plan in effect; settled = 0 while plans
 *                       are still being tried
 *   dvsof_exec_launch   side lanes start behind `stream`, `stream` continues
 *                       behind every lane; nothing else synchronises
 *   dvsof_exec_node     node i in launch order: lane, measured us, number of
 *                       cross-lane waits, kernel name (diagnostics)
 *   dvsof_exec_info     counts (any pointer may be NULL); lane_kernels[l] =
 *                       kernels of lane l for l < max_lanes
 *
 * Data parallelism and gradient accumulation (utils/training.py:156-167,
 * utils/options.py:318-325) under the executor.  The exchange is not a kernel:
 * while the step is captured the reducer leaves MARKS in the stream
 * (dvsof_exec_mark) where the eager loop issues a collective / joins the
 * exchange stream.  The executor never launches a mark; it acts on it:
 *   DVSOF_MARK_BUCKET  (bucket, n): the exchange stream waits for the lane's
 *                      progress, then dvsof_allreduce_bucket(comm, bucket, n)
 *                      on the exchange stream
 *                      Kernels captured behind a BUCKET mark do NOT depend on
 *                      it: they inherit what preceded the mark
 *   DVSOF_MARK_WAIT    (index of a BUCKET mark): the lane waits for THAT
 *                      collective (in front of the update of that bucket's
 *                      parameters when the optimizer runs inside the backward)
 *   DVSOF_MARK_JOIN    the lane waits for the exchange stream (in front of
 *                      the optimizer kernels)
 *   dvsof_exec_set_comm  communicator (dvsof_comm_create) and exchange stream
 *                      of the marks; comm NULL (or never set): marks are
 *                      skipped -- one GPU.  Call before the first replay.
 *   dvsof_exec_marks   number of marks found in the graph
 *   dvsof_exec_node_arg  copies the first nbytes of kernel argument `arg` of
 *                      node i (launch order) -- diagnostics: the pointer audit
 *                      of capture.CapturedTrainStep.audit.  UNCHECKED: a node
 *                      does not know its argument count or sizes (the HIP
 *                      graph API does not expose them); the caller takes both
 *                      from the code-object metadata of the SAME library file
 *                      that is loaded (_audit.py verifies that) -- a wrong
 *                      arg / nbytes is an out-of-bounds host read
 * Every rank replays the same graph, so the collectives are issued in the
 * same order everywhere.
 * ------------------------------------------------------------------ */
#define DVSOF_MARK_BUCKET 1
#define DVSOF_MARK_JOIN 2
#define DVSOF_MARK_WAIT 3
int dvsof_exec_mark(int kind, int index, float *bucket, size_t n, void *stream);
int dvsof_exec_set_comm(void *exec, void *comm, void *exchange_stream);
/* Stream of the UPDATE lane: kernels captured behind nothing but WAIT marks (a
 * bucket's optimizer update, captured on the exchange stream by
 * parallel.GradReducer) are replayed there, each behind its bucket's
 * collective, and no compute lane waits before the JOIN mark.  Without this
 * call they run on the exchange stream itself, between the collectives.  A
 * stream of its own hardware queue (first used before any communicator
 * exists: parallel.claim_streams). */
int dvsof_exec_set_update_stream(void *exec, void *update_stream);
int dvsof_exec_marks(void *exec, int *n_marks);
/* The exchange window of the k-th BUCKET mark (capture order): the kernels
 * captured behind the mark that are not behind its WAIT mark (or, without one,
 * the JOIN mark).  They inherit the mark's dependencies and may run beside
 * the collective, so none of them may touch [bucket, bucket + n).  nodes[] =
 * their positions in the launch order (at most cap; *count = how many there
 * are).  The caller checks the arguments (capture.py at recording time, with
 * the argument layouts of the code objects); DVSOF_EINVAL past the last mark. */
int dvsof_exec_mark_window(void *exec, int k, float **bucket, size_t *n,
                           int *index, int *nodes, int cap, int *count);
int dvsof_exec_node_arg(void *exec, int i, int arg, size_t nbytes, void *out);
int dvsof_exec_create(void *graph, void *const *side_streams, int n_side,
                      void **exec);
int dvsof_exec_info(void *exec, int *n_kernels, int *n_lanes, int *n_events,
                    int *n_waits, int *lane_kernels, int max_lanes);
int dvsof_exec_calibrate(void *exec, void *stream);
int dvsof_exec_launch(void *exec, void *stream);
int dvsof_exec_node(void *exec, int i, int *lane, float *us, int *n_waits,
                    char *name, int name_len);
int dvsof_exec_plan(void *exec, char *name, int name_len, int *settled);
int dvsof_exec_destroy(void *exec);

#ifdef __cplusplus
}
#endif
#endif /* DVSOF_H */
