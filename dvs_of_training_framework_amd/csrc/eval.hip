// Evaluation on the device: ground-truth flow propagation, masked endpoint
// error and the batched event mask (docs/EVAL_SPEC.md), the latter also by
// polarity for the evaluation pictures (docs/EVAL_PANELS_SPEC.md section 1).
//
// Replaces (reference paths): estimate_corresponding_gt_flow / prop_flow
// utils/eval.py:53-184 (a dozen cv2.remap calls over full-resolution maps per
// frame), flow_error_dense utils/eval.py:6-50 (boolean-mask gathers, float32
// mean) and get_count_image utils/data.py:120-136 behind EventCrop
// utils/data.py:24-42, as driven per frame by utils/testing.py:64-93.
//
// All three are HBM-bound and small: one thread per output pixel (or event),
// every frame of a batch in one launch.  The arithmetic is pinned bit for bit
// by the spec; this file relies on -ffp-contract=off (no fused multiply-add
// in the index update, none in the endpoint error).
#include "frame_common.h"

static_assert(sizeof(dvsof_eval_result_t) == 32, "result rows are 32 bytes (eval.py reads them as such)");

namespace {

constexpr int NT = kFrameNT;

// ---------------------------------------------------------------------------
// Propagation.  Pixel (i, j) of the window starts at (x0 + j, y0 + i) on the
// full map and walks the frame's steps: sample both maps at the rounded
// position (round half to even, 0 outside the map), move by flow * scale with
// ONE rounding to float32.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NT) void gt_propagate_kernel(
    const T *__restrict__ xf, const T *__restrict__ yf, int K, int H, int W,
    const int32_t *__restrict__ frame_step_begin, const int32_t *__restrict__ step_map,
    const double *__restrict__ step_scale, const int32_t *__restrict__ frame_mode, int S, int y0,
    int x0, int h, int w, float *__restrict__ u, float *__restrict__ v)
{
    const int f = blockIdx.y;
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= h * w) return;
    const int i = p / w, j = p - i * w;
    const size_t o = (size_t)f * h * w + p;
    const size_t plane = (size_t)H * W;
    // a malformed table reads nothing outside itself: the range is clipped to [0, S]
    const int s0 = max(frame_step_begin[f], 0), s1 = min(frame_step_begin[f + 1], S);

    if (frame_mode[f] == 1) {  // the interval lies inside one ground-truth gap: flow * dt / gt_dt
        float ru = 0.f, rv = 0.f;
        if (s1 - s0 >= 2) {
            const int m = step_map[s0];
            if (m >= 0 && m < K) {
                const double dt = step_scale[s0], gt_dt = step_scale[s0 + 1];
                const size_t q = (size_t)m * plane + (size_t)(y0 + i) * W + (x0 + j);
                ru = (float)(((double)xf[q] * dt) / gt_dt);
                rv = (float)(((double)yf[q] * dt) / gt_dt);
            }
        }
        u[o] = ru;
        v[o] = rv;
        return;
    }

    const float xs = (float)(x0 + j), ys = (float)(y0 + i);
    float x = xs, y = ys;
    bool keep_x = true, keep_y = true;
    for (int s = s0; s < s1; ++s) {
        const int m = step_map[s];
        const double scale = step_scale[s];
        // v_rndne_f32: ties to even.  The comparisons are false for NaN, and with
        // H, W <= kMaxSide a coordinate saturated to the int16 range is outside too.
        const float rx = rintf(x), ry = rintf(y);
        T fx = (T)0, fy = (T)0;
        if (rx >= 0.f && rx < (float)W && ry >= 0.f && ry < (float)H && m >= 0 && m < K) {
            const size_t q = (size_t)m * plane + (size_t)(int)ry * W + (int)rx;
            fx = xf[q];
            fy = yf[q];
        }
        if (fx == (T)0) keep_x = false;
        if (fy == (T)0) keep_y = false;
        x = (float)((double)x + (double)fx * scale);
        y = (float)((double)y + (double)fy * scale);
    }
    u[o] = keep_x ? x - xs : 0.f;
    v[o] = keep_y ? y - ys : 0.f;
}

// ---------------------------------------------------------------------------
// Endpoint error, by the fixed-order reduction of frame_common.h; the result
// row is the accumulator.
// ---------------------------------------------------------------------------
// numpy's max / min: a NaN wins
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

struct ErrorSum {
    using Row = dvsof_eval_result_t;
    static __device__ __forceinline__ Row zero() { return Row{0.0, 0, 0, -__builtin_inff(), __builtin_inff()}; }
    static __device__ __forceinline__ Row add(const Row &a, const Row &b)
    {
        return Row{a.sum_ee + b.sum_ee, a.n_points + b.n_points, a.n_below + b.n_below,
                   nan_max(a.pred_max, b.pred_max), nan_min(a.pred_min, b.pred_min)};
    }
};

__global__ __launch_bounds__(NT) void flow_error_partial_kernel(
    const float *__restrict__ gt_u, const float *__restrict__ gt_v, const float *__restrict__ pred,
    const uint32_t *__restrict__ count, int h, int w, int max_row, int nb,
    dvsof_eval_result_t *__restrict__ part)
{
    const int f = blockIdx.y;
    const int n = h * w, counted = max_row * w;  // rows below max_row are the first max_row * w pixels
    const float *pu = pred + (size_t)f * 2 * n, *pv = pu + n;
    const float *gu = gt_u + (size_t)f * n, *gv = gt_v + (size_t)f * n;
    const uint32_t *cnt = count ? count + (size_t)f * n : nullptr;
    frame_partial<ErrorSum>(n, nb, part, [=](dvsof_eval_result_t &a, int p) {
        const float qu = pu[p], qv = pv[p];
        a.pred_max = nan_max(a.pred_max, nan_max(qu, qv));
        a.pred_min = nan_min(a.pred_min, nan_min(qu, qv));
        if (p < counted && (!cnt || cnt[p] > 0u)) {
            const float tu = gu[p], tv = gv[p];
            if (gt_counts(tu, tv)) {
                const float ee = endpoint_error(tu, tv, qu, qv);
                a.sum_ee += (double)ee;
                a.n_points += 1;
                a.n_below += ee < 3.f ? 1 : 0;
            }
        }
    });
}

// ---------------------------------------------------------------------------
// Count images of a batch, one thread per event.  With the polarity, plane 0
// of a frame counts p > 0 and plane 1 the rest.
// ---------------------------------------------------------------------------
template <bool POLARITY>
__global__ __launch_bounds__(NT) void count_image_batched_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const int64_t *__restrict__ pol,
    int64_t n, const int64_t *__restrict__ begin, int F, int y0, int x0, int h, int w,
    uint32_t *__restrict__ out)
{
    for_each_frame_event(n, begin, F, [=](int64_t e, int f) {
        const int64_t xi = x[e] - x0, yi = y[e] - y0;
        if (xi >= 0 && xi < w && yi >= 0 && yi < h) {
            const size_t plane = POLARITY ? (size_t)f * 2 + (pol[e] > 0 ? 0 : 1) : (size_t)f;
            atomicAdd(&out[(plane * h + (size_t)yi) * w + (size_t)xi], 1u);
        }
    });
}

// dvsof_count_image_batched (pol unused) and dvsof_count_image_polarity_batched
template <bool POLARITY>
int count_images(const int64_t *x, const int64_t *y, const int64_t *pol, int64_t n_events,
                 const int64_t *frame_event_begin, int F, int y0, int x0, int h, int w, uint32_t *out,
                 void *stream)
{
    if (F < 0 || n_events < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (!out || !frame_event_begin || y0 < 0 || x0 < 0 || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide)
        return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || (POLARITY && !pol))) return DVSOF_EINVAL;
    DVSOF_HIP_TRY((hipError_t)fill_u32(out, 0u, sizeof(uint32_t) * (size_t)F * (POLARITY ? 2 : 1) * h * w,
                                       as_stream(stream)));
    if (n_events == 0) return DVSOF_OK;
    hipLaunchKernelGGL(count_image_batched_kernel<POLARITY>, dim3(event_blocks(n_events)), dim3(NT), 0,
                       as_stream(stream), x, y, pol, n_events, frame_event_begin, F, y0, x0, h, w, out);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

bool bad_window(int H, int W, int y0, int x0, int h, int w)
{
    return H < 1 || W < 1 || H > kMaxSide || W > kMaxSide || y0 < 0 || x0 < 0 || h < 1 || w < 1 ||
           (long long)y0 + h > H || (long long)x0 + w > W;
}

}  // namespace

extern "C" {

int dvsof_gt_flow_propagate(const void *x_flow, const void *y_flow, int flow_dtype, int K, int H,
                            int W, const int32_t *frame_step_begin, const int32_t *step_map,
                            const double *step_scale, const int32_t *frame_mode, int F, int S,
                            int y0, int x0, int h, int w, float *u, float *v, void *stream)
{
    if (F < 0 || F > kMaxFrames || S < 0 || K < 0) return DVSOF_EINVAL;
    if (flow_dtype != DVSOF_EVAL_F32 && flow_dtype != DVSOF_EVAL_F64) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (!x_flow || !y_flow || !frame_step_begin || !frame_mode || !u || !v || K < 1) return DVSOF_EINVAL;
    if (S > 0 && (!step_map || !step_scale)) return DVSOF_EINVAL;
    if (bad_window(H, W, y0, x0, h, w)) return DVSOF_EINVAL;
    const dim3 grid((unsigned)(((long long)h * w + NT - 1) / NT), (unsigned)F);
    if (flow_dtype == DVSOF_EVAL_F64)
        hipLaunchKernelGGL(gt_propagate_kernel<double>, grid, dim3(NT), 0, as_stream(stream),
                           (const double *)x_flow, (const double *)y_flow, K, H, W, frame_step_begin,
                           step_map, step_scale, frame_mode, S, y0, x0, h, w, u, v);
    else
        hipLaunchKernelGGL(gt_propagate_kernel<float>, grid, dim3(NT), 0, as_stream(stream),
                           (const float *)x_flow, (const float *)y_flow, K, H, W, frame_step_begin,
                           step_map, step_scale, frame_mode, S, y0, x0, h, w, u, v);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

size_t dvsof_flow_error_workspace_bytes(int F, int h, int w)
{
    if (F < 1 || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide) return 0;
    return sizeof(dvsof_eval_result_t) * (size_t)F * partial_blocks(h, w);
}

int dvsof_flow_error(const float *gt_u, const float *gt_v, const float *pred, const uint32_t *count,
                     int F, int h, int w, int max_row, dvsof_eval_result_t *result, void *workspace,
                     size_t workspace_bytes, void *stream)
{
    if (F < 0 || F > kMaxFrames) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (!gt_u || !gt_v || !pred || !result || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide ||
        max_row < 0 || max_row > h)
        return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_flow_error_workspace_bytes(F, h, w)) return DVSOF_ENOSPACE;
    const int nb = partial_blocks(h, w);
    dvsof_eval_result_t *part = (dvsof_eval_result_t *)workspace;
    hipLaunchKernelGGL(flow_error_partial_kernel, dim3((unsigned)nb, (unsigned)F), dim3(NT), 0,
                       as_stream(stream), gt_u, gt_v, pred, count, h, w, max_row, nb, part);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_final_kernel<ErrorSum>, dim3((unsigned)F), dim3(kWave), 0, as_stream(stream),
                       part, nb, result);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_count_image_batched(const int64_t *x, const int64_t *y, int64_t n_events,
                              const int64_t *frame_event_begin, int F, int y0, int x0, int h, int w,
                              uint32_t *out, void *stream)
{
    return count_images<false>(x, y, nullptr, n_events, frame_event_begin, F, y0, x0, h, w, out, stream);
}

int dvsof_count_image_polarity_batched(const int64_t *x, const int64_t *y, const int64_t *p,
                                       int64_t n_events, const int64_t *frame_event_begin, int F,
                                       int y0, int x0, int h, int w, uint32_t *out, void *stream)
{
    return count_images<true>(x, y, p, n_events, frame_event_begin, F, y0, x0, h, w, out, stream);
}

}  // extern "C"
