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
#include "common.h"

static_assert(sizeof(dvsof_eval_result_t) == 32, "result rows are 32 bytes (eval.py reads them as such)");

namespace {

constexpr int NT = 256;
constexpr int kMaxErrBlocks = 128;  // partials per frame: two per lane of the closing wave
constexpr int kMaxSide = 32767;     // beyond it an int16-saturated coordinate could be inside the map

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
        // H, W <= 32767 a coordinate saturated to the int16 range is outside too.
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
// Endpoint error.  Fixed-order reduction: thread (strided pixels, ascending)
// -> wave (shuffle tree) -> block (waves 0..3) -> frame (partials ascending).
// ---------------------------------------------------------------------------
// numpy's max / min: a NaN wins
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

struct Acc {
    double sum;
    long long n, below;
    float mx, mn;
};
__device__ __forceinline__ Acc acc_zero()
{
    return Acc{0.0, 0, 0, -__builtin_inff(), __builtin_inff()};
}
__device__ __forceinline__ Acc acc_add(const Acc &a, const Acc &b)
{
    return Acc{a.sum + b.sum, a.n + b.n, a.below + b.below, nan_max(a.mx, b.mx), nan_min(a.mn, b.mn)};
}
// valid in lane 0
__device__ __forceinline__ Acc acc_wave(Acc a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Acc b;
        b.sum = __shfl_down(a.sum, off, kWave);
        b.n = __shfl_down(a.n, off, kWave);
        b.below = __shfl_down(a.below, off, kWave);
        b.mx = __shfl_down(a.mx, off, kWave);
        b.mn = __shfl_down(a.mn, off, kWave);
        a = acc_add(a, b);
    }
    return a;
}
__device__ __forceinline__ void acc_store(dvsof_eval_result_t *r, const Acc &a)
{
    r->sum_ee = a.sum;
    r->n_points = a.n;
    r->n_below = a.below;
    r->pred_max = a.mx;
    r->pred_min = a.mn;
}

__global__ __launch_bounds__(NT) void flow_error_partial_kernel(
    const float *__restrict__ gt_u, const float *__restrict__ gt_v, const float *__restrict__ pred,
    const uint32_t *__restrict__ count, int h, int w, int max_row, int nb,
    dvsof_eval_result_t *__restrict__ part)
{
    const int f = blockIdx.y, b = blockIdx.x;
    const int n = h * w, counted = max_row * w;  // rows below max_row are the first max_row * w pixels
    const float *pu = pred + (size_t)f * 2 * n, *pv = pu + n;
    const float *gu = gt_u + (size_t)f * n, *gv = gt_v + (size_t)f * n;
    const uint32_t *cnt = count ? count + (size_t)f * n : nullptr;
    Acc a = acc_zero();
    for (int p = b * NT + threadIdx.x; p < n; p += nb * NT) {
        const float qu = pu[p], qv = pv[p];
        a.mx = nan_max(a.mx, nan_max(qu, qv));
        a.mn = nan_min(a.mn, nan_min(qu, qv));
        if (p < counted && (!cnt || cnt[p] > 0u)) {
            const float tu = gu[p], tv = gv[p];
            if (!isinf(tu) && !isinf(tv) && sqrtf(tu * tu + tv * tv) > 0.f) {
                const float du = tu - qu, dv = tv - qv;
                const float ee = sqrtf(du * du + dv * dv);
                a.sum += (double)ee;
                a.n += 1;
                a.below += ee < 3.f ? 1 : 0;
            }
        }
    }
    a = acc_wave(a);
    __shared__ Acc sh[NT / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        Acc t = sh[0];
#pragma unroll
        for (int k = 1; k < NT / kWave; ++k) t = acc_add(t, sh[k]);
        acc_store(&part[(size_t)f * nb + b], t);
    }
}

__global__ __launch_bounds__(kWave) void flow_error_final_kernel(
    const dvsof_eval_result_t *__restrict__ part, int nb, dvsof_eval_result_t *__restrict__ result)
{
    const int f = blockIdx.x;
    Acc a = acc_zero();
    for (int k = threadIdx.x; k < nb; k += kWave) {
        const dvsof_eval_result_t r = part[(size_t)f * nb + k];
        a = acc_add(a, Acc{r.sum_ee, (long long)r.n_points, (long long)r.n_below, r.pred_max, r.pred_min});
    }
    a = acc_wave(a);
    if (threadIdx.x == 0) acc_store(&result[f], a);
}

int err_blocks(int h, int w)
{
    const long long n = (long long)h * w;
    const long long nb = (n + 4 * NT - 1) / (4 * NT);  // ~4 pixels per thread
    return (int)(nb < 1 ? 1 : (nb > kMaxErrBlocks ? kMaxErrBlocks : nb));
}

// ---------------------------------------------------------------------------
// Count images of a batch.  One thread per event; the frame of event e is the
// last f with frame_event_begin[f] <= e.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void count_image_batched_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, int64_t n,
    const int64_t *__restrict__ begin, int F, int y0, int x0, int h, int w,
    uint32_t *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    const int64_t first = begin[0], last = begin[F];
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        if (e < first || e >= last) continue;
        int lo = 0, hi = F;  // begin[lo] <= e < begin[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (begin[mid] <= e) lo = mid; else hi = mid;
        }
        const int64_t xi = x[e] - x0, yi = y[e] - y0;
        if (xi >= 0 && xi < w && yi >= 0 && yi < h)
            atomicAdd(&out[((size_t)lo * h + (size_t)yi) * w + (size_t)xi], 1u);
    }
}

// The same with the polarity: plane 0 of a frame counts p > 0, plane 1 the rest.
__global__ __launch_bounds__(NT) void count_image_polarity_batched_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const int64_t *__restrict__ pol,
    int64_t n, const int64_t *__restrict__ begin, int F, int y0, int x0, int h, int w,
    uint32_t *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    const int64_t first = begin[0], last = begin[F];
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        if (e < first || e >= last) continue;
        int lo = 0, hi = F;  // begin[lo] <= e < begin[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (begin[mid] <= e) lo = mid; else hi = mid;
        }
        const int64_t xi = x[e] - x0, yi = y[e] - y0;
        if (xi >= 0 && xi < w && yi >= 0 && yi < h) {
            const size_t plane = (size_t)lo * 2 + (pol[e] > 0 ? 0 : 1);
            atomicAdd(&out[(plane * h + (size_t)yi) * w + (size_t)xi], 1u);
        }
    }
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
    if (F < 0 || F > 65535 || S < 0 || K < 0) return DVSOF_EINVAL;
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
    return sizeof(dvsof_eval_result_t) * (size_t)F * err_blocks(h, w);
}

int dvsof_flow_error(const float *gt_u, const float *gt_v, const float *pred, const uint32_t *count,
                     int F, int h, int w, int max_row, dvsof_eval_result_t *result, void *workspace,
                     size_t workspace_bytes, void *stream)
{
    if (F < 0 || F > 65535) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (!gt_u || !gt_v || !pred || !result || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide ||
        max_row < 0 || max_row > h)
        return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_flow_error_workspace_bytes(F, h, w)) return DVSOF_ENOSPACE;
    const int nb = err_blocks(h, w);
    dvsof_eval_result_t *part = (dvsof_eval_result_t *)workspace;
    hipLaunchKernelGGL(flow_error_partial_kernel, dim3((unsigned)nb, (unsigned)F), dim3(NT), 0,
                       as_stream(stream), gt_u, gt_v, pred, count, h, w, max_row, nb, part);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(flow_error_final_kernel, dim3((unsigned)F), dim3(kWave), 0, as_stream(stream),
                       part, nb, result);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_count_image_batched(const int64_t *x, const int64_t *y, int64_t n_events,
                              const int64_t *frame_event_begin, int F, int y0, int x0, int h, int w,
                              uint32_t *out, void *stream)
{
    if (F < 0 || n_events < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (!out || !frame_event_begin || y0 < 0 || x0 < 0 || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide)
        return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y)) return DVSOF_EINVAL;
    DVSOF_HIP_TRY((hipError_t)fill_u32(out, 0u, sizeof(uint32_t) * (size_t)F * h * w, as_stream(stream)));
    if (n_events == 0) return DVSOF_OK;
    const int64_t blocks = (n_events + NT - 1) / NT;
    hipLaunchKernelGGL(count_image_batched_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)),
                       dim3(NT), 0, as_stream(stream), x, y, n_events, frame_event_begin, F, y0, x0, h,
                       w, out);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_count_image_polarity_batched(const int64_t *x, const int64_t *y, const int64_t *p,
                                       int64_t n_events, const int64_t *frame_event_begin, int F,
                                       int y0, int x0, int h, int w, uint32_t *out, void *stream)
{
    if (F < 0 || n_events < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (!out || !frame_event_begin || y0 < 0 || x0 < 0 || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide)
        return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || !p)) return DVSOF_EINVAL;
    DVSOF_HIP_TRY((hipError_t)fill_u32(out, 0u, sizeof(uint32_t) * (size_t)F * 2 * h * w, as_stream(stream)));
    if (n_events == 0) return DVSOF_OK;
    const int64_t blocks = (n_events + NT - 1) / NT;
    hipLaunchKernelGGL(count_image_polarity_batched_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)),
                       dim3(NT), 0, as_stream(stream), x, y, p, n_events, frame_event_begin, F, y0, x0,
                       h, w, out);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
