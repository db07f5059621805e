// Contrast-maximisation term of the training loss and its gradient with
// respect to the flow (docs/CONTRAST_SPEC.md): per frame the image of warped
// events I_f of csrc/iwe.hip and the count image c_f of the same events,
// term = mean_f (1 - var(I_f)/var(c_f)) (Gallego et al., CVPR 2018; the
// normalisation is the flow warp loss of Stoffregen et al., ECCV 2020).
//
// Replaces nothing of the reference: its loss reads the grey frames only.
//
// Forward: the warp and splat of frame_common.h, which are iwe.hip's, with the
// frame found by sample and time window instead of by position in the
// columns, the statistics of dvsof_iwe_stats, one closing wave.  Backward: the
// scatter into the flow gradient collides on almost every active pixel, so it
// is summed in 64-bit fixed point with a per-frame power-of-two unit and
// integer atomics (the sums have no order), and one thread per element
// converts once.  No floating-point atomics anywhere.  This file relies on
// -ffp-contract=off.
#include "frame_common.h"
#include "../../include/dvsof_contrast.h"

namespace {

constexpr int NT = kFrameNT;
constexpr int kUnitBits = 40;  // |one event's addend| < 2^(kUnitBits + 1) units

// one per frame, in the workspace behind the fixed-point sums
struct FrameRec {
    double mean;  // of I_f
    double coef;  // -2 / (N var(c_f)); 0 where var(c_f) is not positive
    double unit;  // 2^k: the flow gradient of the frame is summed in units of 1/unit
    double term;  // 1 - var(I_f)/var(c_f); 0 where var(c_f) is not positive
};
static_assert(sizeof(FrameRec) == 32, "the workspace holds 32 bytes per frame");

// ---------------------------------------------------------------------------
// Forward.  One thread per event; an event takes part in every frame of its
// sample whose window holds its time (both ends included).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void contrast_splat_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t,
    const int64_t *__restrict__ sample, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, const float *__restrict__ flow, int F, int h, int w,
    unsigned long long *__restrict__ q, uint32_t *__restrict__ count)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    const size_t plane = (size_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const int64_t xi = x[e], yi = y[e];
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;  // the -1 slots of cropped and padded events
        const float te = t[e];
        const int64_t s = sample[e];
        const size_t pix = (size_t)yi * w + (size_t)xi;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != s) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;  // a test, not a clamp; false for a NaN
            atomicAdd(count + (size_t)f * plane + pix, 1u);
            Warp p;
            if (!warp_event(te, t0, t1, flow + (size_t)f * 2 * plane + pix, plane, xi, yi, h, w, p)) continue;
            splat_corners(p, h, w, q + (size_t)f * plane);
        }
    }
}

// One wave: the record of every frame (lane k takes frames k, k + 64, ...),
// then lane 0 adds the frames' terms in frame order.
__global__ __launch_bounds__(kWave) void contrast_close_kernel(const dvsof_iwe_result_t *__restrict__ result,
                                                               int F, int h, int w, FrameRec *rec, float *term)
{
    const double N = (double)h * (double)w;
    for (int f = threadIdx.x; f < F; f += kWave) {
        const dvsof_iwe_result_t r = result[f];
        const double mean = (double)r.sum_q * 0x1p-32 / N;
        const double var_i = r.sum_sq / N - mean * mean;
        const double cmean = (double)r.count_sum / N;
        const double var_c = (double)r.count_sq / N - cmean * cmean;
        FrameRec o;
        o.mean = mean;
        o.coef = var_c > 0.0 ? -2.0 / (N * var_c) : 0.0;
        o.term = var_c > 0.0 ? 1.0 - var_i / var_c : 0.0;
        // |G| = |coef (I - mean)| <= gmax < 2^e
        const double gmax = fabs(o.coef) * fmax((double)r.max_q * 0x1p-32 - mean, mean);
        int e = 0;
        if (gmax > 0.0) (void)frexp(gmax, &e);
        o.unit = ldexp(1.0, kUnitBits - e);
        rec[f] = o;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int f = 0; f < F; ++f) s += rec[f].term;
        *term = (float)(s / (double)F);
    }
}

// ---------------------------------------------------------------------------
// Backward.  One thread per event: G = coef (I - mean) at the four corners
// (0 outside the image), the derivative of the bilinear weights, -tau of it to
// the event's own pixel of the flow, in float64, truncated to the frame's unit.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void contrast_bwd_events_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t,
    const int64_t *__restrict__ sample, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, const float *__restrict__ flow, int F, int h, int w,
    const int64_t *__restrict__ q, const FrameRec *__restrict__ rec, unsigned long long *__restrict__ acc)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    const size_t plane = (size_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const int64_t xi = x[e], yi = y[e];
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;
        const float te = t[e];
        const int64_t s = sample[e];
        const size_t pix = (size_t)yi * w + (size_t)xi;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != s) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;
            const FrameRec r = rec[f];
            if (r.coef == 0.0) continue;  // var(c_f) = 0: every addend would be 0
            Warp p;
            if (!warp_event(te, t0, t1, flow + (size_t)f * 2 * plane + pix, plane, xi, yi, h, w, p)) continue;
            const int64_t *img = q + (size_t)f * plane;
            double G[2][2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int xx = p.cx + i, yy = p.cy + j;
                    const bool in = xx >= 0 && xx < w && yy >= 0 && yy < h;
                    G[j][i] = in ? r.coef * ((double)img[(size_t)yy * w + (size_t)xx] * 0x1p-32 - r.mean) : 0.0;
                }
            }
            const double gx = (double)p.wy[0] * (G[0][1] - G[0][0]) + (double)p.wy[1] * (G[1][1] - G[1][0]);
            const double gy = (double)p.wx[0] * (G[1][0] - G[0][0]) + (double)p.wx[1] * (G[1][1] - G[0][1]);
            const double mt = -(double)p.tau;
            // |mt g| < 2^(e+1) (1 + 2^-22), so |a| < 2^41 (1 + 2^-22); the product with the unit is exact
            const long long au = (long long)(mt * gx * r.unit), av = (long long)(mt * gy * r.unit);
            unsigned long long *dst = acc + (size_t)f * 2 * plane + pix;
            if (au != 0) atomicAdd(dst, (unsigned long long)au);
            if (av != 0) atomicAdd(dst + plane, (unsigned long long)av);
        }
    }
}

// One thread per element of grad_flow: convert, clear the sum for the next
// backward of the same forward, store.
__global__ __launch_bounds__(NT) void contrast_bwd_close_kernel(long long *__restrict__ acc,
                                                                const FrameRec *__restrict__ rec,
                                                                const float *__restrict__ seed, float weight, int F,
                                                                size_t per_frame, float *__restrict__ grad)
{
    const size_t total = (size_t)F * per_frame, stride = (size_t)gridDim.x * NT;
    const float sw = seed[0] * weight;
    for (size_t k = (size_t)blockIdx.x * NT + threadIdx.x; k < total; k += stride) {
        const long long a = acc[k];
        acc[k] = 0;
        const double value = (double)a / rec[k / per_frame].unit / (double)F;  // the first division is exact
        grad[k] = sw * (float)value;
    }
}

size_t sums_bytes(int F, int h, int w) { return sizeof(int64_t) * 2 * (size_t)F * h * w; }

}  // namespace

extern "C" {

size_t dvsof_contrast_workspace_bytes(int F, int h, int w)
{
    if (F < 1 || bad_frame_sizes(F, h, w)) return 0;
    return sums_bytes(F, h, w) + sizeof(FrameRec) * (size_t)F + dvsof_iwe_stats_workspace_bytes(F, h, w);
}

int dvsof_contrast_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *sample_index,
                       int64_t n_events, const float *frame_ts, const int64_t *frame_sample, const float *flow,
                       int F, int h, int w, int64_t *q, uint32_t *count, dvsof_iwe_result_t *result, float *term,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    if (F < 0 || n_events < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !count || !result || !term || !frame_ts || !frame_sample || !flow)
        return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || !t || !sample_index)) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_contrast_workspace_bytes(F, h, w)) return DVSOF_ENOSPACE;
    hipStream_t st = as_stream(stream);
    const size_t pixels = (size_t)F * h * w;
    char *ws = (char *)workspace;
    FrameRec *rec = (FrameRec *)(ws + sums_bytes(F, h, w));
    DVSOF_HIP_TRY((hipError_t)fill_u32(q, 0u, sizeof(int64_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(count, 0u, sizeof(uint32_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws, 0u, sums_bytes(F, h, w), st));
    if (n_events > 0) {
        hipLaunchKernelGGL(contrast_splat_kernel, dim3(event_blocks(n_events)), dim3(NT), 0, st, x, y, t,
                           sample_index, n_events, frame_ts, frame_sample, flow, F, h, w, (unsigned long long *)q,
                           count);
        DVSOF_LAUNCH_CHECK();
    }
    const int rc = dvsof_iwe_stats(q, count, F, h, w, result, rec + F, dvsof_iwe_stats_workspace_bytes(F, h, w),
                                   stream);
    if (rc != DVSOF_OK) return rc;
    hipLaunchKernelGGL(contrast_close_kernel, dim3(1), dim3(kWave), 0, st, result, F, h, w, rec, term);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_contrast_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *sample_index,
                       int64_t n_events, const float *frame_ts, const int64_t *frame_sample, const float *flow,
                       int F, int h, int w, const int64_t *q, void *workspace, size_t workspace_bytes,
                       const float *seed, float weight, float *grad_flow, void *stream)
{
    if (F < 0 || n_events < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !seed || !grad_flow || !frame_ts || !frame_sample || !flow)
        return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || !t || !sample_index)) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_contrast_workspace_bytes(F, h, w)) return DVSOF_ENOSPACE;
    hipStream_t st = as_stream(stream);
    char *ws = (char *)workspace;
    const FrameRec *rec = (const FrameRec *)(ws + sums_bytes(F, h, w));
    if (n_events > 0) {
        hipLaunchKernelGGL(contrast_bwd_events_kernel, dim3(event_blocks(n_events)), dim3(NT), 0, st, x, y, t,
                           sample_index, n_events, frame_ts, frame_sample, flow, F, h, w, q, rec,
                           (unsigned long long *)ws);
        DVSOF_LAUNCH_CHECK();
    }
    const size_t per_frame = 2 * (size_t)h * w, total = (size_t)F * per_frame;
    hipLaunchKernelGGL(contrast_bwd_close_kernel, dim3(event_blocks((int64_t)total)), dim3(NT), 0, st,
                       (long long *)ws, rec, seed, weight, F, per_frame, grad_flow);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
