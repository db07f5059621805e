// The contrast-maximisation term of contrast.hip with several reference times
// and with ON and OFF events accumulated apart (docs/CONTRAST_SPEC.md sections
// 11-15; Zhu et al., CVPR 2019 warp to both ends of the window and keep the
// polarities apart, Shiba et al., ECCV 2022 add the middle).  Per frame f,
// reference r and channel c there is an image m = (f R + r) C + c of events
// carried over sig = tau - rho_r, and a count image of the channel's events;
// term = mean_m (1 - var(I_m)/var(c_m)).
//
// Replaces nothing of the reference: its loss reads the grey frames only.
//
// Forward: one thread per event reads the flow at its pixel once per frame and
// splats into the R images of its channel (warp_event_to and splat_corners of
// frame_common.h); the count image is repeated per reference by R atomics in
// the same thread, not by a copy launch; dvsof_iwe_stats on M frames; one
// closing wave.  Backward: the R C images of a frame add into the same 64-bit
// fixed-point sums, with one power-of-two unit per frame taken from the
// largest |G| over the frame's images; a thread adds its R addends in
// registers (integers: no order) and issues one atomic per component.  No
// floating-point atomics anywhere.  This file relies on -ffp-contract=off.
#include "frame_common.h"
#include "../../include/dvsof_contrast_multi.h"

namespace {

constexpr int NT = kFrameNT;
constexpr int kUnitBits = 40;    // R = 1: contrast.hip's unit
constexpr int kSharedBits = 2;   // R > 1: up to three addends of a pixel's event share a sum
constexpr int kMaxRefs = 3;

// one per image, in the workspace behind the fixed-point sums
struct ImageRec {
    double mean;  // of I_m
    double coef;  // -2 / (N var(c_m)); 0 where var(c_m) is not positive
    double gmax;  // |coef (I_m - mean)| <= gmax on every pixel
    double term;  // 1 - var(I_m)/var(c_m); 0 where var(c_m) is not positive
};
static_assert(sizeof(ImageRec) == 32, "the workspace holds 32 bytes per image");

struct Refs {
    float rho[kMaxRefs];  // ascending; the first R are read
};

struct Plan {
    int R, C, M;
    Refs refs;
};

// ---------------------------------------------------------------------------
// Forward.  One thread per event; which frames it takes part in is
// contrast.hip's rule, its channel the sign of p.
// ---------------------------------------------------------------------------
template <int R, bool POL>
__global__ __launch_bounds__(NT) void contrast_multi_splat_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t,
    const int64_t *__restrict__ pol, const int64_t *__restrict__ sample, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, const float *__restrict__ flow, int F, int h, int w, Refs refs,
    unsigned long long *__restrict__ q, uint32_t *__restrict__ count)
{
    constexpr int C = POL ? 2 : 1;
    const int64_t stride = (int64_t)gridDim.x * NT;
    const size_t plane = (size_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const int64_t xi = x[e], yi = y[e];
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;  // the -1 slots of cropped and padded events
        int c = 0;
        if (POL) {
            const int64_t pe = pol[e];
            if (pe == 0) continue;  // in neither channel and in no count
            c = pe < 0;
        }
        const float te = t[e];
        const int64_t s = sample[e];
        const size_t pix = (size_t)yi * w + (size_t)xi;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != s) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;  // a test, not a clamp; false for a NaN
            const float tau = event_tau(te, t0, t1);
            const float *fl = flow + (size_t)f * 2 * plane + pix;
            const float u = fl[0], v = fl[plane];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const size_t m = ((size_t)f * R + r) * C + c;
                atomicAdd(count + m * plane + pix, 1u);
                Warp p;
                if (!warp_event_to(tau, refs.rho[r], u, v, xi, yi, h, w, p)) continue;
                splat_corners(p, h, w, q + m * plane);
            }
        }
    }
}

// One wave: the record of every image (lane k takes images k, k + 64, ...);
// after a barrier the unit of every frame (lane k takes frames k, k + 64, ...;
// a maximum has no order) and, in lane 0, the images' terms in image order.
__global__ __launch_bounds__(kWave) void contrast_multi_close_kernel(const dvsof_iwe_result_t *__restrict__ result,
                                                                     int F, int RC, int h, int w, int unit_bits,
                                                                     ImageRec *rec, double *unit, float *term)
{
    const double N = (double)h * (double)w;
    const int M = F * RC;
    for (int m = threadIdx.x; m < M; m += kWave) {
        const dvsof_iwe_result_t r = result[m];
        const double mean = (double)r.sum_q * 0x1p-32 / N;
        const double var_i = r.sum_sq / N - mean * mean;
        const double cmean = (double)r.count_sum / N;
        const double var_c = (double)r.count_sq / N - cmean * cmean;
        ImageRec o;
        o.mean = mean;
        o.coef = var_c > 0.0 ? -2.0 / (N * var_c) : 0.0;
        o.term = var_c > 0.0 ? 1.0 - var_i / var_c : 0.0;
        o.gmax = fabs(o.coef) * fmax((double)r.max_q * 0x1p-32 - mean, mean);
        rec[m] = o;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < F; f += kWave) {
        double gmax = 0.0;
        for (int k = 0; k < RC; ++k) gmax = fmax(gmax, rec[f * RC + k].gmax);
        int e = 0;
        if (gmax > 0.0) (void)frexp(gmax, &e);  // |G_m| <= gmax < 2^e for every image of the frame
        unit[f] = ldexp(1.0, unit_bits - e);
    }
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s += rec[m].term;
        *term = (float)(s / (double)M);
    }
}

// ---------------------------------------------------------------------------
// Backward.  One thread per event and frame: for every reference G = coef (I -
// mean) at the four corners of the image of its channel, the derivative of the
// bilinear weights, -sig of it in float64, truncated to the frame's unit.
// ---------------------------------------------------------------------------
template <int R, bool POL>
__global__ __launch_bounds__(NT) void contrast_multi_bwd_events_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t,
    const int64_t *__restrict__ pol, const int64_t *__restrict__ sample, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, const float *__restrict__ flow, int F, int h, int w, Refs refs,
    const int64_t *__restrict__ q, const ImageRec *__restrict__ rec, const double *__restrict__ unit,
    unsigned long long *__restrict__ acc)
{
    constexpr int C = POL ? 2 : 1;
    const int64_t stride = (int64_t)gridDim.x * NT;
    const size_t plane = (size_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const int64_t xi = x[e], yi = y[e];
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;
        int c = 0;
        if (POL) {
            const int64_t pe = pol[e];
            if (pe == 0) continue;
            c = pe < 0;
        }
        const float te = t[e];
        const int64_t s = sample[e];
        const size_t pix = (size_t)yi * w + (size_t)xi;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != s) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;
            const float tau = event_tau(te, t0, t1);
            const float *fl = flow + (size_t)f * 2 * plane + pix;
            const float u = fl[0], v = fl[plane];
            const double un = unit[f];
            long long su = 0, sv = 0;  // at most three addends below 2^39 (1 + 2^-22) each
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const size_t m = ((size_t)f * R + r) * C + c;
                const ImageRec a = rec[m];
                if (a.coef == 0.0) continue;  // var(c_m) = 0: every addend would be 0
                Warp p;
                if (!warp_event_to(tau, refs.rho[r], u, v, xi, yi, h, w, p)) continue;
                const int64_t *img = q + m * plane;
                double G[2][2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int xx = p.cx + i, yy = p.cy + j;
                        const bool in = xx >= 0 && xx < w && yy >= 0 && yy < h;
                        G[j][i] = in ? a.coef * ((double)img[(size_t)yy * w + (size_t)xx] * 0x1p-32 - a.mean) : 0.0;
                    }
                }
                const double gx = (double)p.wy[0] * (G[0][1] - G[0][0]) + (double)p.wy[1] * (G[1][1] - G[1][0]);
                const double gy = (double)p.wx[0] * (G[1][0] - G[0][0]) + (double)p.wx[1] * (G[1][1] - G[0][1]);
                const double ms = -(double)p.tau;  // p.tau holds sig; d xw / d u = -sig
                su += (long long)(ms * gx * un);
                sv += (long long)(ms * gy * un);
            }
            unsigned long long *dst = acc + (size_t)f * 2 * plane + pix;
            if (su != 0) atomicAdd(dst, (unsigned long long)su);
            if (sv != 0) atomicAdd(dst + plane, (unsigned long long)sv);
        }
    }
}

// One thread per element of grad_flow: convert, clear the sum for the next
// backward of the same forward, store.
__global__ __launch_bounds__(NT) void contrast_multi_bwd_close_kernel(long long *__restrict__ acc,
                                                                      const double *__restrict__ unit,
                                                                      const float *__restrict__ seed, float weight,
                                                                      int F, int M, size_t per_frame,
                                                                      float *__restrict__ grad)
{
    const size_t total = (size_t)F * per_frame, stride = (size_t)gridDim.x * NT;
    const float sw = seed[0] * weight;
    for (size_t k = (size_t)blockIdx.x * NT + threadIdx.x; k < total; k += stride) {
        const long long a = acc[k];
        acc[k] = 0;
        const double value = (double)a / unit[k / per_frame] / (double)M;  // the first division is exact
        grad[k] = sw * (float)value;
    }
}

size_t sums_bytes(int F, int h, int w) { return sizeof(int64_t) * 2 * (size_t)F * h * w; }

// false: arguments the calls refuse
bool plan_of(int F, int reference_mask, int polarity, Plan &o)
{
    if (reference_mask < 1 || reference_mask > 7 || polarity < 0 || polarity > 1) return false;
    static const float rho[kMaxRefs] = {0.f, 0.5f, 1.f};
    o.R = 0;
    for (int b = 0; b < kMaxRefs; ++b)
        if (reference_mask >> b & 1) o.refs.rho[o.R++] = rho[b];
    for (int r = o.R; r < kMaxRefs; ++r) o.refs.rho[r] = 0.f;
    o.C = polarity ? 2 : 1;
    if (F > kMaxFrames) return false;
    o.M = F * o.R * o.C;
    return o.M <= kMaxFrames;  // the images ride in gridDim.y of the statistics
}

struct Workspace {
    unsigned long long *sums;
    ImageRec *rec;
    double *unit;
    void *stats;
    size_t stats_bytes;
};

Workspace carve(void *workspace, int F, int h, int w, const Plan &pl)
{
    char *ws = (char *)workspace;
    Workspace o;
    o.sums = (unsigned long long *)ws;
    o.rec = (ImageRec *)(ws + sums_bytes(F, h, w));
    o.unit = (double *)(o.rec + pl.M);
    o.stats = o.unit + F;
    o.stats_bytes = dvsof_iwe_stats_workspace_bytes(pl.M, h, w);
    return o;
}

// kernel<R, POL> for the plan's R and C
#define DVSOF_MULTI_DISPATCH(kernel, pl, ...)                                                       \
    do {                                                                                            \
        if ((pl).C == 2) {                                                                          \
            if ((pl).R == 1) hipLaunchKernelGGL((kernel<1, true>), __VA_ARGS__);                    \
            else if ((pl).R == 2) hipLaunchKernelGGL((kernel<2, true>), __VA_ARGS__);               \
            else hipLaunchKernelGGL((kernel<3, true>), __VA_ARGS__);                                \
        } else {                                                                                    \
            if ((pl).R == 1) hipLaunchKernelGGL((kernel<1, false>), __VA_ARGS__);                   \
            else if ((pl).R == 2) hipLaunchKernelGGL((kernel<2, false>), __VA_ARGS__);              \
            else hipLaunchKernelGGL((kernel<3, false>), __VA_ARGS__);                               \
        }                                                                                           \
    } while (0)

}  // namespace

extern "C" {

size_t dvsof_contrast_multi_workspace_bytes(int F, int reference_mask, int polarity, int h, int w)
{
    Plan pl;
    if (F < 1 || bad_frame_sizes(F, h, w) || !plan_of(F, reference_mask, polarity, pl)) return 0;
    return sums_bytes(F, h, w) + sizeof(ImageRec) * (size_t)pl.M + sizeof(double) * (size_t)F +
           dvsof_iwe_stats_workspace_bytes(pl.M, h, w);
}

int dvsof_contrast_multi_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                             const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                             const int64_t *frame_sample, const float *flow, int F, int h, int w,
                             int reference_mask, int polarity, int64_t *q, uint32_t *count,
                             dvsof_iwe_result_t *result, float *term, void *workspace, size_t workspace_bytes,
                             void *stream)
{
    Plan pl;
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !count || !result || !term || !frame_ts || !frame_sample || !flow)
        return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || !t || !sample_index || (polarity && !p))) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_contrast_multi_workspace_bytes(F, reference_mask, polarity, h, w))
        return DVSOF_ENOSPACE;
    hipStream_t st = as_stream(stream);
    const size_t pixels = (size_t)pl.M * h * w;
    const Workspace ws = carve(workspace, F, h, w, pl);
    DVSOF_HIP_TRY((hipError_t)fill_u32(q, 0u, sizeof(int64_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(count, 0u, sizeof(uint32_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws.sums, 0u, sums_bytes(F, h, w), st));
    if (n_events > 0) {
        DVSOF_MULTI_DISPATCH(contrast_multi_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, x, y,
                             t, p, sample_index, n_events, frame_ts, frame_sample, flow, F, h, w, pl.refs,
                             (unsigned long long *)q, count);
        DVSOF_LAUNCH_CHECK();
    }
    const int rc = dvsof_iwe_stats(q, count, pl.M, h, w, result, ws.stats, ws.stats_bytes, stream);
    if (rc != DVSOF_OK) return rc;
    hipLaunchKernelGGL(contrast_multi_close_kernel, dim3(1), dim3(kWave), 0, st, result, F, pl.R * pl.C, h, w,
                       pl.R > 1 ? kUnitBits - kSharedBits : kUnitBits, ws.rec, ws.unit, term);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_contrast_multi_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                             const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                             const int64_t *frame_sample, const float *flow, int F, int h, int w,
                             int reference_mask, int polarity, const int64_t *q, void *workspace,
                             size_t workspace_bytes, const float *seed, float weight, float *grad_flow,
                             void *stream)
{
    Plan pl;
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !seed || !grad_flow || !frame_ts || !frame_sample || !flow)
        return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || !t || !sample_index || (polarity && !p))) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_contrast_multi_workspace_bytes(F, reference_mask, polarity, h, w))
        return DVSOF_ENOSPACE;
    hipStream_t st = as_stream(stream);
    const Workspace ws = carve(workspace, F, h, w, pl);
    if (n_events > 0) {
        DVSOF_MULTI_DISPATCH(contrast_multi_bwd_events_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st,
                             x, y, t, p, sample_index, n_events, frame_ts, frame_sample, flow, F, h, w, pl.refs, q,
                             (const ImageRec *)ws.rec, (const double *)ws.unit, ws.sums);
        DVSOF_LAUNCH_CHECK();
    }
    const size_t per_frame = 2 * (size_t)h * w, total = (size_t)F * per_frame;
    hipLaunchKernelGGL(contrast_multi_bwd_close_kernel, dim3(event_blocks((int64_t)total)), dim3(NT), 0, st,
                       (long long *)ws.sums, (const double *)ws.unit, seed, weight, F, pl.M, per_frame, grad_flow);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
