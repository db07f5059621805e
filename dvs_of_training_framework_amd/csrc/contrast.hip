// Contrast-maximisation term of the training loss and its gradient with
// respect to the flow (docs/CONTRAST_SPEC.md): per image the warped events I_m
// and the count image c_m of the same events,
// term = mean_m (1 - var(I_m)/var(c_m)) (Gallego et al., CVPR 2018; the
// normalisation is the flow warp loss of Stoffregen et al., ECCV 2020).  A
// frame has one image, of all its events carried to the start of its window,
// or one per reference time and polarity channel (sections 11-15; Zhu et al.,
// CVPR 2019 warp to both ends of the window and keep the polarities apart,
// Shiba et al., ECCV 2022 add the middle): m = (f R + r) C + c of
// event_images.h, which iwe.hip shares.
//
// Replaces nothing of the reference: its loss reads the grey frames only.
//
// Forward: one thread per event finds its frames by sample and time window,
// reads the flow at its pixel once per frame and splats into the R images of
// its channel (splat_event of event_images.h; the count image is repeated per
// reference by R atomics in the same thread, not by a copy launch);
// dvsof_iwe_stats on M frames; one closing wave.  Backward: the scatter into
// the flow gradient collides on almost every active pixel, so the R C images
// of a frame add into the same 64-bit fixed-point sums, with one power-of-two
// unit per frame taken from the largest |G| over the frame's images; a thread
// adds its R addends in registers (integers: no order) and issues one integer
// atomic per component, and one thread per element converts once.  No
// floating-point atomics anywhere.  This file relies on -ffp-contract=off.
//
// At the end of the file: the term on every flow scale of the network by one
// splat, one closing wave and one backward for all levels (sections 19-23,
// include/dvsof_contrast_pyramid.h); the kernels above are not touched by it.
#include "event_columns.h"
#include "../../include/dvsof_contrast.h"
#include "../../include/dvsof_contrast_multi.h"
#include "../../include/dvsof_contrast_pyramid.h"
#include "../../include/dvsof_event_terms_encoded.h"

namespace {

constexpr int NT = kFrameNT;
constexpr int kUnitBits = 40;   // R = 1: |one event's addend| < 2^(kUnitBits + 1) units
constexpr int kSharedBits = 2;  // R > 1: up to three addends of a pixel's event share a sum

// one per image, in the workspace behind the fixed-point sums
struct ImageRec {
    double mean;  // of I_m
    double coef;  // -2 / (N var(c_m)); 0 where var(c_m) is not positive
    double gmax;  // |coef (I_m - mean)| <= gmax on every pixel
    double term;  // 1 - var(I_m)/var(c_m); 0 where var(c_m) is not positive
};
static_assert(sizeof(ImageRec) == 32, "the workspace holds 32 bytes per image");

// ---------------------------------------------------------------------------
// Forward.  One thread per event; an event takes part in every frame of its
// sample whose window holds its time (both ends included), in the channel of
// the sign of p.
// ---------------------------------------------------------------------------
template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void contrast_splat_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, const float *__restrict__ flow, int F, int h, int w, Refs refs,
    unsigned long long *__restrict__ q, uint32_t *__restrict__ count)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    const size_t plane = (size_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const EventRow ev = cols.template load<POL>(e);
        const int64_t xi = ev.x, yi = ev.y;
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;  // the -1 slots of cropped and padded events
        int c;
        if (!event_channel<POL>(ev.sign, c)) continue;
        const float te = ev.t;
        const int64_t s = ev.sample;
        const size_t pix = (size_t)yi * w + (size_t)xi;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != s) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;  // a test, not a clamp; false for a NaN
            const float tau = event_tau(te, t0, t1);
            const float *fl = flow + (size_t)f * 2 * plane + pix;
            const float u = fl[0], v = fl[plane];
            splat_event<R, POL, true>(refs, f, c, tau, u, v, xi, yi, pix, plane, h, w, q, count);
        }
    }
}

// 2^k: the flow gradient of a frame is summed in units of 1/unit; |G_m| <= gmax < 2^e for every image of the frame
__device__ __forceinline__ double unit_of(double gmax, int unit_bits)
{
    int e = 0;
    if (gmax > 0.0) (void)frexp(gmax, &e);
    return ldexp(1.0, unit_bits - e);
}

// One wave: the record of every image (lane k takes images k, k + 64, ...);
// after a barrier the unit of every frame (lane k takes frames k, k + 64, ...;
// a maximum has no order) and, in lane 0, the images' terms in image order.
// A frame of one image has its unit from the gmax its lane holds.
__global__ __launch_bounds__(kWave) void contrast_close_kernel(const dvsof_iwe_result_t *__restrict__ result, int F,
                                                               int RC, int h, int w, int unit_bits, ImageRec *rec,
                                                               double *unit, float *term)
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
        if (RC == 1) unit[m] = unit_of(o.gmax, unit_bits);
    }
    __syncthreads();
    if (RC > 1) {
        for (int f = threadIdx.x; f < F; f += kWave) {
            double gmax = 0.0;
            for (int k = 0; k < RC; ++k) gmax = fmax(gmax, rec[f * RC + k].gmax);
            unit[f] = unit_of(gmax, unit_bits);
        }
    }
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s += rec[m].term;
        *term = (float)(s / (double)M);
    }
}

// ---------------------------------------------------------------------------
// Backward.  One thread per event and frame: for every reference G = coef (I -
// mean) at the four corners of the image of its channel (0 outside the image),
// the derivative of the bilinear weights, -sig of it to the event's own pixel
// of the flow, in float64, truncated to the frame's unit.
// ---------------------------------------------------------------------------
template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void contrast_bwd_events_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, const float *__restrict__ flow, int F, int h, int w, Refs refs,
    const int64_t *__restrict__ q, const ImageRec *__restrict__ rec, const double *__restrict__ unit,
    unsigned long long *__restrict__ acc)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    const size_t plane = (size_t)h * w;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const EventRow ev = cols.template load<POL>(e);
        const int64_t xi = ev.x, yi = ev.y;
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;
        int c;
        if (!event_channel<POL>(ev.sign, c)) continue;
        const float te = ev.t;
        const int64_t s = ev.sample;
        const size_t pix = (size_t)yi * w + (size_t)xi;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != s) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;
            const float tau = event_tau(te, t0, t1);
            const float *fl = flow + (size_t)f * 2 * plane + pix;
            const float u = fl[0], v = fl[plane];
            const double un = unit[f];
            // R = 1: |ms g| < 2^(e+1) (1 + 2^-22), so |a| < 2^41 (1 + 2^-22); R > 1: at most three addends
            // below 2^39 (1 + 2^-22) each; the product with the unit is exact
            long long su = 0, sv = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const size_t m = image_of<R, POL>(f, r, c);
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
__global__ __launch_bounds__(NT) void contrast_bwd_close_kernel(long long *__restrict__ acc,
                                                                const double *__restrict__ unit,
                                                                const float *__restrict__ seed, float weight, int F,
                                                                int M, size_t per_frame, float *__restrict__ grad)
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

size_t multi_workspace_bytes(int F, int reference_mask, int polarity, int h, int w);

// the workspace: the sums, M records, F units, the statistics' partials
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

size_t multi_workspace_bytes(int F, int reference_mask, int polarity, int h, int w)
{
    Plan pl;
    if (F < 1 || bad_frame_sizes(F, h, w) || !plan_of(F, reference_mask, polarity, pl)) return 0;
    return sums_bytes(F, h, w) + sizeof(ImageRec) * (size_t)pl.M + sizeof(double) * (size_t)F +
           dvsof_iwe_stats_workspace_bytes(pl.M, h, w);
}

// dvsof_contrast_multi_fwd / _bwd on either form of the event columns (event_columns.h)
template <class Cols>
int multi_fwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
              const float *flow, int F, int h, int w, int reference_mask, int polarity, int64_t *q, uint32_t *count,
              dvsof_iwe_result_t *result, float *term, void *workspace, size_t workspace_bytes, void *stream)
{
    Plan pl;
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !count || !result || !term || !frame_ts || !frame_sample || !flow)
        return DVSOF_EINVAL;
    if (n_events > 0 && !cols.given(polarity)) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < multi_workspace_bytes(F, reference_mask, polarity, h, w))
        return DVSOF_ENOSPACE;
    hipStream_t st = as_stream(stream);
    const size_t pixels = (size_t)pl.M * h * w;
    const Workspace ws = carve(workspace, F, h, w, pl);
    DVSOF_HIP_TRY((hipError_t)fill_u32(q, 0u, sizeof(int64_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(count, 0u, sizeof(uint32_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws.sums, 0u, sums_bytes(F, h, w), st));
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(contrast_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, flow, F, h, w, pl.refs, (unsigned long long *)q,
                                count);
        DVSOF_LAUNCH_CHECK();
    }
    const int rc = dvsof_iwe_stats(q, count, pl.M, h, w, result, ws.stats, ws.stats_bytes, stream);
    if (rc != DVSOF_OK) return rc;
    hipLaunchKernelGGL(contrast_close_kernel, dim3(1), dim3(kWave), 0, st, result, F, pl.R * pl.C, h, w,
                       pl.R > 1 ? kUnitBits - kSharedBits : kUnitBits, ws.rec, ws.unit, term);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

template <class Cols>
int multi_bwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
              const float *flow, int F, int h, int w, int reference_mask, int polarity, const int64_t *q,
              void *workspace, size_t workspace_bytes, const float *seed, float weight, float *grad_flow,
              void *stream)
{
    Plan pl;
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !seed || !grad_flow || !frame_ts || !frame_sample || !flow)
        return DVSOF_EINVAL;
    if (n_events > 0 && !cols.given(polarity)) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < multi_workspace_bytes(F, reference_mask, polarity, h, w))
        return DVSOF_ENOSPACE;
    hipStream_t st = as_stream(stream);
    const Workspace ws = carve(workspace, F, h, w, pl);
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(contrast_bwd_events_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, flow, F, h, w, pl.refs, q,
                                (const ImageRec *)ws.rec, (const double *)ws.unit, ws.sums);
        DVSOF_LAUNCH_CHECK();
    }
    const size_t per_frame = 2 * (size_t)h * w, total = (size_t)F * per_frame;
    hipLaunchKernelGGL(contrast_bwd_close_kernel, dim3(event_blocks((int64_t)total)), dim3(NT), 0, st,
                       (long long *)ws.sums, (const double *)ws.unit, seed, weight, F, pl.M, per_frame, grad_flow);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // namespace

extern "C" {

size_t dvsof_contrast_multi_workspace_bytes(int F, int reference_mask, int polarity, int h, int w)
{
    return multi_workspace_bytes(F, reference_mask, polarity, h, w);
}

int dvsof_contrast_multi_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                             const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                             const int64_t *frame_sample, const float *flow, int F, int h, int w,
                             int reference_mask, int polarity, int64_t *q, uint32_t *count,
                             dvsof_iwe_result_t *result, float *term, void *workspace, size_t workspace_bytes,
                             void *stream)
{
    return multi_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, flow, F, h, w,
                     reference_mask, polarity, q, count, result, term, workspace, workspace_bytes, stream);
}

int dvsof_contrast_multi_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                             const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                             const int64_t *frame_sample, const float *flow, int F, int h, int w,
                             int reference_mask, int polarity, const int64_t *q, void *workspace,
                             size_t workspace_bytes, const float *seed, float weight, float *grad_flow,
                             void *stream)
{
    return multi_bwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, flow, F, h, w,
                     reference_mask, polarity, q, workspace, workspace_bytes, seed, weight, grad_flow, stream);
}

// The encoded twins (include/dvsof_event_terms_encoded.h)
int dvsof_contrast_multi_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                     const int64_t *sample_event_offsets, int B, int64_t n_events,
                                     const float *frame_ts, const int64_t *frame_sample, const float *flow, int F,
                                     int h, int w, int reference_mask, int polarity_channels, int64_t *q,
                                     uint32_t *count, dvsof_iwe_result_t *result, float *term, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    return multi_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample,
                     flow, F, h, w, reference_mask, polarity_channels, q, count, result, term, workspace,
                     workspace_bytes, stream);
}

int dvsof_contrast_multi_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                     const int64_t *sample_event_offsets, int B, int64_t n_events,
                                     const float *frame_ts, const int64_t *frame_sample, const float *flow, int F,
                                     int h, int w, int reference_mask, int polarity_channels, const int64_t *q,
                                     void *workspace, size_t workspace_bytes, const float *seed, float weight,
                                     float *grad_flow, void *stream)
{
    return multi_bwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample,
                     flow, F, h, w, reference_mask, polarity_channels, q, workspace, workspace_bytes, seed, weight,
                     grad_flow, stream);
}

// The term as it was before the references and the polarities: one image per frame, of all its
// events carried to the start of the window.  The refusals are those of the general calls at
// these options, code for code and in the same order (F > 65535 is refused by the plan).
size_t dvsof_contrast_workspace_bytes(int F, int h, int w)
{
    return dvsof_contrast_multi_workspace_bytes(F, 1, 0, h, w);
}

int dvsof_contrast_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *sample_index,
                       int64_t n_events, const float *frame_ts, const int64_t *frame_sample, const float *flow,
                       int F, int h, int w, int64_t *q, uint32_t *count, dvsof_iwe_result_t *result, float *term,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    return dvsof_contrast_multi_fwd(x, y, t, nullptr, sample_index, n_events, frame_ts, frame_sample, flow, F, h, w,
                                    1, 0, q, count, result, term, workspace, workspace_bytes, stream);
}

int dvsof_contrast_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *sample_index,
                       int64_t n_events, const float *frame_ts, const int64_t *frame_sample, const float *flow,
                       int F, int h, int w, const int64_t *q, void *workspace, size_t workspace_bytes,
                       const float *seed, float weight, float *grad_flow, void *stream)
{
    return dvsof_contrast_multi_bwd(x, y, t, nullptr, sample_index, n_events, frame_ts, frame_sample, flow, F, h, w,
                                    1, 0, q, workspace, workspace_bytes, seed, weight, grad_flow, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// The term on every flow scale (docs/CONTRAST_SPEC.md sections 19-23).  The
// columns are read, the frames walked and tau computed once per event; the
// levels are a loop around splat_event / the backward's addends with the
// event's level pixel (y >> s, x >> s), the level's flow, plane and base.  Per
// level the bytes are those of the kernels above at the level's shape.
// ---------------------------------------------------------------------------
namespace {

using Levels = dvsof_contrast_levels_t;
using Level = dvsof_contrast_level_t;
constexpr int kMaxLevels = 8;
constexpr int kMaxShift = 15;
static_assert(sizeof(Levels::level) / sizeof(Level) == kMaxLevels, "the table holds eight levels");

template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void contrast_pyramid_splat_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, int F, int h, int w, Refs refs, const Levels lv,
    unsigned long long *__restrict__ q, uint32_t *__restrict__ count)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const EventRow ev = cols.template load<POL>(e);
        const int64_t xi = ev.x, yi = ev.y;
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;  // at full resolution, before any shift
        int c;
        if (!event_channel<POL>(ev.sign, c)) continue;
        const float te = ev.t;
        const int64_t s = ev.sample;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != s) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;
            const float tau = event_tau(te, t0, t1);
            for (int k = 0; k < lv.K; ++k) {
                const Level &L = lv.level[k];
                const int64_t xs = xi >> L.shift, ys = yi >> L.shift;  // xs <= (w - 1) >> s <= L.w - 1
                const size_t plane = (size_t)L.h * L.w;
                const size_t pix = (size_t)ys * L.w + (size_t)xs;
                const float *fl = L.flow + (size_t)f * 2 * plane + pix;
                const float u = fl[0], v = fl[plane];
                splat_event<R, POL, true>(refs, f, c, tau, u, v, xs, ys, pix, plane, L.h, L.w, q + L.image_offset,
                                          count + L.image_offset);
            }
        }
    }
}

// contrast_close_kernel over the K M images and K F units of all levels (image i = k M + m,
// unit j = k F + f), then in lane 0 every level's term in image order and the weighted sum in
// level order.
__global__ __launch_bounds__(kWave) void contrast_pyramid_close_kernel(const dvsof_iwe_result_t *__restrict__ result,
                                                                       int F, int RC, int unit_bits, const Levels lv,
                                                                       ImageRec *rec, double *unit, float *terms,
                                                                       float *value)
{
    const int M = F * RC, K = lv.K;
    for (int i = threadIdx.x; i < K * M; i += kWave) {
        const Level &L = lv.level[i / M];
        const double N = (double)L.h * (double)L.w;
        const dvsof_iwe_result_t r = result[i];
        const double mean = (double)r.sum_q * 0x1p-32 / N;
        const double var_i = r.sum_sq / N - mean * mean;
        const double cmean = (double)r.count_sum / N;
        const double var_c = (double)r.count_sq / N - cmean * cmean;
        ImageRec o;
        o.mean = mean;
        o.coef = var_c > 0.0 ? -2.0 / (N * var_c) : 0.0;
        o.term = var_c > 0.0 ? 1.0 - var_i / var_c : 0.0;
        o.gmax = fabs(o.coef) * fmax((double)r.max_q * 0x1p-32 - mean, mean);
        rec[i] = o;
        if (RC == 1) unit[i] = unit_of(o.gmax, unit_bits);
    }
    __syncthreads();
    if (RC > 1) {
        for (int j = threadIdx.x; j < K * F; j += kWave) {
            double gmax = 0.0;
            for (int k = 0; k < RC; ++k) gmax = fmax(gmax, rec[(size_t)j * RC + k].gmax);
            unit[j] = unit_of(gmax, unit_bits);
        }
    }
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < K; ++k) {
            double s = 0.0;
            for (int m = 0; m < M; ++m) s += rec[(size_t)k * M + m].term;
            const double term = s / (double)M;
            terms[k] = (float)term;
            total += (double)lv.level[k].weight * term;
        }
        *value = (float)total;
    }
}

template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void contrast_pyramid_bwd_events_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, int F, int h, int w, Refs refs, const Levels lv,
    const int64_t *__restrict__ q, const ImageRec *__restrict__ rec, const double *__restrict__ unit,
    unsigned long long *__restrict__ acc)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    const size_t M = (size_t)F * R * (POL ? 2 : 1);
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const EventRow ev = cols.template load<POL>(e);
        const int64_t xi = ev.x, yi = ev.y;
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;
        int c;
        if (!event_channel<POL>(ev.sign, c)) continue;
        const float te = ev.t;
        const int64_t s = ev.sample;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != s) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;
            const float tau = event_tau(te, t0, t1);
            for (int k = 0; k < lv.K; ++k) {
                const Level &L = lv.level[k];
                const int lh = L.h, lw = L.w;
                const int64_t xs = xi >> L.shift, ys = yi >> L.shift;
                const size_t plane = (size_t)lh * lw;
                const size_t pix = (size_t)ys * lw + (size_t)xs;
                const float *fl = L.flow + (size_t)f * 2 * plane + pix;
                const float u = fl[0], v = fl[plane];
                const double un = unit[(size_t)k * F + f];
                long long su = 0, sv = 0;  // the bounds of contrast_bwd_events_kernel, per level
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const size_t m = image_of<R, POL>(f, r, c);
                    const ImageRec a = rec[(size_t)k * M + m];
                    if (a.coef == 0.0) continue;
                    Warp p;
                    if (!warp_event_to(tau, refs.rho[r], u, v, xs, ys, lh, lw, p)) continue;
                    const int64_t *img = q + L.image_offset + m * plane;
                    double G[2][2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            const int xx = p.cx + i, yy = p.cy + j;
                            const bool in = xx >= 0 && xx < lw && yy >= 0 && yy < lh;
                            G[j][i] =
                                in ? a.coef * ((double)img[(size_t)yy * lw + (size_t)xx] * 0x1p-32 - a.mean) : 0.0;
                        }
                    }
                    const double gx = (double)p.wy[0] * (G[0][1] - G[0][0]) + (double)p.wy[1] * (G[1][1] - G[1][0]);
                    const double gy = (double)p.wx[0] * (G[1][0] - G[0][0]) + (double)p.wx[1] * (G[1][1] - G[0][1]);
                    const double ms = -(double)p.tau;
                    su += (long long)(ms * gx * un);
                    sv += (long long)(ms * gy * un);
                }
                unsigned long long *dst = acc + L.sums_offset + (size_t)f * 2 * plane + pix;
                if (su != 0) atomicAdd(dst, (unsigned long long)su);
                if (sv != 0) atomicAdd(dst + plane, (unsigned long long)sv);
            }
        }
    }
}

// One thread per element of every level's grad_flow: contrast_bwd_close_kernel with the
// level found from the element's place in the sums.
__global__ __launch_bounds__(NT) void contrast_pyramid_bwd_close_kernel(long long *__restrict__ acc,
                                                                        const double *__restrict__ unit,
                                                                        const float *__restrict__ seed, int F, int M,
                                                                        const Levels lv, size_t total)
{
    const size_t stride = (size_t)gridDim.x * NT;
    const float s0 = seed[0];
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += stride) {
        int k = 0;
        while (k + 1 < lv.K && i >= lv.level[k + 1].sums_offset) ++k;
        const Level &L = lv.level[k];
        const size_t local = i - L.sums_offset, per_frame = 2 * (size_t)L.h * L.w;
        const float sw = s0 * L.weight;
        const long long a = acc[i];
        acc[i] = 0;
        const double value = (double)a / unit[(size_t)k * F + local / per_frame] / (double)M;
        L.grad_flow[local] = sw * (float)value;
    }
}

// the workspace as byte offsets: q at 0, sums, count (one zeroed region), K M records, K F
// units, the statistics' partials
struct PyramidLayout {
    size_t sums, count, zeroed_bytes, rec, unit, stats, stats_bytes, bytes;
    size_t sums_elems;
};

// false: a table the calls refuse.  The offsets are looked at only where check_offsets is set
// (dvsof_contrast_pyramid_workspace_bytes reads the shapes alone).
bool pyramid_layout(int F, int h, int w, const Plan &pl, const Levels &lv, bool check_offsets, PyramidLayout &o)
{
    if (lv.K < 1 || lv.K > kMaxLevels || bad_frame_sizes(F, h, w)) return false;
    size_t pixels = 0;
    o.stats_bytes = 0;
    for (int k = 0; k < lv.K; ++k) {
        const Level &L = lv.level[k];
        if (bad_frame_sizes(F, L.h, L.w) || L.shift < 0 || L.shift > kMaxShift) return false;
        const int round = (1 << L.shift) - 1;
        if (L.h != (h + round) >> L.shift || L.w != (w + round) >> L.shift) return false;
        if (check_offsets && (L.image_offset != (size_t)pl.M * pixels || L.row_offset != (size_t)k * pl.M ||
                              L.sums_offset != 2 * (size_t)F * pixels))
            return false;
        pixels += (size_t)L.h * L.w;
        const size_t need = dvsof_iwe_stats_workspace_bytes(pl.M, L.h, L.w);
        o.stats_bytes = need > o.stats_bytes ? need : o.stats_bytes;
    }
    const size_t P = (size_t)pl.M * pixels;
    o.sums_elems = 2 * (size_t)F * pixels;
    o.sums = sizeof(int64_t) * P;
    o.count = o.sums + sizeof(int64_t) * o.sums_elems;
    o.zeroed_bytes = o.count + sizeof(uint32_t) * P;
    o.rec = (o.zeroed_bytes + 7) / 8 * 8;
    o.unit = o.rec + sizeof(ImageRec) * (size_t)lv.K * pl.M;
    o.stats = o.unit + sizeof(double) * (size_t)lv.K * F;
    o.bytes = o.stats + o.stats_bytes;
    return true;
}

struct PyramidWorkspace {
    unsigned long long *q, *sums;
    uint32_t *count;
    ImageRec *rec;
    double *unit;
    void *stats;
};

PyramidWorkspace carve_pyramid(void *workspace, const PyramidLayout &l)
{
    char *ws = (char *)workspace;
    PyramidWorkspace o;
    o.q = (unsigned long long *)ws;
    o.sums = (unsigned long long *)(ws + l.sums);
    o.count = (uint32_t *)(ws + l.count);
    o.rec = (ImageRec *)(ws + l.rec);
    o.unit = (double *)(ws + l.unit);
    o.stats = ws + l.stats;
    return o;
}

// The refusals both calls share, in the order of the header; outputs: the call's own pointers
// are all there.  DVSOF_OK with F == 0: nothing to do.
template <class Cols>
int pyramid_check(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F,
                  int h, int w, int reference_mask, int polarity, const Levels &lv, bool backward, bool outputs,
                  const void *workspace, size_t workspace_bytes, Plan &pl, PyramidLayout &lay)
{
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (lv.K < 1 || lv.K > kMaxLevels) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (!pyramid_layout(F, h, w, pl, lv, true, lay) || !outputs || !frame_ts || !frame_sample) return DVSOF_EINVAL;
    for (int k = 0; k < lv.K; ++k)
        if (!lv.level[k].flow || (backward && !lv.level[k].grad_flow)) return DVSOF_EINVAL;
    if (n_events > 0 && !cols.given(polarity)) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < lay.bytes) return DVSOF_ENOSPACE;
    return DVSOF_OK;
}

// dvsof_contrast_pyramid_fwd / _bwd on either form of the event columns
template <class Cols>
int pyramid_fwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F, int h,
                int w, int reference_mask, int polarity, const Levels &levels, dvsof_iwe_result_t *result,
                float *terms, float *value, void *workspace, size_t workspace_bytes, void *stream)
{
    Plan pl;
    PyramidLayout lay;
    const int rc = pyramid_check(cols, n_events, frame_ts, frame_sample, F, h, w, reference_mask, polarity, levels,
                                 false, result && terms && value, workspace, workspace_bytes, pl, lay);
    if (rc != DVSOF_OK || F == 0) return rc;
    hipStream_t st = as_stream(stream);
    const PyramidWorkspace ws = carve_pyramid(workspace, lay);
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws.q, 0u, lay.zeroed_bytes, st));
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(contrast_pyramid_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st,
                                cols, n_events, frame_ts, frame_sample, F, h, w, pl.refs, levels, ws.q, ws.count);
        DVSOF_LAUNCH_CHECK();
    }
    for (int k = 0; k < levels.K; ++k) {
        const Level &L = levels.level[k];
        const int rs = dvsof_iwe_stats((const int64_t *)ws.q + L.image_offset, ws.count + L.image_offset, pl.M, L.h,
                                       L.w, result + L.row_offset, ws.stats, lay.stats_bytes, stream);
        if (rs != DVSOF_OK) return rs;
    }
    hipLaunchKernelGGL(contrast_pyramid_close_kernel, dim3(1), dim3(kWave), 0, st, result, F, pl.R * pl.C,
                       pl.R > 1 ? kUnitBits - kSharedBits : kUnitBits, levels, ws.rec, ws.unit, terms, value);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

template <class Cols>
int pyramid_bwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F, int h,
                int w, int reference_mask, int polarity, const Levels &levels, void *workspace,
                size_t workspace_bytes, const float *seed, void *stream)
{
    Plan pl;
    PyramidLayout lay;
    const int rc = pyramid_check(cols, n_events, frame_ts, frame_sample, F, h, w, reference_mask, polarity, levels,
                                 true, seed != nullptr, workspace, workspace_bytes, pl, lay);
    if (rc != DVSOF_OK || F == 0) return rc;
    hipStream_t st = as_stream(stream);
    const PyramidWorkspace ws = carve_pyramid(workspace, lay);
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(contrast_pyramid_bwd_events_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st,
                                cols, n_events, frame_ts, frame_sample, F, h, w, pl.refs, levels,
                                (const int64_t *)ws.q, (const ImageRec *)ws.rec, (const double *)ws.unit, ws.sums);
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(contrast_pyramid_bwd_close_kernel, dim3(event_blocks((int64_t)lay.sums_elems)), dim3(NT), 0,
                       st, (long long *)ws.sums, (const double *)ws.unit, seed, F, pl.M, levels, lay.sums_elems);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // namespace

extern "C" {

size_t dvsof_contrast_pyramid_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                              dvsof_contrast_levels_t levels)
{
    Plan pl;
    PyramidLayout lay;
    if (F < 1 || !plan_of(F, reference_mask, polarity, pl) || !pyramid_layout(F, h, w, pl, levels, false, lay))
        return 0;
    return lay.bytes;
}

int dvsof_contrast_pyramid_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                               const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                               const int64_t *frame_sample, int F, int h, int w, int reference_mask, int polarity,
                               dvsof_contrast_levels_t levels, dvsof_iwe_result_t *result, float *terms,
                               float *value, void *workspace, size_t workspace_bytes, void *stream)
{
    return pyramid_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                       reference_mask, polarity, levels, result, terms, value, workspace, workspace_bytes, stream);
}

int dvsof_contrast_pyramid_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                               const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                               const int64_t *frame_sample, int F, int h, int w, int reference_mask, int polarity,
                               dvsof_contrast_levels_t levels, void *workspace, size_t workspace_bytes,
                               const float *seed, void *stream)
{
    return pyramid_bwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                       reference_mask, polarity, levels, workspace, workspace_bytes, seed, stream);
}

int dvsof_contrast_pyramid_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                       const int64_t *sample_event_offsets, int B, int64_t n_events,
                                       const float *frame_ts, const int64_t *frame_sample, int F, int h, int w,
                                       int reference_mask, int polarity_channels, dvsof_contrast_levels_t levels,
                                       dvsof_iwe_result_t *result, float *terms, float *value, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    return pyramid_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample,
                       F, h, w, reference_mask, polarity_channels, levels, result, terms, value, workspace,
                       workspace_bytes, stream);
}

int dvsof_contrast_pyramid_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                       const int64_t *sample_event_offsets, int B, int64_t n_events,
                                       const float *frame_ts, const int64_t *frame_sample, int F, int h, int w,
                                       int reference_mask, int polarity_channels, dvsof_contrast_levels_t levels,
                                       void *workspace, size_t workspace_bytes, const float *seed, void *stream)
{
    return pyramid_bwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample,
                       F, h, w, reference_mask, polarity_channels, levels, workspace, workspace_bytes, seed, stream);
}

}  // extern "C"
