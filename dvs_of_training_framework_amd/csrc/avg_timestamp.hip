// Average-timestamp term of a training from events alone and its gradient
// with respect to the flow (docs/AVG_TIMESTAMP_SPEC.md): beside its bilinear
// weight every warped event splats its distance in time from the reference,
// a = |tau - rho|; per pixel T = A / (I + eps) is the average distance of the
// events that landed there, and per image
// value_m = (sum T^2 / n) / (sum T0^2 / n0), T0 the same at zero flow
// (Zhu et al., CVPR 2019; Hagenaars et al., NeurIPS 2021, who normalise by the
// pixels that hold events).  A flow that brings the events of one edge together
// lowers it; piling unrelated events onto a pixel averages their distances and
// earns nothing, which is what the contrast term of contrast.hip rewards.
//
// Replaces nothing of the reference: its loss reads the grey frames only.
//
// The images, the events that take part in them and the warp are those of
// event_images.h and frame_common.h, so q and count are the bytes of
// dvsof_contrast_multi_fwd.  Forward: one fill of the whole zeroed region; one
// thread per event, which reads the flow at its pixel once per frame and issues
// per reference one 32-bit and up to nine 64-bit integer atomics; the
// fixed-order reduction of frame_common.h over the pixels of every image; one
// closing wave.  Backward: contrast.hip's shape, G(p) = 2 k T D (a - T) at the
// four corners, the R C images of a frame in one set of fixed-point sums with a
// power-of-two unit per frame, one integer atomic per component, one thread per
// element converts and clears.  No floating-point atomics, kernels only.  This
// file relies on -ffp-contract=off.
//
// At the end of the file: the term on every flow scale of the network by one
// fill, one splat, one closing wave and one backward for all levels (sections
// 11-15, include/dvsof_avg_timestamp_pyramid.h).  What one event does to the
// images of a frame, forward and backward, is stated once (avgts_splat_event
// of avg_timestamp_images.h, avgts_bwd_event) and used by the one-level
// kernels and by those.
#include "event_columns.h"
#include "avg_timestamp_images.h"
#include "../../include/dvsof_avg_timestamp.h"
#include "../../include/dvsof_avg_timestamp_pyramid.h"
#include "../../include/dvsof_event_terms_encoded.h"

namespace {

constexpr int NT = kFrameNT;
constexpr int kUnitBits = 40;    // R = 1: |one event's addend| < 2^(kUnitBits + 1) units
constexpr int kSharedBits = 2;   // R > 1: up to three addends of a pixel's event share a sum

// one per image, in the workspace behind the zeroed region
struct ImageRec {
    double S, S0;     // sum_p T^2, sum_p T0^2
    double n, n0;     // pixels with q > 0, with count > 0
    double peak;      // max_p 2 T D
    double value;     // (S / n) / (S0 / n0); 0 without events, 1 when they all left
    double k2;        // 2 n0 / (n S0); 0 where the image has no gradient
    double gmax;      // |G| <= gmax on every pixel, for every event
};
static_assert(sizeof(ImageRec) == 64, "the workspace holds 64 bytes per image");

// ---------------------------------------------------------------------------
// Forward.  What an event does to the images of its frame (avgts_splat_event)
// and the statistics of an image (StatRow, AvgSum, avgts_stats_partial_kernel)
// are those of avg_timestamp_images.h, which the validation metric of iwe.hip
// shares.  Here: the event loop and the frame rule of contrast_splat_kernel.
// ---------------------------------------------------------------------------
template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void avgts_splat_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, const float *__restrict__ flow, int F, int h, int w, Refs refs,
    unsigned long long *__restrict__ q, unsigned long long *__restrict__ s, unsigned long long *__restrict__ base,
    uint32_t *__restrict__ count)
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
        const int64_t smp = ev.sample;
        const size_t pix = (size_t)yi * w + (size_t)xi;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != smp) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;  // a test, not a clamp; false for a NaN
            const float tau = event_tau(te, t0, t1);
            const float *fl = flow + (size_t)f * 2 * plane + pix;
            const float u = fl[0], v = fl[plane];
            avgts_splat_event<R, POL>(refs, f, c, tau, u, v, xi, yi, pix, plane, h, w, q, s, base, count);
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

// the record of an image from its statistics row
__device__ __forceinline__ ImageRec record_of(const StatRow &r)
{
    ImageRec o;
    o.S = r.S;
    o.S0 = r.S0;
    o.n = (double)r.n;
    o.n0 = (double)r.n0;
    o.peak = r.peak;
    const bool live = r.S0 > 0.0, stayed = r.n > 0;
    o.value = !live ? 0.0 : (stayed ? (o.S / o.n) / (o.S0 / o.n0) : 1.0);
    o.k2 = live && stayed ? 2.0 * (o.n0 / (o.n * o.S0)) : 0.0;
    o.gmax = 0.5 * o.k2 * o.peak;
    return o;
}

// One wave: the record of every image (lane k takes images k, k + 64, ...);
// after a barrier the unit of every frame (lane k takes frames k, k + 64, ...;
// a maximum has no order) and, in lane 0, the images' values in image order.
__global__ __launch_bounds__(kWave) void avgts_close_kernel(const StatRow *__restrict__ rows, int F, int RC,
                                                            int unit_bits, ImageRec *rec, double *unit, float *term)
{
    const int M = F * RC;
    for (int m = threadIdx.x; m < M; m += kWave) rec[m] = record_of(rows[m]);
    __syncthreads();
    for (int f = threadIdx.x; f < F; f += kWave) {
        double gmax = 0.0;
        for (int k = 0; k < RC; ++k) gmax = fmax(gmax, rec[f * RC + k].gmax);
        unit[f] = unit_of(gmax, unit_bits);
    }
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int m = 0; m < M; ++m) sum += rec[m].value;
        *term = (float)(sum / (double)M);
    }
}

// ---------------------------------------------------------------------------
// Backward.  One thread per event and frame: for every reference
// G = 2 k T D (a - T) at the four corners of the image of its channel (0
// outside the image), the derivative of the bilinear weights, -sig of it to
// the event's own pixel of the flow, in float64, truncated to the frame's unit
// un.  The event of avgts_splat_event; q, s and rec start at the images of this
// shape.  The R addends are added to su, sv in registers (integers: no order).
// ---------------------------------------------------------------------------
template <int R, bool POL>
__device__ __forceinline__ void avgts_bwd_event(const Refs &refs, int f, int c, float tau, float u, float v,
                                                int64_t xi, int64_t yi, size_t plane, int h, int w,
                                                const int64_t *__restrict__ q, const int64_t *__restrict__ s,
                                                const ImageRec *__restrict__ rec, double un, long long &su,
                                                long long &sv)
{
    // |a - T| <= 1 and 2 k T D <= gmax < 2^e: the bounds of contrast_bwd_events_kernel
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t m = image_of<R, POL>(f, r, c);
        const double k2 = rec[m].k2;
        if (k2 == 0.0) continue;  // no events, or they all left: every addend would be 0
        Warp p;
        if (!warp_event_to(tau, refs.rho[r], u, v, xi, yi, h, w, p)) continue;
        const double a = (double)fabsf(p.tau);
        const int64_t *qm = q + m * plane, *sm = s + m * plane;
        double G[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int xx = p.cx + i, yy = p.cy + j;
                const bool in = xx >= 0 && xx < w && yy >= 0 && yy < h;
                double g = 0.0;
                if (in) {
                    const size_t at = (size_t)yy * w + (size_t)xx;
                    const double den = (double)qm[at] * 0x1p-32 + kEps;
                    const double T = (double)sm[at] * 0x1p-32 / den;
                    const double D = 1.0 / den;
                    g = k2 * T * D * (a - T);
                }
                G[j][i] = g;
            }
        }
        const double gx = (double)p.wy[0] * (G[0][1] - G[0][0]) + (double)p.wy[1] * (G[1][1] - G[1][0]);
        const double gy = (double)p.wx[0] * (G[1][0] - G[0][0]) + (double)p.wx[1] * (G[1][1] - G[0][1]);
        const double ms = -(double)p.tau;  // p.tau holds sig; d xw / d u = -sig
        su += (long long)(ms * gx * un);
        sv += (long long)(ms * gy * un);
    }
}

template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void avgts_bwd_events_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, const float *__restrict__ flow, int F, int h, int w, Refs refs,
    const int64_t *__restrict__ q, const int64_t *__restrict__ s, const ImageRec *__restrict__ rec,
    const double *__restrict__ unit, unsigned long long *__restrict__ acc)
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
        const int64_t smp = ev.sample;
        const size_t pix = (size_t)yi * w + (size_t)xi;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != smp) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;
            const float tau = event_tau(te, t0, t1);
            const float *fl = flow + (size_t)f * 2 * plane + pix;
            const float u = fl[0], v = fl[plane];
            long long su = 0, sv = 0;
            avgts_bwd_event<R, POL>(refs, f, c, tau, u, v, xi, yi, plane, h, w, q, s, rec, unit[f], su, sv);
            unsigned long long *dst = acc + (size_t)f * 2 * plane + pix;
            if (su != 0) atomicAdd(dst, (unsigned long long)su);
            if (sv != 0) atomicAdd(dst + plane, (unsigned long long)sv);
        }
    }
}

// One thread per element of grad_flow: convert, clear the sum for the next
// backward of the same forward, store.
__global__ __launch_bounds__(NT) void avgts_bwd_close_kernel(long long *__restrict__ acc,
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

// the workspace as byte offsets, in the order of the header
struct Layout {
    size_t s, base, sums, count, zeroed_bytes, rec, unit, rows, part, bytes;
    int nb;
};

Layout layout_of(int F, int h, int w, const Plan &pl)
{
    const size_t P = (size_t)pl.M * h * w, S = 2 * (size_t)F * h * w;
    Layout o;
    o.nb = partial_blocks(h, w);
    o.s = sizeof(int64_t) * P;
    o.base = o.s + sizeof(int64_t) * P;
    o.sums = o.base + sizeof(int64_t) * P;
    o.count = o.sums + sizeof(int64_t) * S;
    o.zeroed_bytes = o.count + sizeof(uint32_t) * P;
    o.rec = (o.zeroed_bytes + 7) / 8 * 8;
    o.unit = o.rec + sizeof(ImageRec) * (size_t)pl.M;
    o.rows = o.unit + sizeof(double) * (size_t)F;
    o.part = o.rows + sizeof(StatRow) * (size_t)pl.M;
    o.bytes = o.part + sizeof(StatRow) * (size_t)pl.M * o.nb;
    return o;
}

// The refusals both calls share, in the order of dvsof_contrast_multi_fwd; outputs: the call's
// own pointers are all there.  DVSOF_OK with F == 0: nothing to do.
template <class Cols>
int check_call(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
               const float *flow, int F, int h, int w, int reference_mask, int polarity, bool outputs,
               const void *workspace, size_t workspace_bytes, Plan &pl)
{
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !outputs || !frame_ts || !frame_sample || !flow) return DVSOF_EINVAL;
    if (n_events > 0 && !cols.given(polarity)) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < layout_of(F, h, w, pl).bytes) return DVSOF_ENOSPACE;
    return DVSOF_OK;
}

// dvsof_avg_timestamp_fwd / _bwd on either form of the event columns (event_columns.h)
template <class Cols>
int one_fwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
            const float *flow, int F, int h, int w, int reference_mask, int polarity, float *term, void *workspace,
            size_t workspace_bytes, void *stream)
{
    Plan pl;
    const int rc = check_call(cols, n_events, frame_ts, frame_sample, flow, F, h, w, reference_mask, polarity,
                              term != nullptr, workspace, workspace_bytes, pl);
    if (rc != DVSOF_OK || F == 0) return rc;
    hipStream_t st = as_stream(stream);
    const Layout lay = layout_of(F, h, w, pl);
    char *ws = (char *)workspace;
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws, 0u, lay.zeroed_bytes, st));
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(avgts_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, flow, F, h, w, pl.refs,
                                (unsigned long long *)ws, (unsigned long long *)(ws + lay.s),
                                (unsigned long long *)(ws + lay.base), (uint32_t *)(ws + lay.count));
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(avgts_stats_partial_kernel, dim3((unsigned)lay.nb, (unsigned)pl.M), dim3(NT), 0, st,
                       (const int64_t *)ws, (const int64_t *)(ws + lay.s), (const int64_t *)(ws + lay.base),
                       (const uint32_t *)(ws + lay.count), h, w, lay.nb, (StatRow *)(ws + lay.part));
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_final_kernel<AvgSum>, dim3((unsigned)pl.M), dim3(kWave), 0, st,
                       (const StatRow *)(ws + lay.part), lay.nb, (StatRow *)(ws + lay.rows));
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(avgts_close_kernel, dim3(1), dim3(kWave), 0, st, (const StatRow *)(ws + lay.rows), F,
                       pl.R * pl.C, pl.R > 1 ? kUnitBits - kSharedBits : kUnitBits, (ImageRec *)(ws + lay.rec),
                       (double *)(ws + lay.unit), term);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

template <class Cols>
int one_bwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
            const float *flow, int F, int h, int w, int reference_mask, int polarity, void *workspace,
            size_t workspace_bytes, const float *seed, float weight, float *grad_flow, void *stream)
{
    Plan pl;
    const int rc = check_call(cols, n_events, frame_ts, frame_sample, flow, F, h, w, reference_mask, polarity,
                              seed && grad_flow, workspace, workspace_bytes, pl);
    if (rc != DVSOF_OK || F == 0) return rc;
    hipStream_t st = as_stream(stream);
    const Layout lay = layout_of(F, h, w, pl);
    char *ws = (char *)workspace;
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(avgts_bwd_events_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, flow, F, h, w, pl.refs, (const int64_t *)ws,
                                (const int64_t *)(ws + lay.s), (const ImageRec *)(ws + lay.rec),
                                (const double *)(ws + lay.unit), (unsigned long long *)(ws + lay.sums));
        DVSOF_LAUNCH_CHECK();
    }
    const size_t per_frame = 2 * (size_t)h * w, total = (size_t)F * per_frame;
    hipLaunchKernelGGL(avgts_bwd_close_kernel, dim3(event_blocks((int64_t)total)), dim3(NT), 0, st,
                       (long long *)(ws + lay.sums), (const double *)(ws + lay.unit), seed, weight, F, pl.M,
                       per_frame, grad_flow);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // namespace

extern "C" {

size_t dvsof_avg_timestamp_workspace_bytes(int F, int reference_mask, int polarity, int h, int w)
{
    Plan pl;
    if (F < 1 || bad_frame_sizes(F, h, w) || !plan_of(F, reference_mask, polarity, pl)) return 0;
    return layout_of(F, h, w, pl).bytes;
}

int dvsof_avg_timestamp_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                            const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                            const int64_t *frame_sample, const float *flow, int F, int h, int w,
                            int reference_mask, int polarity, float *term, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    return one_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, flow, F, h, w,
                   reference_mask, polarity, term, workspace, workspace_bytes, stream);
}

int dvsof_avg_timestamp_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                            const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                            const int64_t *frame_sample, const float *flow, int F, int h, int w,
                            int reference_mask, int polarity, void *workspace, size_t workspace_bytes,
                            const float *seed, float weight, float *grad_flow, void *stream)
{
    return one_bwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, flow, F, h, w,
                   reference_mask, polarity, workspace, workspace_bytes, seed, weight, grad_flow, stream);
}

// The encoded twins (include/dvsof_event_terms_encoded.h)
int dvsof_avg_timestamp_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                    const int64_t *sample_event_offsets, int B, int64_t n_events,
                                    const float *frame_ts, const int64_t *frame_sample, const float *flow, int F,
                                    int h, int w, int reference_mask, int polarity_channels, float *term,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    return one_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample,
                   flow, F, h, w, reference_mask, polarity_channels, term, workspace, workspace_bytes, stream);
}

int dvsof_avg_timestamp_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                    const int64_t *sample_event_offsets, int B, int64_t n_events,
                                    const float *frame_ts, const int64_t *frame_sample, const float *flow, int F,
                                    int h, int w, int reference_mask, int polarity_channels, void *workspace,
                                    size_t workspace_bytes, const float *seed, float weight, float *grad_flow,
                                    void *stream)
{
    return one_bwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample,
                   flow, F, h, w, reference_mask, polarity_channels, workspace, workspace_bytes, seed, weight,
                   grad_flow, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// The term on every flow scale (docs/AVG_TIMESTAMP_SPEC.md sections 11-15).
// The columns are read, the frames walked and tau computed once per event; the
// levels are a runtime loop around avgts_splat_event / avgts_bwd_event with the
// event's level pixel (y >> s, x >> s), the level's flow, plane and images.
// Per level the bytes are those of the kernels above at the level's shape.
// ---------------------------------------------------------------------------
namespace {

using Levels = dvsof_contrast_levels_t;
using Level = dvsof_contrast_level_t;
constexpr int kMaxLevels = 8;
constexpr int kMaxShift = 15;
static_assert(sizeof(Levels::level) / sizeof(Level) == kMaxLevels, "the table holds eight levels");

template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void avgts_pyramid_splat_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, int F, int h, int w, Refs refs, const Levels lv,
    unsigned long long *__restrict__ q, unsigned long long *__restrict__ s, unsigned long long *__restrict__ base,
    uint32_t *__restrict__ count)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        const EventRow ev = cols.template load<POL>(e);
        const int64_t xi = ev.x, yi = ev.y;
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;  // at full resolution, before any shift
        int c;
        if (!event_channel<POL>(ev.sign, c)) continue;
        const float te = ev.t;
        const int64_t smp = ev.sample;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != smp) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;
            const float tau = event_tau(te, t0, t1);
#pragma unroll 1
            for (int k = 0; k < lv.K; ++k) {
                const Level &L = lv.level[k];
                const int64_t xs = xi >> L.shift, ys = yi >> L.shift;  // xs <= (w - 1) >> s <= L.w - 1
                const size_t plane = (size_t)L.h * L.w;
                const size_t pix = (size_t)ys * L.w + (size_t)xs;
                const float *fl = L.flow + (size_t)f * 2 * plane + pix;
                const float u = fl[0], v = fl[plane];
                avgts_splat_event<R, POL>(refs, f, c, tau, u, v, xs, ys, pix, plane, L.h, L.w, q + L.image_offset,
                                          s + L.image_offset, base + L.image_offset, count + L.image_offset);
            }
        }
    }
}

// avgts_close_kernel over the K M images and K F units of all levels (image i = k M + m, unit
// j = k F + f, whose images are i = j RC ...), then in lane 0 every level's term in image order
// and the weighted sum in level order.
__global__ __launch_bounds__(kWave) void avgts_pyramid_close_kernel(const StatRow *__restrict__ rows, int F, int RC,
                                                                    int unit_bits, const Levels lv, ImageRec *rec,
                                                                    double *unit, float *terms, float *value)
{
    const int M = F * RC, K = lv.K;
    for (int i = threadIdx.x; i < K * M; i += kWave) rec[i] = record_of(rows[i]);
    __syncthreads();
    for (int j = threadIdx.x; j < K * F; j += kWave) {
        double gmax = 0.0;
        for (int k = 0; k < RC; ++k) gmax = fmax(gmax, rec[(size_t)j * RC + k].gmax);
        unit[j] = unit_of(gmax, unit_bits);
    }
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < K; ++k) {
            double sum = 0.0;
            for (int m = 0; m < M; ++m) sum += rec[(size_t)k * M + m].value;
            const double term = sum / (double)M;
            terms[k] = (float)term;
            total += (double)lv.level[k].weight * term;
        }
        *value = (float)total;
    }
}

template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void avgts_pyramid_bwd_events_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, int F, int h, int w, Refs refs, const Levels lv,
    const int64_t *__restrict__ q, const int64_t *__restrict__ s, const ImageRec *__restrict__ rec,
    const double *__restrict__ unit, unsigned long long *__restrict__ acc)
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
        const int64_t smp = ev.sample;
        for (int f = 0; f < F; ++f) {
            if (frame_sample[f] != smp) continue;
            const float t0 = ts[2 * f], t1 = ts[2 * f + 1];
            if (!(t0 <= te && te <= t1)) continue;
            const float tau = event_tau(te, t0, t1);
#pragma unroll 1
            for (int k = 0; k < lv.K; ++k) {
                const Level &L = lv.level[k];
                const int64_t xs = xi >> L.shift, ys = yi >> L.shift;
                const size_t plane = (size_t)L.h * L.w;
                const size_t pix = (size_t)ys * L.w + (size_t)xs;
                const float *fl = L.flow + (size_t)f * 2 * plane + pix;
                const float u = fl[0], v = fl[plane];
                long long su = 0, sv = 0;
                avgts_bwd_event<R, POL>(refs, f, c, tau, u, v, xs, ys, plane, L.h, L.w, q + L.image_offset,
                                        s + L.image_offset, rec + (size_t)k * M, unit[(size_t)k * F + f], su, sv);
                unsigned long long *dst = acc + L.sums_offset + (size_t)f * 2 * plane + pix;
                if (su != 0) atomicAdd(dst, (unsigned long long)su);
                if (sv != 0) atomicAdd(dst + plane, (unsigned long long)sv);
            }
        }
    }
}

// One thread per element of every level's grad_flow: avgts_bwd_close_kernel with the level
// found from the element's place in the sums.
__global__ __launch_bounds__(NT) void avgts_pyramid_bwd_close_kernel(long long *__restrict__ acc,
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

// the workspace as byte offsets, in the order of the header
struct PyramidLayout {
    size_t s, base, sums, count, zeroed_bytes, rec, unit, rows, part, bytes;
    size_t sums_elems;
};

// false: a table the calls refuse.  The offsets are looked at only where check_offsets is set
// (dvsof_avg_timestamp_pyramid_workspace_bytes reads the shapes alone).
bool pyramid_layout(int F, int h, int w, const Plan &pl, const Levels &lv, bool check_offsets, PyramidLayout &o)
{
    if (lv.K < 1 || lv.K > kMaxLevels || bad_frame_sizes(F, h, w)) return false;
    size_t pixels = 0;
    int nb = 0;
    for (int k = 0; k < lv.K; ++k) {
        const Level &L = lv.level[k];
        if (bad_frame_sizes(F, L.h, L.w) || L.shift < 0 || L.shift > kMaxShift) return false;
        const int round = (1 << L.shift) - 1;
        if (L.h != (h + round) >> L.shift || L.w != (w + round) >> L.shift) return false;
        if (check_offsets && (L.image_offset != (size_t)pl.M * pixels || L.row_offset != (size_t)k * pl.M ||
                              L.sums_offset != 2 * (size_t)F * pixels))
            return false;
        pixels += (size_t)L.h * L.w;
        const int need = partial_blocks(L.h, L.w);
        nb = need > nb ? need : nb;
    }
    const size_t P = (size_t)pl.M * pixels, KM = (size_t)lv.K * pl.M;
    o.sums_elems = 2 * (size_t)F * pixels;
    o.s = sizeof(int64_t) * P;
    o.base = o.s + sizeof(int64_t) * P;
    o.sums = o.base + sizeof(int64_t) * P;
    o.count = o.sums + sizeof(int64_t) * o.sums_elems;
    o.zeroed_bytes = o.count + sizeof(uint32_t) * P;
    o.rec = (o.zeroed_bytes + 7) / 8 * 8;
    o.unit = o.rec + sizeof(ImageRec) * KM;
    o.rows = o.unit + sizeof(double) * (size_t)lv.K * F;
    o.part = o.rows + sizeof(StatRow) * KM;
    o.bytes = o.part + sizeof(StatRow) * (size_t)pl.M * nb;
    return true;
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

// dvsof_avg_timestamp_pyramid_fwd / _bwd on either form of the event columns
template <class Cols>
int pyramid_fwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F, int h,
                int w, int reference_mask, int polarity, const Levels &levels, float *terms, float *value,
                void *workspace, size_t workspace_bytes, void *stream)
{
    Plan pl;
    PyramidLayout lay;
    const int rc = pyramid_check(cols, n_events, frame_ts, frame_sample, F, h, w, reference_mask, polarity, levels,
                                 false, terms && value, workspace, workspace_bytes, pl, lay);
    if (rc != DVSOF_OK || F == 0) return rc;
    hipStream_t st = as_stream(stream);
    char *ws = (char *)workspace;
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws, 0u, lay.zeroed_bytes, st));
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(avgts_pyramid_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, F, h, w, pl.refs, levels,
                                (unsigned long long *)ws, (unsigned long long *)(ws + lay.s),
                                (unsigned long long *)(ws + lay.base), (uint32_t *)(ws + lay.count));
        DVSOF_LAUNCH_CHECK();
    }
    // per level the two launches of the one-level call with its own nb: that order makes the bytes
    for (int k = 0; k < levels.K; ++k) {
        const Level &L = levels.level[k];
        const int nb = partial_blocks(L.h, L.w);
        hipLaunchKernelGGL(avgts_stats_partial_kernel, dim3((unsigned)nb, (unsigned)pl.M), dim3(NT), 0, st,
                           (const int64_t *)ws + L.image_offset, (const int64_t *)(ws + lay.s) + L.image_offset,
                           (const int64_t *)(ws + lay.base) + L.image_offset,
                           (const uint32_t *)(ws + lay.count) + L.image_offset, L.h, L.w, nb,
                           (StatRow *)(ws + lay.part));
        DVSOF_LAUNCH_CHECK();
        hipLaunchKernelGGL(frame_final_kernel<AvgSum>, dim3((unsigned)pl.M), dim3(kWave), 0, st,
                           (const StatRow *)(ws + lay.part), nb, (StatRow *)(ws + lay.rows) + L.row_offset);
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(avgts_pyramid_close_kernel, dim3(1), dim3(kWave), 0, st, (const StatRow *)(ws + lay.rows), F,
                       pl.R * pl.C, pl.R > 1 ? kUnitBits - kSharedBits : kUnitBits, levels,
                       (ImageRec *)(ws + lay.rec), (double *)(ws + lay.unit), terms, value);
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
    char *ws = (char *)workspace;
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(avgts_pyramid_bwd_events_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st,
                                cols, n_events, frame_ts, frame_sample, F, h, w, pl.refs, levels,
                                (const int64_t *)ws, (const int64_t *)(ws + lay.s),
                                (const ImageRec *)(ws + lay.rec), (const double *)(ws + lay.unit),
                                (unsigned long long *)(ws + lay.sums));
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(avgts_pyramid_bwd_close_kernel, dim3(event_blocks((int64_t)lay.sums_elems)), dim3(NT), 0, st,
                       (long long *)(ws + lay.sums), (const double *)(ws + lay.unit), seed, F, pl.M, levels,
                       lay.sums_elems);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // namespace

extern "C" {

size_t dvsof_avg_timestamp_pyramid_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                   dvsof_contrast_levels_t levels)
{
    Plan pl;
    PyramidLayout lay;
    if (F < 1 || !plan_of(F, reference_mask, polarity, pl) || !pyramid_layout(F, h, w, pl, levels, false, lay))
        return 0;
    return lay.bytes;
}

int dvsof_avg_timestamp_pyramid_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                    const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                    const int64_t *frame_sample, int F, int h, int w, int reference_mask,
                                    int polarity, dvsof_contrast_levels_t levels, float *terms, float *value,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    return pyramid_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                       reference_mask, polarity, levels, terms, value, workspace, workspace_bytes, stream);
}

int dvsof_avg_timestamp_pyramid_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                    const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                    const int64_t *frame_sample, int F, int h, int w, int reference_mask,
                                    int polarity, dvsof_contrast_levels_t levels, void *workspace,
                                    size_t workspace_bytes, const float *seed, void *stream)
{
    return pyramid_bwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                       reference_mask, polarity, levels, workspace, workspace_bytes, seed, stream);
}

int dvsof_avg_timestamp_pyramid_fwd_encoded(const int16_t *x, const int16_t *y, const float *t,
                                            const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                            int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                            int F, int h, int w, int reference_mask, int polarity_channels,
                                            dvsof_contrast_levels_t levels, float *terms, float *value,
                                            void *workspace, size_t workspace_bytes, void *stream)
{
    return pyramid_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample,
                       F, h, w, reference_mask, polarity_channels, levels, terms, value, workspace, workspace_bytes,
                       stream);
}

int dvsof_avg_timestamp_pyramid_bwd_encoded(const int16_t *x, const int16_t *y, const float *t,
                                            const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                            int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                            int F, int h, int w, int reference_mask, int polarity_channels,
                                            dvsof_contrast_levels_t levels, void *workspace, size_t workspace_bytes,
                                            const float *seed, void *stream)
{
    return pyramid_bwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample,
                       F, h, w, reference_mask, polarity_channels, levels, workspace, workspace_bytes, seed, stream);
}

}  // extern "C"
