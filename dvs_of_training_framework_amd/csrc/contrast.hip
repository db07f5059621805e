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
// The term on every flow scale of the network (sections 19-23,
// include/dvsof_contrast_pyramid.h) is the same three kernels over a level
// table: every kernel is written once against a view of the call's levels
// (event_term_levels.h) and instantiated for one flow and for a table, with
// one splat, one closing wave and one backward for all levels.  Then the host
// side of the calls on one flow, that of the calls over a table, and the
// gradient-magnitude objective on the same images (sections 27-31,
// include/dvsof_contrast_gradient.h), a stencil over q through LDS.
#include "event_term_levels.h"
#include "event_term_records.h"
#include "tiled_splat.h"
#include "../../include/dvsof_contrast.h"
#include "../../include/dvsof_contrast_multi.h"
#include "../../include/dvsof_contrast_pyramid.h"
#include "../../include/dvsof_event_terms_encoded.h"
#include "../../include/dvsof_event_images_tiled.h"
#include "../../include/dvsof_event_pyramids_tiled.h"
#include "../../include/dvsof_contrast_gradient.h"

namespace {

constexpr int NT = kFrameNT;
// the unit bits, unit_of and the record of an image: event_term_records.h
using ImageRec = ContrastRec;

// ---------------------------------------------------------------------------
// Forward.  One thread per event; an event takes part in every frame of its
// sample whose window holds its time (both ends included), in the channel of
// the sign of p.  The columns are read, the frames walked and tau computed once
// per event; the levels are a loop around splat_event with the event's level
// pixel (y >> s, x >> s), the level's flow, plane and base.
// ---------------------------------------------------------------------------
template <int R, bool POL, class Cols, class View>
__global__ __launch_bounds__(NT) void contrast_splat_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, int F, int h, int w, Refs refs, const View view,
    unsigned long long *__restrict__ q, uint32_t *__restrict__ count)
{
    const auto splat = [=, &view](int64_t xi, int64_t yi, int c, int f, float tau) {
        for (int k = 0; k < view.levels(); ++k) {
            const Level &L = view.at(k);
            const int64_t xs = xi >> L.shift, ys = yi >> L.shift;  // xs <= (w - 1) >> s <= L.w - 1
            const size_t plane = (size_t)L.h * L.w;
            const size_t pix = (size_t)ys * L.w + (size_t)xs;
            float u, v;
            flow_at(L.flow, f, plane, pix, u, v);
            splat_event<R, POL, true>(refs, f, c, tau, u, v, xs, ys, pix, plane, L.h, L.w, q + L.image_offset,
                                      count + L.image_offset);
        }
    };
    for_each_window_event<POL>(cols, n, ts, frame_sample, F, h, w, splat);
}

// One wave over the K M images and K F units of all levels (image i = k M + m, unit j = k F + f):
// the record of every image (lane k takes images k, k + 64, ...); after a barrier the unit of
// every frame (lane k takes frames k, k + 64, ...; a maximum has no order; a frame of one image
// has its unit from the gmax its lane holds) and, in lane 0, every level's term in image order.
// Over a table also the weighted sum in level order; on one flow terms is the call's term and
// value is not written.
template <class View>
__global__ __launch_bounds__(kWave) void contrast_close_kernel(const dvsof_iwe_result_t *__restrict__ result, int F,
                                                               int RC, int unit_bits, const View view, ImageRec *rec,
                                                               double *unit, float *terms, float *value)
{
    const int M = F * RC, K = view.levels();
    for (int i = threadIdx.x; i < K * M; i += kWave) {
        const Level &L = view.at(K == 1 ? 0 : i / M);
        const double N = (double)L.h * (double)L.w;
        const ImageRec o = contrast_record_of(result[i], N);
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
            if (View::kTable) total += (double)view.at(k).weight * term;
        }
        if (View::kTable) *value = (float)total;
    }
}

// ---------------------------------------------------------------------------
// Backward.  One thread per event and frame: for every reference G = coef (I -
// mean) at the four corners of the image of its channel (0 outside the image),
// the derivative of the bilinear weights, -sig of it to the event's own pixel
// of the flow, in float64, truncated to the frame's unit (corner_addends of
// event_term_levels.h, per level as in the splat); then one thread per element
// converts (event_term_bwd_close_kernel, likewise).
// ---------------------------------------------------------------------------
// The one kernel of the terms that writes the walk of for_each_window_event out: through the walk
// its <3, true> instances over a table take 74-76 VGPRs for 70, seven waves a SIMD down to six.
template <int R, bool POL, class Cols, class View>
__global__ __launch_bounds__(NT) void contrast_bwd_events_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, int F, int h, int w, Refs refs, const View view,
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
            for (int k = 0; k < view.levels(); ++k) {
                const Level &L = view.at(k);
                const int lh = L.h, lw = L.w;
                const int64_t xs = xi >> L.shift, ys = yi >> L.shift;
                const size_t plane = (size_t)lh * lw;
                const size_t pix = (size_t)ys * lw + (size_t)xs;
                float u, v;
                flow_at(L.flow, f, plane, pix, u, v);
                const double un = unit[(size_t)k * F + f];
                // R = 1: |ms g| < 2^(e+1) (1 + 2^-22), so |a| < 2^41 (1 + 2^-22); R > 1: at most three
                // addends below 2^39 (1 + 2^-22) each; the product with the unit is exact
                long long su = 0, sv = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const size_t m = image_of<R, POL>(f, r, c);
                    const ImageRec a = rec[(size_t)k * M + m];
                    if (a.coef == 0.0) continue;  // var(c_m) = 0: every addend would be 0
                    Warp p;
                    if (!warp_event_to(tau, refs.rho[r], u, v, xs, ys, lh, lw, p)) continue;
                    const int64_t *img = q + L.image_offset + m * plane;
                    // corner_addends written out: through it the <3, true, WireColumns> table instance
                    // took 224.9 us for 219.3 (spread 3.2) at the same 70 VGPRs
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
              dvsof_iwe_result_t *result, float *term, void *workspace, size_t workspace_bytes, void *stream,
              const TiledSplat tiled = TiledSplat{nullptr, 0, -1})
{
    Plan pl;
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !count || !result || !term || !frame_ts || !frame_sample || !flow)
        return DVSOF_EINVAL;
    if (n_events > 0 && !cols.given(polarity)) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < multi_workspace_bytes(F, reference_mask, polarity, h, w))
        return DVSOF_ENOSPACE;
    TilePlan tp;
    const int by_tiles = tile_decide<EventImages>(tiled, F, reference_mask, polarity, h, w, n_events, tp);
    if (by_tiles != DVSOF_OK && by_tiles != 1) return by_tiles;
    hipStream_t st = as_stream(stream);
    const size_t pixels = (size_t)pl.M * h * w;
    const Workspace ws = carve(workspace, F, h, w, pl);
    const OneLevel view{h, w, flow, 0.f, nullptr};
    DVSOF_HIP_TRY((hipError_t)fill_u32(q, 0u, sizeof(int64_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(count, 0u, sizeof(uint32_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws.sums, 0u, sums_bytes(F, h, w), st));
    if (by_tiles == DVSOF_OK) {
        const int rs = TiledLaunch<EventImages>::term(plain(cols), n_events, frame_ts, frame_sample, flow, F, h, w,
                                                      reference_mask, polarity, tp, EventImages{q, count},
                                                      tiled.workspace, st);
        if (rs != DVSOF_OK) return rs;
    } else if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(contrast_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, F, h, w, pl.refs, view, (unsigned long long *)q,
                                count);
        DVSOF_LAUNCH_CHECK();
    }
    const int rc = dvsof_iwe_stats(q, count, pl.M, h, w, result, ws.stats, ws.stats_bytes, stream);
    if (rc != DVSOF_OK) return rc;
    hipLaunchKernelGGL(contrast_close_kernel<OneLevel>, dim3(1), dim3(kWave), 0, st, result, F, pl.R * pl.C,
                       pl.R > 1 ? kUnitBits - kSharedBits : kUnitBits, view, ws.rec, ws.unit, term, (float *)nullptr);
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
    const OneLevel view{h, w, flow, weight, grad_flow};
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(contrast_bwd_events_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, F, h, w, pl.refs, view, q,
                                (const ImageRec *)ws.rec, (const double *)ws.unit, ws.sums);
        DVSOF_LAUNCH_CHECK();
    }
    const size_t total = 2 * (size_t)F * h * w;
    hipLaunchKernelGGL(event_term_bwd_close_kernel<OneLevel>, dim3(event_blocks((int64_t)total)), dim3(NT), 0, st,
                       (long long *)ws.sums, (const double *)ws.unit, seed, F, pl.M, view, total);
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

// The tiled twins (include/dvsof_event_images_tiled.h): the forward above with the splat by tiles
int dvsof_contrast_multi_fwd_tiled(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                   const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                   const int64_t *frame_sample, const float *flow, int F, int h, int w,
                                   int reference_mask, int polarity, int64_t *q, uint32_t *count,
                                   dvsof_iwe_result_t *result, float *term, void *workspace, size_t workspace_bytes,
                                   void *stream, void *tile_workspace, size_t tile_workspace_bytes, int mode)
{
    if (mode != 0 && mode != 1) return DVSOF_EINVAL;
    return multi_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, flow, F, h, w,
                     reference_mask, polarity, q, count, result, term, workspace, workspace_bytes, stream,
                     TiledSplat{tile_workspace, tile_workspace_bytes, mode});
}

int dvsof_contrast_multi_fwd_encoded_tiled(const int16_t *x, const int16_t *y, const float *t,
                                           const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                           int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                           const float *flow, int F, int h, int w, int reference_mask,
                                           int polarity_channels, int64_t *q, uint32_t *count,
                                           dvsof_iwe_result_t *result, float *term, void *workspace,
                                           size_t workspace_bytes, void *stream, void *tile_workspace,
                                           size_t tile_workspace_bytes, int mode)
{
    if (mode != 0 && mode != 1) return DVSOF_EINVAL;
    return multi_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample,
                     flow, F, h, w, reference_mask, polarity_channels, q, count, result, term, workspace,
                     workspace_bytes, stream, TiledSplat{tile_workspace, tile_workspace_bytes, mode});
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
// kernels are those above over the table's view; the workspace holds q and
// count of all levels, so the bytes of a level are those of the calls on one
// flow at the level's shape.
// ---------------------------------------------------------------------------
namespace {

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
    const size_t pixels = level_table_pixels(F, h, w, lv, check_offsets ? pl.M : 0);
    if (pixels == 0) return false;
    o.stats_bytes = 0;
    for (int k = 0; k < lv.K; ++k) {
        const size_t need = dvsof_iwe_stats_workspace_bytes(pl.M, lv.level[k].h, lv.level[k].w);
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
                float *terms, float *value, void *workspace, size_t workspace_bytes, void *stream,
                const TiledSplat tiled = TiledSplat{nullptr, 0, -1})
{
    Plan pl;
    PyramidLayout lay;
    const int rc = pyramid_check(cols, n_events, frame_ts, frame_sample, F, h, w, reference_mask, polarity, levels,
                                 false, result && terms && value, workspace, workspace_bytes, pl, lay);
    if (rc != DVSOF_OK || F == 0) return rc;
    PyramidTilePlan tp;
    const int by_tiles =
        pyramid_tile_decide<EventImages>(tiled, F, reference_mask, polarity, h, w, levels, n_events, tp);
    if (by_tiles != DVSOF_OK && by_tiles != 1) return by_tiles;
    hipStream_t st = as_stream(stream);
    const PyramidWorkspace ws = carve_pyramid(workspace, lay);
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws.q, 0u, lay.zeroed_bytes, st));
    if (by_tiles == DVSOF_OK) {
        const int rs = TiledLaunch<EventImages>::pyramid(plain(cols), n_events, frame_ts, frame_sample, F, h, w,
                                                         reference_mask, polarity, levels, tp,
                                                         EventImages{(int64_t *)ws.q, ws.count}, tiled.workspace, st);
        if (rs != DVSOF_OK) return rs;
    } else if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(contrast_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, F, h, w, pl.refs, TableView{levels}, ws.q, ws.count);
        DVSOF_LAUNCH_CHECK();
    }
    for (int k = 0; k < levels.K; ++k) {
        const Level &L = levels.level[k];
        const int rs = dvsof_iwe_stats((const int64_t *)ws.q + L.image_offset, ws.count + L.image_offset, pl.M, L.h,
                                       L.w, result + L.row_offset, ws.stats, lay.stats_bytes, stream);
        if (rs != DVSOF_OK) return rs;
    }
    hipLaunchKernelGGL(contrast_close_kernel<TableView>, dim3(1), dim3(kWave), 0, st, result, F, pl.R * pl.C,
                       pl.R > 1 ? kUnitBits - kSharedBits : kUnitBits, TableView{levels}, ws.rec, ws.unit, terms,
                       value);
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
        DVSOF_REFS_POL_DISPATCH(contrast_bwd_events_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, F, h, w, pl.refs, TableView{levels},
                                (const int64_t *)ws.q, (const ImageRec *)ws.rec, (const double *)ws.unit, ws.sums);
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(event_term_bwd_close_kernel<TableView>, dim3(event_blocks((int64_t)lay.sums_elems)), dim3(NT),
                       0, st, (long long *)ws.sums, (const double *)ws.unit, seed, F, pl.M, TableView{levels},
                       lay.sums_elems);
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

// The tiled twins (include/dvsof_event_pyramids_tiled.h): the forward above with the splat by tiles
int dvsof_contrast_pyramid_fwd_tiled(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                     const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                     const int64_t *frame_sample, int F, int h, int w, int reference_mask,
                                     int polarity, dvsof_contrast_levels_t levels, dvsof_iwe_result_t *result,
                                     float *terms, float *value, void *workspace, size_t workspace_bytes,
                                     void *stream, void *tile_workspace, size_t tile_workspace_bytes, int mode)
{
    if (mode != 0 && mode != 1) return DVSOF_EINVAL;
    return pyramid_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                       reference_mask, polarity, levels, result, terms, value, workspace, workspace_bytes, stream,
                       TiledSplat{tile_workspace, tile_workspace_bytes, mode});
}

int dvsof_contrast_pyramid_fwd_encoded_tiled(const int16_t *x, const int16_t *y, const float *t,
                                             const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                             int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                             int F, int h, int w, int reference_mask, int polarity_channels,
                                             dvsof_contrast_levels_t levels, dvsof_iwe_result_t *result,
                                             float *terms, float *value, void *workspace, size_t workspace_bytes,
                                             void *stream, void *tile_workspace, size_t tile_workspace_bytes,
                                             int mode)
{
    if (mode != 0 && mode != 1) return DVSOF_EINVAL;
    return pyramid_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample,
                       F, h, w, reference_mask, polarity_channels, levels, result, terms, value, workspace,
                       workspace_bytes, stream, TiledSplat{tile_workspace, tile_workspace_bytes, mode});
}

}  // extern "C"

// ---------------------------------------------------------------------------
// The gradient-magnitude objective (docs/CONTRAST_SPEC.md sections 27-31;
// Gallego et al., CVPR 2019): term_m = 1 - GM(I_m)/GM(c_m), GM the sum of the
// squared differences of every adjacent pair of pixels.  The images, the splat
// and the backward's closing kernel are those above.  New here: the statistics,
// a 5-point stencil over q and count by tiles through LDS, which also stores
// the integer Laplacian of q, the adjoint of the differences; one closing wave;
// the backward over events, which gathers that plane where the variance's
// gathers q.  Differences of q are integers, so Lap and GM(c) are exact and
// only GM(I) is a float64 sum, in a fixed order.
// ---------------------------------------------------------------------------
namespace {

constexpr int kTileW = 64, kTileH = 16;              // owned pixels of a workgroup
constexpr int kHaloW = kTileW + 2, kHaloH = kTileH + 2;
constexpr int kTileRows = kTileH / (NT / kTileW);    // owned pixels of a thread, one per row
static_assert(NT % kTileW == 0 && kTileH % (NT / kTileW) == 0, "a thread keeps its column");

// what a tile adds to an image, and an image's sums: the reduction's accumulator
struct GradRow {
    double gm_i;             // GM(I): sum over owned pairs of ((double)d 2^-32)^2
    unsigned long long gm_c; // GM(c): the same pairs of the count image, exact
    long long lap_max;       // max |Lap| in units of 2^-32
};
static_assert(sizeof(GradRow) == 24, "rows are 24 bytes");

struct GradSum {
    using Row = GradRow;
    static __device__ __forceinline__ Row zero() { return Row{0.0, 0ull, 0ll}; }
    static __device__ __forceinline__ Row add(const Row &a, const Row &b)
    {
        return Row{a.gm_i + b.gm_i, a.gm_c + b.gm_c, a.lap_max > b.lap_max ? a.lap_max : b.lap_max};
    }
};

// the record of an image in the workspace (include/dvsof_contrast_gradient.h)
struct GradRec {
    double coef;  // -2 / GM(c_m); 0 where GM(c_m) is 0
    double gmax;  // |coef Lap 2^-32| <= gmax on every pixel
    double term;  // 1 - GM(I_m)/GM(c_m); 0 where GM(c_m) is 0
    double gm_i;
    unsigned long long gm_c;
    long long lap_max;
};
static_assert(sizeof(GradRec) == 48, "the workspace holds 48 bytes per image");

inline int tiles_across(int w) { return (w + kTileW - 1) / kTileW; }
inline int tiles_down(int h) { return (h + kTileH - 1) / kTileH; }

// Grid (tiles, M), NT threads.  Staging: halo position k = thread, thread + NT, ... of the
// 66 x 18 window whose corner is one pixel up and left of the tile; a row of the window is a
// run of consecutive addresses.  A position outside the image is filled with 0 and not read;
// whether a neighbour exists is asked of its coordinates, never of the filled value.  Thread t
// owns column t % 64 of rows t / 64 + 4 j, j ascending: a pixel inside the image stores its
// Laplacian and adds the pair to its right, then the pair below it, where the neighbour is
// inside the image, in this tile or the next (every pair once, by its left or upper pixel).
__global__ __launch_bounds__(NT) void contrast_gradient_stats_kernel(const int64_t *__restrict__ q,
                                                                     const uint32_t *__restrict__ count, int h,
                                                                     int w, int tx, int64_t *__restrict__ lap,
                                                                     GradRow *__restrict__ part)
{
    __shared__ int64_t sq[kHaloH][kHaloW];
    __shared__ uint32_t sc[kHaloH][kHaloW];
    const int m = blockIdx.y, tile = blockIdx.x;
    const int x0 = (tile % tx) * kTileW, y0 = (tile / tx) * kTileH;
    const size_t plane = (size_t)h * w;
    const int64_t *qm = q + (size_t)m * plane;
    const uint32_t *cm = count + (size_t)m * plane;
    for (int k = threadIdx.x; k < kHaloH * kHaloW; k += NT) {
        const int ly = k / kHaloW, lx = k % kHaloW;
        const int gx = x0 + lx - 1, gy = y0 + ly - 1;
        const bool in = gx >= 0 && gx < w && gy >= 0 && gy < h;
        const size_t at = in ? (size_t)gy * w + (size_t)gx : 0;
        sq[ly][lx] = in ? qm[at] : 0;
        sc[ly][lx] = in ? cm[at] : 0u;
    }
    __syncthreads();
    GradRow a = GradSum::zero();
    const int lx = threadIdx.x % kTileW + 1, gx = x0 + lx - 1;
#pragma unroll
    for (int j = 0; j < kTileRows; ++j) {
        const int ly = threadIdx.x / kTileW + j * (NT / kTileW) + 1, gy = y0 + ly - 1;
        if (gx >= w || gy >= h) continue;
        const int64_t qc = sq[ly][lx];
        const int64_t cc = (int64_t)sc[ly][lx];
        int64_t L = 0;
        if (gx > 0) L += qc - sq[ly][lx - 1];
        if (gy > 0) L += qc - sq[ly - 1][lx];
        if (gx + 1 < w) {
            const int64_t d = sq[ly][lx + 1] - qc, dc = (int64_t)sc[ly][lx + 1] - cc;
            const double di = (double)d * 0x1p-32;
            a.gm_i += di * di;
            a.gm_c += (unsigned long long)(dc * dc);
            L -= d;
        }
        if (gy + 1 < h) {
            const int64_t d = sq[ly + 1][lx] - qc, dc = (int64_t)sc[ly + 1][lx] - cc;
            const double di = (double)d * 0x1p-32;
            a.gm_i += di * di;
            a.gm_c += (unsigned long long)(dc * dc);
            L -= d;
        }
        lap[(size_t)m * plane + (size_t)gy * w + (size_t)gx] = L;
        const long long mag = L < 0 ? -L : L;
        a.lap_max = a.lap_max > mag ? a.lap_max : mag;
    }
    a = block_tree<GradSum>(a);
    if (threadIdx.x == 0) part[(size_t)m * gridDim.x + tile] = a;
}

// One wave, on the pattern of contrast_close_kernel: the record of every image from its row,
// after a barrier the unit of every frame from the largest gmax of its images, and in lane 0
// the images' terms in image order.
__global__ __launch_bounds__(kWave) void contrast_gradient_close_kernel(const GradRow *__restrict__ row, int F,
                                                                        int RC, int unit_bits, GradRec *rec,
                                                                        double *unit, float *term)
{
    const int M = F * RC;
    for (int m = threadIdx.x; m < M; m += kWave) {
        const GradRow r = row[m];
        const bool edges = r.gm_c > 0;
        const double gc = (double)r.gm_c;
        GradRec o;
        o.coef = edges ? -2.0 / gc : 0.0;
        o.gmax = fabs(o.coef) * ((double)r.lap_max * 0x1p-32);
        o.term = edges ? 1.0 - r.gm_i / gc : 0.0;
        o.gm_i = r.gm_i;
        o.gm_c = r.gm_c;
        o.lap_max = r.lap_max;
        rec[m] = o;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < F; f += kWave) {
        double gmax = 0.0;
        for (int k = 0; k < RC; ++k) gmax = fmax(gmax, rec[f * RC + k].gmax);
        unit[f] = unit_of(gmax, unit_bits);
    }
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s += rec[m].term;
        *term = (float)(s / (double)M);
    }
}

// contrast_bwd_events_kernel with G = coef Lap 2^-32 gathered from the Laplacian plane: the
// same factors, the same truncation to the frame's unit, the same sums and bounds (|G| <= gmax).
template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void contrast_gradient_bwd_events_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, const float *__restrict__ flow, int F, int h, int w, Refs refs,
    const int64_t *__restrict__ lap, const GradRec *__restrict__ rec, const double *__restrict__ unit,
    unsigned long long *__restrict__ acc)
{
    const size_t plane = (size_t)h * w;
    const auto addends = [=](int64_t xi, int64_t yi, int c, int f, float tau) {
        const size_t pix = (size_t)yi * w + (size_t)xi;
        float u, v;
        flow_at(flow, f, plane, pix, u, v);
        const double un = unit[f];
        long long su = 0, sv = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const size_t m = image_of<R, POL>(f, r, c);
            const double coef = rec[m].coef;
            if (coef == 0.0) continue;  // GM(c_m) = 0: every addend would be 0
            Warp p;
            if (!warp_event_to(tau, refs.rho[r], u, v, xi, yi, h, w, p)) continue;
            const int64_t *img = lap + m * plane;
            corner_addends(p, h, w, un, [&](size_t at) { return coef * ((double)img[at] * 0x1p-32); }, su, sv);
        }
        unsigned long long *dst = acc + (size_t)f * 2 * plane + pix;
        if (su != 0) atomicAdd(dst, (unsigned long long)su);
        if (sv != 0) atomicAdd(dst + plane, (unsigned long long)sv);
    };
    for_each_window_event<POL>(cols, n, ts, frame_sample, F, h, w, addends);
}

// the workspace as byte offsets, in the order of the header
struct GradLayout {
    size_t lap, rec, unit, row, part, bytes;
    int tx, tiles;
};

GradLayout gradient_layout(int F, int h, int w, const Plan &pl)
{
    GradLayout o;
    o.tx = tiles_across(w);
    o.tiles = o.tx * tiles_down(h);
    o.lap = sums_bytes(F, h, w);
    o.rec = o.lap + sizeof(int64_t) * (size_t)pl.M * h * w;
    o.unit = o.rec + sizeof(GradRec) * (size_t)pl.M;
    o.row = o.unit + sizeof(double) * (size_t)F;
    o.part = o.row + sizeof(GradRow) * (size_t)pl.M;
    o.bytes = o.part + sizeof(GradRow) * (size_t)pl.M * o.tiles;
    return o;
}

size_t gradient_workspace_bytes(int F, int reference_mask, int polarity, int h, int w)
{
    Plan pl;
    if (F < 1 || bad_frame_sizes(F, h, w) || !plan_of(F, reference_mask, polarity, pl)) return 0;
    return gradient_layout(F, h, w, pl).bytes;
}

// dvsof_contrast_gradient_fwd / _bwd on either form of the event columns
template <class Cols>
int gradient_fwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                 const float *flow, int F, int h, int w, int reference_mask, int polarity, int64_t *q,
                 uint32_t *count, float *term, void *workspace, size_t workspace_bytes, void *stream)
{
    Plan pl;
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !count || !term || !frame_ts || !frame_sample || !flow) return DVSOF_EINVAL;
    if (n_events > 0 && !cols.given(polarity)) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < gradient_workspace_bytes(F, reference_mask, polarity, h, w))
        return DVSOF_ENOSPACE;
    hipStream_t st = as_stream(stream);
    const size_t pixels = (size_t)pl.M * h * w;
    const GradLayout lay = gradient_layout(F, h, w, pl);
    char *ws = (char *)workspace;
    DVSOF_HIP_TRY((hipError_t)fill_u32(q, 0u, sizeof(int64_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(count, 0u, sizeof(uint32_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws, 0u, sums_bytes(F, h, w), st));
    if (n_events > 0) {
        const OneLevel view{h, w, flow, 0.f, nullptr};
        DVSOF_REFS_POL_DISPATCH(contrast_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, F, h, w, pl.refs, view, (unsigned long long *)q,
                                count);
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(contrast_gradient_stats_kernel, dim3((unsigned)lay.tiles, (unsigned)pl.M), dim3(NT), 0, st,
                       (const int64_t *)q, (const uint32_t *)count, h, w, lay.tx, (int64_t *)(ws + lay.lap),
                       (GradRow *)(ws + lay.part));
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_final_kernel<GradSum>, dim3((unsigned)pl.M), dim3(kWave), 0, st,
                       (const GradRow *)(ws + lay.part), lay.tiles, (GradRow *)(ws + lay.row));
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(contrast_gradient_close_kernel, dim3(1), dim3(kWave), 0, st, (const GradRow *)(ws + lay.row),
                       F, pl.R * pl.C, pl.R > 1 ? kUnitBits - kSharedBits : kUnitBits, (GradRec *)(ws + lay.rec),
                       (double *)(ws + lay.unit), term);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

template <class Cols>
int gradient_bwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                 const float *flow, int F, int h, int w, int reference_mask, int polarity, const int64_t *q,
                 void *workspace, size_t workspace_bytes, const float *seed, float weight, float *grad_flow,
                 void *stream)
{
    Plan pl;
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !seed || !grad_flow || !frame_ts || !frame_sample || !flow) return DVSOF_EINVAL;
    if (n_events > 0 && !cols.given(polarity)) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < gradient_workspace_bytes(F, reference_mask, polarity, h, w))
        return DVSOF_ENOSPACE;
    hipStream_t st = as_stream(stream);
    const GradLayout lay = gradient_layout(F, h, w, pl);
    char *ws = (char *)workspace;
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(contrast_gradient_bwd_events_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st,
                                cols, n_events, frame_ts, frame_sample, flow, F, h, w, pl.refs,
                                (const int64_t *)(ws + lay.lap), (const GradRec *)(ws + lay.rec),
                                (const double *)(ws + lay.unit), (unsigned long long *)ws);
        DVSOF_LAUNCH_CHECK();
    }
    const size_t total = 2 * (size_t)F * h * w;
    hipLaunchKernelGGL(event_term_bwd_close_kernel<OneLevel>, dim3(event_blocks((int64_t)total)), dim3(NT), 0, st,
                       (long long *)ws, (const double *)(ws + lay.unit), seed, F, pl.M,
                       OneLevel{h, w, flow, weight, grad_flow}, total);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // namespace

extern "C" {

size_t dvsof_contrast_gradient_workspace_bytes(int F, int reference_mask, int polarity, int h, int w)
{
    return gradient_workspace_bytes(F, reference_mask, polarity, h, w);
}

int dvsof_contrast_gradient_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                const int64_t *frame_sample, const float *flow, int F, int h, int w,
                                int reference_mask, int polarity, int64_t *q, uint32_t *count, float *term,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    return gradient_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, flow, F, h, w,
                        reference_mask, polarity, q, count, term, workspace, workspace_bytes, stream);
}

int dvsof_contrast_gradient_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                const int64_t *frame_sample, const float *flow, int F, int h, int w,
                                int reference_mask, int polarity, const int64_t *q, void *workspace,
                                size_t workspace_bytes, const float *seed, float weight, float *grad_flow,
                                void *stream)
{
    return gradient_bwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, flow, F, h, w,
                        reference_mask, polarity, q, workspace, workspace_bytes, seed, weight, grad_flow, stream);
}

int dvsof_contrast_gradient_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                        const int64_t *sample_event_offsets, int B, int64_t n_events,
                                        const float *frame_ts, const int64_t *frame_sample, const float *flow,
                                        int F, int h, int w, int reference_mask, int polarity_channels, int64_t *q,
                                        uint32_t *count, float *term, void *workspace, size_t workspace_bytes,
                                        void *stream)
{
    return gradient_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts,
                        frame_sample, flow, F, h, w, reference_mask, polarity_channels, q, count, term, workspace,
                        workspace_bytes, stream);
}

int dvsof_contrast_gradient_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                        const int64_t *sample_event_offsets, int B, int64_t n_events,
                                        const float *frame_ts, const int64_t *frame_sample, const float *flow,
                                        int F, int h, int w, int reference_mask, int polarity_channels,
                                        const int64_t *q, void *workspace, size_t workspace_bytes,
                                        const float *seed, float weight, float *grad_flow, void *stream)
{
    return gradient_bwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts,
                        frame_sample, flow, F, h, w, reference_mask, polarity_channels, q, workspace,
                        workspace_bytes, seed, weight, grad_flow, stream);
}

}  // extern "C"
