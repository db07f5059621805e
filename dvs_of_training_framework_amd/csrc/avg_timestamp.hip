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
// The term on every flow scale of the network (sections 11-15,
// include/dvsof_avg_timestamp_pyramid.h) is the same kernels and the same host
// functions over a level table: each is written once against a view of the
// call's levels (event_term_levels.h) and instantiated for one flow and for a
// table, with one fill, one splat, one closing wave and one backward for all
// levels.  What one event does to the images of a frame, forward and backward,
// is stated once (avgts_splat_event of avg_timestamp_images.h,
// avgts_bwd_event).  Behind that: this term and the contrast term of
// contrast.hip together, from this term's splat (section 19,
// include/dvsof_event_terms_joint.h).
#include <type_traits>
#include "avg_timestamp_images.h"
#include "event_term_levels.h"
#include "event_term_records.h"
#include "tiled_splat.h"
#include "../../include/dvsof_avg_timestamp.h"
#include "../../include/dvsof_avg_timestamp_pyramid.h"
#include "../../include/dvsof_event_terms_encoded.h"
#include "../../include/dvsof_avg_timestamp_tiled.h"
#include "../../include/dvsof_event_pyramids_tiled.h"
#include "../../include/dvsof_event_terms_joint.h"

namespace {

constexpr int NT = kFrameNT;
// the unit bits and unit_of: event_term_records.h, which the contrast term shares

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
// The columns are read, the frames walked and tau computed once per event; the
// levels are a runtime loop around avgts_splat_event with the event's level
// pixel (y >> s, x >> s), the level's flow, plane and images.
// ---------------------------------------------------------------------------
template <int R, bool POL, class Cols, class View>
__global__ __launch_bounds__(NT) void avgts_splat_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, int F, int h, int w, Refs refs, const View view,
    unsigned long long *__restrict__ q, unsigned long long *__restrict__ s, unsigned long long *__restrict__ base,
    uint32_t *__restrict__ count)
{
    const auto splat = [=, &view](int64_t xi, int64_t yi, int c, int f, float tau) {
#pragma unroll 1
        for (int k = 0; k < view.levels(); ++k) {
            const Level &L = view.at(k);
            const int64_t xs = xi >> L.shift, ys = yi >> L.shift;  // xs <= (w - 1) >> s <= L.w - 1
            const size_t plane = (size_t)L.h * L.w;
            const size_t pix = (size_t)ys * L.w + (size_t)xs;
            float u, v;
            flow_at(L.flow, f, plane, pix, u, v);
            avgts_splat_event<R, POL>(refs, f, c, tau, u, v, xs, ys, pix, plane, L.h, L.w, q + L.image_offset,
                                      s + L.image_offset, base + L.image_offset, count + L.image_offset);
        }
    };
    for_each_window_event<POL>(cols, n, ts, frame_sample, F, h, w, splat);
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

// One wave over the K M images and K F units of all levels (image i = k M + m, unit j = k F + f,
// whose images are i = j RC ...): the record of every image (lane k takes images k, k + 64, ...);
// after a barrier the unit of every frame (lane k takes frames k, k + 64, ...; a maximum has no
// order) and, in lane 0, every level's term in image order.  Over a table also the weighted sum
// in level order; on one flow terms is the call's term and value is not written.
template <class View>
__global__ __launch_bounds__(kWave) void avgts_close_kernel(const StatRow *__restrict__ rows, int F, int RC,
                                                            int unit_bits, const View view, ImageRec *rec,
                                                            double *unit, float *terms, float *value)
{
    const int M = F * RC, K = view.levels();
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
            if (View::kTable) total += (double)view.at(k).weight * term;
        }
        if (View::kTable) *value = (float)total;
    }
}

// ---------------------------------------------------------------------------
// Backward.  One thread per event and frame: for every reference
// G = 2 k T D (a - T) at the four corners of the image of its channel (0
// outside the image), the derivative of the bilinear weights, -sig of it to
// the event's own pixel of the flow, in float64, truncated to the frame's unit
// un (corner_addends of event_term_levels.h).  The event of avgts_splat_event;
// q, s and rec start at the images of this shape.  The R addends are added to
// su, sv in registers (integers: no order).
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
        const auto G_at = [&](size_t at) {
            const double den = (double)qm[at] * 0x1p-32 + kEps;
            const double T = (double)sm[at] * 0x1p-32 / den;
            const double D = 1.0 / den;
            return k2 * T * D * (a - T);
        };
        corner_addends(p, h, w, un, G_at, su, sv);
    }
}

// per level as in the splat; the sums of a level start at its sums_offset
template <int R, bool POL, class Cols, class View>
__global__ __launch_bounds__(NT) void avgts_bwd_events_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts,
    const int64_t *__restrict__ frame_sample, int F, int h, int w, Refs refs, const View view,
    const int64_t *__restrict__ q, const int64_t *__restrict__ s, const ImageRec *__restrict__ rec,
    const double *__restrict__ unit, unsigned long long *__restrict__ acc)
{
    const size_t M = (size_t)F * R * (POL ? 2 : 1);
    const auto addends = [=, &view](int64_t xi, int64_t yi, int c, int f, float tau) {
#pragma unroll 1
        for (int k = 0; k < view.levels(); ++k) {
            const Level &L = view.at(k);
            const int64_t xs = xi >> L.shift, ys = yi >> L.shift;
            const size_t plane = (size_t)L.h * L.w;
            const size_t pix = (size_t)ys * L.w + (size_t)xs;
            float u, v;
            flow_at(L.flow, f, plane, pix, u, v);
            long long su = 0, sv = 0;
            avgts_bwd_event<R, POL>(refs, f, c, tau, u, v, xs, ys, plane, L.h, L.w, q + L.image_offset,
                                    s + L.image_offset, rec + (size_t)k * M, unit[(size_t)k * F + f], su, sv);
            unsigned long long *dst = acc + L.sums_offset + (size_t)f * 2 * plane + pix;
            if (su != 0) atomicAdd(dst, (unsigned long long)su);
            if (sv != 0) atomicAdd(dst + plane, (unsigned long long)sv);
        }
    };
    for_each_window_event<POL>(cols, n, ts, frame_sample, F, h, w, addends);
}

// the workspace as byte offsets, in the order of the headers (a call on one flow: K = 1)
struct PyramidLayout {
    size_t s, base, sums, count, zeroed_bytes, rec, unit, rows, part, bytes;
    size_t sums_elems;
};

// false: a table the calls refuse.  The offsets are looked at only where check_offsets is set
// (the workspace_bytes calls read the shapes alone).
bool pyramid_layout(int F, int h, int w, const Plan &pl, const Levels &lv, bool check_offsets, PyramidLayout &o)
{
    const size_t pixels = level_table_pixels(F, h, w, lv, check_offsets ? pl.M : 0);
    if (pixels == 0) return false;
    int nb = 0;
    for (int k = 0; k < lv.K; ++k) {
        const int need = partial_blocks(lv.level[k].h, lv.level[k].w);
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

// The refusals both calls share up to the workspace, in the order of the headers; outputs: the
// call's own pointers are all there.  DVSOF_OK with F == 0: nothing to do.  A call on one flow
// asks with its table of one level: its flow and grad_flow are the level's, and every refusal
// between F == 0 and the columns is DVSOF_EINVAL, so code and order are those of
// dvsof_contrast_multi_fwd.  The level table of the contrast term has the same packed offsets at
// its own M and the same refusals (dvsof_contrast_pyramid.h), so the joint calls at the end of
// the file ask this for either term.
template <class Cols>
int pyramid_refusals(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F,
                     int h, int w, int reference_mask, int polarity, const Levels &lv, bool backward, bool outputs,
                     Plan &pl, PyramidLayout &lay)
{
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (lv.K < 1 || lv.K > kMaxLevels) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (!pyramid_layout(F, h, w, pl, lv, true, lay) || !outputs || !frame_ts || !frame_sample) return DVSOF_EINVAL;
    for (int k = 0; k < lv.K; ++k)
        if (!lv.level[k].flow || (backward && !lv.level[k].grad_flow)) return DVSOF_EINVAL;
    if (n_events > 0 && !cols.given(polarity)) return DVSOF_EINVAL;
    return DVSOF_OK;
}

template <class Cols>
int pyramid_check(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F,
                  int h, int w, int reference_mask, int polarity, const Levels &lv, bool backward, bool outputs,
                  const void *workspace, size_t workspace_bytes, Plan &pl, PyramidLayout &lay)
{
    const int rc = pyramid_refusals(cols, n_events, frame_ts, frame_sample, F, h, w, reference_mask, polarity, lv,
                                    backward, outputs, pl, lay);
    if (rc != DVSOF_OK || F == 0) return rc;
    if (!workspace || workspace_bytes < lay.bytes) return DVSOF_ENOSPACE;
    return DVSOF_OK;
}

// 0 for arguments the calls refuse
size_t term_workspace_bytes(int F, int reference_mask, int polarity, int h, int w, const Levels &levels)
{
    Plan pl;
    PyramidLayout lay;
    if (F < 1 || !plan_of(F, reference_mask, polarity, pl) || !pyramid_layout(F, h, w, pl, levels, false, lay))
        return 0;
    return lay.bytes;
}

// dvsof_avg_timestamp_fwd / _bwd (View: OneLevel; terms is the call's term, value is null) and
// dvsof_avg_timestamp_pyramid_fwd / _bwd (TableView) on either form of the event columns
// (event_columns.h).  The two tiled schedules stay apart (tiled_splat.h): the view picks one.
template <class Cols, class View>
int term_fwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F, int h,
             int w, int reference_mask, int polarity, const View &view, float *terms, float *value, void *workspace,
             size_t workspace_bytes, void *stream, const TiledSplat tiled = TiledSplat{nullptr, 0, -1})
{
    const Levels levels = view.table();
    Plan pl;
    PyramidLayout lay;
    const int rc = pyramid_check(cols, n_events, frame_ts, frame_sample, F, h, w, reference_mask, polarity, levels,
                                 false, terms && (value || !View::kTable), workspace, workspace_bytes, pl, lay);
    if (rc != DVSOF_OK || F == 0) return rc;
    std::conditional_t<View::kTable, PyramidTilePlan, TilePlan> tp;
    int by_tiles;
    if constexpr (View::kTable)
        by_tiles = pyramid_tile_decide<AvgtsImages>(tiled, F, reference_mask, polarity, h, w, levels, n_events, tp);
    else
        by_tiles = tile_decide<AvgtsImages>(tiled, F, reference_mask, polarity, h, w, n_events, tp);
    if (by_tiles != DVSOF_OK && by_tiles != 1) return by_tiles;
    hipStream_t st = as_stream(stream);
    char *ws = (char *)workspace;
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws, 0u, lay.zeroed_bytes, st));
    if (by_tiles == DVSOF_OK) {
        const AvgtsImages img{(int64_t *)ws, (int64_t *)(ws + lay.s), (int64_t *)(ws + lay.base),
                              (uint32_t *)(ws + lay.count)};
        int rs;
        if constexpr (View::kTable)
            rs = TiledLaunch<AvgtsImages>::pyramid(plain(cols), n_events, frame_ts, frame_sample, F, h, w,
                                                   reference_mask, polarity, levels, tp, img, tiled.workspace, st);
        else
            rs = TiledLaunch<AvgtsImages>::term(plain(cols), n_events, frame_ts, frame_sample, view.flow, F, h, w,
                                                reference_mask, polarity, tp, img, tiled.workspace, st);
        if (rs != DVSOF_OK) return rs;
    } else if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(avgts_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, F, h, w, pl.refs, view,
                                (unsigned long long *)ws, (unsigned long long *)(ws + lay.s),
                                (unsigned long long *)(ws + lay.base), (uint32_t *)(ws + lay.count));
        DVSOF_LAUNCH_CHECK();
    }
    // per level the two launches of the statistics with its own nb: that order makes the bytes
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
    hipLaunchKernelGGL(avgts_close_kernel<View>, dim3(1), dim3(kWave), 0, st, (const StatRow *)(ws + lay.rows), F,
                       pl.R * pl.C, pl.R > 1 ? kUnitBits - kSharedBits : kUnitBits, view, (ImageRec *)(ws + lay.rec),
                       (double *)(ws + lay.unit), terms, value);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

template <class Cols, class View>
int term_bwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F, int h,
             int w, int reference_mask, int polarity, const View &view, void *workspace, size_t workspace_bytes,
             const float *seed, void *stream)
{
    const Levels levels = view.table();
    Plan pl;
    PyramidLayout lay;
    const int rc = pyramid_check(cols, n_events, frame_ts, frame_sample, F, h, w, reference_mask, polarity, levels,
                                 true, seed != nullptr, workspace, workspace_bytes, pl, lay);
    if (rc != DVSOF_OK || F == 0) return rc;
    hipStream_t st = as_stream(stream);
    char *ws = (char *)workspace;
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(avgts_bwd_events_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, F, h, w, pl.refs, view, (const int64_t *)ws,
                                (const int64_t *)(ws + lay.s), (const ImageRec *)(ws + lay.rec),
                                (const double *)(ws + lay.unit), (unsigned long long *)(ws + lay.sums));
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(event_term_bwd_close_kernel<View>, dim3(event_blocks((int64_t)lay.sums_elems)), dim3(NT), 0, st,
                       (long long *)(ws + lay.sums), (const double *)(ws + lay.unit), seed, F, pl.M, view,
                       lay.sums_elems);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // namespace

extern "C" {

size_t dvsof_avg_timestamp_workspace_bytes(int F, int reference_mask, int polarity, int h, int w)
{
    return term_workspace_bytes(F, reference_mask, polarity, h, w, OneLevel{h, w, nullptr, 0.f, nullptr}.table());
}

int dvsof_avg_timestamp_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                            const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                            const int64_t *frame_sample, const float *flow, int F, int h, int w,
                            int reference_mask, int polarity, float *term, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    return term_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                    reference_mask, polarity, OneLevel{h, w, flow, 0.f, nullptr}, term, nullptr, workspace,
                    workspace_bytes, stream);
}

int dvsof_avg_timestamp_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                            const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                            const int64_t *frame_sample, const float *flow, int F, int h, int w,
                            int reference_mask, int polarity, void *workspace, size_t workspace_bytes,
                            const float *seed, float weight, float *grad_flow, void *stream)
{
    return term_bwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                    reference_mask, polarity, OneLevel{h, w, flow, weight, grad_flow}, workspace, workspace_bytes,
                    seed, stream);
}

// The encoded twins (include/dvsof_event_terms_encoded.h)
int dvsof_avg_timestamp_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                    const int64_t *sample_event_offsets, int B, int64_t n_events,
                                    const float *frame_ts, const int64_t *frame_sample, const float *flow, int F,
                                    int h, int w, int reference_mask, int polarity_channels, float *term,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    return term_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample, F,
                    h, w, reference_mask, polarity_channels, OneLevel{h, w, flow, 0.f, nullptr}, term, nullptr,
                    workspace, workspace_bytes, stream);
}

int dvsof_avg_timestamp_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                    const int64_t *sample_event_offsets, int B, int64_t n_events,
                                    const float *frame_ts, const int64_t *frame_sample, const float *flow, int F,
                                    int h, int w, int reference_mask, int polarity_channels, void *workspace,
                                    size_t workspace_bytes, const float *seed, float weight, float *grad_flow,
                                    void *stream)
{
    return term_bwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample, F,
                    h, w, reference_mask, polarity_channels, OneLevel{h, w, flow, weight, grad_flow}, workspace,
                    workspace_bytes, seed, stream);
}

// The tiled twins (include/dvsof_avg_timestamp_tiled.h): the forward above with the splat by tiles
int dvsof_avg_timestamp_fwd_tiled(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                  const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                  const int64_t *frame_sample, const float *flow, int F, int h, int w,
                                  int reference_mask, int polarity, float *term, void *workspace,
                                  size_t workspace_bytes, void *stream, void *tile_workspace,
                                  size_t tile_workspace_bytes, int mode)
{
    if (mode != 0 && mode != 1) return DVSOF_EINVAL;
    return term_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                    reference_mask, polarity, OneLevel{h, w, flow, 0.f, nullptr}, term, nullptr, workspace,
                    workspace_bytes, stream, TiledSplat{tile_workspace, tile_workspace_bytes, mode});
}

int dvsof_avg_timestamp_fwd_encoded_tiled(const int16_t *x, const int16_t *y, const float *t,
                                          const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                          int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                          const float *flow, int F, int h, int w, int reference_mask,
                                          int polarity_channels, float *term, void *workspace,
                                          size_t workspace_bytes, void *stream, void *tile_workspace,
                                          size_t tile_workspace_bytes, int mode)
{
    if (mode != 0 && mode != 1) return DVSOF_EINVAL;
    return term_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample, F,
                    h, w, reference_mask, polarity_channels, OneLevel{h, w, flow, 0.f, nullptr}, term, nullptr,
                    workspace, workspace_bytes, stream, TiledSplat{tile_workspace, tile_workspace_bytes, mode});
}

// The term on every flow scale (include/dvsof_avg_timestamp_pyramid.h)
size_t dvsof_avg_timestamp_pyramid_workspace_bytes(int F, int reference_mask, int polarity, int h, int w,
                                                   dvsof_contrast_levels_t levels)
{
    return term_workspace_bytes(F, reference_mask, polarity, h, w, levels);
}

int dvsof_avg_timestamp_pyramid_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                    const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                    const int64_t *frame_sample, int F, int h, int w, int reference_mask,
                                    int polarity, dvsof_contrast_levels_t levels, float *terms, float *value,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    return term_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                    reference_mask, polarity, TableView{levels}, terms, value, workspace, workspace_bytes, stream);
}

int dvsof_avg_timestamp_pyramid_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                    const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                    const int64_t *frame_sample, int F, int h, int w, int reference_mask,
                                    int polarity, dvsof_contrast_levels_t levels, void *workspace,
                                    size_t workspace_bytes, const float *seed, void *stream)
{
    return term_bwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                    reference_mask, polarity, TableView{levels}, workspace, workspace_bytes, seed, stream);
}

int dvsof_avg_timestamp_pyramid_fwd_encoded(const int16_t *x, const int16_t *y, const float *t,
                                            const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                            int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                            int F, int h, int w, int reference_mask, int polarity_channels,
                                            dvsof_contrast_levels_t levels, float *terms, float *value,
                                            void *workspace, size_t workspace_bytes, void *stream)
{
    return term_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample, F,
                    h, w, reference_mask, polarity_channels, TableView{levels}, terms, value, workspace,
                    workspace_bytes, stream);
}

int dvsof_avg_timestamp_pyramid_bwd_encoded(const int16_t *x, const int16_t *y, const float *t,
                                            const uint8_t *polarity, const int64_t *sample_event_offsets, int B,
                                            int64_t n_events, const float *frame_ts, const int64_t *frame_sample,
                                            int F, int h, int w, int reference_mask, int polarity_channels,
                                            dvsof_contrast_levels_t levels, void *workspace, size_t workspace_bytes,
                                            const float *seed, void *stream)
{
    return term_bwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample, F,
                    h, w, reference_mask, polarity_channels, TableView{levels}, workspace, workspace_bytes, seed,
                    stream);
}

// The tiled twins (include/dvsof_event_pyramids_tiled.h): the forward above with the splat by tiles
int dvsof_avg_timestamp_pyramid_fwd_tiled(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                          const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                          const int64_t *frame_sample, int F, int h, int w, int reference_mask,
                                          int polarity, dvsof_contrast_levels_t levels, float *terms, float *value,
                                          void *workspace, size_t workspace_bytes, void *stream,
                                          void *tile_workspace, size_t tile_workspace_bytes, int mode)
{
    if (mode != 0 && mode != 1) return DVSOF_EINVAL;
    return term_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w,
                    reference_mask, polarity, TableView{levels}, terms, value, workspace, workspace_bytes, stream,
                    TiledSplat{tile_workspace, tile_workspace_bytes, mode});
}

int dvsof_avg_timestamp_pyramid_fwd_encoded_tiled(const int16_t *x, const int16_t *y, const float *t,
                                                  const uint8_t *polarity, const int64_t *sample_event_offsets,
                                                  int B, int64_t n_events, const float *frame_ts,
                                                  const int64_t *frame_sample, int F, int h, int w,
                                                  int reference_mask, int polarity_channels,
                                                  dvsof_contrast_levels_t levels, float *terms, float *value,
                                                  void *workspace, size_t workspace_bytes, void *stream,
                                                  void *tile_workspace, size_t tile_workspace_bytes, int mode)
{
    if (mode != 0 && mode != 1) return DVSOF_EINVAL;
    return term_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample, F,
                    h, w, reference_mask, polarity_channels, TableView{levels}, terms, value, workspace,
                    workspace_bytes, stream, TiledSplat{tile_workspace, tile_workspace_bytes, mode});
}

}  // extern "C"

// ---------------------------------------------------------------------------
// This term and the contrast term of contrast.hip together
// (include/dvsof_event_terms_joint.h; docs/AVG_TIMESTAMP_SPEC.md section 19,
// docs/CONTRAST_SPEC.md section 26).  q and count of this term's image of
// (f, rho, c) are the contrast term's image of the same (f, rho, c), so the
// forward is this file's fill and splat over the level table, unchanged; the
// statistics reduce the rows of both terms from one read of a pixel and keep
// its T and D; one wave closes both terms; one event kernel walks the events
// once for both gradients, which stay in sums of their own.  Every float64
// expression is the one the two terms' own kernels evaluate, in their order.
// ---------------------------------------------------------------------------
namespace {

// The contrast term's references among this term's R: bit r is set where this term's
// reference r (the r-th set bit of avg_mask) is also the contrast term's.
inline int joint_subset(int contrast_mask, int avg_mask)
{
    int sub = 0, r = 0;
    for (int b = 0; b < kMaxRefs; ++b) {
        if (!(avg_mask >> b & 1)) continue;
        if (contrast_mask >> b & 1) sub |= 1 << r;
        ++r;
    }
    return sub;
}

// The image mapping: the contrast term's image (f Rc + rc) C + c that this term's image of frame
// f, reference r and channel c also is, rc the contrast references before r; -1 where r is none
// of the contrast term's.  Rc: the bits of sub.
__host__ __device__ __forceinline__ int64_t joint_contrast_image(int sub, int Rc, int C, int f, int r, int c)
{
    if (!(sub >> r & 1)) return -1;
    const int rc = __builtin_popcount((unsigned)(sub & ((1 << r) - 1)));
    return ((int64_t)f * Rc + rc) * C + c;
}

// the statistics row of an image for both terms
struct JointRow {
    StatRow a;
    dvsof_iwe_result_t c;
};
static_assert(sizeof(JointRow) == 80, "the workspace holds 80 bytes per row");

// componentwise, so every component is reduced in the order of its own term's launches
struct JointSum {
    using Row = JointRow;
    static __device__ __forceinline__ Row zero() { return Row{AvgSum::zero(), IweSum::zero()}; }
    static __device__ __forceinline__ Row add(const Row &a, const Row &b)
    {
        return Row{AvgSum::add(a.a, b.a), IweSum::add(a.c, b.c)};
    }
};

// avgts_stats_partial_kernel and iwe_stats_partial_kernel on one read of the pixel, with the
// pixel's T and D kept for the backward
__global__ __launch_bounds__(NT) void joint_stats_partial_kernel(
    const int64_t *__restrict__ q, const int64_t *__restrict__ s, const int64_t *__restrict__ base,
    const uint32_t *__restrict__ count, int h, int w, int nb, JointRow *__restrict__ part, double *__restrict__ T,
    double *__restrict__ D)
{
    const int m = blockIdx.y;
    const int n = h * w;
    const int64_t *qm = q + (size_t)m * n, *sm = s + (size_t)m * n, *bm = base + (size_t)m * n;
    const uint32_t *cm = count + (size_t)m * n;
    double *Tm = T + (size_t)m * n, *Dm = D + (size_t)m * n;
    frame_partial<JointSum>(n, nb, part, [=](JointRow &a, int p) {
        const int64_t Q = qm[p];
        const uint32_t c = cm[p];
        const AvgPixel px = avgts_pixel(Q, sm[p], bm[p], c);
        avgts_stats_pixel(a.a, Q, c, px);
        iwe_stats_pixel(a.c, Q, (int64_t)c);
        Tm[p] = px.T;
        Dm[p] = px.D;
    });
}

// avgts_close_kernel and contrast_close_kernel of contrast.hip over a table in one wave: the
// records of both terms from the joint rows (the contrast term's rows go to its result), after a
// barrier both units of every level and frame, each the maximum over its own term's images, and
// the terms and values, the contrast term's in lane 0 and this term's in lane 1.
__global__ __launch_bounds__(kWave) void joint_close_kernel(const JointRow *__restrict__ rows, int F, int Ra, int C,
                                                            int sub, const Levels lc, const Levels la,
                                                            ImageRec *arec, double *aunit, ContrastRec *crec,
                                                            double *cunit, dvsof_iwe_result_t *result,
                                                            float *cterms, float *cvalue, float *aterms,
                                                            float *avalue)
{
    const int Rc = __builtin_popcount((unsigned)sub), K = la.K;
    const int Ma = F * Ra * C, Mc = F * Rc * C;
    for (int i = threadIdx.x; i < K * Ma; i += kWave) {
        const int k = i / Ma, m = i - k * Ma;
        const JointRow row = rows[i];
        arec[i] = record_of(row.a);
        const int64_t mc = joint_contrast_image(sub, Rc, C, m / (Ra * C), m / C % Ra, m % C);
        if (mc < 0) continue;
        const Level &L = la.level[k];
        result[(size_t)k * Mc + mc] = row.c;
        crec[(size_t)k * Mc + mc] = contrast_record_of(row.c, (double)L.h * (double)L.w);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < K * F; j += kWave) {
        double ga = 0.0, gc = 0.0;
        for (int k = 0; k < Ra * C; ++k) ga = fmax(ga, arec[(size_t)j * Ra * C + k].gmax);
        for (int k = 0; k < Rc * C; ++k) gc = fmax(gc, crec[(size_t)j * Rc * C + k].gmax);
        aunit[j] = unit_of(ga, Ra > 1 ? kUnitBits - kSharedBits : kUnitBits);
        cunit[j] = unit_of(gc, Rc > 1 ? kUnitBits - kSharedBits : kUnitBits);
    }
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < K; ++k) {
            double sum = 0.0;
            for (int m = 0; m < Mc; ++m) sum += crec[(size_t)k * Mc + m].term;
            const double term = sum / (double)Mc;
            cterms[k] = (float)term;
            total += (double)lc.level[k].weight * term;
        }
        *cvalue = (float)total;
    }
    if (threadIdx.x == 1) {
        double total = 0.0;
        for (int k = 0; k < K; ++k) {
            double sum = 0.0;
            for (int m = 0; m < Ma; ++m) sum += arec[(size_t)k * Ma + m].value;
            const double term = sum / (double)Ma;
            aterms[k] = (float)term;
            total += (double)la.level[k].weight * term;
        }
        *avalue = (float)total;
    }
}

// avgts_bwd_events_kernel and contrast_bwd_events_kernel over a table in one walk: per event,
// frame and level one flow read, per reference one warp and one set of corners, at each corner
// inside the image T and D (this term: G = k2 T D (a - T), the stored T and D being what
// avgts_bwd_event computes) and, where the reference is also the contrast term's, q
// (G = coef (q 2^-32 - mean)).  Two pairs of integer sums in registers, each truncated to its
// own term's unit, into sums of their own.  57 (<1, false>) to 102 (<3, true>) VGPRs, seven to
// four waves a SIMD, no scratch (profiles/event_terms_joint/README.md).
template <int R, bool POL, class Cols>
__global__ __launch_bounds__(NT) void joint_bwd_events_kernel(
    const Cols cols, int64_t n, const float *__restrict__ ts, const int64_t *__restrict__ frame_sample, int F, int h,
    int w, Refs refs, int sub, const Levels la, const int64_t *__restrict__ q, const double *__restrict__ T,
    const double *__restrict__ D, const ImageRec *__restrict__ arec, const double *__restrict__ aunit,
    const ContrastRec *__restrict__ crec, const double *__restrict__ cunit, unsigned long long *__restrict__ aacc,
    unsigned long long *__restrict__ cacc)
{
    constexpr int C = POL ? 2 : 1;
    const int Rc = __builtin_popcount((unsigned)sub);
    const size_t Ma = (size_t)F * R * C, Mc = (size_t)F * Rc * C;
    const auto addends = [=, &la](int64_t xi, int64_t yi, int c, int f, float tau) {
#pragma unroll 1
        for (int k = 0; k < la.K; ++k) {
            const Level &L = la.level[k];
            const int lh = L.h, lw = L.w;
            const int64_t xs = xi >> L.shift, ys = yi >> L.shift;
            const size_t plane = (size_t)lh * lw;
            const size_t pix = (size_t)ys * lw + (size_t)xs;
            float u, v;
            flow_at(L.flow, f, plane, pix, u, v);
            const double ua = aunit[(size_t)k * F + f], uc = cunit[(size_t)k * F + f];
            long long asu = 0, asv = 0, csu = 0, csv = 0;  // the bounds of the two kernels, per term
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const size_t m = image_of<R, POL>(f, r, c);
                const double k2 = arec[(size_t)k * Ma + m].k2;
                const int64_t mc = joint_contrast_image(sub, Rc, C, f, r, c);
                double coef = 0.0, mean = 0.0;
                if (mc >= 0) {
                    const ContrastRec cr = crec[(size_t)k * Mc + (size_t)mc];
                    coef = cr.coef;
                    mean = cr.mean;
                }
                const bool ta = !(k2 == 0.0), tc = !(coef == 0.0);  // a term whose every addend would be 0
                if (!ta && !tc) continue;
                Warp p;
                if (!warp_event_to(tau, refs.rho[r], u, v, xs, ys, lh, lw, p)) continue;
                const double a = (double)fabsf(p.tau);
                const size_t image = L.image_offset + m * plane;
                double Ga[2][2], Gc[2][2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int xx = p.cx + i, yy = p.cy + j;
                        const bool in = xx >= 0 && xx < lw && yy >= 0 && yy < lh;
                        const size_t at = image + (size_t)yy * lw + (size_t)xx;
                        double ga = 0.0, gc = 0.0;
                        if (in && ta) {
                            const double Tp = T[at];
                            ga = k2 * Tp * D[at] * (a - Tp);
                        }
                        if (in && tc) gc = coef * ((double)q[at] * 0x1p-32 - mean);
                        Ga[j][i] = ga;
                        Gc[j][i] = gc;
                    }
                }
                const double ms = -(double)p.tau;  // p.tau holds sig; d xw / d u = -sig
                if (ta) {
                    const double gx = (double)p.wy[0] * (Ga[0][1] - Ga[0][0]) + (double)p.wy[1] * (Ga[1][1] - Ga[1][0]);
                    const double gy = (double)p.wx[0] * (Ga[1][0] - Ga[0][0]) + (double)p.wx[1] * (Ga[1][1] - Ga[0][1]);
                    asu += (long long)(ms * gx * ua);
                    asv += (long long)(ms * gy * ua);
                }
                if (tc) {
                    const double gx = (double)p.wy[0] * (Gc[0][1] - Gc[0][0]) + (double)p.wy[1] * (Gc[1][1] - Gc[1][0]);
                    const double gy = (double)p.wx[0] * (Gc[1][0] - Gc[0][0]) + (double)p.wx[1] * (Gc[1][1] - Gc[0][1]);
                    csu += (long long)(ms * gx * uc);
                    csv += (long long)(ms * gy * uc);
                }
            }
            const size_t at = L.sums_offset + (size_t)f * 2 * plane + pix;
            if (asu != 0) atomicAdd(aacc + at, (unsigned long long)asu);
            if (asv != 0) atomicAdd(aacc + at + plane, (unsigned long long)asv);
            if (csu != 0) atomicAdd(cacc + at, (unsigned long long)csu);
            if (csv != 0) atomicAdd(cacc + at + plane, (unsigned long long)csv);
        }
    };
    for_each_window_event<POL>(cols, n, ts, frame_sample, F, h, w, addends);
}

// event_term_bwd_close_kernel for both terms: one thread per element of a level's grad_flow
// converts, clears and stores this term's sum and the contrast term's, each with its own unit,
// M, weight, seed and grad_flow.
__global__ __launch_bounds__(NT) void joint_bwd_close_kernel(long long *__restrict__ aacc, long long *__restrict__ cacc,
                                                             const double *__restrict__ aunit,
                                                             const double *__restrict__ cunit,
                                                             const float *__restrict__ aseed,
                                                             const float *__restrict__ cseed, int F, int Ma, int Mc,
                                                             const Levels la, const Levels lc, size_t total)
{
    const size_t stride = (size_t)gridDim.x * NT;
    const float as0 = aseed[0], cs0 = cseed[0];
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += stride) {
        int k = 0;
        while (k + 1 < la.K && i >= la.level[k + 1].sums_offset) ++k;
        const Level &L = la.level[k];
        const size_t local = i - L.sums_offset, per_frame = 2 * (size_t)L.h * L.w;
        const size_t j = (size_t)k * F + local / per_frame;
        const long long a = aacc[i], c = cacc[i];
        aacc[i] = 0;
        cacc[i] = 0;
        const double avalue = (double)a / aunit[j] / (double)Ma;  // the first division is exact
        const double cvalue = (double)c / cunit[j] / (double)Mc;
        L.grad_flow[local] = (as0 * L.weight) * (float)avalue;
        lc.level[k].grad_flow[local] = (cs0 * lc.level[k].weight) * (float)cvalue;
    }
}

// the workspace as byte offsets, in the order of the header
struct JointLayout {
    size_t s, base, asums, csums, count, zeroed_bytes, T, D, arec, aunit, crec, cunit, rows, part, bytes;
    size_t sums_elems;
};

// of tables the calls accept
JointLayout joint_layout(int F, const Plan &pa, const Plan &pc, const Levels &la)
{
    size_t pixels = 0;
    int nb = 0;
    for (int k = 0; k < la.K; ++k) {
        pixels += (size_t)la.level[k].h * la.level[k].w;
        const int need = partial_blocks(la.level[k].h, la.level[k].w);
        nb = need > nb ? need : nb;
    }
    const size_t P = (size_t)pa.M * pixels, K = (size_t)la.K;
    JointLayout o;
    o.sums_elems = 2 * (size_t)F * pixels;
    o.s = sizeof(int64_t) * P;
    o.base = o.s + sizeof(int64_t) * P;
    o.asums = o.base + sizeof(int64_t) * P;
    o.csums = o.asums + sizeof(int64_t) * o.sums_elems;
    o.count = o.csums + sizeof(int64_t) * o.sums_elems;
    o.zeroed_bytes = o.count + sizeof(uint32_t) * P;
    o.T = (o.zeroed_bytes + 7) / 8 * 8;
    o.D = o.T + sizeof(double) * P;
    o.arec = o.D + sizeof(double) * P;
    o.aunit = o.arec + sizeof(ImageRec) * K * pa.M;
    o.crec = o.aunit + sizeof(double) * K * F;
    o.cunit = o.crec + sizeof(ContrastRec) * K * pc.M;
    o.rows = o.cunit + sizeof(double) * K * F;
    o.part = o.rows + sizeof(JointRow) * K * pa.M;
    o.bytes = o.part + sizeof(JointRow) * (size_t)pa.M * nb;
    return o;
}

// what the header asks of the two masks and tables beyond each term's own refusals
bool joint_agree(int contrast_mask, int avg_mask, const Levels &lc, const Levels &la)
{
    if ((contrast_mask & ~avg_mask) != 0 || lc.K != la.K) return false;
    for (int k = 0; k < la.K; ++k) {
        const Level &a = la.level[k], &c = lc.level[k];
        if (a.h != c.h || a.w != c.w || a.shift != c.shift || a.flow != c.flow) return false;
    }
    return true;
}

// The refusals both calls share, in the order of the header; couts, aouts: the call's own
// pointers of either term are all there.  DVSOF_OK with F == 0: nothing to do.
template <class Cols>
int joint_check(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F, int h,
                int w, int contrast_mask, int avg_mask, int polarity, const Levels &lc, const Levels &la,
                bool backward, bool couts, bool aouts, const void *workspace, size_t workspace_bytes, Plan &pc,
                Plan &pa, JointLayout &lay)
{
    PyramidLayout own;
    int rc = pyramid_refusals(cols, n_events, frame_ts, frame_sample, F, h, w, contrast_mask, polarity, lc, backward,
                              couts, pc, own);
    if (rc != DVSOF_OK) return rc;
    rc = pyramid_refusals(cols, n_events, frame_ts, frame_sample, F, h, w, avg_mask, polarity, la, backward, aouts,
                          pa, own);
    if (rc != DVSOF_OK || F == 0) return rc;
    if (!joint_agree(contrast_mask, avg_mask, lc, la)) return DVSOF_EINVAL;
    lay = joint_layout(F, pa, pc, la);
    if (!workspace || workspace_bytes < lay.bytes) return DVSOF_ENOSPACE;
    return DVSOF_OK;
}

// dvsof_event_terms_joint_fwd / _bwd on either form of the event columns
template <class Cols>
int joint_fwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F, int h,
              int w, int contrast_mask, int avg_mask, int polarity, const Levels &lc, const Levels &la,
              dvsof_iwe_result_t *result, float *cterms, float *cvalue, float *aterms, float *avalue,
              void *workspace, size_t workspace_bytes, void *stream, const TiledSplat tiled)
{
    if (tiled.mode < -1 || tiled.mode > 1) return DVSOF_EINVAL;
    Plan pc, pa;
    JointLayout lay;
    const int rc = joint_check(cols, n_events, frame_ts, frame_sample, F, h, w, contrast_mask, avg_mask, polarity, lc,
                               la, false, result && cterms && cvalue, aterms && avalue, workspace, workspace_bytes,
                               pc, pa, lay);
    if (rc != DVSOF_OK || F == 0) return rc;
    PyramidTilePlan tp;
    const int by_tiles = pyramid_tile_decide<AvgtsImages>(tiled, F, avg_mask, polarity, h, w, la, n_events, tp);
    if (by_tiles != DVSOF_OK && by_tiles != 1) return by_tiles;
    hipStream_t st = as_stream(stream);
    char *ws = (char *)workspace;
    DVSOF_HIP_TRY((hipError_t)fill_u32(ws, 0u, lay.zeroed_bytes, st));
    if (by_tiles == DVSOF_OK) {
        const AvgtsImages img{(int64_t *)ws, (int64_t *)(ws + lay.s), (int64_t *)(ws + lay.base),
                              (uint32_t *)(ws + lay.count)};
        const int rs = TiledLaunch<AvgtsImages>::pyramid(plain(cols), n_events, frame_ts, frame_sample, F, h, w,
                                                         avg_mask, polarity, la, tp, img, tiled.workspace, st);
        if (rs != DVSOF_OK) return rs;
    } else if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(avgts_splat_kernel, pa, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols, n_events,
                                frame_ts, frame_sample, F, h, w, pa.refs, TableView{la}, (unsigned long long *)ws,
                                (unsigned long long *)(ws + lay.s), (unsigned long long *)(ws + lay.base),
                                (uint32_t *)(ws + lay.count));
        DVSOF_LAUNCH_CHECK();
    }
    // per level with its own nb, as in both terms' calls: that order makes the bytes
    for (int k = 0; k < la.K; ++k) {
        const Level &L = la.level[k];
        const int nb = partial_blocks(L.h, L.w);
        hipLaunchKernelGGL(joint_stats_partial_kernel, dim3((unsigned)nb, (unsigned)pa.M), dim3(NT), 0, st,
                           (const int64_t *)ws + L.image_offset, (const int64_t *)(ws + lay.s) + L.image_offset,
                           (const int64_t *)(ws + lay.base) + L.image_offset,
                           (const uint32_t *)(ws + lay.count) + L.image_offset, L.h, L.w, nb,
                           (JointRow *)(ws + lay.part), (double *)(ws + lay.T) + L.image_offset,
                           (double *)(ws + lay.D) + L.image_offset);
        DVSOF_LAUNCH_CHECK();
        hipLaunchKernelGGL(frame_final_kernel<JointSum>, dim3((unsigned)pa.M), dim3(kWave), 0, st,
                           (const JointRow *)(ws + lay.part), nb, (JointRow *)(ws + lay.rows) + L.row_offset);
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(joint_close_kernel, dim3(1), dim3(kWave), 0, st, (const JointRow *)(ws + lay.rows), F, pa.R,
                       pa.C, joint_subset(contrast_mask, avg_mask), lc, la, (ImageRec *)(ws + lay.arec),
                       (double *)(ws + lay.aunit), (ContrastRec *)(ws + lay.crec), (double *)(ws + lay.cunit), result,
                       cterms, cvalue, aterms, avalue);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

template <class Cols>
int joint_bwd(const Cols &cols, int64_t n_events, const float *frame_ts, const int64_t *frame_sample, int F, int h,
              int w, int contrast_mask, int avg_mask, int polarity, const Levels &lc, const Levels &la,
              void *workspace, size_t workspace_bytes, const float *cseed, const float *aseed, void *stream)
{
    Plan pc, pa;
    JointLayout lay;
    const int rc = joint_check(cols, n_events, frame_ts, frame_sample, F, h, w, contrast_mask, avg_mask, polarity, lc,
                               la, true, cseed != nullptr, aseed != nullptr, workspace, workspace_bytes, pc, pa, lay);
    if (rc != DVSOF_OK || F == 0) return rc;
    hipStream_t st = as_stream(stream);
    char *ws = (char *)workspace;
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(joint_bwd_events_kernel, pa, dim3(event_blocks(n_events)), dim3(NT), 0, st, cols,
                                n_events, frame_ts, frame_sample, F, h, w, pa.refs,
                                joint_subset(contrast_mask, avg_mask), la, (const int64_t *)ws,
                                (const double *)(ws + lay.T), (const double *)(ws + lay.D),
                                (const ImageRec *)(ws + lay.arec), (const double *)(ws + lay.aunit),
                                (const ContrastRec *)(ws + lay.crec), (const double *)(ws + lay.cunit),
                                (unsigned long long *)(ws + lay.asums), (unsigned long long *)(ws + lay.csums));
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(joint_bwd_close_kernel, dim3(event_blocks((int64_t)lay.sums_elems)), dim3(NT), 0, st,
                       (long long *)(ws + lay.asums), (long long *)(ws + lay.csums),
                       (const double *)(ws + lay.aunit), (const double *)(ws + lay.cunit), aseed, cseed, F, pa.M,
                       pc.M, la, lc, lay.sums_elems);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // namespace

extern "C" {

size_t dvsof_event_terms_joint_workspace_bytes(int F, int contrast_mask, int avg_timestamp_mask, int polarity, int h,
                                               int w, dvsof_contrast_levels_t contrast_levels,
                                               dvsof_contrast_levels_t avg_timestamp_levels)
{
    Plan pc, pa;
    PyramidLayout own;
    if (F < 1 || !plan_of(F, contrast_mask, polarity, pc) || !plan_of(F, avg_timestamp_mask, polarity, pa) ||
        !pyramid_layout(F, h, w, pc, contrast_levels, false, own) ||
        !pyramid_layout(F, h, w, pa, avg_timestamp_levels, false, own))
        return 0;
    // the tables' pointers are not looked at here
    for (int k = 0; k < avg_timestamp_levels.K; ++k) contrast_levels.level[k].flow = avg_timestamp_levels.level[k].flow;
    if (!joint_agree(contrast_mask, avg_timestamp_mask, contrast_levels, avg_timestamp_levels)) return 0;
    return joint_layout(F, pa, pc, avg_timestamp_levels).bytes;
}

int dvsof_event_terms_joint_fwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                const int64_t *frame_sample, int F, int h, int w, int contrast_mask,
                                int avg_timestamp_mask, int polarity, dvsof_contrast_levels_t contrast_levels,
                                dvsof_contrast_levels_t avg_timestamp_levels, dvsof_iwe_result_t *contrast_result,
                                float *contrast_terms, float *contrast_value, float *avg_timestamp_terms,
                                float *avg_timestamp_value, void *workspace, size_t workspace_bytes, void *stream,
                                void *tile_workspace, size_t tile_workspace_bytes, int mode)
{
    return joint_fwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w, contrast_mask,
                     avg_timestamp_mask, polarity, contrast_levels, avg_timestamp_levels, contrast_result,
                     contrast_terms, contrast_value, avg_timestamp_terms, avg_timestamp_value, workspace,
                     workspace_bytes, stream, TiledSplat{tile_workspace, tile_workspace_bytes, mode});
}

int dvsof_event_terms_joint_bwd(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                                const int64_t *sample_index, int64_t n_events, const float *frame_ts,
                                const int64_t *frame_sample, int F, int h, int w, int contrast_mask,
                                int avg_timestamp_mask, int polarity, dvsof_contrast_levels_t contrast_levels,
                                dvsof_contrast_levels_t avg_timestamp_levels, void *workspace,
                                size_t workspace_bytes, const float *contrast_seed, const float *avg_timestamp_seed,
                                void *stream)
{
    return joint_bwd(WireColumns{x, y, t, p, sample_index}, n_events, frame_ts, frame_sample, F, h, w, contrast_mask,
                     avg_timestamp_mask, polarity, contrast_levels, avg_timestamp_levels, workspace, workspace_bytes,
                     contrast_seed, avg_timestamp_seed, stream);
}

int dvsof_event_terms_joint_fwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                        const int64_t *sample_event_offsets, int B, int64_t n_events,
                                        const float *frame_ts, const int64_t *frame_sample, int F, int h, int w,
                                        int contrast_mask, int avg_timestamp_mask, int polarity_channels,
                                        dvsof_contrast_levels_t contrast_levels,
                                        dvsof_contrast_levels_t avg_timestamp_levels,
                                        dvsof_iwe_result_t *contrast_result, float *contrast_terms,
                                        float *contrast_value, float *avg_timestamp_terms,
                                        float *avg_timestamp_value, void *workspace, size_t workspace_bytes,
                                        void *stream, void *tile_workspace, size_t tile_workspace_bytes, int mode)
{
    return joint_fwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample, F,
                     h, w, contrast_mask, avg_timestamp_mask, polarity_channels, contrast_levels,
                     avg_timestamp_levels, contrast_result, contrast_terms, contrast_value, avg_timestamp_terms,
                     avg_timestamp_value, workspace, workspace_bytes, stream,
                     TiledSplat{tile_workspace, tile_workspace_bytes, mode});
}

int dvsof_event_terms_joint_bwd_encoded(const int16_t *x, const int16_t *y, const float *t, const uint8_t *polarity,
                                        const int64_t *sample_event_offsets, int B, int64_t n_events,
                                        const float *frame_ts, const int64_t *frame_sample, int F, int h, int w,
                                        int contrast_mask, int avg_timestamp_mask, int polarity_channels,
                                        dvsof_contrast_levels_t contrast_levels,
                                        dvsof_contrast_levels_t avg_timestamp_levels, void *workspace,
                                        size_t workspace_bytes, const float *contrast_seed,
                                        const float *avg_timestamp_seed, void *stream)
{
    return joint_bwd(EncodedColumns{x, y, t, polarity, sample_event_offsets, B}, n_events, frame_ts, frame_sample, F,
                     h, w, contrast_mask, avg_timestamp_mask, polarity_channels, contrast_levels,
                     avg_timestamp_levels, workspace, workspace_bytes, contrast_seed, avg_timestamp_seed, stream);
}

}  // extern "C"
