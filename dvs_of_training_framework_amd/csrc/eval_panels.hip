// Evaluation panels on the device (docs/EVAL_PANELS_SPEC.md): per frame one
// picture of four panels, events over the grey image | prediction | ground
// truth | endpoint error, prediction and ground truth on one colour scale.
//
// Replaces nothing the reference draws: its test.py reports two numbers per
// sequence.  The counted-pixel predicate and the endpoint error are those of
// dvsof_flow_error (frame_common.h), the flow colours those of
// flow_render_kernel (render.hip, through render_common.h).
//
// Two launches whatever the number of frames: per (frame, chunk) partial
// statistics, then one workgroup per (frame, panel, chunk) that reduces the
// at most 64 partials of its frame and writes BGR bytes straight into the
// picture.  Both are HBM-bound and small.  Integers and min / max only in the
// statistics; this file relies on -ffp-contract=off.
#include "render_common.h"

static_assert(sizeof(dvsof_eval_panel_stats_t) == 32, "stats rows are 32 bytes (visualization.py reads them as such)");

namespace {

constexpr int NT = kRenderNT;
constexpr int kMaxChunks = kRenderMaxChunks;
constexpr int kPanels = 4;

// The stats row is the accumulator.  mag >= +0 for finite components (never NaN), so fminf / fmaxf
// select the same bits in any order.
struct PanelSum {
    using Row = dvsof_eval_panel_stats_t;
    static __device__ __forceinline__ Row zero()
    {
        return Row{__builtin_inff(), -__builtin_inff(), 0, __builtin_inff(), -__builtin_inff(), 0, 0, 0};
    }
    static __device__ __forceinline__ Row add(const Row &a, const Row &b)
    {
        return Row{fminf(a.pred_lo, b.pred_lo), fmaxf(a.pred_hi, b.pred_hi), a.pred_nonfinite + b.pred_nonfinite,
                   fminf(a.gt_lo, b.gt_lo), fmaxf(a.gt_hi, b.gt_hi), a.gt_nonfinite + b.gt_nonfinite,
                   a.n_counted + b.n_counted, a.n_below + b.n_below};
    }
};

// What one frame's panels read.  counted = max_row * w: rows below max_row are the first
// max_row * w pixels of a plane.
struct Frame {
    const float *pu, *pv, *gu, *gv;
    const uint32_t *on, *off;  // NULL: dense
    int counted;
    // whether dvsof_flow_error counts pixel p, and its endpoint error
    __device__ __forceinline__ bool counts(int p, float *ee) const
    {
        if (p >= counted || (on && (on[p] | off[p]) == 0u)) return false;
        const float tu = gu[p], tv = gv[p];
        if (!gt_counts(tu, tv)) return false;
        *ee = endpoint_error(tu, tv, pu[p], pv[p]);
        return true;
    }
};
__device__ __forceinline__ Frame frame_of(const float *pred, const float *gt_u, const float *gt_v,
                                          const uint32_t *count2, int f, int h, int w, int max_row)
{
    const size_t n = (size_t)h * w;
    Frame fr;
    fr.pu = pred + (size_t)f * 2 * n;
    fr.pv = fr.pu + n;
    fr.gu = gt_u + (size_t)f * n;
    fr.gv = gt_v + (size_t)f * n;
    fr.on = count2 ? count2 + (size_t)f * 2 * n : nullptr;
    fr.off = count2 ? fr.on + n : nullptr;
    fr.counted = max_row * w;
    return fr;
}

// ---------------------------------------------------------------------------
// Launch 1: block (frame f, chunk c) = blockIdx.x / chunks, blockIdx.x % chunks.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void eval_panels_stats_kernel(
    const float *__restrict__ pred, const float *__restrict__ gt_u, const float *__restrict__ gt_v,
    const uint32_t *__restrict__ count2, int h, int w, int max_row, int step, int chunks,
    dvsof_eval_panel_stats_t *__restrict__ part)
{
    const int f = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const Frame fr = frame_of(pred, gt_u, gt_v, count2, f, h, w, max_row);
    const int row0 = c * step, rows = min(step, h - row0);
    const int p0 = row0 * w, p1 = p0 + rows * w;  // <= kMaxSide^2 < 2^31
    dvsof_eval_panel_stats_t a = PanelSum::zero();
    for (int p = p0 + threadIdx.x; p < p1; p += NT) {
        const float qu = fr.pu[p], qv = fr.pv[p], tu = fr.gu[p], tv = fr.gv[p];
        if (finite2(qu, qv)) {
            const float mag = sqrtf(qu * qu + qv * qv);
            a.pred_lo = fminf(a.pred_lo, mag);
            a.pred_hi = fmaxf(a.pred_hi, mag);
        } else {
            ++a.pred_nonfinite;
        }
        if (finite2(tu, tv)) {
            const float mag = sqrtf(tu * tu + tv * tv);
            a.gt_lo = fminf(a.gt_lo, mag);
            a.gt_hi = fmaxf(a.gt_hi, mag);
        } else {
            ++a.gt_nonfinite;
        }
        float ee;
        if (fr.counts(p, &ee)) {
            a.n_counted += 1;
            a.n_below += ee < 3.f ? 1 : 0;
        }
    }
    a = block_tree<PanelSum>(a);
    if (threadIdx.x == 0) part[(size_t)f * kMaxChunks + c] = a;
}

// ---------------------------------------------------------------------------
// Launch 2: block ((f * 4 + panel) * chunks + c).
// ---------------------------------------------------------------------------
struct EventsColour {
    const uint32_t *on, *off;  // NULL: no events
    const uint8_t *grey;       // NULL: black
    uint32_t gain;
    __device__ __forceinline__ Bgr operator()(size_t p) const
    {
        const uint32_t n_on = on ? on[p] : 0u, n_off = on ? off[p] : 0u;
        if ((n_on | n_off) == 0u) {
            const uint32_t g = grey ? grey[p] : 0u;
            return Bgr{g, g, g};
        }
        return Bgr{min(255u, min(n_off, 255u) * gain), 0u, min(255u, min(n_on, 255u) * gain)};
    }
};
struct ErrorColour {
    Frame fr;
    float scale;  // 255 / err_max
    __device__ __forceinline__ Bgr operator()(size_t p) const
    {
        float ee;
        if (!fr.counts((int)p, &ee)) return Bgr{64u, 64u, 64u};
        // fminf returns the other operand for a NaN: a NaN error draws at the maximum
        const int t3 = 3 * (int)truncf(fminf(ee * scale, 255.0f));
        return Bgr{(uint32_t)min(max(t3 - 510, 0), 255), (uint32_t)min(max(t3 - 255, 0), 255),
                   (uint32_t)min(t3, 255)};
    }
};

__global__ __launch_bounds__(NT) void eval_panels_kernel(
    const float *__restrict__ pred, const float *__restrict__ gt_u, const float *__restrict__ gt_v,
    const uint32_t *__restrict__ count2, const uint8_t *__restrict__ frames, int h, int w, int max_row,
    float flow_scale, float err_max, int gain, int step, int chunks,
    const dvsof_eval_panel_stats_t *__restrict__ part, uint8_t *__restrict__ canvas, int64_t frame_stride,
    int64_t row_stride, dvsof_eval_panel_stats_t *__restrict__ stats)
{
    const int c = blockIdx.x % chunks, fk = blockIdx.x / chunks;
    const int f = fk / kPanels, panel = fk % kPanels;
    const Frame fr = frame_of(pred, gt_u, gt_v, count2, f, h, w, max_row);
    dvsof_render_item_t it = {};
    it.dst_offset = (int64_t)f * frame_stride;
    it.dst_stride = row_stride;
    it.h = h;
    it.w = w;
    it.x0 = panel * w;
    it.row0 = c * step;
    it.rows = min(step, h - it.row0);
    if (panel == 0) {
        emit_rows(it, canvas, EventsColour{fr.on, fr.off, frames ? frames + (size_t)f * h * w : nullptr, (uint32_t)gain});
        return;
    }
    if (panel == 3) {
        emit_rows(it, canvas, ErrorColour{fr, 255.0f / err_max});
        return;
    }
    // the partials of this frame: at most 64 uniform loads, the same in every lane
    dvsof_eval_panel_stats_t a = PanelSum::zero();
    const dvsof_eval_panel_stats_t *mine = part + (size_t)f * kMaxChunks;
    for (int k = 0; k < chunks; ++k) a = PanelSum::add(a, mine[k]);
    if (panel == 1 && c == 0 && threadIdx.x == 0) stats[f] = a;
    const float m = flow_scale > 0.f ? flow_scale : (__builtin_isfinite(a.gt_hi) && a.gt_hi > 0.f ? a.gt_hi : a.pred_hi);
    FlowColour colour;
    if (panel == 1) {
        colour.fx = fr.pu;
        colour.fy = fr.pv;
        colour.set_scale(a.pred_lo, a.pred_hi, m);
    } else {
        colour.fx = fr.gu;
        colour.fy = fr.gv;
        colour.set_scale(a.gt_lo, a.gt_hi, m);
    }
    emit_rows(it, canvas, colour);
}

bool bad_sources(const float *pred, const float *gt_u, const float *gt_v, int F, int h, int w, int max_row)
{
    return !pred || !gt_u || !gt_v || bad_frame_sizes(F, h, w) || max_row < 0 || max_row > h;
}

}  // namespace

extern "C" {

size_t dvsof_eval_panels_workspace_bytes(int F)
{
    if (F < 1) return 0;
    return sizeof(dvsof_eval_panel_stats_t) * (size_t)F * kMaxChunks;
}

int dvsof_eval_panels_stats(const float *pred, const float *gt_u, const float *gt_v, const uint32_t *count2,
                            int F, int h, int w, int max_row, void *workspace, size_t workspace_bytes,
                            void *stream)
{
    if (F < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_sources(pred, gt_u, gt_v, F, h, w, max_row)) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_eval_panels_workspace_bytes(F)) return DVSOF_ENOSPACE;
    const int step = chunk_rows(h, w), chunks = (h + step - 1) / step;
    hipLaunchKernelGGL(eval_panels_stats_kernel, dim3((unsigned)F * chunks), dim3(NT), 0, as_stream(stream), pred,
                       gt_u, gt_v, count2, h, w, max_row, step, chunks, (dvsof_eval_panel_stats_t *)workspace);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_eval_panels(const float *pred, const float *gt_u, const float *gt_v, const uint32_t *count2,
                      const uint8_t *frames, int F, int h, int w, int max_row, float flow_scale, float err_max,
                      int gain, const void *workspace, size_t workspace_bytes, uint8_t *canvas,
                      size_t canvas_bytes, int64_t frame_stride, int64_t row_stride,
                      dvsof_eval_panel_stats_t *stats, void *stream)
{
    if (F < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_sources(pred, gt_u, gt_v, F, h, w, max_row) || !canvas || !stats) return DVSOF_EINVAL;
    if (!(err_max > 0.f) || !__builtin_isfinite(err_max) || gain < 1 || gain > 255) return DVSOF_EINVAL;
    // every picture inside the canvas, none on another (all terms < 2^63: the strides are bounded first)
    if (row_stride < (int64_t)kPanels * 3 * w || row_stride > (int64_t)1 << 40) return DVSOF_EINVAL;
    if (F > 1 && (frame_stride < (int64_t)h * row_stride || frame_stride > (int64_t)1 << 56)) return DVSOF_EINVAL;
    const unsigned __int128 end = (unsigned __int128)(F > 1 ? (uint64_t)frame_stride : 0u) * (uint64_t)(F - 1) +
                                  (uint64_t)(h - 1) * (uint64_t)row_stride + (uint64_t)kPanels * 3u * (uint64_t)w;
    if (end > (unsigned __int128)canvas_bytes) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_eval_panels_workspace_bytes(F)) return DVSOF_ENOSPACE;
    const int step = chunk_rows(h, w), chunks = (h + step - 1) / step;
    hipLaunchKernelGGL(eval_panels_kernel, dim3((unsigned)F * kPanels * chunks), dim3(NT), 0, as_stream(stream),
                       pred, gt_u, gt_v, count2, frames, h, w, max_row, flow_scale, err_max, gain, step, chunks,
                       (const dvsof_eval_panel_stats_t *)workspace, canvas, F > 1 ? frame_stride : (int64_t)0,
                       row_stride, stats);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
