// Image of warped events and its flow warp loss on the device
// (docs/IWE_SPEC.md): every event of a window is moved along the predicted
// flow to the start of the window and splatted bilinearly; the variance of
// that image over the variance of the unwarped count image says whether the
// flow sharpens the events it was computed from (Stoffregen et al., ECCV 2020).
//
// Replaces nothing of the reference: its test.py needs ground truth.
//
// The splat is a scatter with collisions on almost every pixel.  Weights are
// 64-bit fixed point (2^-32), so the sums have no order: the same events give
// the same bytes in any order, in a batch or alone.  One thread per event and
// four integer atomics, the structure of the learnable layer's small-input
// path; no tiled LDS pass (a validation batch is a few hundred thousand
// events).  The frame search, the warp, the splat and the fixed-order
// reduction of the statistics are those of frame_common.h.
//
// The same kernel splats at several reference times of the window and with ON
// and OFF events accumulated apart (docs/IWE_SPEC.md sections 8-13; the images
// are those of event_images.h, which contrast.hip shares): it then writes the
// count image of every channel too, repeated per reference, so that
// dvsof_iwe_stats and dvsof_iwe_render take the M images as M frames.
//
// Beside the flow warp loss, the ratio of squared average timestamps
// (docs/IWE_SPEC.md sections 14-21, include/dvsof_iwe_avg_timestamp.h): the
// same events by the same frame rule, what each does to q, s, base and count
// and the statistics of an image those of the training term
// (avg_timestamp_images.h, which avg_timestamp.hip shares), so that one splat
// serves both metrics.
// This file relies on -ffp-contract=off.
#include "render_common.h"
#include "avg_timestamp_images.h"
#include "../../include/dvsof_iwe_multi.h"
#include "../../include/dvsof_iwe_avg_timestamp.h"

static_assert(sizeof(dvsof_iwe_result_t) == 48, "result rows are 48 bytes (eval.py reads them as such)");

namespace {

constexpr int NT = kFrameNT;
constexpr int kPanels = 2;

// ---------------------------------------------------------------------------
// Splat.  One thread per event of a frame: it reads the flow at its pixel once
// and issues, per reference, one 32-bit count atomic (COUNT) and up to four
// 64-bit integer atomics (splat_event of event_images.h).
// ---------------------------------------------------------------------------
template <int R, bool POL, bool COUNT = true>
__global__ __launch_bounds__(NT) void iwe_splat_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t,
    const int64_t *__restrict__ pol, int64_t n, const int64_t *__restrict__ begin, const float *__restrict__ ts,
    const float *__restrict__ flow, int F, int h, int w, Refs refs, unsigned long long *__restrict__ q,
    uint32_t *__restrict__ count)
{
    const size_t plane = (size_t)h * w;
    for_each_frame_event(n, begin, F, [=](int64_t e, int f) {
        const int64_t xi = x[e], yi = y[e];
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) return;  // the -1 slots of cropped and padded events
        int c;
        if (!event_channel<POL>(pol, e, c)) return;
        const size_t pix = (size_t)yi * w + (size_t)xi;
        const float tau = event_tau(t[e], ts[2 * f], ts[2 * f + 1]);
        const float *fl = flow + (size_t)f * 2 * plane + pix;
        const float u = fl[0], v = fl[plane];
        splat_event<R, POL, COUNT>(refs, f, c, tau, u, v, xi, yi, pix, plane, h, w, q, count);
    });
}

// The same events by the same rule, each doing to the four average-timestamp
// images what it does in the training term (avgts_splat_event): per reference
// one 32-bit atomic and up to nine 64-bit integer atomics.
template <int R, bool POL>
__global__ __launch_bounds__(NT) void iwe_avgts_splat_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t,
    const int64_t *__restrict__ pol, int64_t n, const int64_t *__restrict__ begin, const float *__restrict__ ts,
    const float *__restrict__ flow, int F, int h, int w, Refs refs, unsigned long long *__restrict__ q,
    unsigned long long *__restrict__ s, unsigned long long *__restrict__ base, uint32_t *__restrict__ count)
{
    const size_t plane = (size_t)h * w;
    for_each_frame_event(n, begin, F, [=](int64_t e, int f) {
        const int64_t xi = x[e], yi = y[e];
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) return;  // the -1 slots of cropped and padded events
        int c;
        if (!event_channel<POL>(pol, e, c)) return;
        const size_t pix = (size_t)yi * w + (size_t)xi;
        const float tau = event_tau(t[e], ts[2 * f], ts[2 * f + 1]);
        const float *fl = flow + (size_t)f * 2 * plane + pix;
        const float u = fl[0], v = fl[plane];
        avgts_splat_event<R, POL>(refs, f, c, tau, u, v, xi, yi, pix, plane, h, w, q, s, base, count);
    });
}

// ---------------------------------------------------------------------------
// Statistics, by the fixed-order reduction of frame_common.h; the result row
// is the accumulator.
// ---------------------------------------------------------------------------
struct IweSum {
    using Row = dvsof_iwe_result_t;
    static __device__ __forceinline__ Row zero() { return Row{0.0, 0, 0, 0, 0, 0}; }
    static __device__ __forceinline__ Row add(const Row &a, const Row &b)
    {
        return Row{a.sum_sq + b.sum_sq, a.sum_q + b.sum_q, a.max_q > b.max_q ? a.max_q : b.max_q,
                   a.count_sum + b.count_sum, a.count_sq + b.count_sq,
                   a.count_max > b.count_max ? a.count_max : b.count_max};
    }
};

__global__ __launch_bounds__(NT) void iwe_stats_partial_kernel(
    const int64_t *__restrict__ q, const uint32_t *__restrict__ count, int h, int w, int nb,
    dvsof_iwe_result_t *__restrict__ part)
{
    const int f = blockIdx.y;
    const int n = h * w;
    const int64_t *qf = q + (size_t)f * n;
    const uint32_t *cf = count + (size_t)f * n;
    frame_partial<IweSum>(n, nb, part, [=](dvsof_iwe_result_t &a, int p) {
        const int64_t Q = qf[p], c = cf[p];
        const double I = (double)Q * 0x1p-32;
        a.sum_sq += I * I;
        a.sum_q += Q;
        a.max_q = a.max_q > Q ? a.max_q : Q;
        a.count_sum += c;
        a.count_sq += c * c;
        a.count_max = a.count_max > c ? a.count_max : c;
    });
}

// ---------------------------------------------------------------------------
// Render.  One workgroup per (frame, panel, chunk of rows): the count image on
// the left, the IWE on the right, each grey on its own scale.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t grey_of(float value, float m)
{
    return m > 0.f ? (uint32_t)min(255, (int)(value / m * 255.f + 0.5f)) : 0u;
}
struct CountGrey {
    const uint32_t *src;
    float m;
    __device__ __forceinline__ Bgr operator()(size_t p) const
    {
        const uint32_t g = grey_of((float)src[p], m);
        return Bgr{g, g, g};
    }
};
struct IweGrey {
    const int64_t *src;
    float m;
    __device__ __forceinline__ Bgr operator()(size_t p) const
    {
        const uint32_t g = grey_of((float)((double)src[p] * 0x1p-32), m);
        return Bgr{g, g, g};
    }
};

__global__ __launch_bounds__(kRenderNT) void iwe_render_kernel(
    const int64_t *__restrict__ q, const uint32_t *__restrict__ count,
    const dvsof_iwe_result_t *__restrict__ result, int h, int w, int step, int chunks,
    uint8_t *__restrict__ canvas)
{
    const int c = blockIdx.x % chunks, fk = blockIdx.x / chunks;
    const int f = fk / kPanels, panel = fk % kPanels;
    const size_t n = (size_t)h * w;
    dvsof_render_item_t it = {};
    it.dst_stride = (int64_t)kPanels * 3 * w;
    it.dst_offset = (int64_t)f * h * it.dst_stride;
    it.h = h;
    it.w = w;
    it.x0 = panel * w;
    it.row0 = c * step;
    it.rows = min(step, h - it.row0);
    if (panel == 0)
        emit_rows(it, canvas, CountGrey{count + (size_t)f * n, (float)result[f].count_max});
    else
        emit_rows(it, canvas, IweGrey{q + (size_t)f * n, (float)((double)result[f].max_q * 0x1p-32)});
}

// The average distance in time at zero flow on the left, after the warp on the
// right, on the fixed scale [0, 1): T < 1 on every pixel.
struct AvgtsGrey {
    const int64_t *q, *s, *base;
    const uint32_t *count;
    bool warped;
    __device__ __forceinline__ Bgr operator()(size_t p) const
    {
        const AvgPixel px = avgts_pixel(q[p], s[p], base[p], count[p]);
        const uint32_t g = grey_of((float)(warped ? px.T : px.T0), 1.f);
        return Bgr{g, g, g};
    }
};

__global__ __launch_bounds__(kRenderNT) void iwe_avgts_render_kernel(
    const int64_t *__restrict__ q, const int64_t *__restrict__ s, const int64_t *__restrict__ base,
    const uint32_t *__restrict__ count, int h, int w, int step, int chunks, uint8_t *__restrict__ canvas)
{
    const int c = blockIdx.x % chunks, mk = blockIdx.x / chunks;
    const int m = mk / kPanels, panel = mk % kPanels;
    const size_t at = (size_t)m * h * w;
    dvsof_render_item_t it = {};
    it.dst_stride = (int64_t)kPanels * 3 * w;
    it.dst_offset = (int64_t)m * h * it.dst_stride;
    it.h = h;
    it.w = w;
    it.x0 = panel * w;
    it.row0 = c * step;
    it.rows = min(step, h - it.row0);
    emit_rows(it, canvas, AvgtsGrey{q + at, s + at, base + at, count + at, panel == 1});
}

// the region of images as byte offsets, in the order of the header
struct AvgtsLayout {
    size_t s, base, count, zeroed_bytes, bytes;
};

AvgtsLayout avgts_layout(int h, int w, const Plan &pl)
{
    const size_t P = (size_t)pl.M * h * w;
    AvgtsLayout o;
    o.s = sizeof(int64_t) * P;
    o.base = o.s + sizeof(int64_t) * P;
    o.count = o.base + sizeof(int64_t) * P;
    o.zeroed_bytes = o.count + sizeof(uint32_t) * P;
    o.bytes = (o.zeroed_bytes + 7) / 8 * 8;
    return o;
}

}  // namespace

extern "C" {

int dvsof_iwe_splat(const int64_t *x, const int64_t *y, const float *t, int64_t n_events,
                    const int64_t *frame_event_begin, const float *frame_ts, const float *flow, int F, int h,
                    int w, int64_t *q, void *stream)
{
    if (F < 0 || n_events < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !frame_event_begin || !frame_ts || !flow) return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || !t)) return DVSOF_EINVAL;
    DVSOF_HIP_TRY((hipError_t)fill_u32(q, 0u, sizeof(int64_t) * (size_t)F * h * w, as_stream(stream)));
    if (n_events == 0) return DVSOF_OK;
    Plan pl;
    (void)plan_of(F, 1, 0, pl);  // the start of the window, the polarities together; no count image
    hipLaunchKernelGGL((iwe_splat_kernel<1, false, false>), dim3(event_blocks(n_events)), dim3(NT), 0,
                       as_stream(stream), x, y, t, (const int64_t *)nullptr, n_events, frame_event_begin, frame_ts,
                       flow, F, h, w, pl.refs, (unsigned long long *)q, (uint32_t *)nullptr);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_iwe_multi_images(int F, int reference_mask, int polarity)
{
    Plan pl;
    return plan_of(F, reference_mask, polarity, pl) ? pl.M : 0;
}

int dvsof_iwe_splat_multi(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                          int64_t n_events, const int64_t *frame_event_begin, const float *frame_ts,
                          const float *flow, int F, int h, int w, int reference_mask, int polarity, int64_t *q,
                          uint32_t *count, void *stream)
{
    Plan pl;
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !count || !frame_event_begin || !frame_ts || !flow) return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || !t || (polarity && !p))) return DVSOF_EINVAL;
    hipStream_t st = as_stream(stream);
    const size_t pixels = (size_t)pl.M * h * w;
    DVSOF_HIP_TRY((hipError_t)fill_u32(q, 0u, sizeof(int64_t) * pixels, st));
    DVSOF_HIP_TRY((hipError_t)fill_u32(count, 0u, sizeof(uint32_t) * pixels, st));
    if (n_events == 0) return DVSOF_OK;
    DVSOF_REFS_POL_DISPATCH(iwe_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, x, y, t, p,
                            n_events, frame_event_begin, frame_ts, flow, F, h, w, pl.refs,
                            (unsigned long long *)q, count);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

size_t dvsof_iwe_stats_workspace_bytes(int F, int h, int w)
{
    if (F < 1 || bad_frame_sizes(F, h, w)) return 0;
    return sizeof(dvsof_iwe_result_t) * (size_t)F * partial_blocks(h, w);
}

int dvsof_iwe_stats(const int64_t *q, const uint32_t *count, int F, int h, int w, dvsof_iwe_result_t *result,
                    void *workspace, size_t workspace_bytes, void *stream)
{
    if (F < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !count || !result) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_iwe_stats_workspace_bytes(F, h, w)) return DVSOF_ENOSPACE;
    const int nb = partial_blocks(h, w);
    dvsof_iwe_result_t *part = (dvsof_iwe_result_t *)workspace;
    hipLaunchKernelGGL(iwe_stats_partial_kernel, dim3((unsigned)nb, (unsigned)F), dim3(NT), 0, as_stream(stream),
                       q, count, h, w, nb, part);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_final_kernel<IweSum>, dim3((unsigned)F), dim3(kWave), 0, as_stream(stream), part, nb,
                       result);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_iwe_render(const int64_t *q, const uint32_t *count, const dvsof_iwe_result_t *result, int F, int h,
                     int w, uint8_t *canvas, void *stream)
{
    if (F < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !q || !count || !result || !canvas) return DVSOF_EINVAL;
    const int step = chunk_rows(h, w), chunks = (h + step - 1) / step;
    hipLaunchKernelGGL(iwe_render_kernel, dim3((unsigned)F * kPanels * chunks), dim3(kRenderNT), 0,
                       as_stream(stream), q, count, result, h, w, step, chunks, canvas);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

size_t dvsof_iwe_avg_timestamp_image_bytes(int F, int h, int w, int reference_mask, int polarity)
{
    Plan pl;
    if (F < 1 || bad_frame_sizes(F, h, w) || !plan_of(F, reference_mask, polarity, pl)) return 0;
    return avgts_layout(h, w, pl).bytes;
}

size_t dvsof_iwe_avg_timestamp_workspace_bytes(int F, int h, int w, int reference_mask, int polarity)
{
    Plan pl;
    if (F < 1 || bad_frame_sizes(F, h, w) || !plan_of(F, reference_mask, polarity, pl)) return 0;
    return sizeof(StatRow) * (size_t)pl.M * partial_blocks(h, w);
}

int dvsof_iwe_avg_timestamp(const int64_t *x, const int64_t *y, const float *t, const int64_t *p,
                            int64_t n_events, const int64_t *frame_event_begin, const float *frame_ts,
                            const float *flow, int F, int h, int w, int reference_mask, int polarity, void *images,
                            size_t image_bytes, void *rows, void *workspace, size_t workspace_bytes, void *stream)
{
    Plan pl;
    if (F < 0 || n_events < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !images || !rows || !frame_event_begin || !frame_ts || !flow)
        return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || !t || (polarity && !p))) return DVSOF_EINVAL;
    const AvgtsLayout lay = avgts_layout(h, w, pl);
    const int nb = partial_blocks(h, w);
    if (image_bytes < lay.bytes) return DVSOF_ENOSPACE;
    if (!workspace || workspace_bytes < sizeof(StatRow) * (size_t)pl.M * nb) return DVSOF_ENOSPACE;
    hipStream_t st = as_stream(stream);
    char *im = (char *)images;
    DVSOF_HIP_TRY((hipError_t)fill_u32(im, 0u, lay.zeroed_bytes, st));
    if (n_events > 0) {
        DVSOF_REFS_POL_DISPATCH(iwe_avgts_splat_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, x, y, t,
                                p, n_events, frame_event_begin, frame_ts, flow, F, h, w, pl.refs,
                                (unsigned long long *)im, (unsigned long long *)(im + lay.s),
                                (unsigned long long *)(im + lay.base), (uint32_t *)(im + lay.count));
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(avgts_stats_partial_kernel, dim3((unsigned)nb, (unsigned)pl.M), dim3(NT), 0, st,
                       (const int64_t *)im, (const int64_t *)(im + lay.s), (const int64_t *)(im + lay.base),
                       (const uint32_t *)(im + lay.count), h, w, nb, (StatRow *)workspace);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_final_kernel<AvgSum>, dim3((unsigned)pl.M), dim3(kWave), 0, st,
                       (const StatRow *)workspace, nb, (StatRow *)rows);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_iwe_avg_timestamp_render(const void *images, int F, int h, int w, int reference_mask, int polarity,
                                   uint8_t *canvas, void *stream)
{
    Plan pl;
    if (F < 0 || !plan_of(F, reference_mask, polarity, pl)) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_frame_sizes(F, h, w) || !images || !canvas) return DVSOF_EINVAL;
    const AvgtsLayout lay = avgts_layout(h, w, pl);
    const char *im = (const char *)images;
    const int step = chunk_rows(h, w), chunks = (h + step - 1) / step;
    hipLaunchKernelGGL(iwe_avgts_render_kernel, dim3((unsigned)pl.M * kPanels * chunks), dim3(kRenderNT), 0,
                       as_stream(stream), (const int64_t *)im, (const int64_t *)(im + lay.s),
                       (const int64_t *)(im + lay.base), (const uint32_t *)(im + lay.count), h, w, step, chunks,
                       canvas);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
