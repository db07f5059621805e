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
// events).  The statistics follow dvsof_flow_error's fixed-order reduction.
// This file relies on -ffp-contract=off.
#include "render_common.h"

static_assert(sizeof(dvsof_iwe_result_t) == 48, "result rows are 48 bytes (eval.py reads them as such)");

namespace {

constexpr int NT = 256;
constexpr int kMaxStatBlocks = 128;  // partials per frame: two per lane of the closing wave
constexpr int kMaxSide = kRenderMaxSide;
constexpr int kMaxFrames = 65535;  // as dvsof_flow_error
constexpr int kPanels = 2;
constexpr float kOne = 4294967296.f;  // 2^32: the fixed-point unit

// ---------------------------------------------------------------------------
// Splat.  One thread per event; the frame of event e is the last f with
// begin[f] <= e (count_image_batched_kernel's search).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void iwe_splat_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t, int64_t n,
    const int64_t *__restrict__ begin, const float *__restrict__ ts, const float *__restrict__ flow, int F,
    int h, int w, unsigned long long *__restrict__ q)
{
    const int64_t stride = (int64_t)gridDim.x * NT;
    const int64_t first = begin[0], last = begin[F];
    const size_t plane = (size_t)h * w;
    const float fw = (float)w, fh = (float)h;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n; e += stride) {
        if (e < first || e >= last) continue;
        int lo = 0, hi = F;  // begin[lo] <= e < begin[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (begin[mid] <= e) lo = mid; else hi = mid;
        }
        const int64_t xi = x[e], yi = y[e];
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) continue;  // the -1 slots of cropped and padded events
        const float t0 = ts[2 * lo], d = ts[2 * lo + 1] - t0;
        const float tau = d > 0.f ? fminf(fmaxf((t[e] - t0) / d, 0.f), 1.f) : 0.f;
        const float *fl = flow + (size_t)lo * 2 * plane + (size_t)yi * w + (size_t)xi;
        const float u = fl[0], v = fl[plane];
        const float xw = (float)xi - tau * u, yw = (float)yi - tau * v;
        // in float, before any conversion: false for a NaN, an infinity, 1e30
        if (!(xw > -1.f && xw < fw && yw > -1.f && yw < fh)) continue;
        const float flx = floorf(xw), fly = floorf(yw);  // in [-1, side - 1]
        const float fx = xw - flx, fy = yw - fly;
        const float wx[2] = {1.f - fx, fx}, wy[2] = {1.f - fy, fy};
        const int cx = (int)flx, cy = (int)fly;
        unsigned long long *img = q + (size_t)lo * plane;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int xx = cx + i, yy = cy + j;
                if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
                const int64_t Q = (int64_t)(wy[j] * wx[i] * kOne);  // truncates; 0 <= Q <= 2^32
                if (Q > 0) atomicAdd(img + (size_t)yy * w + (size_t)xx, (unsigned long long)Q);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Statistics.  Fixed-order reduction: thread (strided pixels, ascending)
// -> wave (shuffle tree) -> block (waves 0..3) -> frame (partials ascending).
// ---------------------------------------------------------------------------
struct Acc {
    double sq;
    long long sum, mx, csum, csq, cmx;
};
__device__ __forceinline__ Acc acc_zero() { return Acc{0.0, 0, 0, 0, 0, 0}; }
__device__ __forceinline__ Acc acc_add(const Acc &a, const Acc &b)
{
    return Acc{a.sq + b.sq, a.sum + b.sum, a.mx > b.mx ? a.mx : b.mx, a.csum + b.csum, a.csq + b.csq,
               a.cmx > b.cmx ? a.cmx : b.cmx};
}
// valid in lane 0
__device__ __forceinline__ Acc acc_wave(Acc a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Acc b;
        b.sq = __shfl_down(a.sq, off, kWave);
        b.sum = __shfl_down(a.sum, off, kWave);
        b.mx = __shfl_down(a.mx, off, kWave);
        b.csum = __shfl_down(a.csum, off, kWave);
        b.csq = __shfl_down(a.csq, off, kWave);
        b.cmx = __shfl_down(a.cmx, off, kWave);
        a = acc_add(a, b);
    }
    return a;
}
__device__ __forceinline__ void acc_store(dvsof_iwe_result_t *r, const Acc &a)
{
    r->sum_sq = a.sq;
    r->sum_q = a.sum;
    r->max_q = a.mx;
    r->count_sum = a.csum;
    r->count_sq = a.csq;
    r->count_max = a.cmx;
}

__global__ __launch_bounds__(NT) void iwe_stats_partial_kernel(
    const int64_t *__restrict__ q, const uint32_t *__restrict__ count, int h, int w, int nb,
    dvsof_iwe_result_t *__restrict__ part)
{
    const int f = blockIdx.y, b = blockIdx.x;
    const int n = h * w;
    const int64_t *qf = q + (size_t)f * n;
    const uint32_t *cf = count + (size_t)f * n;
    Acc a = acc_zero();
    for (int p = b * NT + threadIdx.x; p < n; p += nb * NT) {
        const long long Q = qf[p], c = cf[p];
        const double I = (double)Q * 0x1p-32;
        a.sq += I * I;
        a.sum += Q;
        a.mx = a.mx > Q ? a.mx : Q;
        a.csum += c;
        a.csq += c * c;
        a.cmx = a.cmx > c ? a.cmx : c;
    }
    a = acc_wave(a);
    __shared__ Acc sh[NT / kWave];
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        Acc s = sh[0];
#pragma unroll
        for (int k = 1; k < NT / kWave; ++k) s = acc_add(s, sh[k]);
        acc_store(&part[(size_t)f * nb + b], s);
    }
}

__global__ __launch_bounds__(kWave) void iwe_stats_final_kernel(
    const dvsof_iwe_result_t *__restrict__ part, int nb, dvsof_iwe_result_t *__restrict__ result)
{
    const int f = blockIdx.x;
    Acc a = acc_zero();
    for (int k = threadIdx.x; k < nb; k += kWave) {
        const dvsof_iwe_result_t r = part[(size_t)f * nb + k];
        a = acc_add(a, Acc{r.sum_sq, (long long)r.sum_q, (long long)r.max_q, (long long)r.count_sum,
                           (long long)r.count_sq, (long long)r.count_max});
    }
    a = acc_wave(a);
    if (threadIdx.x == 0) acc_store(&result[f], a);
}

int stat_blocks(int h, int w)
{
    const long long n = (long long)h * w;
    const long long nb = (n + 4 * NT - 1) / (4 * NT);  // ~4 pixels per thread
    return (int)(nb < 1 ? 1 : (nb > kMaxStatBlocks ? kMaxStatBlocks : nb));
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

bool bad_sizes(int F, int h, int w)
{
    return F > kMaxFrames || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide;
}

}  // namespace

extern "C" {

int dvsof_iwe_splat(const int64_t *x, const int64_t *y, const float *t, int64_t n_events,
                    const int64_t *frame_event_begin, const float *frame_ts, const float *flow, int F, int h,
                    int w, int64_t *q, void *stream)
{
    if (F < 0 || n_events < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_sizes(F, h, w) || !q || !frame_event_begin || !frame_ts || !flow) return DVSOF_EINVAL;
    if (n_events > 0 && (!x || !y || !t)) return DVSOF_EINVAL;
    DVSOF_HIP_TRY((hipError_t)fill_u32(q, 0u, sizeof(int64_t) * (size_t)F * h * w, as_stream(stream)));
    if (n_events == 0) return DVSOF_OK;
    const int64_t blocks = (n_events + NT - 1) / NT;
    hipLaunchKernelGGL(iwe_splat_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(NT), 0,
                       as_stream(stream), x, y, t, n_events, frame_event_begin, frame_ts, flow, F, h, w,
                       (unsigned long long *)q);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

size_t dvsof_iwe_stats_workspace_bytes(int F, int h, int w)
{
    if (F < 1 || bad_sizes(F, h, w)) return 0;
    return sizeof(dvsof_iwe_result_t) * (size_t)F * stat_blocks(h, w);
}

int dvsof_iwe_stats(const int64_t *q, const uint32_t *count, int F, int h, int w, dvsof_iwe_result_t *result,
                    void *workspace, size_t workspace_bytes, void *stream)
{
    if (F < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_sizes(F, h, w) || !q || !count || !result) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_iwe_stats_workspace_bytes(F, h, w)) return DVSOF_ENOSPACE;
    const int nb = stat_blocks(h, w);
    dvsof_iwe_result_t *part = (dvsof_iwe_result_t *)workspace;
    hipLaunchKernelGGL(iwe_stats_partial_kernel, dim3((unsigned)nb, (unsigned)F), dim3(NT), 0, as_stream(stream),
                       q, count, h, w, nb, part);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(iwe_stats_final_kernel, dim3((unsigned)F), dim3(kWave), 0, as_stream(stream), part, nb,
                       result);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_iwe_render(const int64_t *q, const uint32_t *count, const dvsof_iwe_result_t *result, int F, int h,
                     int w, uint8_t *canvas, void *stream)
{
    if (F < 0) return DVSOF_EINVAL;
    if (F == 0) return DVSOF_OK;
    if (bad_sizes(F, h, w) || !q || !count || !result || !canvas) return DVSOF_EINVAL;
    const int step = chunk_rows(h, w), chunks = (h + step - 1) / step;
    hipLaunchKernelGGL(iwe_render_kernel, dim3((unsigned)F * kPanels * chunks), dim3(kRenderNT), 0,
                       as_stream(stream), q, count, result, h, w, step, chunks, canvas);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
