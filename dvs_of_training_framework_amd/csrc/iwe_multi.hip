// The image of warped events of iwe.hip at several reference times of the
// window and with ON and OFF events accumulated apart (docs/IWE_SPEC.md
// sections 8-13): the validation side of contrast_multi.hip.  Per frame f,
// reference r and channel c there is an image m = (f R + r) C + c of events
// carried over sig = tau - rho_r, and the count image of the channel's events,
// repeated per reference, so that dvsof_iwe_stats and dvsof_iwe_render take
// the M images as M frames.
//
// Replaces nothing of the reference: its test.py needs ground truth.
//
// Which events belong to a frame is iwe.hip's rule (the position in the
// columns against frame_event_begin), the images are contrast_multi.hip's
// (warp_event_to and splat_corners of frame_common.h).  One thread per event
// reads the flow at its pixel once and issues R 32-bit count atomics and up to
// 4 R 64-bit integer atomics: the sums have no order, the same events give the
// same bytes in any order, in a batch or alone.  No floating-point atomics, no
// LDS.  This file relies on -ffp-contract=off.
#include "frame_common.h"
#include "../../include/dvsof_iwe_multi.h"

namespace {

constexpr int NT = kFrameNT;
constexpr int kMaxRefs = 3;

struct Refs {
    float rho[kMaxRefs];  // ascending; the first R are read
};

struct Plan {
    int R, C, M;
    Refs refs;
};

template <int R, bool POL>
__global__ __launch_bounds__(NT) void iwe_splat_multi_kernel(
    const int64_t *__restrict__ x, const int64_t *__restrict__ y, const float *__restrict__ t,
    const int64_t *__restrict__ pol, int64_t n, const int64_t *__restrict__ begin, const float *__restrict__ ts,
    const float *__restrict__ flow, int F, int h, int w, Refs refs, unsigned long long *__restrict__ q,
    uint32_t *__restrict__ count)
{
    constexpr int C = POL ? 2 : 1;
    const size_t plane = (size_t)h * w;
    for_each_frame_event(n, begin, F, [=](int64_t e, int f) {
        const int64_t xi = x[e], yi = y[e];
        if (xi < 0 || xi >= w || yi < 0 || yi >= h) return;  // the -1 slots of cropped and padded events
        int c = 0;
        if (POL) {
            const int64_t pe = pol[e];
            if (pe == 0) return;  // in neither channel and in no count
            c = pe < 0;
        }
        const size_t pix = (size_t)yi * w + (size_t)xi;
        const float tau = event_tau(t[e], ts[2 * f], ts[2 * f + 1]);
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
    });
}

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
    if (F < 0 || F > kMaxFrames) return false;
    o.M = F * o.R * o.C;
    return o.M <= kMaxFrames;  // the images ride in gridDim.y of the statistics
}

// kernel<R, POL> for the plan's R and C
#define DVSOF_IWE_MULTI_DISPATCH(kernel, pl, ...)                                                   \
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
    DVSOF_IWE_MULTI_DISPATCH(iwe_splat_multi_kernel, pl, dim3(event_blocks(n_events)), dim3(NT), 0, st, x, y, t, p,
                             n_events, frame_event_begin, frame_ts, flow, F, h, w, pl.refs,
                             (unsigned long long *)q, count);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
