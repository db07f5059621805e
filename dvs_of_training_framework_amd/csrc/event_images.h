// What the two families of images of warped events share (iwe.hip: the
// validation metric, docs/IWE_SPEC.md sections 8-13; contrast.hip: the training
// term, docs/CONTRAST_SPEC.md sections 11-15): the reference times and
// polarity channels of a call, and what one event does to the images of its
// frame.  Per frame f, reference r and channel c there is an image
// m = (f R + r) C + c of events carried over sig = tau - rho_r, and a count
// image of the channel's events, repeated per reference.  Which events belong
// to a frame is each family's own rule.  Everything here relies on
// -ffp-contract=off.
#pragma once
#include "frame_common.h"

namespace {

constexpr int kMaxRefs = 3;

struct Refs {
    float rho[kMaxRefs];  // ascending; the first R are read
};

struct Plan {
    int R, C, M;
    Refs refs;
};

// false: arguments the calls refuse
inline bool plan_of(int F, int reference_mask, int polarity, Plan &o)
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
#define DVSOF_REFS_POL_DISPATCH(kernel, pl, ...)                                                    \
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

// The channel of event e: 0 without polarity, else the sign of its entry of the
// polarity column; false: p == 0, in neither channel and in no count.
template <bool POL>
__device__ __forceinline__ bool event_channel(const int64_t *__restrict__ pol, int64_t e, int &c)
{
    c = 0;
    if (POL) {
        const int64_t pe = pol[e];
        if (pe == 0) return false;
        c = pe < 0;
    }
    return true;
}

// The image of frame f, reference r and channel c
template <int R, bool POL>
__device__ __forceinline__ size_t image_of(int f, int r, int c)
{
    return ((size_t)f * R + r) * (POL ? 2 : 1) + c;
}

// An event at (xi, yi) = pixel pix inside the frame, of channel c, at tau of
// the window of its frame f, with the flow (u, v) at its own pixel (read once
// for all references): per reference one count (COUNT) and the splat of the
// event carried to that reference.  plane: h w.
template <int R, bool POL, bool COUNT>
__device__ __forceinline__ void splat_event(const Refs &refs, int f, int c, float tau, float u, float v, int64_t xi,
                                            int64_t yi, size_t pix, size_t plane, int h, int w,
                                            unsigned long long *__restrict__ q, uint32_t *__restrict__ count)
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t m = image_of<R, POL>(f, r, c);
        if (COUNT) atomicAdd(count + m * plane + pix, 1u);
        Warp p;
        if (!warp_event_to(tau, refs.rho[r], u, v, xi, yi, h, w, p)) continue;
        splat_corners(p, h, w, q + m * plane);
    }
}

}  // namespace
