// Device helpers shared by the renderers (render.hip, eval_panels.hip): the
// colour of a flow pixel (docs/RENDER_SPEC.md section 2) and the row writer
// with its head / aligned-dword-triple / tail stores (section 3).  Everything
// here relies on -ffp-contract=off.
#pragma once
#include "frame_common.h"

namespace {

constexpr int kRenderNT = kFrameNT;
constexpr int kRenderMaxChunks = DVSOF_RENDER_MAX_CHUNKS;
constexpr int kRenderMaxSide = kMaxSide;
constexpr int kRenderChunkPixels = 2048;  // 8 per thread: enough to hide the launch of a workgroup

__device__ __forceinline__ bool finite2(float a, float b)
{
    return __builtin_isfinite(a) && __builtin_isfinite(b);
}

// Three bytes per pixel: a row segment of the destination starts at an
// arbitrary byte, so a row is cut into a head of (address & 3) pixels, after
// which 3 * head more bytes make the address a multiple of 4, groups of
// 4 pixels = three aligned dwords, and a tail of fewer than 4 pixels.  Head
// and tail go out as bytes.  Consecutive threads take consecutive groups: a
// wave's dword stores cover 768 contiguous bytes.
struct Bgr {
    uint32_t b, g, r;
};

// OpenCV's float HSV -> BGR for 8-bit input, hue range 180, S = 255
__device__ __forceinline__ Bgr hsv2bgr(int h, int V)
{
    const int sector = (h / 30) % 6;
    const float f = (float)(h % 30) / 30.0f;
    const float v = (float)V / 255.0f;
    const float tab[4] = {v, 0.f, v * (1.f - f), v * f};
    // {b, g, r} indices into tab, two bits each
    constexpr uint32_t kSector[6] = {1 | 3 << 2 | 0 << 4, 1 | 0 << 2 | 2 << 4, 3 | 0 << 2 | 1 << 4,
                                     0 | 2 << 2 | 1 << 4, 0 | 1 << 2 | 3 << 4, 2 | 1 << 2 | 0 << 4};
    const uint32_t s = kSector[sector];
    auto pick = [&](uint32_t k) -> float { return k == 0 ? tab[0] : (k == 1 ? tab[1] : (k == 2 ? tab[2] : tab[3])); };
    Bgr c;
    c.b = (uint32_t)rintf(pick(s & 3) * 255.0f);
    c.g = (uint32_t)rintf(pick((s >> 2) & 3) * 255.0f);
    c.r = (uint32_t)rintf(pick((s >> 4) & 3) * 255.0f);
    return c;
}

struct FlowColour {
    const float *fx, *fy;  // the image's planes
    float lo, scale, clamp;  // clamp > 0: caller-given scale
    // from the image's own lo / hi, or from a scale m > 0 (lo = 0, hi = m, mag clamped to m)
    __device__ __forceinline__ void set_scale(float own_lo, float own_hi, float m)
    {
        clamp = m > 0.f ? m : 0.f;
        if (m > 0.f) {
            own_lo = 0.f;
            own_hi = m;
        }
        lo = own_lo;
        scale = own_hi - own_lo > 0.f ? 255.0f / (own_hi - own_lo) : 0.f;
    }
    __device__ __forceinline__ Bgr operator()(size_t p) const
    {
        const float x = fx[p], y = fy[p];
        if (!finite2(x, y)) return Bgr{0u, 0u, 0u};
        float mag = sqrtf(x * x + y * y);
        if (clamp > 0.f) mag = fminf(mag, clamp);
        const int V = (int)truncf(fminf((mag - lo) * scale, 255.0f));
        const float a = (atan2f(y, x) + 3.14159265358979323846f) * (float)(180.0 / 3.14159265358979323846 / 2.0);
        return hsv2bgr((int)truncf(a), V);
    }
};
struct GreyColour {
    const uint8_t *src;
    __device__ __forceinline__ Bgr operator()(size_t p) const
    {
        const uint32_t g = src[p];
        return Bgr{g, g, g};
    }
};
struct NoColour {
    __device__ __forceinline__ Bgr operator()(size_t) const { return Bgr{0u, 0u, 0u}; }
};

// Rows [row0, row0 + rows) of an h x w source to pixel (x0, y0 + row0) of the
// destination at canvas + dst_offset; colour(p) is the pixel at offset p of
// the source plane.
template <typename Colour>
__device__ __forceinline__ void emit_rows(const dvsof_render_item_t &it, uint8_t *__restrict__ canvas,
                                          const Colour &colour)
{
    const int units = (it.w + 3) / 4 + 1;  // per row: the head, then groups (the last one may be the tail)
    const int total = it.rows * units;     // < 2^15 * 2^13
    for (int k = threadIdx.x; k < total; k += kRenderNT) {
        const int r = it.row0 + k / units, u = k % units;
        uint8_t *row = canvas + it.dst_offset + (int64_t)(it.y0 + r) * it.dst_stride + 3 * (int64_t)it.x0;
        const int head = min((int)((uintptr_t)row & 3), it.w);
        const int p0 = u == 0 ? 0 : head + 4 * (u - 1);
        const int p1 = u == 0 ? head : min(p0 + 4, it.w);
        if (p0 >= p1) continue;
        const size_t src = (size_t)r * it.w;
        if (p1 - p0 == 4) {  // u >= 1: row + 3 * p0 is a multiple of 4
            const Bgr c0 = colour(src + p0), c1 = colour(src + p0 + 1), c2 = colour(src + p0 + 2),
                      c3 = colour(src + p0 + 3);
            uint32_t *q = (uint32_t *)(row + 3 * (size_t)p0);
            q[0] = c0.b | c0.g << 8 | c0.r << 16 | c1.b << 24;
            q[1] = c1.g | c1.r << 8 | c2.b << 16 | c2.g << 24;
            q[2] = c2.r | c3.b << 8 | c3.g << 16 | c3.r << 24;
        } else {
            for (int p = p0; p < p1; ++p) {
                const Bgr c = colour(src + p);
                row[3 * (size_t)p + 0] = (uint8_t)c.b;
                row[3 * (size_t)p + 1] = (uint8_t)c.g;
                row[3 * (size_t)p + 2] = (uint8_t)c.r;
            }
        }
    }
}

// dvsof_flow_render_chunk_rows; 0 for sides outside [1, kMaxSide]
inline int chunk_rows(int h, int w)
{
    if (h < 1 || w < 1 || h > kRenderMaxSide || w > kRenderMaxSide) return 0;
    const int by_pixels = (kRenderChunkPixels + w - 1) / w, by_count = (h + kRenderMaxChunks - 1) / kRenderMaxChunks;
    return by_pixels > by_count ? by_pixels : by_count;
}

}  // namespace
