// The tiled voxelisers' launch plan and workspace layout, shared by the fixed
// voxeliser (voxel.hip) and the order-independent learned forward
// (learned_voxel.hip): tile geometry, bucket capacity, control words, records
// and overflow list.  Host side only; the kernels live in the two .hip files.
#pragma once
#include "common.h"
#include <stdlib.h>

namespace {

// A tile is 2^lp pixels (lp = 10, or 9 when many bins would not leave room for
// several workgroups' 8-byte accumulators in LDS), 2^lx wide and 2^(lp-lx) high;
// lx is chosen per call (v2_plan): as wide as the frame allows, so that a
// workgroup stores long contiguous runs of every output row it owns.
constexpr int VPX_MAX = 1024;
// events per thread in pass 1: 4 up to ~2 M events, 8 above, 16 from ~3 M (measured, whole
// path, EPT 4 / 8 / 16: 16.8 / 19.2 / 24.7 us at 0.5 M events, 79.0 / 76.4 / 71.3 us at 4.2 M,
// 105.9 / 82.5 / 72.6 us at 4 M events on 512 x 512 x 12)
constexpr int64_t EPT8_FROM = 1 << 21;
// 16 from ~4 M events: half the bucket-cursor atomics, twice as long record runs per tile
constexpr int64_t EPT16_FROM = 3 << 20;
// LDS histogram + base of the bucket pass: 8 bytes per tile.  At 8192 tiles that is 64 KiB dynamic
// + 8 bytes static: measured on gfx950 (160 KiB LDS per workgroup), the launch needs no raised
// dynamic-LDS limit (tests/test_gpu_voxel_exact.py, tiles8192)
constexpr int V2_MAX_TILES = 8192;

struct VoxV2 {
    // wire format (int64 columns) ...
    const int64_t *x, *y, *pol, *sample;
    // ... or the reference's encoded columns (utils/dataset.py:286-289):
    // int16 x, int16 y, bool polarity; the sample of event i is found in
    // ev_off[B+1] (first event of every sample)
    const int16_t *x16, *y16;
    const uint8_t *p8;
    const int64_t *ev_off;
    int enc;
    const float *t, *t0, *t1;
    int64_t n;
    int B, C, H, W, TX, TY, ntile, cap, lx, lp;   // lx = log2(tile width), lp = log2(tile pixels)
    int32_t *cursor;      // [ntile] events reserved per tile (may exceed cap)
    int32_t *ovf_count;   // [1] overflow records
    int32_t *ovf_tiles;   // [1] tiles whose bucket overflowed
    int32_t *done;        // [1] of those, finished
    uint2 *records;       // [ntile][cap]
    int4 *ovf;            // [n]  {tile, key, bits(frac), 0}
    int64_t ovf_cap;
    float *out;
    int32_t *bin0;
    int64_t *lin0;
};

inline bool v2_plan(int64_t n, int B, int C, int H, int W, VoxV2 &P)
{
    // tile: 1024 pixels, or 512 when C 8-byte accumulators per pixel would leave
    // fewer than three workgroups per CU (160 KiB LDS)
    const int lp = (size_t)C * 1024 * 8 > 52 * 1024 ? 9 : 10;
    P.lp = lp;
    // tile width 2^lx, 64 <= 2^lx <= 2^lp: the widest one whose column padding
    // (TX * 2^lx - W) stays within an eighth of the frame, else the one with
    // the least padding (640 -> 128, 346 -> 128, 256 -> 256, 512 -> 512)
    int lx = 6, best_pad = 1 << 30;
    for (int c = 6; c <= lp; ++c) {
        const int wd = 1 << c, padded = (W + wd - 1) / wd * wd;
        if (padded * 8 <= W * 9) {
            lx = c;             // within 12.5 %: wider is better
            best_pad = 0;
        } else if (best_pad && padded - W < best_pad) {
            best_pad = padded - W;
            lx = c;
        }
    }
    P.lx = lx;
    const int vtx = 1 << lx, vty = 1 << (lp - lx);
    P.TX = (W + vtx - 1) / vtx;
    P.TY = (H + vty - 1) / vty;
    const int64_t nt = (int64_t)B * P.TX * P.TY;
    if (nt > V2_MAX_TILES || ((size_t)C << lp) * 8 > 150 * 1024 || C > 1023) return false;
    P.ntile = (int)nt;
    int64_t cap = 2 * (n / nt) + 256;
    cap = (cap + 63) / 64 * 64;
    if (cap > (1 << 24)) return false;
    P.cap = (int)cap;
    P.ovf_cap = n;
    return true;
}

inline size_t v2_control_bytes(const VoxV2 &P) { return (((size_t)P.ntile + 3) * 4 + 255) / 256 * 256; }

inline size_t v2_bytes(const VoxV2 &P, int64_t n)
{
    return v2_control_bytes(P) + (size_t)P.ntile * P.cap * 8 + (size_t)n * 16 + 256;
}

// control words first (that is the region DVSOF_VOX_WS_CLEAN speaks about)
inline void v2_bind(VoxV2 &P, void *workspace)
{
    unsigned char *w = (unsigned char *)workspace;
    P.cursor = (int32_t *)w;
    P.ovf_count = P.cursor + P.ntile;
    P.ovf_tiles = P.ovf_count + 1;
    P.done = P.ovf_count + 2;
    w += v2_control_bytes(P);
    P.records = (uint2 *)w;
    w += (size_t)P.ntile * P.cap * 8;
    P.ovf = (int4 *)(((uintptr_t)w + 15) & ~(uintptr_t)15);
}

}  // namespace
