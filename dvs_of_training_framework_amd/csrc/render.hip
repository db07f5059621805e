// Predicted flow as a colour image on the device (docs/RENDER_SPEC.md).
//
// Replaces (reference paths): flow2img utils/visualization.py:5-18 (norm,
// arctan2, cv2.normalize, cv2.cvtColor: four passes over host copies of every
// pyramid level of every sample) and the canvas assembly of visualize.py:
// put_image / visualize_prediction / visualize_predictions / join_images
// (:37-127).
//
// Two launches over one host-built item table, whatever the batch and the
// number of levels: per-item min / max / non-finite count, then one workgroup
// per item that reduces the few partials of its image and writes BGR bytes
// straight into the mosaic.  Both are HBM-bound and small.  The arithmetic is
// pinned operation by operation by the spec; this file relies on
// -ffp-contract=off.
#include "render_common.h"

static_assert(sizeof(dvsof_render_item_t) == 64, "items are 64 bytes (visualization.py packs them as such)");
static_assert(sizeof(dvsof_render_stats_t) == 16, "stats rows are 16 bytes (visualization.py reads them as such)");

namespace {

constexpr int NT = kRenderNT;
constexpr int kMaxChunks = kRenderMaxChunks;

// ---------------------------------------------------------------------------
// Launch 1.  mag >= +0 for finite components (never NaN, +inf on overflow), so
// fminf / fmaxf select the same bits in any order.
// ---------------------------------------------------------------------------
struct MagnitudeRange {
    struct Row {
        float lo, hi;
        int bad;
    };
    static __device__ __forceinline__ Row zero() { return Row{__builtin_inff(), -__builtin_inff(), 0}; }
    static __device__ __forceinline__ Row add(const Row &a, const Row &b)
    {
        return Row{fminf(a.lo, b.lo), fmaxf(a.hi, b.hi), a.bad + b.bad};
    }
};

__global__ __launch_bounds__(NT) void flow_render_stats_kernel(
    const dvsof_render_item_t *__restrict__ items, dvsof_render_stats_t *__restrict__ part)
{
    const dvsof_render_item_t it = items[blockIdx.x];
    const size_t plane = (size_t)it.h * it.w;
    const float *fx = (const float *)it.src + (size_t)it.row0 * it.w, *fy = fx + plane;
    const int n = it.rows * it.w;  // <= kMaxSide^2 < 2^31
    MagnitudeRange::Row a = MagnitudeRange::zero();
    for (int p = threadIdx.x; p < n; p += NT) {
        const float x = fx[p], y = fy[p];
        if (finite2(x, y)) {
            const float mag = sqrtf(x * x + y * y);
            a.lo = fminf(a.lo, mag);
            a.hi = fmaxf(a.hi, mag);
        } else {
            ++a.bad;
        }
    }
    a = block_tree<MagnitudeRange>(a);
    if (threadIdx.x == 0) part[(size_t)it.image * kMaxChunks + it.chunk] = dvsof_render_stats_t{a.lo, a.hi, a.bad, 0};
}

// ---------------------------------------------------------------------------
// Launch 2.  The colours and the row stores are those of render_common.h.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void flow_render_kernel(
    const dvsof_render_item_t *__restrict__ items, const dvsof_render_stats_t *__restrict__ part,
    const float *__restrict__ max_magnitude, uint8_t *__restrict__ canvas,
    dvsof_render_stats_t *__restrict__ stats)
{
    const dvsof_render_item_t it = items[blockIdx.x];
    if (it.kind == DVSOF_RENDER_FILL) {
        emit_rows(it, canvas, NoColour{});
        return;
    }
    if (it.kind == DVSOF_RENDER_FRAME) {
        emit_rows(it, canvas, GreyColour{(const uint8_t *)it.src});
        return;
    }
    // the partials of this image: at most 64 uniform loads, the same in every lane
    float lo = __builtin_inff(), hi = -__builtin_inff();
    int bad = 0;
    const dvsof_render_stats_t *mine = part + (size_t)it.image * kMaxChunks;
    for (int c = 0; c < it.chunks; ++c) {
        lo = fminf(lo, mine[c].lo);
        hi = fmaxf(hi, mine[c].hi);
        bad += mine[c].nonfinite;
    }
    if (it.chunk == 0 && threadIdx.x == 0) stats[it.image] = dvsof_render_stats_t{lo, hi, bad, 0};
    const float m = max_magnitude ? max_magnitude[it.image] : 0.f;
    FlowColour colour;
    colour.fx = (const float *)it.src;
    colour.fy = colour.fx + (size_t)it.h * it.w;
    colour.set_scale(lo, hi, m);
    emit_rows(it, canvas, colour);
}

// The source side of the table: n_flow flow items, the chunks of an image
// together, in order, tiling its rows; every image exactly once.
bool bad_flow_items(const dvsof_render_item_t *items, int n_flow, int n_images)
{
    if (n_flow < 0 || n_images < 0 || n_images > n_flow) return true;
    if (n_flow == 0) return false;
    if (!items) return true;
    uint64_t *seen = new uint64_t[((size_t)n_images + 63) / 64]();
    bool bad = false;
    int images = 0;
    for (int i = 0; i < n_flow && !bad; ++i) {
        const dvsof_render_item_t &it = items[i];
        bad = it.kind != DVSOF_RENDER_FLOW || !it.src || it.h < 1 || it.w < 1 || it.h > kMaxSide ||
              it.w > kMaxSide || it.rows < 1 || it.row0 < 0 || it.row0 > it.h - it.rows || it.image < 0 ||
              it.image >= n_images || it.chunks < 1 || it.chunks > kMaxChunks || it.chunk < 0 ||
              it.chunk >= it.chunks;
        if (bad) break;
        if (it.chunk == 0) {
            uint64_t &word = seen[it.image / 64];
            bad = it.row0 != 0 || (word >> (it.image % 64) & 1u);
            word |= (uint64_t)1 << (it.image % 64);
            ++images;
        } else if (i == 0) {
            bad = true;
        } else {
            const dvsof_render_item_t &prev = items[i - 1];
            bad = prev.image != it.image || prev.chunk + 1 != it.chunk || prev.chunks != it.chunks ||
                  prev.src != it.src || prev.h != it.h || prev.w != it.w || prev.row0 + prev.rows != it.row0;
        }
        if (!bad && it.chunk == it.chunks - 1) bad = it.row0 + it.rows != it.h;
        if (!bad && it.chunk != it.chunks - 1) bad = i + 1 >= n_flow;  // the image's last chunk is missing
    }
    delete[] seen;
    return bad || images != n_images;
}

// The destination side: every item inside its row and inside the canvas.
bool bad_destinations(const dvsof_render_item_t *items, int n_items, int n_flow, size_t canvas_bytes)
{
    for (int i = 0; i < n_items; ++i) {
        const dvsof_render_item_t &it = items[i];
        if ((it.kind == DVSOF_RENDER_FLOW) != (i < n_flow)) return true;
        if (it.kind != DVSOF_RENDER_FLOW && it.kind != DVSOF_RENDER_FRAME && it.kind != DVSOF_RENDER_FILL) return true;
        if (it.kind == DVSOF_RENDER_FRAME && !it.src) return true;
        if (it.h < 1 || it.w < 1 || it.h > kMaxSide || it.w > kMaxSide || it.rows < 1 || it.row0 < 0 ||
            it.row0 > it.h - it.rows)
            return true;
        if (it.x0 < 0 || it.y0 < 0 || it.dst_offset < 0 || it.dst_stride < 3 * ((int64_t)it.x0 + it.w)) return true;
        // the last byte of the item's last row (all terms < 2^63: stride is checked below)
        if (it.dst_stride > (int64_t)1 << 40 || (uint64_t)it.dst_offset > canvas_bytes) return true;
        const uint64_t end = (uint64_t)it.dst_offset + (uint64_t)((int64_t)it.y0 + it.h - 1) * (uint64_t)it.dst_stride +
                             3u * ((uint64_t)it.x0 + it.w);
        if (end > canvas_bytes) return true;
    }
    return false;
}

}  // namespace

extern "C" {

int dvsof_flow_render_chunk_rows(int h, int w) { return chunk_rows(h, w); }

size_t dvsof_flow_render_workspace_bytes(int n_images)
{
    if (n_images < 1) return 0;
    return sizeof(dvsof_render_stats_t) * (size_t)n_images * kMaxChunks;
}

int dvsof_flow_render_stats(const dvsof_render_item_t *items, const dvsof_render_item_t *items_dev, int n_flow,
                            int n_images, void *workspace, size_t workspace_bytes, void *stream)
{
    if (bad_flow_items(items, n_flow, n_images)) return DVSOF_EINVAL;
    if (n_flow == 0) return DVSOF_OK;
    if (!items_dev) return DVSOF_EINVAL;
    if (!workspace || workspace_bytes < dvsof_flow_render_workspace_bytes(n_images)) return DVSOF_ENOSPACE;
    hipLaunchKernelGGL(flow_render_stats_kernel, dim3((unsigned)n_flow), dim3(NT), 0, as_stream(stream), items_dev,
                       (dvsof_render_stats_t *)workspace);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_flow_render(const dvsof_render_item_t *items, const dvsof_render_item_t *items_dev, int n_items, int n_flow,
                      int n_images, const float *max_magnitude, const void *workspace, size_t workspace_bytes,
                      uint8_t *canvas, size_t canvas_bytes, dvsof_render_stats_t *stats, void *stream)
{
    if (n_items < 0 || n_flow > n_items || bad_flow_items(items, n_flow, n_images)) return DVSOF_EINVAL;
    if (n_items == 0) return DVSOF_OK;
    if (!items || !items_dev || !canvas || (n_flow > 0 && !stats)) return DVSOF_EINVAL;
    if (bad_destinations(items, n_items, n_flow, canvas_bytes)) return DVSOF_EINVAL;
    if (n_flow > 0 && (!workspace || workspace_bytes < dvsof_flow_render_workspace_bytes(n_images)))
        return DVSOF_ENOSPACE;
    hipLaunchKernelGGL(flow_render_kernel, dim3((unsigned)n_items), dim3(NT), 0, as_stream(stream), items_dev,
                       (const dvsof_render_stats_t *)workspace, max_magnitude, canvas, stats);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
