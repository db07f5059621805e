// Checkpoint snapshot: ONE launch gathers every float32 tensor of a training
// state (parameters, optimizer moments) into one contiguous device slab and
// counts the non-finite values on the way (docs/CHECKPOINT_SPEC.md).
//
// Work is a table of (tensor, chunk) items like the optimizers' (optim.hip): a
// workgroup takes items grid-strided, an item is CHUNK consecutive floats of
// one tensor's storage.  Destination offsets are multiples of 16 bytes and
// CHUNK * 4 is one too, so every item starts 16-byte aligned in the slab and
// has its source's alignment: the vector width is chosen per item from the
// source address and is uniform across the item (16, 8 or 4 bytes; loads and
// stores of the same width), with a scalar tail.  Values travel as integers:
// -0.0, denormals and NaN payloads arrive bit for bit.
//
// Pure HBM copy: 2 x bytes of traffic, no LDS, no atomics unless a wave met a
// NaN or an Inf.
#include "common.h"

namespace {

constexpr int CHUNK = 4096;        // floats per work item (16 KiB: 4 float4 per lane)
constexpr int MAX_BLOCKS = 2048;   // grid cap, items beyond it are grid-strided

__device__ __forceinline__ int nonfinite(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u; }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
#define DVSOF_GLOBAL __attribute__((address_space(1)))     // the sources arrive as integers: say they are global memory

__device__ __forceinline__ int count_nonfinite(u32x4 v)
{
    return nonfinite(v.x) + nonfinite(v.y) + nonfinite(v.z) + nonfinite(v.w);
}
__device__ __forceinline__ int count_nonfinite(u32x2 v) { return nonfinite(v.x) + nonfinite(v.y); }
__device__ __forceinline__ int count_nonfinite(uint32_t v) { return nonfinite(v); }

// n floats (n <= CHUNK) from s to d in vectors of V, then the scalar tail
template <typename V>
__device__ __forceinline__ int copy_item(const DVSOF_GLOBAL uint32_t *__restrict__ s,
                                         DVSOF_GLOBAL uint32_t *__restrict__ d, int n)
{
    constexpr int W = (int)(sizeof(V) / 4);
    const int nv = n / W;
    const DVSOF_GLOBAL V *__restrict__ sv = (const DVSOF_GLOBAL V *)s;
    DVSOF_GLOBAL V *__restrict__ dv = (DVSOF_GLOBAL V *)d;
    int bad = 0;
    if (W == 4 && n == CHUNK) {     // a full item, the common case: its loads in flight together
        constexpr int PER = CHUNK / 4 / 256;
        V v[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) v[k] = sv[threadIdx.x + 256 * k];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            dv[threadIdx.x + 256 * k] = v[k];
            bad += count_nonfinite(v[k]);
        }
        return bad;
    }
    for (int i = threadIdx.x; i < nv; i += 256) {
        const V v = sv[i];
        dv[i] = v;
        bad += count_nonfinite(v);
    }
    const int i = nv * W + threadIdx.x;     // fewer than W floats are left
    if (W > 1 && i < n) {
        const uint32_t v = s[i];
        d[i] = v;
        bad += nonfinite(v);
    }
    return bad;
}

// header: word[parity] receives this launch's count, word[parity ^ 1] is zeroed
// for the next launch (a zero-fill racing with this launch's own atomics could
// lose counts: the word a launch adds to was zeroed by the launch before it)
__global__ __launch_bounds__(256) void snapshot_pack_kernel(const uint64_t *__restrict__ srcs,
                                                            const int64_t *__restrict__ counts,
                                                            const int64_t *__restrict__ offsets,
                                                            const int32_t *__restrict__ items, int num_items,
                                                            uint32_t *__restrict__ slab, int parity)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) slab[parity ^ 1] = 0u;
    int bad = 0;
    for (int it = blockIdx.x; it < num_items; it += gridDim.x) {
        const int t = items[2 * it], c = items[2 * it + 1];
        const int64_t base = (int64_t)c * CHUNK;
        const int64_t left = counts[t] - base;
        const int n = left < CHUNK ? (int)left : CHUNK;
        const DVSOF_GLOBAL uint32_t *s = (const DVSOF_GLOBAL uint32_t *)(uintptr_t)srcs[t] + base;
        DVSOF_GLOBAL uint32_t *d = (DVSOF_GLOBAL uint32_t *)slab + offsets[t] + base;
        const unsigned a = (unsigned)((uintptr_t)s & 15u);      // uniform across the workgroup
        if (a == 0)
            bad += copy_item<u32x4>(s, d, n);
        else if (a == 8)
            bad += copy_item<u32x2>(s, d, n);
        else
            bad += copy_item<uint32_t>(s, d, n);
    }
    const int wave_bad = wave_sum(bad);     // every lane is here: no early exit above
    if ((threadIdx.x & (kWave - 1)) == 0 && wave_bad != 0) atomicAdd(slab + parity, (uint32_t)wave_bad);
}

}  // namespace

extern "C" {

int dvsof_snapshot_chunk_elems(void) { return CHUNK; }

int dvsof_snapshot_header_bytes(void) { return DVSOF_SNAPSHOT_HEADER_BYTES; }

int dvsof_snapshot_pack(const uint64_t *srcs, const int64_t *counts, const int64_t *offsets,
                        const int32_t *items, int num_items, void *slab, int parity, void *stream)
{
    if (num_items == 0) return 0;
    if (num_items < 0 || !srcs || !counts || !offsets || !items || !slab) return DVSOF_EINVAL;
    if (((uintptr_t)slab & 15u) != 0 || (parity != 0 && parity != 1)) return DVSOF_EINVAL;
    const int blocks = num_items < MAX_BLOCKS ? num_items : MAX_BLOCKS;
    hipLaunchKernelGGL(snapshot_pack_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), srcs, counts,
                       offsets, items, num_items, (uint32_t *)slab, parity);
    DVSOF_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
