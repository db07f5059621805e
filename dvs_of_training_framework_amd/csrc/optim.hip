// Fused multi-tensor AdamW (amsgrad) step: one launch per parameter group.
// Replaces torch.optim.AdamW(amsgrad=True).step() as constructed at
// train_flownet.py:57-75 and called at utils/training.py:164 (foreach /
// unfused ATen ops: ~10 launches per tensor).  HBM-bound: reads p,g,m,v,vmax,
// writes p,m,v,vmax = 36 B per parameter.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

struct AdamArgs {
    float lr, beta1, beta2, eps, weight_decay;
    float step_size;  // lr / (1 - beta1^t)
    float bc2_sqrt;   // sqrt(1 - beta2^t)
    int amsgrad;
};

#ifndef DVSOF_ADAM_CHUNK
#define DVSOF_ADAM_CHUNK 1024   // (measured in the step: 1024 3150, 2048 3133, 4096 3118, 8192 3091 samples/s)
#endif
constexpr int CHUNK = DVSOF_ADAM_CHUNK;  // elements per workgroup

// The 32-byte record of the step guard (docs/STEP_GUARD_SPEC.md): written by guard_close_kernel,
// read by every workgroup of a guarded update.
struct GuardRecord {
    float scale;            // gradient multiplier of this step (1: no clipping)
    uint32_t skip;          // 1: this step writes nothing
    double norm;            // global gradient norm; NaN when bad > 0
    uint32_t bad;           // non-finite gradient elements of this step (saturating)
    uint32_t skipped;       // steps skipped since the record was made
    uint32_t clipped;       // steps with scale < 1
    uint32_t consecutive;   // skipped steps in a row
};
static_assert(sizeof(GuardRecord) == DVSOF_GUARD_RECORD_BYTES, "guard record layout");

// op order of torch.optim.adam._single_tensor_adam (decoupled weight decay)
__device__ __forceinline__ void adam_elem(float &p, float g, float &m, float &v, float &vm,
                                          const AdamArgs &a)
{
    p = p * (1.f - a.lr * a.weight_decay);
    m = m + (g - m) * (1.f - a.beta1);           // lerp_
    v = v * a.beta2 + (1.f - a.beta2) * g * g;   // mul_().addcmul_()
    float denom;
    if (a.amsgrad) {
        vm = fmaxf(vm, v);
        denom = sqrtf(vm) / a.bc2_sqrt + a.eps;
    } else {
        denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    }
    p = p - a.step_size * (m / denom);
}

// table: per tensor {p, g, m, v, vmax} pointers and element count; chunk
// table: (tensor id, chunk index) per workgroup.
// dyn (optional, device): {lr, lr / (1 - beta1^t), sqrt(1 - beta2^t)} of THIS
// step.  A step captured in a hipGraph bakes its kernel arguments in; what
// changes from step to step (learning-rate schedule, bias corrections) then
// comes from this table, which the host refreshes before every replay.
// GUARD: the step obeys the guard record -- a skipped step returns before any load or store,
// otherwise every gradient is multiplied by the record's scale (one multiply; exact at 1.0f).
// The unguarded instantiation never reads `guard`.
template <bool GUARD>
__global__ __launch_bounds__(256) void adamw_kernel(const uint64_t *__restrict__ ptrs,
                                                    const int64_t *__restrict__ sizes,
                                                    const int32_t *__restrict__ chunks,
                                                    const AdamArgs a_in,
                                                    const float *__restrict__ dyn,
                                                    const GuardRecord *__restrict__ guard)
{
    float gs = 1.f;
    if (GUARD) {
        if (guard->skip) return;    // uniform over the launch
        gs = guard->scale;
    }
    AdamArgs a = a_in;
    if (dyn) {
        a.lr = dyn[0];
        a.step_size = dyn[1];
        a.bc2_sqrt = dyn[2];
    }
    const int t = chunks[2 * blockIdx.x], c = chunks[2 * blockIdx.x + 1];
    float *p = (float *)ptrs[5 * t + 0];
    const float *g = (const float *)ptrs[5 * t + 1];
    float *m = (float *)ptrs[5 * t + 2];
    float *v = (float *)ptrs[5 * t + 3];
    float *vm = (float *)ptrs[5 * t + 4];
    const int64_t n = sizes[t];
    const int64_t base = (int64_t)c * CHUNK;
#pragma unroll
    for (int it = 0; it < CHUNK / 1024; ++it) {
        const int64_t i = base + it * 1024 + threadIdx.x * 4;
        if (i + 3 < n) {
            f32x4 P = *(f32x4u *)(p + i), G = *(const f32x4u *)(g + i);
            f32x4 M = *(f32x4u *)(m + i), V = *(f32x4u *)(v + i);
            f32x4 X = a.amsgrad ? *(f32x4u *)(vm + i) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = P[j], mj = M[j], vj = V[j], xj = X[j];
                adam_elem(pj, GUARD ? G[j] * gs : G[j], mj, vj, xj, a);
                P[j] = pj; M[j] = mj; V[j] = vj; X[j] = xj;
            }
            *(f32x4u *)(p + i) = P;
            *(f32x4u *)(m + i) = M;
            *(f32x4u *)(v + i) = V;
            if (a.amsgrad) *(f32x4u *)(vm + i) = X;
        } else {
            for (int64_t j = i; j < n && j < i + 4; ++j) {
                float x = a.amsgrad ? vm[j] : 0.f;
                adam_elem(p[j], GUARD ? g[j] * gs : g[j], m[j], v[j], x, a);
                if (a.amsgrad) vm[j] = x;
            }
        }
    }
}

// The per-step table of a captured step ({lr, lr/bc1, sqrt(bc2)} per group) written from
// KERNEL ARGUMENTS: a 16-byte host-to-device copy is a blit kernel with system-scope fences
// (4 us + an 11 us bubble in front of the next kernel, at the head of every step)
constexpr int DYN_VALUES = 64;
struct DynValues {
    float v[DYN_VALUES];
};
__global__ void set_dynamic_kernel(float *dyn, DynValues vals, int n)
{
    if ((int)threadIdx.x < n) dyn[threadIdx.x] = vals.v[threadIdx.x];
}

}  // namespace

extern "C" {

int dvsof_adamw_chunk_elems(void) { return CHUNK; }

// one body for a step and its guarded twin: guard == nullptr launches the unguarded kernel
static int adamw_step(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                      int num_chunks, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int step, int amsgrad, const GuardRecord *guard,
                      void *stream)
{
    if (!ptrs || !sizes || !chunks || num_chunks < 0 || step < 1) return DVSOF_EINVAL;
    if (num_chunks == 0) return DVSOF_OK;
    AdamArgs a = {};
    a.lr = lr;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.eps = eps;
    a.weight_decay = weight_decay;
    // bias corrections in double like the Python reference (python floats)
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    a.step_size = (float)((double)lr / bc1);
    a.bc2_sqrt = (float)sqrt(bc2);
    a.amsgrad = amsgrad;
    if (guard)
        hipLaunchKernelGGL(adamw_kernel<true>, dim3(num_chunks), dim3(256), 0, as_stream(stream), ptrs,
                           sizes, chunks, a, (const float *)nullptr, guard);
    else
        hipLaunchKernelGGL(adamw_kernel<false>, dim3(num_chunks), dim3(256), 0, as_stream(stream), ptrs,
                           sizes, chunks, a, (const float *)nullptr, (const GuardRecord *)nullptr);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_adamw_step(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                     int num_chunks, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, int amsgrad, void *stream)
{
    return adamw_step(ptrs, sizes, chunks, num_chunks, lr, beta1, beta2, eps, weight_decay, step,
                      amsgrad, nullptr, stream);
}

int dvsof_adamw_step_guarded(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                             int num_chunks, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int step, int amsgrad, const void *guard,
                             void *stream)
{
    if (!guard) return DVSOF_EINVAL;
    return adamw_step(ptrs, sizes, chunks, num_chunks, lr, beta1, beta2, eps, weight_decay, step,
                      amsgrad, (const GuardRecord *)guard, stream);
}

void dvsof_adamw_dynamic(float lr, float beta1, float beta2, int step, float *host_out3)
{
    // the same double-precision bias corrections as dvsof_adamw_step
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    host_out3[0] = lr;
    host_out3[1] = (float)((double)lr / bc1);
    host_out3[2] = (float)sqrt(bc2);
}

int dvsof_adamw_set_dynamic(float *dyn, const float *host_values, int n, void *stream)
{
    if (!dyn || !host_values || n < 0) return DVSOF_EINVAL;
    for (int o = 0; o < n; o += DYN_VALUES) {   // the values travel as kernel arguments
        DynValues v;
        const int m = n - o < DYN_VALUES ? n - o : DYN_VALUES;
        for (int i = 0; i < DYN_VALUES; ++i) v.v[i] = i < m ? host_values[o + i] : 0.f;
        hipLaunchKernelGGL(set_dynamic_kernel, dim3(1), dim3(DYN_VALUES), 0, as_stream(stream), dyn + o, v, m);
        DVSOF_LAUNCH_CHECK();
    }
    return DVSOF_OK;
}

static int adamw_step_dyn(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                          int num_chunks, const float *dyn, float beta1, float beta2, float eps,
                          float weight_decay, int amsgrad, const GuardRecord *guard, void *stream)
{
    if (!ptrs || !sizes || !chunks || !dyn || num_chunks < 0) return DVSOF_EINVAL;
    if (num_chunks == 0) return DVSOF_OK;
    AdamArgs a = {};
    a.lr = a.step_size = a.bc2_sqrt = 0.f;   // from dyn
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.eps = eps;
    a.weight_decay = weight_decay;
    a.amsgrad = amsgrad;
    if (guard)
        hipLaunchKernelGGL(adamw_kernel<true>, dim3(num_chunks), dim3(256), 0, as_stream(stream), ptrs,
                           sizes, chunks, a, dyn, guard);
    else
        hipLaunchKernelGGL(adamw_kernel<false>, dim3(num_chunks), dim3(256), 0, as_stream(stream), ptrs,
                           sizes, chunks, a, dyn, (const GuardRecord *)nullptr);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_adamw_step_dyn(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                         int num_chunks, const float *dyn, float beta1, float beta2, float eps,
                         float weight_decay, int amsgrad, void *stream)
{
    return adamw_step_dyn(ptrs, sizes, chunks, num_chunks, dyn, beta1, beta2, eps, weight_decay,
                          amsgrad, nullptr, stream);
}

int dvsof_adamw_step_dyn_guarded(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                                 int num_chunks, const float *dyn, float beta1, float beta2,
                                 float eps, float weight_decay, int amsgrad, const void *guard,
                                 void *stream)
{
    if (!guard) return DVSOF_EINVAL;
    return adamw_step_dyn(ptrs, sizes, chunks, num_chunks, dyn, beta1, beta2, eps, weight_decay,
                          amsgrad, (const GuardRecord *)guard, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// RAdam (Liu et al., ICLR 2020) and Ranger (= RAdam + Lookahead k, alpha
// [+ gradient centralisation]).  Replace RAdam.radam.RAdam and ranger.Ranger
// as constructed at train_flownet.py:62-71 (un-vendored submodules upstream:
// arithmetic restated from the published algorithms, oracle/ref_optim.py).
// ---------------------------------------------------------------------------
namespace {

struct RAdamArgs {
    float lr, beta1, beta2, eps, weight_decay;
    float step_size;   // already divided by (1 - beta1^t)
    int rectified;     // N_sma above the threshold: adaptive step
    int lookahead;     // Ranger: this is a k-th step
    float la_alpha;
};

__device__ __forceinline__ void radam_elem(float &p, float g, float &m, float &v, float &slow,
                                           const RAdamArgs &a)
{
    v = v * a.beta2 + (1.f - a.beta2) * g * g;
    m = m * a.beta1 + (1.f - a.beta1) * g;
    // decay only where an update is taken: RAdam without degenerate-to-SGD leaves p alone
    // while the variance is not tractable (step_size -1); Ranger's step size is never -1
    if (a.weight_decay != 0.f && (a.rectified || a.step_size > 0.f))
        p = p - a.weight_decay * a.lr * p;
    if (a.rectified) p = p - a.step_size * a.lr * (m / (sqrtf(v) + a.eps));
    else if (a.step_size > 0.f) p = p - a.step_size * a.lr * m;
    if (a.lookahead) {
        slow = slow + a.la_alpha * (p - slow);
        p = slow;
    }
}

// dyn (optional, device): {lr, step size, rectified, Lookahead-sync-now} of THIS step, as
// floats (the two decisions 0 / 1), for a step captured in a hipGraph -- see adamw_kernel.
// All four are uniform over the launch: on a non-sync step no lane touches the slow buffer.
// GUARD: as in adamw_kernel; a skipped step also leaves the slow buffer and the Lookahead
// synchronisation alone.
template <bool GUARD>
__global__ __launch_bounds__(256) void radam_kernel(const uint64_t *__restrict__ ptrs,
                                                    const int64_t *__restrict__ sizes,
                                                    const int32_t *__restrict__ chunks,
                                                    const RAdamArgs a_in, const int use_slow,
                                                    const float *__restrict__ dyn,
                                                    const GuardRecord *__restrict__ guard)
{
    float gs = 1.f;
    if (GUARD) {
        if (guard->skip) return;    // uniform over the launch
        gs = guard->scale;
    }
    RAdamArgs a = a_in;
    if (dyn) {
        a.lr = dyn[0];
        a.step_size = dyn[1];
        a.rectified = dyn[2] != 0.f;
        a.lookahead = dyn[3] != 0.f;
    }
    const int t = chunks[2 * blockIdx.x], c = chunks[2 * blockIdx.x + 1];
    float *p = (float *)ptrs[5 * t + 0];
    const float *g = (const float *)ptrs[5 * t + 1];
    float *m = (float *)ptrs[5 * t + 2];
    float *v = (float *)ptrs[5 * t + 3];
    float *sl = (float *)ptrs[5 * t + 4];
    const int64_t n = sizes[t];
    const int64_t base = (int64_t)c * CHUNK;
#pragma unroll
    for (int it = 0; it < CHUNK / 1024; ++it) {
        const int64_t i = base + it * 1024 + threadIdx.x * 4;
        if (i + 3 < n) {
            f32x4 P = *(f32x4u *)(p + i), G = *(const f32x4u *)(g + i);
            f32x4 M = *(f32x4u *)(m + i), V = *(f32x4u *)(v + i);
            f32x4 S = (use_slow && a.lookahead) ? *(f32x4u *)(sl + i) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = P[j], mj = M[j], vj = V[j], sj = S[j];
                radam_elem(pj, GUARD ? G[j] * gs : G[j], mj, vj, sj, a);
                P[j] = pj; M[j] = mj; V[j] = vj; S[j] = sj;
            }
            *(f32x4u *)(p + i) = P;
            *(f32x4u *)(m + i) = M;
            *(f32x4u *)(v + i) = V;
            if (use_slow && a.lookahead) *(f32x4u *)(sl + i) = S;
        } else {
            for (int64_t j = i; j < n && j < i + 4; ++j) {
                float s = (use_slow && a.lookahead) ? sl[j] : 0.f;
                radam_elem(p[j], GUARD ? g[j] * gs : g[j], m[j], v[j], s, a);
                if (use_slow && a.lookahead) sl[j] = s;
            }
        }
    }
}

// Gradient centralisation: row[:] -= mean(row[:]) by one workgroup of 256: per-thread strided
// double sums, then the wave, then the four waves in a fixed order.
__device__ __forceinline__ void centralize_row(float *row, int row_len)
{
    __shared__ double red[4];
    double s = 0;
    for (int i = threadIdx.x; i < row_len; i += 256) s += (double)row[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const float mean = (float)(((red[0] + red[1]) + (red[2] + red[3])) / (double)row_len);
    for (int i = threadIdx.x; i < row_len; i += 256) row[i] -= mean;
}

// g[r][:] -= mean(g[r][:]), one workgroup per row of ONE tensor.
__global__ __launch_bounds__(256) void grad_centralize_kernel(float *g, int row_len)
{
    centralize_row(g + (size_t)blockIdx.x * row_len, row_len);
}

// The same for the rows of MANY tensors in one launch: rows[2r] = address of row r,
// rows[2r+1] = its length; one workgroup per row.
__global__ __launch_bounds__(256) void grad_centralize_multi_kernel(const int64_t *__restrict__ rows)
{
    centralize_row((float *)(uint64_t)rows[2 * blockIdx.x], (int)rows[2 * blockIdx.x + 1]);
}

// What a RAdam / Ranger step takes from the step count, in double like the Python references.
// degenerate_to_sgd: the flag word of dvsof_radam_step.  step_size -1: no update.
void radam_rectify(float beta1, float beta2, int step, float nsma_threshold, int degenerate_to_sgd,
                   int *rectified, float *step_size)
{
    const double b2t = pow((double)beta2, (double)step);
    const double nmax = 2.0 / (1.0 - (double)beta2) - 1.0;
    const double nsma = nmax - 2.0 * step * b2t / (1.0 - b2t);
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    *rectified = (degenerate_to_sgd & 2) ? nsma >= (double)nsma_threshold   // RAdam: ">="
                                         : nsma > (double)nsma_threshold;   // Ranger: ">"
    if (*rectified)
        *step_size = (float)(sqrt((1.0 - b2t) * (nsma - 4.0) / (nmax - 4.0) * (nsma - 2.0) / nsma *
                                  nmax / (nmax - 2.0)) / bc1);
    else
        *step_size = (degenerate_to_sgd & 1) ? (float)(1.0 / bc1) : -1.f;
}

}  // namespace

extern "C" {

static int radam_step(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                      int num_chunks, float lr, float beta1, float beta2, float eps,
                      float weight_decay, int step, float nsma_threshold, int degenerate_to_sgd,
                      int lookahead_now, float lookahead_alpha, const GuardRecord *guard,
                      void *stream)
{
    if (!ptrs || !sizes || !chunks || num_chunks < 0 || step < 1) return DVSOF_EINVAL;
    if (num_chunks == 0) return DVSOF_OK;
    RAdamArgs a = {};
    a.lr = lr;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.eps = eps;
    a.weight_decay = weight_decay;
    radam_rectify(beta1, beta2, step, nsma_threshold, degenerate_to_sgd, &a.rectified, &a.step_size);
    a.lookahead = lookahead_now;
    a.la_alpha = lookahead_alpha;
    if (guard)
        hipLaunchKernelGGL(radam_kernel<true>, dim3(num_chunks), dim3(256), 0, as_stream(stream), ptrs,
                           sizes, chunks, a, lookahead_alpha > 0.f ? 1 : 0, (const float *)nullptr,
                           guard);
    else
        hipLaunchKernelGGL(radam_kernel<false>, dim3(num_chunks), dim3(256), 0, as_stream(stream), ptrs,
                           sizes, chunks, a, lookahead_alpha > 0.f ? 1 : 0, (const float *)nullptr,
                           (const GuardRecord *)nullptr);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_radam_step(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                     int num_chunks, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, float nsma_threshold, int degenerate_to_sgd,
                     int lookahead_now, float lookahead_alpha, void *stream)
{
    return radam_step(ptrs, sizes, chunks, num_chunks, lr, beta1, beta2, eps, weight_decay, step,
                      nsma_threshold, degenerate_to_sgd, lookahead_now, lookahead_alpha, nullptr,
                      stream);
}

int dvsof_radam_step_guarded(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                             int num_chunks, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int step, float nsma_threshold,
                             int degenerate_to_sgd, int lookahead_now, float lookahead_alpha,
                             const void *guard, void *stream)
{
    if (!guard) return DVSOF_EINVAL;
    return radam_step(ptrs, sizes, chunks, num_chunks, lr, beta1, beta2, eps, weight_decay, step,
                      nsma_threshold, degenerate_to_sgd, lookahead_now, lookahead_alpha,
                      (const GuardRecord *)guard, stream);
}

void dvsof_radam_dynamic(float lr, float beta1, float beta2, int step, float nsma_threshold,
                         int degenerate_to_sgd, int lookahead_k, float *host_out4)
{
    int rectified = 0;
    float step_size = 0.f;
    radam_rectify(beta1, beta2, step, nsma_threshold, degenerate_to_sgd, &rectified, &step_size);
    host_out4[0] = lr;
    host_out4[1] = step_size;
    host_out4[2] = rectified ? 1.f : 0.f;
    host_out4[3] = (lookahead_k > 0 && step % lookahead_k == 0) ? 1.f : 0.f;
}

static int radam_step_dyn(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                          int num_chunks, const float *dyn, float beta1, float beta2, float eps,
                          float weight_decay, float lookahead_alpha, const GuardRecord *guard,
                          void *stream)
{
    if (!ptrs || !sizes || !chunks || !dyn || num_chunks < 0) return DVSOF_EINVAL;
    if (num_chunks == 0) return DVSOF_OK;
    RAdamArgs a = {};   // lr, step_size, rectified, lookahead: from dyn
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.eps = eps;
    a.weight_decay = weight_decay;
    a.la_alpha = lookahead_alpha;
    if (guard)
        hipLaunchKernelGGL(radam_kernel<true>, dim3(num_chunks), dim3(256), 0, as_stream(stream), ptrs,
                           sizes, chunks, a, lookahead_alpha > 0.f ? 1 : 0, dyn, guard);
    else
        hipLaunchKernelGGL(radam_kernel<false>, dim3(num_chunks), dim3(256), 0, as_stream(stream), ptrs,
                           sizes, chunks, a, lookahead_alpha > 0.f ? 1 : 0, dyn,
                           (const GuardRecord *)nullptr);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_radam_step_dyn(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                         int num_chunks, const float *dyn, float beta1, float beta2, float eps,
                         float weight_decay, float lookahead_alpha, void *stream)
{
    return radam_step_dyn(ptrs, sizes, chunks, num_chunks, dyn, beta1, beta2, eps, weight_decay,
                          lookahead_alpha, nullptr, stream);
}

int dvsof_radam_step_dyn_guarded(const uint64_t *ptrs, const int64_t *sizes, const int32_t *chunks,
                                 int num_chunks, const float *dyn, float beta1, float beta2,
                                 float eps, float weight_decay, float lookahead_alpha,
                                 const void *guard, void *stream)
{
    if (!guard) return DVSOF_EINVAL;
    return radam_step_dyn(ptrs, sizes, chunks, num_chunks, dyn, beta1, beta2, eps, weight_decay,
                          lookahead_alpha, (const GuardRecord *)guard, stream);
}

int dvsof_grad_centralize_multi(const int64_t *rows, int num_rows, void *stream)
{
    if (!rows || num_rows < 0) return DVSOF_EINVAL;
    if (num_rows == 0) return DVSOF_OK;
    hipLaunchKernelGGL(grad_centralize_multi_kernel, dim3(num_rows), dim3(256), 0, as_stream(stream),
                       rows);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_grad_centralize(float *grad, int rows, int row_len, void *stream)
{
    if (!grad || rows < 1 || row_len < 1) return DVSOF_EINVAL;
    hipLaunchKernelGGL(grad_centralize_kernel, dim3(rows), dim3(256), 0, as_stream(stream), grad,
                       row_len);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Step guard (docs/STEP_GUARD_SPEC.md): the global gradient norm and the count of non-finite
// gradient elements of one step, reduced on the device in a fixed order, and the decision the
// guarded updates above obey.  Two launches in stream order -- partials, then close -- and no
// hand-off between workgroups inside a launch: no atomics, no flags, nothing that waits.
// ---------------------------------------------------------------------------
namespace {

struct GuardPartial {
    double sumsq;       // sum of (double)g * (double)g over the finite elements of one work item
    uint32_t bad;       // elements whose exponent field is all ones (NaN, +-Inf)
    uint32_t pad;
};
static_assert(sizeof(GuardPartial) == DVSOF_GUARD_PARTIAL_BYTES, "guard partial layout");

__device__ __forceinline__ void guard_elem(float g, double &s, int &bad)
{
    if ((__builtin_bit_cast(uint32_t, g) & 0x7f800000u) == 0x7f800000u)    // as snapshot.hip:nonfinite
        ++bad;
    else
        s += (double)g * (double)g;
}

// One workgroup per (tensor, chunk) work item of the update kernels' chunk table; the same
// vector / tail split as theirs.  grads[t * ptr_stride] is the gradient of tensor t.
__global__ __launch_bounds__(256) void guard_partials_kernel(const uint64_t *__restrict__ grads,
                                                             const int ptr_stride,
                                                             const int64_t *__restrict__ sizes,
                                                             const int32_t *__restrict__ chunks,
                                                             GuardPartial *__restrict__ partials)
{
    __shared__ double red_s[4];
    __shared__ int red_b[4];
    const int t = chunks[2 * blockIdx.x], c = chunks[2 * blockIdx.x + 1];
    const float *g = (const float *)grads[(int64_t)t * ptr_stride];
    const int64_t n = sizes[t];
    const int64_t base = (int64_t)c * CHUNK;
    double s = 0.0;
    int bad = 0;
#pragma unroll
    for (int it = 0; it < CHUNK / 1024; ++it) {
        const int64_t i = base + it * 1024 + threadIdx.x * 4;
        if (i + 3 < n) {
            const f32x4 G = *(const f32x4u *)(g + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) guard_elem(G[j], s, bad);
        } else {
            for (int64_t j = i; j < n && j < i + 4; ++j) guard_elem(g[j], s, bad);
        }
    }
    s = wave_sum(s);            // shuffle tree, valid in lane 0
    bad = wave_sum(bad);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        red_s[threadIdx.x >> 6] = s;
        red_b[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        GuardPartial out;
        out.sumsq = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        out.bad = (uint32_t)((red_b[0] + red_b[1]) + (red_b[2] + red_b[3]));
        out.pad = 0u;
        partials[blockIdx.x] = out;
    }
}

// ONE workgroup: thread i takes partials i, i + 256, ... in that order, then the wave, then the
// four waves; thread 0 writes the record and moves its counters.
__global__ __launch_bounds__(256) void guard_close_kernel(const GuardPartial *__restrict__ partials,
                                                          const int num_partials, const double max_norm,
                                                          const int skip_nonfinite,
                                                          GuardRecord *__restrict__ rec)
{
    __shared__ double red_s[4];
    __shared__ unsigned long long red_b[4];
    double s = 0.0;
    unsigned long long bad = 0;
    for (int i = threadIdx.x; i < num_partials; i += 256) {
        s += partials[i].sumsq;
        bad += partials[i].bad;
    }
    s = wave_sum(s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        red_s[threadIdx.x >> 6] = s;
        red_b[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double sumsq = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    const unsigned long long nbad = (red_b[0] + red_b[1]) + (red_b[2] + red_b[3]);
    const double norm = nbad ? __builtin_nan("") : sqrt(sumsq);
    float scale = 1.f;
    if (max_norm > 0.0 && !nbad) {
        const double r = max_norm / (norm + 1e-6);
        scale = (float)(r < 1.0 ? r : 1.0);
    }
    const uint32_t skip = (nbad && skip_nonfinite) ? 1u : 0u;
    rec->scale = scale;
    rec->skip = skip;
    rec->norm = norm;
    rec->bad = nbad > 0xffffffffull ? 0xffffffffu : (uint32_t)nbad;
    rec->skipped += skip;
    rec->clipped += scale < 1.f ? 1u : 0u;
    rec->consecutive = skip ? rec->consecutive + 1u : 0u;
}

}  // namespace

extern "C" {

int dvsof_grad_guard_record_bytes(void) { return DVSOF_GUARD_RECORD_BYTES; }

int dvsof_grad_guard_partial_bytes(void) { return DVSOF_GUARD_PARTIAL_BYTES; }

int dvsof_grad_guard(const uint64_t *grads, int ptr_stride, const int64_t *sizes,
                     const int32_t *chunks, int num_chunks, void *partials, size_t partials_bytes,
                     double max_norm, int skip_nonfinite, void *guard, void *stream)
{
    if (num_chunks < 0 || !guard || ((uintptr_t)guard & 7u) != 0 || max_norm != max_norm)
        return DVSOF_EINVAL;
    if (num_chunks > 0) {
        if (!grads || ptr_stride < 1 || !sizes || !chunks || !partials || ((uintptr_t)partials & 7u) != 0)
            return DVSOF_EINVAL;
        if (partials_bytes < (size_t)num_chunks * sizeof(GuardPartial)) return DVSOF_ENOSPACE;
        hipLaunchKernelGGL(guard_partials_kernel, dim3(num_chunks), dim3(256), 0, as_stream(stream), grads,
                           ptr_stride, sizes, chunks, (GuardPartial *)partials);
        DVSOF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(guard_close_kernel, dim3(1), dim3(256), 0, as_stream(stream),
                       (const GuardPartial *)partials, num_chunks, max_norm, skip_nonfinite,
                       (GuardRecord *)guard);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
