// Ternary census term of the framed loss (Meister, Hur and Roth, AAAI 2018),
// forward and analytic backward, all scales in one launch each
// (include/dvsof_census.h, docs/CENSUS_SPEC.md).
//
// A dense 7x7 stencil over two images: the first frame A and the bilinearly
// warped second frame Bw.  A 256-thread workgroup owns a 64x16 pixel tile of one
// sample at one scale, as in loss.hip: wave v owns rows 4v..4v+3, lane l column
// l, so a thread holds a 4-pixel column strip and lanes read consecutive LDS
// columns.  The tile and a 3-pixel halo (70x22) of every plane live in LDS.
//
// Forward: Bw is computed ONCE per staged pixel (one flow read, four gathered
// taps) and written to the workspace by the tile that owns the pixel.  A strip
// walks the 7 patch columns; per column it reads the 10 rows its 4 centres
// share (70 LDS reads per plane and strip instead of 196), the centres and the
// running distances stay in registers.  Per centre it stores
// r = [counted] d rho / d dist, and the workgroup adds its sum of rho and its
// number of counted pixels into the level's 64-bit integer accumulators
// (2^-20 fixed point and plain counts; no-return agent-scope atomics: integer
// addition commutes, so the totals do not depend on the arrival order).  One
// closing wave divides and writes terms, value and the factor of the backward.
//
// Backward: a GATHER.  With r stored, the gradient at a pixel q needs A, Bw
// and r on q's own 7x7 patch only: the contribution of centre e = q - d through
// t_Bw(e, d) and the contribution of q as a centre through t_Bw(q, -d) are the
// same number c(e, d) (t is odd, everything else even), weighed r(e) and r(q):
//   G(q) = factor * sum_{e in patch(q), e != q} c(e, q - e) (r(e) + r(q)).
// So the same 3-pixel halo, one evaluation per neighbour, no atomics, nothing
// to zero, and the same input gives the same bytes.
#include "common.h"
#include "../../include/dvsof_census.h"

namespace {

constexpr int TW = 64, TH = 16, NT = 256;
constexpr int RAD = 3, PATCH = 2 * RAD + 1;
constexpr int LW = TW + 2 * RAD, LH = TH + 2 * RAD, NPIX = LW * LH;
constexpr int FILL = (NPIX + NT - 1) / NT;
constexpr int NP = TH / (NT / kWave);            // pixels of a strip
constexpr int NROW = NP + 2 * RAD;               // rows a strip's patches span
constexpr int NW = NT / kWave;
constexpr int HEADER_ACC = 2 * DVSOF_MAX_SCALES;  // uint64 words
constexpr size_t HEADER_BYTES = HEADER_ACC * sizeof(unsigned long long) + DVSOF_MAX_SCALES * sizeof(float);
constexpr float FIX_SCALE = 1048576.f;           // 2^20
constexpr double FIX_INV = 1.0 / 1048576.0;
constexpr float T_EPS = 0.81f, S_EPS = 0.1f;     // UnFlow's constants for 0..255 images

struct Level {
    const float *frames, *flow;
    float *grad, *bw, *r;
    int h, w;
    int tiles_x, tiles_per_sample, block_begin;
};

struct Params {
    Level s[DVSOF_MAX_SCALES];
    int K, N;
    const int32_t *start, *stop;
    unsigned long long *acc;    // [K][2]: sum of rho (2^-20), counted pixels
    float *factor;              // [K]: weight / (K * max(count, 1))
    float *terms, *value;
    const float *seed;
    float weight;
};

__device__ __forceinline__ int find_level(const Params &P, int bid)
{
    int k = 0;
#pragma unroll
    for (int i = 1; i < DVSOF_MAX_SCALES; ++i)
        if (i < P.K && bid >= P.s[i].block_begin) k = i;
    return k;
}

// The four taps of the bilinear sample of B at (x + u, y + v): floor
// convention, a tap outside the image is 0 and is not read.  The corner index
// is clamped BEFORE it becomes an integer, so an infinite or NaN flow reads
// nothing out of bounds (its taps are all outside or all valid).
struct Taps {
    float fx, fy, nw, ne, sw, se;
    bool inside;    // m: the sample position is inside [0, w-1] x [0, h-1]
};
__device__ __forceinline__ Taps gather_taps(const float *B, int h, int w, int x, int y, float u, float v, bool live)
{
    const float sx = (float)x + u, sy = (float)y + v;
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    Taps t;
    t.fx = sx - fx0;
    t.fy = sy - fy0;
    t.inside = live & (sx >= 0.f) & (sx <= (float)(w - 1)) & (sy >= 0.f) & (sy <= (float)(h - 1));
    const int x0 = (int)fminf(fmaxf(fx0, -2.f), (float)w + 1.f);
    const int y0 = (int)fminf(fmaxf(fy0, -2.f), (float)h + 1.f);
    const bool vx0 = (unsigned)x0 < (unsigned)w, vx1 = (unsigned)(x0 + 1) < (unsigned)w;
    const bool vy0 = live & ((unsigned)y0 < (unsigned)h), vy1 = live & ((unsigned)(y0 + 1) < (unsigned)h);
    const int o = y0 * w + x0;
    t.nw = (vy0 & vx0) ? B[o] : 0.f;
    t.ne = (vy0 & vx1) ? B[o + 1] : 0.f;
    t.sw = (vy1 & vx0) ? B[o + w] : 0.f;
    t.se = (vy1 & vx1) ? B[o + w + 1] : 0.f;
    return t;
}
__device__ __forceinline__ float bilinear(const Taps &t)
{
    const float wx0 = 1.f - t.fx, wy0 = 1.f - t.fy;
    return wy0 * (wx0 * t.nw + t.fx * t.ne) + t.fy * (wx0 * t.sw + t.fx * t.se);
}

// t = D / sqrt(0.81 + D D) as D * rsq(q): one v_rsq_f32 (1 ulp) and two
// roundings; rs is kept for the derivative 0.81 rs^3.
__device__ __forceinline__ float ternary(float D, float &rs)
{
    rs = __builtin_amdgcn_rsqf(D * D + T_EPS);
    return D * rs;
}

struct Tile {
    int k, n, ty0, tx0;
};
__device__ __forceinline__ Tile find_tile(const Params &P, int bid)
{
    Tile T;
    T.k = find_level(P, bid);
    const Level &S = P.s[T.k];
    const int local = bid - S.block_begin;
    T.n = local / S.tiles_per_sample;
    const int t = local - T.n * S.tiles_per_sample;
    T.ty0 = (t / S.tiles_x) * TH;
    T.tx0 = (t % S.tiles_x) * TW;
    return T;
}

__global__ __launch_bounds__(NT) void census_fwd_kernel(const Params P)
{
    __shared__ float sA[NPIX], sB[NPIX];
    __shared__ unsigned char sM[NPIX];
    __shared__ float red_v[NW];
    __shared__ int red_c[NW];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const Tile T = find_tile(P, blockIdx.x);
    const Level &S = P.s[T.k];
    const int h = S.h, w = S.w;
    const size_t hw = (size_t)h * w;
    const float *A = S.frames + (size_t)P.start[T.n] * hw;
    const float *B = S.frames + (size_t)P.stop[T.n] * hw;
    const float *U = S.flow + (size_t)T.n * 2 * hw;
    float *BW = S.bw + (size_t)T.n * hw, *RR = S.r + (size_t)T.n * hw;

    // tile + halo -> LDS.  Fixed trip count, the loads of a phase first, so
    // that they are in flight together: A and the flow, then the four taps.
    {
        float a[FILL], u[FILL], v[FILL];
        int off[FILL];
#pragma unroll
        for (int it = 0; it < FILL; ++it) {
            const int i = tid + it * NT;
            const int ly = i / LW, lx = i - ly * LW;
            const int gy = T.ty0 + ly - RAD, gx = T.tx0 + lx - RAD;
            const bool in = (i < NPIX) & ((unsigned)gy < (unsigned)h) & ((unsigned)gx < (unsigned)w);
            off[it] = in ? gy * w + gx : -1;
            a[it] = in ? A[off[it]] : 0.f;
            u[it] = in ? U[off[it]] : 0.f;
            v[it] = in ? U[hw + off[it]] : 0.f;
        }
        Taps t[FILL];
#pragma unroll
        for (int it = 0; it < FILL; ++it) {
            const int i = tid + it * NT;
            const int ly = i / LW, lx = i - ly * LW;
            t[it] = gather_taps(B, h, w, T.tx0 + lx - RAD, T.ty0 + ly - RAD, u[it], v[it], off[it] >= 0);
        }
#pragma unroll
        for (int it = 0; it < FILL; ++it) {
            const int i = tid + it * NT;
            if (i >= NPIX) continue;
            const int ly = i / LW, lx = i - ly * LW;
            const float b = off[it] >= 0 ? bilinear(t[it]) : 0.f;
            sA[i] = a[it];
            sB[i] = b;
            sM[i] = t[it].inside;
            // the tile that owns the pixel keeps Bw for the backward
            if (off[it] >= 0 && (unsigned)(ly - RAD) < (unsigned)TH && (unsigned)(lx - RAD) < (unsigned)TW)
                BW[off[it]] = b;
        }
    }
    __syncthreads();

    const int ly0 = wave * NP;
    float cA[NP], cB[NP], dist[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        cA[j] = sA[(ly0 + j + RAD) * LW + lane + RAD];
        cB[j] = sB[(ly0 + j + RAD) * LW + lane + RAD];
        dist[j] = 0.f;
    }
    // patch columns left to right, each top to bottom: the order of the sum
#pragma unroll
    for (int dx = 0; dx < PATCH; ++dx) {
        float colA[NROW], colB[NROW];
#pragma unroll
        for (int r = 0; r < NROW; ++r) {
            colA[r] = sA[(ly0 + r) * LW + lane + dx];
            colB[r] = sB[(ly0 + r) * LW + lane + dx];
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
#pragma unroll
            for (int dy = 0; dy < PATCH; ++dy) {
                if (dx == RAD && dy == RAD) continue;
                float ra, rb;
                const float ta = ternary(colA[j + dy] - cA[j], ra);
                const float tb = ternary(colB[j + dy] - cB[j], rb);
                const float df = ta - tb, s = df * df;
                dist[j] = dist[j] + s * __builtin_amdgcn_rcpf(S_EPS + s);
            }
        }
    }

    const int x = T.tx0 + lane;
    float rho[NP];
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int y = T.ty0 + ly0 + j;
        const bool counted = (x >= RAD) & (x < w - RAD) & (y >= RAD) & (y < h - RAD) &
                             (sM[(ly0 + j + RAD) * LW + lane + RAD] != 0);
        const Charb c = charbonnier(dist[j]);
        rho[j] = counted ? c.val : 0.f;
        cnt += counted;
        if (x < w && y < h) RR[y * w + x] = counted ? c.der : 0.f;
    }
    const float sum = wave_sum((rho[0] + rho[1]) + (rho[2] + rho[3]));
    cnt = wave_sum(cnt);
    if (lane == 0) {
        red_v[wave] = sum;
        red_c[wave] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        const int c = (red_c[0] + red_c[1]) + (red_c[2] + red_c[3]);
        if (c > 0) {    // rho > 0 at every counted pixel: nothing to add otherwise
            const float v = (red_v[0] + red_v[1]) + (red_v[2] + red_v[3]);
            const long long q = (long long)__builtin_rintf(v * FIX_SCALE);
            __hip_atomic_fetch_add(P.acc + 2 * T.k, (unsigned long long)q, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(P.acc + 2 * T.k + 1, (unsigned long long)c, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Clears the accumulators of the sweep (a kernel, not a memset: common.h).
__global__ __launch_bounds__(kWave) void census_clear_kernel(const Params P)
{
    if (threadIdx.x < HEADER_ACC) P.acc[threadIdx.x] = 0;
    if (threadIdx.x < DVSOF_MAX_SCALES) P.factor[threadIdx.x] = 0.f;
}

// One wave behind the sweep (the kernel boundary orders it behind the atomics):
// lane k closes level k, the mean over the levels is taken in level order.
__global__ __launch_bounds__(kWave) void census_close_kernel(const Params P)
{
    const int k = threadIdx.x;
    double term = 0.0;
    if (k < P.K) {
        const double sum = (double)(long long)P.acc[2 * k] * FIX_INV;
        const unsigned long long c = P.acc[2 * k + 1];
        const double n = c > 0 ? (double)c : 1.0;
        term = sum / n;
        P.terms[k] = (float)term;
        P.factor[k] = (float)((double)P.weight / ((double)P.K * n));
    }
    double total = 0.0;
    for (int i = 0; i < P.K; ++i) total += __shfl(term, i, kWave);
    if (k == 0) P.value[0] = (float)((double)P.weight * (total / (double)P.K));
}

__global__ __launch_bounds__(NT) void census_bwd_kernel(const Params P)
{
    __shared__ float sA[NPIX], sB[NPIX], sR[NPIX];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const Tile T = find_tile(P, blockIdx.x);
    const Level &S = P.s[T.k];
    const int h = S.h, w = S.w;
    const size_t hw = (size_t)h * w;
    const float *A = S.frames + (size_t)P.start[T.n] * hw;
    const float *B = S.frames + (size_t)P.stop[T.n] * hw;
    const float *U = S.flow + (size_t)T.n * 2 * hw;
    const float *BW = S.bw + (size_t)T.n * hw, *RR = S.r + (size_t)T.n * hw;
    float *GU = S.grad + (size_t)T.n * 2 * hw;

    {
        float a[FILL], b[FILL], r[FILL];
#pragma unroll
        for (int it = 0; it < FILL; ++it) {
            const int i = tid + it * NT;
            const int ly = i / LW, lx = i - ly * LW;
            const int gy = T.ty0 + ly - RAD, gx = T.tx0 + lx - RAD;
            const bool in = (i < NPIX) & ((unsigned)gy < (unsigned)h) & ((unsigned)gx < (unsigned)w);
            const int o = in ? gy * w + gx : 0;
            a[it] = in ? A[o] : 0.f;
            b[it] = in ? BW[o] : 0.f;
            r[it] = in ? RR[o] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < FILL; ++it) {
            const int i = tid + it * NT;
            if (i >= NPIX) continue;
            sA[i] = a[it];
            sB[i] = b[it];
            sR[i] = r[it];
        }
    }

    // the derivative of the bilinear kernel at the strip's own pixels: issued
    // before the walk, which hides the flow -> taps round trips
    const int x = T.tx0 + lane, ly0 = wave * NP;
    float du[NP], dv[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int y = T.ty0 + ly0 + j;
        const bool live = (x < w) & (y < h);
        const int o = live ? y * w + x : 0;
        const float u = live ? U[o] : 0.f, v = live ? U[hw + o] : 0.f;
        const Taps t = gather_taps(B, h, w, x, y, u, v, live);
        du[j] = (1.f - t.fy) * (t.ne - t.nw) + t.fy * (t.se - t.sw);
        dv[j] = (1.f - t.fx) * (t.sw - t.nw) + t.fx * (t.se - t.ne);
    }
    __syncthreads();

    float cA[NP], cB[NP], cR[NP], g[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        cA[j] = sA[(ly0 + j + RAD) * LW + lane + RAD];
        cB[j] = sB[(ly0 + j + RAD) * LW + lane + RAD];
        cR[j] = sR[(ly0 + j + RAD) * LW + lane + RAD];
        g[j] = 0.f;
    }
#pragma unroll
    for (int dx = 0; dx < PATCH; ++dx) {
        float colA[NROW], colB[NROW], colR[NROW];
#pragma unroll
        for (int r = 0; r < NROW; ++r) {
            colA[r] = sA[(ly0 + r) * LW + lane + dx];
            colB[r] = sB[(ly0 + r) * LW + lane + dx];
            colR[r] = sR[(ly0 + r) * LW + lane + dx];
        }
#pragma unroll
        for (int j = 0; j < NP; ++j) {
#pragma unroll
            for (int dy = 0; dy < PATCH; ++dy) {
                if (dx == RAD && dy == RAD) continue;
                // centre e = the neighbour, offset d = q - e: D = I(q) - I(e)
                float ra, rb;
                const float ta = ternary(cA[j] - colA[j + dy], ra);
                const float tb = ternary(cB[j] - colB[j + dy], rb);
                const float df = ta - tb, s = df * df;
                const float rc = __builtin_amdgcn_rcpf(S_EPS + s);
                const float dg = (S_EPS * rc) * rc;             // d (s / (0.1 + s)) / d s
                const float dt = (T_EPS * rb) * (rb * rb);      // d t / d D at D_Bw
                const float c = ((-2.f * df) * dg) * dt;        // d dist(e) / d Bw(q)
                g[j] = g[j] + c * (colR[j + dy] + cR[j]);
            }
        }
    }
    const float scale = P.seed[0] * P.factor[T.k];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int y = T.ty0 + ly0 + j;
        if (x < w && y < h) {
            const float G = scale * g[j];
            GU[y * w + x] = G * du[j];
            GU[hw + y * w + x] = G * dv[j];
        }
    }
}

// workspace: [acc 16 u64][factor 8 f32][per level: Bw N*h*w f32, r N*h*w f32]
int build_params(const dvsof_loss_scale_t *sc, int K, int N, void *ws, Params &P, int &total_blocks,
                 size_t &bytes)
{
    if (!sc || K < 1 || K > DVSOF_MAX_SCALES || N < 1) return DVSOF_EINVAL;
    P.K = K;
    P.N = N;
    long long begin = 0;
    size_t o = HEADER_BYTES;
    for (int k = 0; k < K; ++k) {
        const int h = sc[k].h, w = sc[k].w;
        if (h < 1 || w < 1 || (long long)h * w >= (1ll << 30) || !sc[k].frames || !sc[k].flow)
            return DVSOF_EINVAL;
        Level &S = P.s[k];
        S.frames = sc[k].frames;
        S.flow = sc[k].flow;
        S.grad = sc[k].grad_flow;
        S.h = h;
        S.w = w;
        S.tiles_x = (w + TW - 1) / TW;
        S.tiles_per_sample = S.tiles_x * ((h + TH - 1) / TH);
        S.block_begin = (int)begin;
        begin += (long long)N * S.tiles_per_sample;
        if (begin > 0x7fffffffll) return DVSOF_EINVAL;
        const size_t plane = (size_t)N * h * w * sizeof(float);
        S.bw = (float *)((char *)ws + o);
        S.r = (float *)((char *)ws + o + plane);
        o += 2 * plane;
    }
    P.acc = (unsigned long long *)ws;
    P.factor = (float *)((char *)ws + HEADER_ACC * sizeof(unsigned long long));
    total_blocks = (int)begin;
    bytes = o;
    return DVSOF_OK;
}

}  // namespace

extern "C" {

size_t dvsof_census_workspace_bytes(const dvsof_loss_scale_t *sc, int K, int N)
{
    Params P = {};
    int nb = 0;
    size_t bytes = 0;
    if (build_params(sc, K, N, nullptr, P, nb, bytes) != DVSOF_OK) return 0;
    return bytes;
}

int dvsof_census_fwd(const dvsof_loss_scale_t *sc, int K, int N, const int32_t *start, const int32_t *stop,
                     float weight, float *terms, float *value, void *ws, size_t ws_bytes, void *stream)
{
    Params P = {};
    int nb = 0;
    size_t bytes = 0;
    const int rc = build_params(sc, K, N, ws, P, nb, bytes);
    if (rc) return rc;
    if (!start || !stop || !terms || !value) return DVSOF_EINVAL;
    if (!ws || ws_bytes < bytes) return DVSOF_ENOSPACE;
    P.start = start;
    P.stop = stop;
    P.terms = terms;
    P.value = value;
    P.weight = weight;
    hipLaunchKernelGGL(census_clear_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), P);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(census_fwd_kernel, dim3(nb), dim3(NT), 0, as_stream(stream), P);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(census_close_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), P);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_census_bwd(const dvsof_loss_scale_t *sc, int K, int N, const int32_t *start, const int32_t *stop,
                     const float *seed, void *ws, size_t ws_bytes, void *stream)
{
    Params P = {};
    int nb = 0;
    size_t bytes = 0;
    const int rc = build_params(sc, K, N, ws, P, nb, bytes);
    if (rc) return rc;
    if (!start || !stop || !seed) return DVSOF_EINVAL;
    for (int k = 0; k < K; ++k)
        if (!sc[k].grad_flow) return DVSOF_EINVAL;
    if (!ws || ws_bytes < bytes) return DVSOF_ENOSPACE;
    P.start = start;
    P.stop = stop;
    P.seed = seed;
    hipLaunchKernelGGL(census_bwd_kernel, dim3(nb), dim3(NT), 0, as_stream(stream), P);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
