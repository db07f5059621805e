// The two terms of the multi-scale loss that read no frame -- Charbonnier
// smoothness and the out-of-border regulariser -- forward and analytic
// backward, all scales in one sweep: the loss of a training run from an
// event-only recording (include/dvsof_loss_frameless.h, docs/FRAMELESS_SPEC.md).
//
// Replaces (reference paths): utils/loss.py:76-90 (smoothness), :92-119
// (out-of-border) and the autograd backward through them.
//
// This is loss.hip without its photometric half: no pyramid, no frame reads,
// no bilinear gather.  The arithmetic of what remains is loss.hip's, restated
// here op for op (the helpers are kept local so that loss.hip's kernels stay
// the instructions they are): warp_grid / div_exact in float32, the strict +-1
// comparison, the exp2(-0.55 log2 s) power, every neighbour pair evaluated ONCE
// at its anchor pixel, the per-sample normaliser 1 / (2 c_n N).
// Three launches per evaluation, kernels only:
//   A  frameless_count_kernel: out-of-border pixels per tile (plain stores, no
//      atomics, nothing to zero); workgroup 0 clears the group accumulators of
//      launch B.  The border gradient needs a sample's count before the sweep;
//   B  frameless_sweep_kernel: all scales, forward sums and flow gradients;
//   C  frameless_close_kernel: one workgroup (a wave per scale) combines the
//      per-group sums, applies the normalisers, writes terms, loss and counts.
// Layout and tiling as in loss.hip: flow [N,2,h,w] row-major; a 256-thread
// workgroup owns a 64x16 pixel tile of one sample at one scale, wave v rows
// 4v..4v+3, lane l column l; the flow tile + 1 px halo is staged in LDS.
// Reduction: a workgroup adds its 6 sums into its (scale, sample) group's
// 64-bit FIXED-POINT accumulators (2^-20; integer atomics without return) --
// integer addition commutes, so the totals are bitwise reproducible whatever
// the arrival order; the kernel boundary orders launch C behind them.  No
// float atomics anywhere.
#include "common.h"
#include "../../include/dvsof_loss_frameless.h"

namespace {

constexpr int TW = 64, TH = 16, NT = 256;
constexpr int LW = TW + 2, LH = TH + 2;
constexpr int NW = NT / kWave;
constexpr int NSUM = 6;     // smooth x4 (->, v, \, /), border sum, border count
constexpr int NGROUP = 8;   // accumulators per group: the 6 sums + pad (64 contiguous bytes)
constexpr float FIX_SCALE = 1048576.f;              // 2^20
constexpr double FIX_INV = 1.0 / 1048576.0;

struct ScaleDev {
    const float *flow;
    float *grad;
    int h, w;
    int tiles_x, tiles_per_sample, block_begin;
    float half_w, half_h;          // (w-1)/2, (h-1)/2 (utils/loss.py:152-154)
    float rcp_half_w, rcp_half_h;  // correctly rounded reciprocals (0 when the side is 1)
    float k_smooth[3];             // 1/(4*count) for ->, v, diagonal crops
    double c_smooth[3];            // crop element counts (utils/loss.py:77-85)
};

struct Params {
    ScaleDev s[DVSOF_MAX_SCALES];
    int K, N;
    int32_t *oob;               // [K*N] out-of-border pixels per (scale, sample), written by launch C
    int32_t *oob_tile;          // [nb] the same per tile (launch A)
    unsigned long long *gacc;   // [K*N][NGROUP] group sums, 2^-20 fixed point (two's complement)
    float seed_smooth, seed_border;     // w / K * loss_scale
    float *terms, *loss_out;
    float w_smooth, w_border, loss_scale;
};

__device__ __forceinline__ int find_scale(const Params &P, int bid)
{
    int k = 0;
#pragma unroll
    for (int i = 1; i < DVSOF_MAX_SCALES; ++i)
        if (i < P.K && bid >= P.s[i].block_begin) k = i;
    return k;
}

// a / b correctly rounded from r = RN(1/b) (Markstein; see loss.hip): the bits of IEEE `/`
__device__ __forceinline__ float div_exact(float a, float b, float r)
{
    const float q0 = a * r;
    const float e = __builtin_fmaf(-b, q0, a);
    return __builtin_fmaf(e, r, q0);
}

// utils/loss.py:150-156 in fp32, op for op
__device__ __forceinline__ void warp_grid(const ScaleDev &S, int x, int y, float u, float v,
                                          float &gx, float &gy)
{
    gx = div_exact((float)x + u, S.half_w, S.rcp_half_w) - 1.f;
    gy = div_exact((float)y + v, S.half_h, S.rcp_half_h) - 1.f;
}
__device__ __forceinline__ bool out_of_border(float gx, float gy)
{  // utils/loss.py:92-94 (strict)
    return (gx < -1.f) | (gx > 1.f) | (gy < -1.f) | (gy > 1.f);
}

__device__ __forceinline__ void accumulate(unsigned long long *p, float v)
{
    const long long q = (long long)__builtin_rintf(v * FIX_SCALE);
    __hip_atomic_fetch_add(p, (unsigned long long)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double group_value(const unsigned long long *p)
{
    return (double)(long long)*p * FIX_INV;
}

// ---- launch A: per-tile out-of-border counts, one int per tile ----------------------------
__global__ __launch_bounds__(NT) void frameless_count_kernel(const Params P)
{
    __shared__ int red[NW];
    const int tid = threadIdx.x, bid = blockIdx.x;
    if (bid == 0)       // group accumulators of the sweep that follows
        for (int i = tid; i < P.K * P.N * NGROUP; i += NT) P.gacc[i] = 0ull;
    const int k = find_scale(P, bid);
    const ScaleDev &S = P.s[k];
    const int local = bid - S.block_begin;
    const int n = local / S.tiles_per_sample;
    const int t = local - n * S.tiles_per_sample;
    const int ty0 = (t / S.tiles_x) * TH, tx0 = (t % S.tiles_x) * TW;
    const int h = S.h, w = S.w;
    const size_t hw = (size_t)h * w;
    const float *U = S.flow + (size_t)n * 2 * hw;
    const int x = tx0 + (tid & (TW - 1)), tr = tid >> 6;
    int cnt = 0;
    float uu[TH / 4], vv[TH / 4];       // all eight loads first (clamped addresses)
    const int xc = min(x, w - 1);
#pragma unroll
    for (int j = 0; j < TH / 4; ++j) {
        const size_t o = (size_t)min(ty0 + tr + 4 * j, h - 1) * w + xc;
        uu[j] = U[o];
        vv[j] = U[hw + o];
    }
#pragma unroll
    for (int j = 0; j < TH / 4; ++j) {
        const int y = ty0 + tr + 4 * j;
        float gx, gy;
        warp_grid(S, x, y, uu[j], vv[j], gx, gy);
        cnt += ((y < h) & (x < w) & out_of_border(gx, gy)) ? 1 : 0;
    }
    cnt = wave_sum(cnt);
    if ((tid & (kWave - 1)) == 0) red[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) P.oob_tile[bid] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- launch B: the sweep -------------------------------------------------------------------
__global__ __launch_bounds__(NT) void frameless_sweep_kernel(const Params P)
{
    // flow tile + 1-pixel halo, (u, v) interleaved; padded to FILL x NT entries: the fill
    // writes unconditionally
    constexpr int FILL = (LH * LW + NT - 1) / NT;
    __shared__ f32x2 sF[FILL * NT];
    __shared__ float red[NW][NGROUP];
    __shared__ int s_cnt[NW];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int bid = blockIdx.x;
    const int k = find_scale(P, bid);
    const ScaleDev &S = P.s[k];
    const int local = bid - S.block_begin;
    const int n = local / S.tiles_per_sample;
    const int t = local - n * S.tiles_per_sample;
    const int ty0 = (t / S.tiles_x) * TH, tx0 = (t % S.tiles_x) * TW;
    const int h = S.h, w = S.w;
    const size_t hw = (size_t)h * w;
    const float *U = S.flow + (size_t)n * 2 * hw;

    // flow tile + halo -> LDS, loads first.  Entries outside the frame read as zero through
    // the buffer range check (an offset past the sample's two planes)
    {
        const __amdgpu_buffer_rsrc_t rf =
            __builtin_amdgcn_make_buffer_rsrc((void *)U, 0, (int)(2 * hw * 4), 0x00020000);
        constexpr unsigned OOB = 0xffffffffu;
        float fu[FILL], fv[FILL];
#pragma unroll
        for (int it = 0; it < FILL; ++it) {
            const int i = tid + it * NT;
            const int ly = i / LW, lx = i - ly * LW;
            const int gy = ty0 + ly - 1, gx = tx0 + lx - 1;
            const bool in = (i < LH * LW) & ((unsigned)gy < (unsigned)h) & ((unsigned)gx < (unsigned)w);
            const unsigned o = (unsigned)((gy * w + gx) * 4);
            fu[it] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rf, in ? o : OOB, 0, 0));
            fv[it] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rf, in ? o + (unsigned)(hw * 4) : OOB, 0, 0));
        }
#pragma unroll
        for (int it = 0; it < FILL; ++it) sF[tid + it * NT] = f32x2{fu[it], fv[it]};
    }
    auto F2 = [&](int ly, int lx) -> f32x2 { return sF[ly * LW + lx]; };
    // the sample's out-of-border count: integer sum of the per-tile counts of launch A, any order
    float k_border;
    {
        int c = 0;
        const int32_t *ot = P.oob_tile + S.block_begin + n * S.tiles_per_sample;
        for (int b = tid; b < S.tiles_per_sample; b += NT) c += ot[b];
        c = wave_sum(c);
        if (lane == 0) s_cnt[wave] = c;
        __syncthreads();        // also: the LDS tile is complete
        const int cnt = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        k_border = cnt > 0 ? P.seed_border / (2.f * (float)cnt * (float)P.N) : 0.f;
    }

    float acc[NSUM] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int x = tx0 + lane;
    const int ly0 = wave * 4;            // tile-local row of the strip's first pixel
    constexpr int NP = 4;                // pixels per thread: rows ly0 .. ly0 + 3
    bool valid[NP];
    float gu[NP], gv[NP];

    // out-of-border, utils/loss.py:96-119
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int y = ty0 + ly0 + j;
        valid[j] = (y < h) & (x < w);
        gu[j] = gv[j] = 0.f;
        const f32x2 uv = F2(ly0 + j + 1, lane + 1);
        float gx, gy;
        warp_grid(S, x, y, uv.x, uv.y, gx, gy);
        if (valid[j] && out_of_border(gx, gy)) {
            const Charb bu = charbonnier(uv.x), bv = charbonnier(uv.y);
            acc[4] += bu.val + bv.val;
            acc[5] += 1.f;
            gu[j] += k_border * bu.der;
            gv[j] += k_border * bv.der;
        }
    }

    // left-edge column (x = tx0 - 1) derivatives the strip's lane 0 needs: lane
    // 12 c + 4 kind + r (< 24) of every wave evaluates one -- kind 0: d0(r, xe),
    // 1: d2(r-1, xe), 2: d3(r, xe) -- and lane 0 picks them up with v_readlane
    float edge;
    {
        const int l = lane < 24 ? lane : 0;
        const int c = l / 12, q = l - 12 * c, kind = q >> 2, r = q & 3;
        const int db = kind == 1 ? -1 : (kind == 2 ? 1 : 0);
        const int ya = ty0 + ly0 + r, yb = ya + db;
        const bool ok = (tx0 >= 1) & (ya >= 0) & (ya < h) & (yb >= 0) & (yb < h);
        const f32x2 fa2 = F2(ly0 + r + 1, 1), fb2 = F2(ly0 + r + 1 + db, 0);
        const float fa = c ? fa2.y : fa2.x, fb = c ? fb2.y : fb2.x;
        edge = ok ? charbonnier(fa - fb).der : 0.f;
    }
    const int edge_bits = __builtin_bit_cast(int, edge);
    auto edge_at = [&](int src) -> float {      // uniform value of lane `src`
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(edge_bits, src));
    };

    // smoothness, utils/loss.py:76-90.  Anchor (r, x), r = -1..3 relative to the
    // strip: d0 = rho'(F[r][x+1] - F[r][x]), d1 = rho'(F[r+1][x] - F[r][x]),
    // d2 = rho'(F[r+1][x+1] - F[r][x]), d3 = rho'(F[r][x+1] - F[r+1][x]).
    // Pixel (r, x) is the SECOND operand of its own d0, d1, d2, the FIRST of
    // d0(r, x-1), d1(r-1, x), d2(r-1, x-1), d3(r, x-1), the SECOND of d3(r-1, x).
    // Branch-free: the LDS halo is zero-filled outside the frame, so every pair
    // is evaluated and then multiplied by its 0/1 validity.
    {
        const float mx = x < w ? 1.f : 0.f, mxr = x + 1 < w ? 1.f : 0.f;
        float mrow[6];                     // rows -1..4 of the strip inside the frame
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const int y = ty0 + ly0 + r - 1;
            mrow[r] = ((y >= 0) & (y < h)) ? 1.f : 0.f;
        }
        f32x2 s1 = {0.f, 0.f}, s2 = s1, s3 = s1, s4 = s1;
        f32x2 p0 = F2(ly0, lane + 1);     // row -1: columns x, x + 1
        f32x2 p1 = F2(ly0, lane + 2);
        f32x2 d1p = s1, d2p = s1, d3p = s1;                           // anchor row r - 1
        const float k0 = S.k_smooth[0] * P.seed_smooth, k1 = S.k_smooth[1] * P.seed_smooth,
                    k2 = S.k_smooth[2] * P.seed_smooth;
#pragma unroll
        for (int r = 0; r < 5; ++r) {          // anchor strip row r - 1
            const f32x2 n0 = F2(ly0 + r + 1, lane + 1);
            const f32x2 n1 = F2(ly0 + r + 1, lane + 2);
            const bool own = r >= 1;           // anchor row of this strip: sums count
            const float m0 = mrow[r] * mxr, mv = mrow[r] * mrow[r + 1];
            const float m1 = mv * mx, m2 = mv * mxr;
            f32x2 d0c = {0.f, 0.f};
            if (own) {
                const Charb2 q = charbonnier2(p1 - p0);
                s1 += q.val * m0;
                d0c = q.der * m0;
            }
            const Charb2 q1 = charbonnier2(n0 - p0);
            const Charb2 q2 = charbonnier2(n1 - p0);
            const Charb2 q3 = charbonnier2(p1 - n0);
            if (own) {
                s2 += q1.val * m1;
                s3 += q2.val * m2;
                s4 += q3.val * m2;
            }
            const f32x2 d1c = q1.der * m1, d2c = q2.der * m2, d3c = q3.der * m2;
            if (own) {
                const int j = r - 1;
                // from the column to the left: lane - 1 by a DPP wave shift (wave_shr:1);
                // lane 0 keeps the shift's `old` operand = the edge column's value
                auto from_left = [&](float v, int src) -> float {
                    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
                        __builtin_bit_cast(int, edge_at(src)), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
                };
                const f32x2 in0 = {from_left(d0c.x, j), from_left(d0c.y, 12 + j)};
                const f32x2 in2 = {from_left(d2p.x, 4 + j), from_left(d2p.y, 16 + j)};
                const f32x2 in3 = {from_left(d3c.x, 8 + j), from_left(d3c.y, 20 + j)};
                const f32x2 g = (in0 - d0c) * k0 + (d1p - d1c) * k1 + ((in2 - d2c) + (in3 - d3p)) * k2;
                gu[j] += g.x;
                gv[j] += g.y;
            }
            d1p = d1c;
            d2p = d2c;
            d3p = d3c;
            p0 = n0;
            p1 = n1;
        }
        acc[0] = s1.x + s1.y;
        acc[1] = s2.x + s2.y;
        acc[2] = s3.x + s3.y;
        acc[3] = s4.x + s4.y;
    }

    // ---- tail: every wave stores its gradients; wave 0 adds the workgroup's sums to its
    // group's accumulators.  Pixels outside the frame get an offset past the sample's two
    // planes: the buffer range check drops the store
    {
        const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(S.grad + (size_t)n * 2 * hw), 0, (int)(2 * hw * 4), 0x00020000);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const unsigned o = valid[j] ? (unsigned)(((ty0 + ly0 + j) * w + x) * 4) : 0xffffffffu;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, gu[j]), rg, o, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, gv[j]), rg,
                                                  valid[j] ? o + (unsigned)(hw * 4) : 0xffffffffu, 0, 0);
        }
    }
#pragma unroll
    for (int i = 0; i < NSUM; ++i) {
        const float v = wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (wave == 0 && lane < NSUM)
        accumulate(P.gacc + ((size_t)k * P.N + n) * NGROUP + lane,
                   (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]));
}

// ---- launch C: one workgroup, wave v the scales v, v + 4.  A group's 8 accumulators are 64
// contiguous bytes: lane l reads element l % 8 of sample 8 j + l / 8; lanes of equal l % 8 add
// their samples in j order and the eight lane groups meet by three shuffle steps.  Elements
// 0..3: sums over the samples of the four smoothness directions (exact multiples of 2^-20 in
// double: exact, whatever the order); element 4: border term = sum_n bs_n / (2 c_n N) with
// c_n = element 5 of the same sample (utils/loss.py:101,113), in the fixed order above.
__global__ __launch_bounds__(NT) void frameless_close_kernel(const Params P)
{
    __shared__ double s_tot[DVSOF_MAX_SCALES][2];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6, e = lane & 7, g = lane >> 3;
    constexpr int UB = 8;       // sample blocks of 8 per pass: UB loads in flight per lane
    for (int kk = wave; kk < P.K; kk += NW) {
        double acc = 0;
        for (int n0 = 0; n0 < P.N; n0 += 8 * UB) {
            double x[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int nn = min(n0 + 8 * u + g, P.N - 1);
                x[u] = group_value(P.gacc + ((size_t)kk * P.N + nn) * NGROUP + e);
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int nn = n0 + 8 * u + g;
                const double c = __shfl(x[u], (lane & ~7) | 5, kWave);    // the sample's count
                if (nn >= P.N) continue;
                if (e < 4) acc += x[u];
                else if (e == 4 && c > 0) acc += x[u] / (2.0 * c * (double)P.N);
                else if (e == 5) P.oob[kk * P.N + nn] = (int)c;
            }
        }
        acc += __shfl_xor(acc, 8, kWave);
        acc += __shfl_xor(acc, 16, kWave);
        acc += __shfl_xor(acc, 32, kWave);
        double a5[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) a5[j] = __shfl(acc, j, kWave);
        if (lane == 0) {
            const ScaleDev &S = P.s[kk];
            // empty crops contribute 0 (utils/loss.py:29-30)
            const double sm = ((S.c_smooth[0] > 0 ? a5[0] / S.c_smooth[0] : 0) +
                               (S.c_smooth[1] > 0 ? a5[1] / S.c_smooth[1] : 0) +
                               (S.c_smooth[2] > 0 ? (a5[2] + a5[3]) / S.c_smooth[2] : 0)) / 4.0;
            const double border = a5[4];
            P.terms[0 * P.K + kk] = (float)sm;
            P.terms[1 * P.K + kk] = 0.f;        // no photometric term: +0
            P.terms[2 * P.K + kk] = (float)border;
            s_tot[kk][0] = sm;
            s_tot[kk][1] = border;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total[2] = {0, 0};
        for (int kk = 0; kk < P.K; ++kk)
            for (int i = 0; i < 2; ++i) total[i] += s_tot[kk][i];
        P.loss_out[0] = (float)((P.w_smooth * total[0] + P.w_border * total[1]) / (double)P.K *
                                (double)P.loss_scale);
    }
}

int build_params(const dvsof_loss_scale_t *sc, int K, int N, Params &P, int &total_blocks)
{
    if (!sc || K < 1 || K > DVSOF_MAX_SCALES || N < 1) return DVSOF_EINVAL;
    P.K = K;
    P.N = N;
    long long begin = 0;
    for (int k = 0; k < K; ++k) {
        const int h = sc[k].h, w = sc[k].w;
        if (h < 1 || w < 1 || !sc[k].flow || !sc[k].grad_flow) return DVSOF_EINVAL;
        // (byte offsets inside a sample's two planes are 32-bit in the kernels)
        if ((long long)h * w > 0x0fffffff) return DVSOF_EINVAL;
        ScaleDev &S = P.s[k];
        S.flow = sc[k].flow;
        S.grad = sc[k].grad_flow;
        S.h = h;
        S.w = w;
        S.tiles_x = (w + TW - 1) / TW;
        S.tiles_per_sample = S.tiles_x * ((h + TH - 1) / TH);
        S.block_begin = (int)begin;
        begin += (long long)N * S.tiles_per_sample;
        if (begin > 0x3fffffff) return DVSOF_EINVAL;
        S.half_w = (float)((w - 1) / 2.0);
        S.half_h = (float)((h - 1) / 2.0);
        // RN(1/b) via double: b = m/2 with m < 2^24 an integer, so no double-rounding tie
        S.rcp_half_w = w > 1 ? (float)(1.0 / (double)S.half_w) : 0.f;
        S.rcp_half_h = h > 1 ? (float)(1.0 / (double)S.half_h) : 0.f;
        S.c_smooth[0] = (double)N * 2 * h * (w - 1);
        S.c_smooth[1] = (double)N * 2 * (h - 1) * w;
        S.c_smooth[2] = (double)N * 2 * (h - 1) * (w - 1);
        for (int i = 0; i < 3; ++i)
            S.k_smooth[i] = S.c_smooth[i] > 0 ? (float)(1.0 / (4.0 * S.c_smooth[i])) : 0.f;
    }
    total_blocks = (int)begin;
    return DVSOF_OK;
}

// workspace: [gacc K*N*NGROUP u64][oob_tile nb i32]
size_t ws_layout(int nb, int K, int N, size_t &tile_off)
{
    size_t o = (size_t)K * N * NGROUP * sizeof(unsigned long long);
    tile_off = o;
    o += (size_t)nb * sizeof(int32_t);
    return ((o + 15) & ~(size_t)15) + 16;
}

}  // namespace

extern "C" {

size_t dvsof_loss_frameless_workspace_bytes(const dvsof_loss_scale_t *sc, int K, int N)
{
    Params P = {};
    int nb = 0;
    if (build_params(sc, K, N, P, nb) != DVSOF_OK) return 0;
    size_t t;
    return ws_layout(nb, K, N, t);
}

int dvsof_loss_frameless(const dvsof_loss_scale_t *sc, int K, int N, const float *w, float loss_scale,
                         float *terms, float *loss_out, int32_t *oob, void *ws, size_t ws_bytes,
                         void *stream)
{
    Params P = {};
    int nb = 0;
    const int rc = build_params(sc, K, N, P, nb);
    if (rc) return rc;
    if (!w || !terms || !loss_out || !oob) return DVSOF_EINVAL;
    size_t t;
    if (!ws || ws_bytes < ws_layout(nb, K, N, t)) return DVSOF_ENOSPACE;
    P.gacc = (unsigned long long *)ws;
    P.oob_tile = (int32_t *)((char *)ws + t);
    P.oob = oob;
    P.terms = terms;
    P.loss_out = loss_out;
    P.w_smooth = w[0];
    P.w_border = w[1];
    P.loss_scale = loss_scale;
    P.seed_smooth = w[0] / (float)K * loss_scale;
    P.seed_border = w[1] / (float)K * loss_scale;
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(frameless_count_kernel, dim3(nb), dim3(NT), 0, st, P);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(frameless_sweep_kernel, dim3(nb), dim3(NT), 0, st, P);
    DVSOF_LAUNCH_CHECK();
    hipLaunchKernelGGL(frameless_close_kernel, dim3(1), dim3(NT), 0, st, P);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

}  // extern "C"
