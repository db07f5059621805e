// The general weight gradient's plan: which kernels a launch runs, with what tile, K splits and
// workspace layout, decided ONCE per call by wgrad_plan and read by everything else
// (wgrad_launch, the workspace and tile queries of conv_api.hip).  Pure host code: shape tests,
// split rules and tuning switches, no kernel and no HIP call.
//
// The families: v1 tiles (wgrad.hip, exact f32, any geometry), v2 (wgrad2.hip, LDS-DMA, rows of
// whole 16-pixel groups), the patch-resident kernels of the decoder stages on bf16 twins or in
// exact f32 (wgrad_patch.hip), the nine-product form of the latter (wgrad_min.hip), and the flat
// members' VALU / matrix-core kernels (wgrad.hip).
#include "conv_host.h"
#include <stdlib.h>

namespace {

int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

void tile_dims(int tile, int &bm, int &bn)
{
    switch (tile) {
    case 1: bm = 128; bn = 128; break;
    case 2: bm = 128; bn = 64; break;
    case 3: bm = 64; bn = 64; break;
    case 4: bm = 64; bn = 128; break;
    default: bm = 32; bn = 128; break;
    }
}

// (tile, K splits) by a small occupancy model.  A CU runs `slots` workgroups of a
// tile at once (LDS ring footprint); workgroups are dealt round-robin to 256
// CUs, so the launch ends when the fullest CU has worked through its k blocks:
//   g(k) = full rounds of `slots` blocks + the last partial round, where a lone
//   block on a CU only reaches ~80 % of the matrix rate.
// Cost = (K steps per block + fixed prologue/epilogue) * g * step time / tile
// efficiency + the slab write/read when there is more than one slab.
// (Residual layers, 144 tiles of 128x128: S=4 -> 576 blocks on 512 slots ran
// 123 us, S=3 -> 432 blocks 105 us.)
int pick_tile_and_splits(const WGradParams &P, int *S_out)
{
    const int taps = P.ks * P.ks;
    static const int cand[5] = {1, 4, 3, 5, 2};
    static const int slots_of[6] = {0, 2, 3, 5, 3, 3};          // by tile id
    // (64x64 is 2.6-3 % faster than 64x128 on the three wide decoder layers one at a time,
    // tools/wgrad_sweep.sh, but beside the data-gradient stream the step then alternates
    // between 2340 and 2470 samples/s from run to run; 64x128 gives a steady 2445)
    static const double eff_of[6] = {0, 0.85, 0.80, 0.70, 0.80, 0.65};
    int best = -1, bestS = 1;
    double best_cost = 1e300;
    const long long ksteps = (P.M + BK - 1) / BK;
    for (int i = 0; i < 5; ++i) {
        int bm, bn;
        tile_dims(cand[i], bm, bn);
        if (bm > 32 && bm / 2 >= P.Cout) continue;      // mostly padding rows
        long long tiles = 0;
        for (int s = 0; s < P.nsrc; ++s)
            if (!P.src[s].flat) tiles += (taps * P.src[s].C + bn - 1) / bn;
        if (tiles == 0)
            for (int s = 0; s < P.nsrc; ++s) tiles += (taps * P.src[s].C + bn - 1) / bn;
        const long long rows = (P.Cout + bm - 1) / bm;
        tiles *= rows * P.nph;
        const int slots = slots_of[cand[i]];
        const double step_us = 2.0 * bm * bn * BK / (157.3e12 / 256) * 1e6 / eff_of[cand[i]];
        int maxS = (int)((P.M + 511) / 512);              // >= 32 K steps per split
        if (maxS > 64) maxS = 64;
        if (maxS < 1) maxS = 1;
        for (int S = 1; S <= maxS; ++S) {
            const long long blocks = tiles * S;
            const long long kmax = (blocks + 255) / 256;  // blocks on the fullest CU
            const long long full = kmax / slots, r = kmax % slots;
            const double g = (double)full * slots + (r == 1 ? 1.25 : (double)r);
            const double steps = (double)((ksteps + S - 1) / S) + 4.0;
            const double slab = (S * P.nph > 1)
                                    ? 2.0 * S * P.nph * P.Cout * taps * (double)P.Cin_tot * 4.0 / 4e6
                                    : 0.0;                 // us at ~4 TB/s
            const double cost = steps * g * step_us + slab;
            if (cost < best_cost) {
                best_cost = cost;
                best = cand[i];
                bestS = S;
            }
        }
    }
    if (S_out) *S_out = bestS;
    return best;
}

// ---- flat members (2-channel flow, voxel grid) on kernels of their own ------------------------
bool flat_ncol_ok(int ncol)
{
    return ncol == 18 || ncol == 27 || ncol == 45 || ncol == 81 || ncol == 108;
}

// Does this flat member take the matrix-core kernel?
// measured (batch 8): MFMA 33 vs VALU 46 us at M = 524288 / 18 columns, 39 vs 52 us at
// M = 131072 / 45 columns; a tie at M = 131072 / 18 columns; VALU wins below
bool flat_uses_mfma(const FlatWG &F)
{
    const int ncb = (F.ncol + 31) / 32;
    const bool big = F.M >= 262144 || (ncb == 2 && F.M >= 65536);
    return big && (F.Cout % 32) == 0 && ncb <= 2 && F.Wo >= 2;
}

// ---- the patch-resident kernels ---------------------------------------------------------------
// Decoder stages: four sub-pixel phases of 2x2 taps over vector members whose channel counts
// are multiples of 32, 32 | Cout, 16 | width (otherwise: the column-tile kernel).
// The shape alone: what sizing mode plans for, whether or not the twins are bound yet.
bool patch_shape_ok(const WGradParams &P)
{
    if (P.nph != 4 || P.ks != 2 || P.stride != 1 || P.up != UP_NONE) return false;
    if (P.ph_pad != 1 || P.pad != 1 || P.src_ph_stride != 0) return false;
    if ((P.Cout & 31) || (P.Wo % 16) || (P.Ho & 1) || P.Ho != P.Hv || P.Wo != P.Wv) return false;
    // flat members (the 2-channel flow of a decoder stage) are not this kernel's: their
    // columns belong to the caller (dvsof_flow_fold_grads) or to the flat-member kernels
    int nvec = 0;
    for (int s = 0; s < P.nsrc; ++s) {
        if (P.src[s].flat) continue;
        if (P.src[s].sc != 1 || (P.src[s].C & 31)) return false;
        ++nvec;
    }
    return nvec >= 1;
}

// exact-f32 operand mode: wgrad_patch_f32_kernel
bool patch_f32(const WGradParams &P) { return !P.twins && P.mfma_bf16 == 0; }

// ... and the call's pointers: the twins bound, or 16-byte loads of the f32 tensors
bool patch_eligible(const WGradParams &P)
{
    if (!patch_shape_ok(P)) return false;
    if (patch_f32(P)) {
        if (!P.gout || (reinterpret_cast<uintptr_t>(P.gout) & 15)) return false;
        if ((P.g_sb | P.g_sy | P.g_sx | P.g_py | P.g_px) & 3) return false;
        for (int s = 0; s < P.nsrc; ++s)
            if (!P.src[s].flat && (!P.src[s].p || (reinterpret_cast<uintptr_t>(P.src[s].p) & 15) ||
                                   ((P.src[s].sb | P.src[s].sy | P.src[s].sx) & 3)))
                return false;
        return true;
    }
    if (!P.twins || !P.gout16) return false;
    for (int s = 0; s < P.nsrc; ++s)
        if (!P.src[s].flat && !P.src[s].p16) return false;
    return true;
}

// The exact-f32 decoder stages take the nine-product kernel when every vector member has a
// multiple of 64 channels (otherwise: the sixteen-product patch kernel)
bool min9_ok(const WGradParams &P)
{
    if (!patch_f32(P)) return false;
    for (int s = 0; s < P.nsrc; ++s)
        if (!P.src[s].flat && (P.src[s].C & 63)) return false;
    return true;
}

// Bound on the K splits: >= 2 stages per split; a slab is a whole phase-form gradient -- at
// most ~32 MB of partial sums per layer, and no more than 64 slabs per phase (the fold reads
// them all)
long long patch_max_splits(const WGradParams &P)
{
    const long long blocks = (long long)P.B * (P.Hv / 2) * (P.Wv / 16);
    long long maxS = blocks / 2 > 0 ? blocks / 2 : 1;
    const long long slab_bytes = 4LL * P.Cout * 4 * P.Cin_tot * 4;
    long long capS = (32LL << 20) / (slab_bytes > 0 ? slab_bytes : 1);
    if (capS > 64) capS = 64;
    if (capS < 1) capS = 1;
    return maxS < capS ? maxS : capS;
}

// 64 input channels per workgroup halve the gradient planes' re-reads
int patch_channel_tile(const WGradParams &P)
{
    long long ct = 0;
    for (int s = 0; s < P.nsrc; ++s) {
        if (P.src[s].flat) continue;
        if (P.src[s].C & 63) return 32;
        ct += P.src[s].C / 64;
    }
    // exact f32: matrix-bound once the planes are read half as often -- as long as one
    // workgroup per CU remains
    if (patch_f32(P)) return (P.Cout / 32) * ct * patch_max_splits(P) >= 256 ? 64 : 32;
    // bf16 twins, measured (batch 8, the four decoder stages): 32 wins everywhere -- the slab
    // bound on the K splits leaves the 64-channel form with 224-256 workgroups
    return 32;
}

// K splits of the patch-resident kernels (workgroups are K splits there).  Nine-product: one
// workgroup (8 waves) per CU, >= 2 blocks per split, <= 128 slabs.  Patch kernels: enough
// workgroups for two per CU.
int patch_splits(const WGradParams &P)
{
    const bool min9 = min9_ok(P);
    const int CT = min9 ? WG_MIN_CT : patch_channel_tile(P);
    long long tiles = 0;
    for (int s = 0; s < P.nsrc; ++s)
        if (!P.src[s].flat) tiles += P.src[s].C / CT;
    tiles *= P.Cout / 32;
    long long S;
    if (min9) {
        S = (256 + tiles - 1) / (tiles > 0 ? tiles : 1);
        const long long blocks = (long long)P.B * (P.Hv / 2) * (P.Wv / 16);
        if (S > blocks / 2) S = blocks / 2;
        if (S > 128) S = 128;
    } else {
        S = (512 + tiles - 1) / tiles;
        const long long maxS = patch_max_splits(P);
        if (S > maxS) S = maxS;
    }
    return S < 1 ? 1 : (int)S;
}

// the column-tile kernels' own rule, with the sweeps' overrides (tools/wgrad_sweep.sh):
// DVSOF_WGRAD_TILE forces the tile, DVSOF_WGRAD_SPLITS the K splits
int general_splits(const WGradParams &P, int model_S, int *tile)
{
    static const int tile_env = env_int("DVSOF_WGRAD_TILE", 0);
    static const int s_env = env_int("DVSOF_WGRAD_SPLITS", 0);
    if (tile_env >= 1 && tile_env <= 5) *tile = tile_env;
    if (s_env < 1) return model_S;
    const long long cap = (P.M + BK - 1) / BK;
    const int S = s_env > 64 ? 64 : s_env;
    return S > cap ? (int)cap : S;
}

// [slabs | bias or column-sum partials | flat partials]: the one place that lays the workspace out
// (+ 1 per flat row: room for the bias column of the matrix-core kernel's partial rows; the
// flat members' room is kept whether or not they take kernels of their own)
void lay_out(WGradPlan &pl, const WGradParams &P, const FlatWG *flat, int nflat, bool with_bias)
{
    const int nslab = pl.S * P.nph;
    pl.bias_off = nslab <= 1 ? 0 : (size_t)nslab * P.Cout * P.ks * P.ks * P.Cin_tot;
    size_t off = pl.bias_off + (with_bias ? (size_t)WG_COLSUM_BLOCKS * P.Cout : 0);
    for (int i = 0; i < nflat; ++i) {
        pl.flat_off[i] = off;
        off += (size_t)WG_FLAT_BLOCKS * flat[i].Cout * (flat[i].ncol + 1);
    }
    pl.total = off;
}

}  // namespace

int wgrad_enumerate_tiles(WGradParams &P, int cols_per_channel, int width, bool vec, bool flat)
{
    int t = 0;
    for (int s = 0; s < P.nsrc; ++s) {
        P.tile_begin[s] = t;
        if (P.src[s].flat ? flat : vec) t += (cols_per_channel * P.src[s].C + width - 1) / width;
    }
    P.tile_begin[P.nsrc] = t;
    return t;
}

// v2 handles the vector members when image rows are whole 16-pixel groups.
bool wgrad2_eligible(const WGradParams &P)
{
    if (P.Wo % BK || P.klen % BK || P.up != UP_NONE) return false;
    for (int s = 0; s < P.nsrc; ++s)
        if (!P.src[s].flat && (P.src[s].sc != 1 || (P.src[s].C & 3))) return false;
    long long bytes = (long long)P.B * P.g_sb * 4;
    for (int s = 0; s < P.nsrc; ++s) {
        const long long b = (long long)P.B * P.src[s].sb * 4;
        bytes = b > bytes ? b : bytes;
    }
    return bytes < 0x7fffffffLL;
}

WGradPlan wgrad_plan(const WGradParams &P0, const FlatWG *flat, int nflat, bool with_bias, bool sizing)
{
    WGradParams P = P0;
    WGradPlan pl = {};
    pl.rc = DVSOF_OK;
    bool any_vec = false, has_flat = false;
    for (int s = 0; s < P.nsrc; ++s) {
        if (P.src[s].flat) has_flat = true;
        else {
            any_vec = true;
            if (P.src[s].sc != 1 || (P.src[s].C & 3)) pl.rc = DVSOF_EINVAL;
        }
    }
    // ---- tile and K splits --------------------------------------------------------------------
    int model_S = 1;
    pl.tile = pick_tile_and_splits(P, &model_S);
    if (sizing) {
        // THE invariant of the workspace: the pointers of a call (twins bound or not, aligned or
        // not) choose between the two split rules, so sizing takes the larger of both; every
        // other term of the layout is fixed by the shape or grows with what sizing assumes
        // (a bias gradient, every flat member)
        pl.S = general_splits(P, model_S, &pl.tile);
        if (patch_shape_ok(P) && patch_splits(P) > pl.S) pl.S = patch_splits(P);
        lay_out(pl, P, flat, nflat, with_bias);
        return pl;
    }
    // A patch-eligible call takes the patch rule's split count (and the model's tile, without
    // DVSOF_WGRAD_TILE) even where the patch kernels then do not run: a direct launch, or flat
    // members on the v1 tiles beside v2.  Known oddity, kept: v2 and the v1 tiles then run with
    // a count made for another kernel.
    const bool patch_ok = patch_eligible(P);
    pl.S = patch_ok ? patch_splits(P) : general_splits(P, model_S, &pl.tile);
    pl.klen = (((P.M + pl.S - 1) / pl.S) + BK - 1) / BK * BK;
    P.klen = pl.klen;
    const bool direct = pl.S * P.nph == 1;
    int bm;
    tile_dims(pl.tile, bm, pl.bn);
    // ---- kernels ------------------------------------------------------------------------------
    // flat members: kernels of their own when every one of them qualifies
    bool flat_own = nflat > 0;
    for (int i = 0; i < nflat; ++i) flat_own = flat_own && flat_ncol_ok(flat[i].ncol);
    const bool v2 = wgrad2_eligible(P);
    if (!any_vec) pl.vec = WGV_NONE;
    else if (!v2) pl.vec = WGV_V1;
    // (flat members on the v1 tiles would write phase-form columns into the patch kernels' slabs)
    else if (direct || !patch_ok || !(flat_own || nflat == 0)) pl.vec = WGV_V2;
    else pl.vec = !patch_f32(P) ? WGV_PATCH_TWINS : min9_ok(P) ? WGV_MIN9 : WGV_PATCH_F32;
    if (pl.vec >= WGV_PATCH_TWINS) pl.bn = pl.vec == WGV_MIN9 ? WG_MIN_CT : patch_channel_tile(P);
    pl.ntiles = pl.vec <= WGV_V2 ? wgrad_enumerate_tiles(P, P.ks * P.ks, pl.bn, true, false)
                                 : wgrad_enumerate_tiles(P, 1, pl.bn, true, false);
    // beside v2 only the flat members handed over run (nflat = 0: their columns are the caller's);
    // the v1 tiles otherwise take every flat member of the layer
    pl.flat = flat_own ? WGF_OWN : (v2 ? nflat > 0 : has_flat) ? WGF_V1 : WGF_NONE;
    for (int i = 0; i < nflat; ++i) pl.flat_mfma[i] = flat_own && flat_uses_mfma(flat[i]);
    const bool v1 = pl.vec == WGV_V1 || pl.flat == WGF_V1;
    // ---- bias gradient and reduce -------------------------------------------------------------
    // v2 and the patch kernels leave per-slab column sums of gout; a flat-only layer on the
    // matrix-core flat kernel gets it as one more output column; else a pass over gout
    if (!with_bias) pl.bias = WGB_NONE;
    else if (pl.vec >= WGV_V2) pl.bias = WGB_VECTOR;
    else if (pl.flat_mfma[0] && (flat[0].ncol % 32) != 0) pl.bias = WGB_FLAT;
    else pl.bias = WGB_COLSUM;
    pl.bias_tail = pl.bias == WGB_VECTOR && !direct;
    if (direct || (!any_vec && flat_own)) pl.reduce = WGR_NONE;     // (the flat kernels write dW themselves)
    else if (pl.vec >= WGV_PATCH_TWINS) pl.reduce = WGR_PATCH;
    else pl.reduce = P.nph == 4 ? WGR_SUBPIXEL : WGR_SLABS;
    pl.zg = pl.S <= 2 ? 1 : pl.S <= 8 ? 4 : 16;
    lay_out(pl, P, flat, nflat, with_bias);
    // ---- what the call reports: the vector members' kernel, else the v1 tiles, else the flat kernels
    const int mode = P.twins ? 3 : P.mfma_bf16;
    switch (pl.vec) {
    case WGV_V2: pl.family = DVSOF_KERNEL_GENERAL_V2; pl.mode = mode; break;
    case WGV_PATCH_TWINS:
    case WGV_PATCH_F32: pl.family = DVSOF_KERNEL_WGRAD_PATCH; pl.mode = mode; break;
    case WGV_MIN9: pl.family = DVSOF_KERNEL_WGRAD_MIN; break;
    default:    // exact f32 in every mode
        pl.family = v1 ? DVSOF_KERNEL_GENERAL_V1 : flat_own ? DVSOF_KERNEL_FLAT_VALU : DVSOF_KERNEL_NONE;
    }
    return pl;
}
