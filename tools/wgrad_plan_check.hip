// Stand-alone host program for the weight gradient's planner (csrc/wgrad_plan.hip): fills
// WGradParams / FlatWG as conv_api.hip does for a few 3x3 / pad 1 / stride 1 layers (the last
// five of tests/conv_cases.py and two decoder stages), plans every combination of operand
// mode, pointers and bias, prints the outcome and checks that the sized workspace covers the
// call's.  It makes no HIP call and needs no GPU; build it with the host sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/wgrad_plan_check.hip dvs_of_training_framework_amd/csrc/wgrad_plan.hip -o wgrad_plan_check
#include "../dvs_of_training_framework_amd/csrc/conv_host.h"
#include <stdio.h>

void conv_note_kernel(int, int) {}

struct Member { int C; bool planar; };
struct Layer { int B, H, W; Member m[3]; int n, Cout; bool up; };

static GSrc src(const Member &m, int H, int W, const float *p, const unsigned short *p16)
{
    GSrc s = {};
    s.p = p;
    s.C = m.C;
    s.flat = m.planar || (m.C & 3) || m.C < BK;
    s.sb = (long long)m.C * H * W;
    s.sy = m.planar ? W : W * m.C;
    s.sx = m.planar ? 1 : m.C;
    s.sc = m.planar ? H * W : 1;
    s.p16 = m.planar ? nullptr : p16;
    return s;
}

int main()
{
    const Layer layers[] = {
        {1, 8, 16, {{32, false}, {32, false}, {4, true}}, 3, 32, true},
        {2, 9, 11, {{24, false}, {2, true}}, 2, 30, false},
        {1, 512, 512, {{2, true}}, 1, 32, false},
        {1, 16, 16, {{4, true}}, 1, 32, false},
        {2, 16, 32, {{8, false}, {4, true}}, 2, 12, false},
        {2, 16, 16, {{64, false}, {64, false}, {2, true}}, 3, 32, true},
        {1, 8, 16, {{32, false}, {96, false}}, 2, 64, true},
    };
    static float buf[8];    // addresses only: 16-byte aligned at buf, not at buf + 1
    alignas(16) static unsigned short buf16[8];
    int bad = 0;
    for (const Layer &L : layers)
        for (int mode = 0; mode < 4; ++mode)
            for (int combo = 0; combo < 16; ++combo) {
                const bool aligned = combo & 1, twins = combo & 2, bias = combo & 4, skip = combo & 8;
                if (twins && mode != 3) continue;
                const float *base = (const float *)(((uintptr_t)buf + 15) & ~(uintptr_t)15) + (aligned ? 0 : 1);
                const int Ho = L.up ? 2 * L.H : L.H, Wo = L.up ? 2 * L.W : L.W;
                WGradParams P = {};
                FlatWG F[3] = {};
                int nflat = 0, ctot = 0;
                P.mfma_bf16 = mode == 3 ? 1 : mode;
                P.nsrc = L.n;
                P.gout = base;
                P.gout16 = twins ? buf16 : nullptr;
                P.twins = twins && (L.Cout % 8) == 0;
                for (int i = 0; i < L.n; ++i) {
                    P.src[i] = src(L.m[i], L.H, L.W, base, twins ? buf16 : nullptr);
                    if (!P.src[i].flat && (!P.src[i].p16 || (P.src[i].C % 8))) P.twins = 0;
                    ctot += L.m[i].C;
                }
                P.B = L.B;
                P.Hv = Ho; P.Wv = Wo; P.Ho = Ho; P.Wo = Wo;
                P.up = L.up ? UP_NEAREST : UP_NONE;
                P.stride = 1; P.pad = 1; P.ks = 3;
                P.M = L.B * Ho * Wo;
                P.Cout = L.Cout;
                P.Cin_tot = ctot;
                P.nph = 1; P.S = 1;
                P.g_sb = (long long)Ho * Wo * L.Cout;
                P.g_sy = Wo * L.Cout;
                P.g_sx = L.Cout;
                for (int i = 0, coff = 0; i < L.n; coff += L.m[i++].C)
                    if (P.src[i].flat) {     // in the layer's original geometry
                        FlatWG &f = F[nflat++];
                        f.S = P.src[i]; f.gout = base;
                        f.B = L.B; f.Hv = Ho; f.Wv = Wo; f.up = P.up; f.Ho = Ho; f.Wo = Wo;
                        f.stride = 1; f.pad = 1; f.ks = 3; f.Cout = L.Cout; f.M = P.M;
                        f.ncol = 9 * L.m[i].C; f.coff = coff; f.Cin_tot = ctot;
                    }
                if (L.up) {     // four sub-pixel phases of 2x2 taps on the low-resolution frame
                    P.up = UP_NONE;
                    P.Hv = P.Ho = L.H; P.Wv = P.Wo = L.W;
                    P.ks = 2;
                    P.M = L.B * L.H * L.W;
                    P.nph = 4; P.ph_pad = 1;
                    P.g_py = P.g_sy; P.g_px = P.g_sx;
                    P.g_sy *= 2; P.g_sx *= 2;
                }
                WGradParams Q = P;      // sizing: the shape alone
                Q.gout = nullptr; Q.gout16 = nullptr; Q.twins = 0;
                for (int i = 0; i < L.n; ++i) Q.src[i].p = nullptr, Q.src[i].p16 = nullptr;
                const WGradPlan size = wgrad_plan(Q, F, nflat, true, true);
                if (skip) nflat = 0;    // DVSOF_CONV_WGRAD_SKIP_FLAT: the flat members' columns are the caller's
                const WGradPlan pl = wgrad_plan(P, F, nflat, bias, false);
                const bool ok = pl.rc == DVSOF_OK && pl.total <= size.total && pl.S <= size.S &&
                                pl.bias_off <= pl.total && (nflat == 0 || pl.flat_off[nflat - 1] < pl.total);
                bad += !ok;
                printf("%s %dx%dx%d Cout %d mode %d aligned %d twins %d bias %d skip %d: vec %d tile %d nt %d S %d klen %d flat %d "
                       "bias %d tail %d reduce %d zg %d total %zu <= %zu family %d/%d\n", ok ? "ok " : "BAD", L.B, L.H, L.W,
                       L.Cout, mode, aligned, twins, bias, skip, pl.vec, pl.tile, pl.ntiles, pl.S, pl.klen, pl.flat, pl.bias,
                       pl.bias_tail, pl.reduce, pl.zg, pl.total, size.total, pl.family, pl.mode);
            }
    printf("%d bad\n", bad);
    return bad != 0;
}
