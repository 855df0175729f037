// Pointwise / dense GEMM lab: every kernel form of csrc/pw_gemm.hip, pw_bx3.hip, pw_b16.hip and pw_ws.hip - k_pw_gemm, k_pw_pipe,
// k_pw_naive, k_pw_bx3 (six and one product), k_pw_bx3p, k_pw_b16 (six and one product), k_pw_b16s, k_pw_ws (six and one product),
// k_pw_lat and the implicit-GEMM convolution k_pw_gemm<IM> - through the library's own entries (launch_pw_gemm, launch_pw_bx3,
// launch_conv_igemm) on synthetic layers, without a model.  Every output element is held to a plain fp64 loop nest
// act(sum_k a scale w + bias) + res on the host; a plain sequential fp32 evaluation of the same case next to it sizes the tolerance
// (gates: below, and DESIGN.md, "Pointwise GEMM family: what is pinned per kernel form").  The output lies between guard words that
// must stay intact; A, the scale, the bias, the residual, the weights and the weight image are sized exactly and lie between NaNs.
// The case list is fixed (the data of a case is seeded by its name).  The form that will run is predicted from the library's public
// predicates and checked against the launch counters.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I birdnet-go_amd/csrc -o pw64_lab tools/ubench/pw64_lab.cpp \
//         -L birdnet-go_amd/lib -lbnhip -Wl,-rpath,birdnet-go_amd/lib
//   BNHIP_PW_FILL=0 pw64_lab     every dispatcher branch at the tile it names (the switch is read once per process: pw_fill_grid then
//                                changes no tile); exit status 1 on any failed check, 3 on a HIP error (nothing is launched after one)
//   pw64_lab                     without the switch: the cases whose tile pw_fill_grid shrinks - what a call of a few clips runs
//   pw64_lab --list              print the cases of that process (by the same switch) with the predicted form and tile; touches no device
//   pw64_lab --ref-dump NAME DIR write the inputs, parameters and fp64 result of one case as raw arrays (no device)
//   pw64_lab --only SUBSTR       run the cases whose name contains SUBSTR
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "kernels.h"
using namespace bnhip;

extern "C" long bnhip_debug_pw_ws_launches(void);
extern "C" long bnhip_debug_pw_lat_launches(void);
extern "C" long bnhip_debug_pw_b16_launches(void);

static uint16_t bf16_rne(float f) {
    unsigned u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static float bf16_widen(uint16_t h) { unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }
static float bf16_round(float f) { return bf16_widen(bf16_rne(f)); }

static double act64(double v, int act) {
    switch (act) {
        case ACT_RELU: return std::max(v, 0.0);
        case ACT_RELU6: return std::min(std::max(v, 0.0), 6.0);
        case ACT_SWISH: return v / (1.0 + std::exp(-v));
        case ACT_SIGMOID: return 1.0 / (1.0 + std::exp(-v));
        case ACT_HARD_SWISH: return v * std::min(std::max(v + 3.0, 0.0), 6.0) / 6.0;
        default: return v;
    }
}
static float act32(float v, int act) {
    switch (act) {
        case ACT_RELU: return fmaxf(v, 0.0f);
        case ACT_RELU6: return fminf(fmaxf(v, 0.0f), 6.0f);
        case ACT_SWISH: return v / (1.0f + expf(-v));
        case ACT_SIGMOID: return 1.0f / (1.0f + expf(-v));
        case ACT_HARD_SWISH: return v * fminf(fmaxf(v + 3.0f, 0.0f), 6.0f) / 6.0f;
        default: return v;
    }
}
static const char* act_name(int a) {
    return a == ACT_SWISH ? "swish" : a == ACT_RELU6 ? "relu6" : a == ACT_RELU ? "relu" : a == ACT_SIGMOID ? "sigmoid" : a == ACT_HARD_SWISH ? "hardswish" : "none";
}
static const int kActs[6] = {ACT_NONE, ACT_SWISH, ACT_RELU6, ACT_RELU, ACT_SIGMOID, ACT_HARD_SWISH};      // every activation apply_act implements
static std::mt19937 rng_of(const std::string& name) {      // FNV-1a of the case's name: the same data on every run and machine
    unsigned seed = 2166136261u;
    for (char ch : name) seed = (seed ^ (unsigned char)ch) * 16777619u;
    return std::mt19937(seed);
}

// ------------------------------------------------------------------------------------------ cases
enum { E_GEMM = 0, E_BX3 = 1, E_IGEMM = 2 };
struct Case {
    std::string name; const char* tag = "";
    int entry = E_GEMM, pass = 1;      // pass 1: the process with BNHIP_PW_FILL=0; pass 2: the one without (the shrink)
    int M = 0, N = 0, K = 0, HW = 0;   // HW 0: no squeeze-excite scale (PwParams::HW = M)
    int wm = 0, nt = 0, prec = 0, sw = 0;
    int a16 = 0, o16 = 0, r16 = 0, bias = 1, res = 0, act = ACT_NONE;
    int B = 0, H = 0, W = 0, Cin = 0, kh = 0, kw = 0, st = 1, dil = 1, valid = 0, Ho = 0, Wo = 0, pt = 0, pl = 0;      // implicit GEMM
};

static void name_case(Case& c) {
    char buf[256];
    if (c.entry == E_IGEMM)
        snprintf(buf, sizeof buf, "%s_k%dx%d_s%d_d%d_%s_B%d_H%d_W%d_ci%d_co%d_wm%d_nt%d_%s_b%d%s", c.tag, c.kh, c.kw, c.st, c.dil, c.valid ? "valid" : "same", c.B, c.H, c.W,
                 c.Cin, c.N, c.wm, c.nt, act_name(c.act), c.bias, c.pass == 2 ? "_shrink" : "");
    else
        snprintf(buf, sizeof buf, "%s_wm%d_nt%d_M%d_N%d_K%d_hw%d_a%do%dr%d_b%dres%d_%s%s", c.tag, c.wm, c.nt, c.M, c.N, c.K, c.HW, c.a16, c.o16, c.r16, c.bias, c.res,
                 act_name(c.act), c.pass == 2 ? "_shrink" : "");
    c.name = buf;
}

// a kernel family as the dispatcher names it: entry, PwParams::wm, precision, bf16 A, the widest nt it has
struct Fam { const char* tag; int entry, wm, prec, a16, ntmax; };
static const Fam F_GEMM1{"gemm", E_GEMM, 1, 0, 0, 8}, F_GEMM2{"gemm", E_GEMM, 2, 0, 0, 8}, F_PIPE3{"pipe", E_GEMM, 3, 0, 0, 4}, F_PIPE4{"pipe", E_GEMM, 4, 0, 0, 4},
    F_BX5{"bx3", E_BX3, 5, 0, 0, 8}, F_BX6{"bx3", E_BX3, 6, 0, 0, 8}, F_BXP7{"bx3p", E_BX3, 7, 0, 0, 8}, F_BXP8{"bx3p", E_BX3, 8, 0, 0, 8},
    F_B16S10{"b16six", E_BX3, 10, 0, 0, 8}, F_B16S9{"b16six", E_BX3, 9, 0, 0, 8}, F_B16O{"b16one", E_BX3, 9, 1, 0, 8}, F_B16OA{"b16one", E_BX3, 9, 1, 1, 8},
    F_BXP1{"bx3pone", E_BX3, 8, 1, 0, 8}, F_BXP1A{"bx3pone", E_BX3, 7, 1, 1, 8}, F_BX1{"bx3one", E_BX3, 5, 1, 0, 8}, F_BX1A{"bx3one", E_BX3, 5, 1, 1, 8}, F_BX1F{"bx3one", E_BX3, 10, 1, 0, 8},      // (wm 10 on a one-product engine falls through to k_pw_bx3)
    F_LAT{"lat", E_BX3, 6, 0, 0, 8}, F_B16SK{"b16s", E_BX3, 11, 1, 0, 2}, F_B16SKA{"b16s", E_BX3, 11, 1, 1, 2}, F_WS6{"ws", E_BX3, 12, 0, 0, 8},
    F_WS1{"wsone", E_BX3, 12, 1, 0, 4}, F_WS1A{"wsone", E_BX3, 12, 1, 1, 4}, F_HOLE{"hole", E_BX3, 9, 0, 1, 8};
static int fam_rows(const Fam& f) { return (f.wm == 1 || f.wm == 3 || f.wm == 5 || f.wm == 7 || f.wm == 10) ? 64 : 128; }

static std::vector<Case> build_cases() {
    std::vector<Case> v;
    std::set<std::string> seen;
    auto add = [&](Case c) { name_case(c); if (seen.insert(c.name).second) v.push_back(c); };
    auto mk = [&](const Fam& f, int nt, int M, int N, int K) {
        Case c; c.tag = f.tag; c.entry = f.entry; c.wm = f.wm; c.prec = f.prec; c.a16 = f.a16; c.nt = nt; c.M = M; c.N = N; c.K = K;
        if (f.entry == E_BX3) c.sw = PW_SW_LAT_OFF;              // (a tiled request with a long K and few tiles would be taken by k_pw_lat)
        if (&f == &F_LAT) c.sw = 0;
        if (&f == &F_WS6 || &f == &F_WS1 || &f == &F_WS1A) c.sw = PW_SW_LAT_OFF | PW_SW_WS_FORCE;      // (pw_ws_fills is a speed rule)
        return c;
    };
    const Fam* tiled[] = {&F_GEMM1, &F_GEMM2, &F_PIPE3, &F_PIPE4, &F_BX5, &F_BX6, &F_BXP7, &F_BXP8, &F_B16S10, &F_B16S9, &F_B16O, &F_B16OA, &F_BX1, &F_BX1A, &F_BX1F};
    int rot = 0;
    // ---- every tiled dispatcher branch x every nt: two row blocks x two column blocks, once with full and once with ragged last blocks
    for (const Fam* f : tiled)
        for (int nt = 1; nt <= f->ntmax; nt++) {
            const int rows = fam_rows(*f);
            const bool pipe = f->tag[0] == 'p' || !strncmp(f->tag, "bx3p", 4);
            Case c = mk(*f, nt, 2 * rows, 32 * nt, 64);          // full tiles, two slabs
            c.act = kActs[rot % 6]; c.res = rot & 1; rot++;
            add(c);
            c = mk(*f, nt, rows + 1 + 16 * (nt % 3), 16 * nt + 4 * (1 + nt % 3), pipe ? (f->entry == E_GEMM ? 96 : 100) : f->a16 ? 40 : 36);      // ragged rows, ragged columns, a K tail
            c.act = kActs[rot % 6]; c.res = rot & 1; rot++;
            add(c);
        }
    // ---- K: a tail inside the only slab, 1, 2, 3 and >= 4 slabs with and without a tail, the shipped tails 232 and 136
    const Fam* kf[] = {&F_GEMM2, &F_PIPE3, &F_PIPE4, &F_BX6, &F_BXP7, &F_BXP8, &F_B16S9, &F_B16S10, &F_B16O, &F_B16OA, &F_BX1, &F_BX1A, &F_BXP1, &F_BXP1A};
    for (int K : {16, 20, 32, 36, 64, 96, 100, 128, 136, 232})
        for (const Fam* f : kf) {
            if (f->a16 && (K & 7)) continue;                     // (bf16 A: the planner hands a GEMM bf16 storage only with K % 8 == 0)
            Case c = mk(*f, 2, fam_rows(*f) + 2, 36, K);
            c.act = kActs[rot++ % 6];
            add(c);
        }
    // ---- rows
    const Fam* rf[] = {&F_GEMM1, &F_GEMM2, &F_PIPE4, &F_BX5, &F_BX6, &F_BXP8, &F_B16S9, &F_B16S10, &F_B16O, &F_B16OA, &F_BX1};
    for (int M : {1, 15, 16, 17, 63, 64, 65, 127, 129, 293})
        for (const Fam* f : rf) {
            Case c = mk(*f, 2, M, 36, f->a16 ? 40 : (f == &F_PIPE4 || f == &F_BXP8 || f == &F_BXP1) ? 64 : 36);
            c.res = rot++ & 1;
            add(c);
        }
    // ---- columns: one quad, ragged quads, N % 4 != 0 (scalar bias and store paths, fp32 storage), with a residual
    const Fam* cf[] = {&F_GEMM2, &F_PIPE3, &F_BX5, &F_BXP8, &F_B16S10, &F_B16O, &F_BX1};
    for (int N : {4, 12, 16, 20, 36, 68, 132, 7, 33, 130})
        for (const Fam* f : cf) {
            Case c = mk(*f, 3, 70, N, (f == &F_PIPE3 || f == &F_BXP8) ? 64 : 36);
            c.res = 1; c.act = kActs[rot++ % 6];
            add(c);
        }
    // ---- squeeze-excite scale: HW 1, 16, 48 (a 16-row tile inside one clip), 7, 23 (two or three clips per tile), 200 (a block inside one clip)
    const Fam* sf[] = {&F_GEMM1, &F_GEMM2, &F_PIPE4, &F_BX5, &F_BX6, &F_BXP8, &F_B16S9, &F_B16S10, &F_B16O, &F_B16OA, &F_BX1, &F_BX1A, &F_BXP1, &F_HOLE, &F_LAT};
    for (int HW : {1, 16, 48, 7, 23, 200})
        for (const Fam* f : sf) {
            const int M = HW == 1 ? 130 : HW == 16 ? 144 : HW == 48 ? 144 : HW == 7 ? 133 : HW == 23 ? 138 : 600;
            Case c = mk(*f, 2, M, 36, f == &F_LAT ? 256 : f->a16 ? 40 : (f == &F_PIPE4 || f == &F_BXP8 || f == &F_BXP1) ? 64 : 36);
            c.HW = HW; c.res = rot & 1; c.act = (rot % 3 == 0) ? ACT_SWISH : ACT_NONE; rot++;
            add(c);
        }
    // ---- epilogue: residual and output storage in all four combinations, no bias, every activation
    const Fam* ef[] = {&F_GEMM2, &F_PIPE4, &F_BX6, &F_BXP8, &F_B16S9, &F_B16O, &F_BX1, &F_HOLE, &F_LAT, &F_WS6, &F_WS1, &F_B16SK};
    for (const Fam* f : ef) {
        const bool ws = f == &F_WS6 || f == &F_WS1, sk = f == &F_B16SK;
        const int M = ws ? 293 : 130, N = ws ? 68 : sk ? 28 : 36, K = f == &F_LAT ? 260 : ws ? 96 : f->a16 ? 40 : (f == &F_PIPE4 || f == &F_BXP8 || f == &F_BXP1) ? 64 : 36;
        const int nt = ws ? 4 : 2;
        for (int combo = 0; combo < 4; combo++) {
            Case c = mk(*f, nt, M, N, K);
            c.res = 1; c.r16 = combo & 1; c.o16 = combo >> 1; c.act = combo == 3 ? ACT_SWISH : ACT_NONE;
            add(c);
        }
        { Case c = mk(*f, nt, M, N, K); c.o16 = 1; c.act = ACT_RELU6; add(c); }       // bf16 output without a residual
        { Case c = mk(*f, nt, M, N, K); c.bias = 0; add(c); }
        { Case c = mk(*f, nt, M, N, K); c.bias = 0; c.res = 1; c.act = ACT_SWISH; add(c); }
        for (int a : kActs) { Case c = mk(*f, nt, M, N, K); c.act = a; add(c); }
    }
    // ---- k_pw_b16s: NT 1 / 2 x NS 1 .. 6 x scale x A storage; N 16, 12 (NT 1), 32, 28 (NT 2)
    for (int nt = 1; nt <= 2; nt++)
        for (int ns = 1; ns <= 6; ns++)
            for (int sc = 0; sc < 2; sc++)
                for (int a16 = 0; a16 < 2; a16++) {
                    const bool tail = (ns + sc + a16) & 1;
                    const int K = 32 * ns - (tail ? (a16 ? 8 : 12) : 0);
                    const int N = nt == 1 ? (tail ? 12 : 16) : (tail ? 28 : 32);
                    Case c = mk(a16 ? F_B16SKA : F_B16SK, nt, sc ? (ns & 1 ? 144 : 160) : (tail ? 100 : 129), N, K);
                    c.HW = sc ? (ns & 1 ? 48 : 16) : 0; c.res = ns & 1; c.act = kActs[rot++ % 6];
                    add(c);
                }
    // ---- k_pw_ws, six products: (slabs, nt) as the kernel has them; M / 16 = 2 WS_NW exactly and an odd number of row tiles
    const int wsf[][2] = {{3, 4}, {3, 6}, {3, 8}, {4, 4}, {4, 6}, {4, 8}, {5, 4}, {5, 6}, {5, 8}, {6, 4}, {6, 6}, {6, 8}, {8, 4}, {8, 6}, {10, 4}};
    for (auto& sn : wsf) {
        const int ns = sn[0], nt = sn[1];
        Case c = mk(F_WS6, nt, 256, 32 * nt, 32 * ns);
        c.act = kActs[rot++ % 6];
        add(c);
        c = mk(F_WS6, nt, 293, 16 * nt + 20, ns == 4 ? 100 : ns == 5 ? 136 : ns == 8 ? 232 : 32 * ns - 12);
        c.res = 1; c.act = kActs[rot++ % 6];
        add(c);
    }
    for (int ns = 3; ns <= 6; ns++)
        for (int a16 = 0; a16 < 2; a16++) {
            Case c = mk(a16 ? F_WS1A : F_WS1, 4, 256, 128, 32 * ns);
            c.act = kActs[rot++ % 6];
            add(c);
            c = mk(a16 ? F_WS1A : F_WS1, 4, 293, 68, 32 * ns - (a16 ? 8 : 12));
            c.res = 1;
            add(c);
        }
    // ---- k_pw_lat: a group of four slabs with one, two and none left over, N % 4 != 0; nt 2 needs >= 1024 (row tile, column tile) pairs
    for (int K : {256, 260, 416, 512})
        for (int sc = 0; sc < 2; sc++) {
            Case c = mk(F_LAT, 2, sc ? 46 : 17, K == 416 ? 7 : K == 512 ? 132 : 20, K);
            c.HW = sc ? 23 : 0; c.res = sc; c.act = kActs[rot++ % 6];
            add(c);
        }
    for (int sc = 0; sc < 2; sc++) {
        Case c = mk(F_LAT, 2, 1009, 256, 256);
        c.HW = sc ? 100 : 0; c.res = sc; c.act = sc ? ACT_NONE : ACT_SWISH;
        add(c);
    }
    { Case c = mk(F_LAT, 2, 1, 36, 256); add(c); }
    // ---- k_pw_naive
    for (int K : {5, 18}) {
        Case c = mk(F_GEMM2, 2, 37, 7, K);
        c.tag = "naive"; c.res = 1; c.act = ACT_SWISH;
        add(c);
        c = mk(F_GEMM2, 2, 300, 20, K);
        c.tag = "naive"; c.HW = 100; c.act = ACT_RELU6;
        add(c);
    }
    // ---- the contract hole: a six-product call whose A is bf16, tuned onto k_pw_b16 - launch_pw_bx3 keeps it on k_pw_bx3
    for (int nt : {1, 4}) {
        Case c = mk(F_HOLE, nt, 129, 16 * nt + 4, 72);
        c.res = nt == 4;
        add(c);
        c.wm = 10; add(c);
        c.wm = 6; c.sw |= PW_SW_B16_FORCE; c.tag = "holeforce"; add(c);
    }
    // ---- implicit GEMM
    auto ig = [&](int kh, int kw, int st, int dil, int valid, int B, int H, int W, int Cin, int Cout, int wm, int nt, int act, int bias) {
        Case c; c.tag = "igemm"; c.entry = E_IGEMM; c.kh = kh; c.kw = kw; c.st = st; c.dil = dil; c.valid = valid; c.B = B; c.H = H; c.W = W; c.Cin = Cin; c.N = Cout;
        c.wm = wm; c.nt = nt; c.act = act; c.bias = bias;
        const int eh = (kh - 1) * dil + 1, ew = (kw - 1) * dil + 1;
        if (valid) { c.Ho = (H - eh) / st + 1; c.Wo = (W - ew) / st + 1; }
        else {    // SAME, TensorFlow's rule: the smaller half of the padding in front
            c.Ho = (H + st - 1) / st; c.Wo = (W + st - 1) / st;
            c.pt = std::max((c.Ho - 1) * st + eh - H, 0) / 2; c.pl = std::max((c.Wo - 1) * st + ew - W, 0) / 2;
        }
        c.M = B * c.Ho * c.Wo; c.K = kh * kw * Cin; c.HW = 0;
        // a grid of fewer than 64 blocks runs the 64 x 16 tile whatever was asked (launch_conv_igemm's own rule, not BNHIP_PW_FILL's):
        // pass 1 asks for that tile by name, pass 2 for the larger one, which the rule then replaces
        if (pw_grid(c.M, c.N, nt, wm == 1 ? 1 : 2).nblk < 64 && (nt > 1 || wm > 1)) {
            c.pass = 2; add(c);
            c.pass = 1; c.wm = 1; c.nt = 1;
        }
        add(c);
    };
    ig(3, 3, 1, 1, 0, 3, 9, 11, 4, 7, 2, 2, ACT_RELU6, 1);           // small grid: nt = wm = 1; padding 1
    ig(3, 3, 2, 1, 0, 3, 9, 11, 8, 20, 2, 4, ACT_SWISH, 1);          // stride 2 on an odd image: padding 1
    ig(3, 3, 2, 1, 0, 1, 12, 10, 12, 48, 1, 1, ACT_NONE, 0);         // stride 2 on an even image: padding 0 in front
    ig(5, 5, 1, 1, 0, 3, 7, 9, 4, 20, 2, 3, ACT_RELU, 1);            // padding 2
    ig(5, 5, 2, 1, 0, 1, 13, 12, 8, 7, 2, 2, ACT_HARD_SWISH, 1);
    ig(2, 2, 1, 1, 0, 3, 8, 9, 8, 48, 2, 2, ACT_SIGMOID, 1);         // even kernel: padding 0 in front, 1 behind
    ig(2, 2, 2, 1, 1, 1, 10, 12, 12, 20, 2, 2, ACT_NONE, 1);
    ig(1, 1, 2, 1, 0, 3, 9, 12, 32, 7, 2, 2, ACT_SWISH, 1);          // 1 x 1, stride 2
    ig(3, 3, 1, 2, 0, 3, 9, 11, 4, 20, 2, 2, ACT_RELU6, 1);          // dilation 2: padding 2
    ig(3, 3, 1, 1, 1, 1, 9, 11, 12, 7, 2, 2, ACT_NONE, 1);           // VALID
    ig(3, 3, 1, 2, 1, 3, 10, 9, 8, 48, 2, 2, ACT_SWISH, 0);
    ig(3, 3, 1, 1, 0, 2, 64, 64, 4, 48, 2, 2, ACT_SWISH, 1);         // >= 64 blocks: 128-row tiles, nt 2
    ig(3, 3, 1, 1, 0, 2, 64, 64, 4, 48, 2, 4, ACT_NONE, 1);          //               128-row tiles, nt 4 (48 of 64 columns live)
    ig(5, 5, 2, 1, 0, 2, 127, 65, 4, 20, 1, 2, ACT_RELU6, 1);        //               64-row tiles, nt 2, ragged rows and columns
    ig(3, 3, 2, 2, 0, 2, 63, 65, 8, 7, 1, 1, ACT_NONE, 1);           //               stride 2 with dilation 2, N % 4 != 0

    // ---- pass 2: the shrink (a process without BNHIP_PW_FILL; the grid target is the chip's compute units, 256 on an MI355X)
    auto shrink = [&](const Fam& f, int nt, int M, int N, int K, int HW, int res) {
        Case c = mk(f, nt, M, N, K);
        c.pass = 2; c.HW = HW; c.res = res;
        add(c);
    };
    shrink(F_GEMM2, 1, 16384, 16, 36, 0, 0);         // 128 -> 64 rows, nt kept: 128 -> 256 blocks
    shrink(F_BX6, 1, 16384, 16, 36, 0, 1);
    shrink(F_B16S9, 1, 16384, 16, 36, 0, 0);
    shrink(F_GEMM1, 2, 8200, 32, 36, 0, 0);          // nt halved once
    shrink(F_BX5, 2, 4100, 36, 36, 0, 0);
    shrink(F_B16S10, 2, 8200, 32, 36, 100, 0);
    shrink(F_GEMM1, 4, 4100, 64, 36, 0, 1);          // nt halved twice
    shrink(F_BX5, 4, 4100, 68, 36, 0, 0);
    shrink(F_B16S10, 8, 2100, 128, 36, 0, 0);        // nt 8 -> 4 -> 2 -> 1
    shrink(F_BX6, 5, 2100, 80, 36, 0, 0);            // rows, then 5 -> 3 -> 2 -> 1
    shrink(F_GEMM2, 3, 4100, 48, 36, 0, 0);          // rows, then 3 -> 2 -> 1
    shrink(F_PIPE4, 2, 2048, 64, 64, 0, 0);          // a pipelined request falls back to the plain kernel
    shrink(F_PIPE3, 2, 3000, 36, 96, 48, 1);
    shrink(F_BXP8, 4, 2048, 64, 64, 0, 0);
    shrink(F_BXP7, 2, 3000, 36, 100, 48, 1);
    shrink(F_B16O, 4, 768, 192, 64, 0, 0);           // a one-product 128-row request lands on k_pw_bx3 with prec = 1
    shrink(F_B16OA, 2, 384, 36, 40, 48, 1);
    shrink(F_B16O, 2, 48, 20, 36, 16, 0);
    shrink(F_BX6, 4, 48, 192, 96, 48, 1);            // one clip of a late layer
    shrink(F_GEMM2, 2, 192, 24, 96, 192, 0);
    shrink(F_B16S9, 6, 48, 100, 136, 0, 0);
    return v;
}

// ------------------------------------------------------------------------------------------ the form a case will run
struct Pred { std::string form; int rows = 0, nt = 0; bool tiled = false, six = false, one = false, ws = false, lat = false, b16 = false; };
static PwParams params_of(const Case& c) {
    PwParams p{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c.M, c.N, c.K, c.HW ? c.HW : c.M, c.act, c.nt, c.wm};
    p.prec = c.prec; p.a_bf16 = c.a16; p.out_bf16 = c.o16; p.res_bf16 = c.r16; p.sw = c.sw;
    if (c.HW) p.ascale = reinterpret_cast<const float*>(16);      // (the predicates only ask whether there is one)
    return p;
}
// From the public predicates, in the launchers' order (launch_pw_gemm, launch_pw_bx3).  Restated rather than asked: the row tile a wm
// names, k_pw_lat's two column tiles per wave from 1024 tile pairs on, and launch_conv_igemm's small-grid rule (fewer than 64 blocks:
// the 64 x 16 tile) - none of them has a public predicate; the first and the last are checked against pw_grid, the counters check
// k_pw_lat, k_pw_ws and k_pw_b16 / k_pw_b16s.
static Pred predict(const Case& c) {
    Pred r;
    const PwParams p = params_of(c);
    if (c.entry == E_IGEMM) {
        int nt = c.nt, wm = c.wm == 1 ? 1 : 2;
        if (pw_grid(c.M, c.N, nt, wm).nblk < 64 && (nt > 1 || wm > 1)) nt = wm = 1;
        r.form = "k_pw_gemm_IM"; r.rows = 64 * wm; r.nt = nt; r.tiled = true;
        return r;
    }
    if (c.entry == E_GEMM) {
        if (c.K & 3) { r.form = "k_pw_naive"; return r; }
        int nt = c.nt, wm = (c.wm == 1 || c.wm == 3) ? 1 : 2;
        bool pipe = (c.wm == 3 || c.wm == 4) && pw_pipe_ok(nt, c.wm - 2, c.K);
        PwGrid g = pw_grid(c.M, c.N, nt, wm);
        if (pw_fill_grid(c.M, c.N, &nt, &wm, &g)) pipe = false;
        r.form = pipe ? "k_pw_pipe" : "k_pw_gemm"; r.rows = 64 * wm; r.nt = nt; r.tiled = true;
        return r;
    }
    r.six = c.prec == 0; r.one = c.prec == 1;
    if (!(c.sw & (PW_SW_B16_FORCE | PW_SW_B16S_FORCE | PW_SW_WS_FORCE)) && pw_lat_ok(p)) {
        r.form = "k_pw_lat"; r.lat = true;
        r.nt = (long)((c.M + 15) / 16) * ((c.N + 15) / 16) >= 1024 ? 2 : 1;
        return r;
    }
    if ((c.wm == 11 || (c.sw & PW_SW_B16S_FORCE)) && pw_b16s_ok(p)) { r.form = "k_pw_b16s"; r.b16 = true; r.nt = (c.N + 15) / 16; return r; }
    if (((c.wm == 12 && pw_ws_fills(p)) || (c.sw & PW_SW_WS_FORCE)) && pw_ws_ok(p)) { r.form = r.six ? "k_pw_ws_six" : "k_pw_ws_one"; r.ws = true; r.nt = r.six ? c.nt : 4; return r; }
    int nt = c.nt, wm = (c.wm == 5 || c.wm == 7 || c.wm == 10) ? 1 : 2;
    bool pipe = (c.wm == 7 || c.wm == 8) && pw_bx3p_ok(nt, wm, c.K);
    PwGrid g = pw_grid(c.M, c.N, nt, wm);
    if (pw_fill_grid(c.M, c.N, &nt, &wm, &g)) pipe = false;
    r.rows = 64 * wm; r.nt = nt; r.tiled = true;
    if ((c.wm == 9 || c.wm == 10 || (c.sw & PW_SW_B16_FORCE)) && (wm == 2 || c.prec == 0) && pw_b16_ok(c.prec, c.K, c.sw, c.a16)) {
        r.form = r.six ? "k_pw_b16_six" : "k_pw_b16_one"; r.b16 = true;
        return r;
    }
    r.form = pipe ? (r.six ? "k_pw_bx3p" : "k_pw_bx3p_one") : (r.six ? "k_pw_bx3" : "k_pw_bx3_one");
    return r;
}
static int req_rows(const Case& c) {
    if (c.entry == E_IGEMM) return c.wm == 1 ? 64 : 128;
    if (c.entry == E_GEMM) return (c.wm == 1 || c.wm == 3) ? 64 : 128;
    return (c.wm == 5 || c.wm == 7 || c.wm == 10) ? 64 : 128;
}

// ------------------------------------------------------------------------------------------ data and the host references
struct Data {
    std::vector<float> a /* A, or the image of an implicit GEMM; bf16 A: the bf16 values */, w, bias, sc, res;
    std::vector<float> xr, wr;                // one-product forms: the operands as the kernel rounds them
    std::vector<double> y64; std::vector<float> y32;
    double sabs = 0, clip = -1;               // max_{m,n} sum_k |a scale w|; the share a ReLU6 clips
};
static void gen(const Case& c, bool one, Data& d) {
    std::mt19937 rng = rng_of(c.name);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::uniform_real_distribution<float> ud(0.5f, 1.5f);
    const int M = c.M, N = c.N, K = c.K, HW = c.HW ? c.HW : M, nclips = (M + HW - 1) / HW;
    const bool im = c.entry == E_IGEMM;
    d.a.resize(im ? (size_t)c.B * c.H * c.W * c.Cin : (size_t)M * K);
    for (auto& v : d.a) v = nd(rng);
    if (c.a16) for (auto& v : d.a) v = bf16_round(v);
    d.w.resize((size_t)N * K);
    for (auto& v : d.w) v = 0.05f * nd(rng);
    d.bias.assign(N, 0.f);
    // (ReLU6: pre-activations are about N(0, 0.05 sqrt K); one sigma of offset puts the clipped share near 16 %)
    if (c.bias) for (auto& v : d.bias) v = 0.1f * nd(rng) + (c.act == ACT_RELU6 ? 0.05f * std::sqrt((float)K) : 0.f);
    if (c.HW) { d.sc.resize((size_t)nclips * K); for (auto& v : d.sc) v = ud(rng); }      // 0.5 .. 1.5: a row of the wrong clip is far outside the gate
    if (c.res) { d.res.resize((size_t)M * N); for (auto& v : d.res) v = nd(rng); if (c.r16) for (auto& v : d.res) v = bf16_round(v); }
    std::vector<double> wd((size_t)N * K);
    std::vector<float> w32((size_t)N * K);
    for (size_t i = 0; i < wd.size(); i++) { w32[i] = one ? bf16_round(d.w[i]) : d.w[i]; wd[i] = w32[i]; }
    if (one) { d.wr = w32; d.xr.resize((size_t)M * K); }
    d.y64.resize((size_t)M * N); d.y32.resize((size_t)M * N);
    std::vector<double> xd(K); std::vector<float> x32(K);
    size_t clipped = 0;
    const int HoWo = im ? c.Ho * c.Wo : 1;
    for (int m = 0; m < M; m++) {
        if (im) {
            const int b = m / HoWo, oh = m % HoWo / c.Wo, ow = m % c.Wo;
            for (int i = 0; i < c.kh; i++)
                for (int j = 0; j < c.kw; j++) {
                    const int ih = oh * c.st - c.pt + i * c.dil, iw = ow * c.st - c.pl + j * c.dil;
                    const bool in = ih >= 0 && ih < c.H && iw >= 0 && iw < c.W;
                    for (int ci = 0; ci < c.Cin; ci++) {
                        const float xv = in ? d.a[(((size_t)b * c.H + ih) * c.W + iw) * c.Cin + ci] : 0.f;
                        x32[(i * c.kw + j) * c.Cin + ci] = xv; xd[(i * c.kw + j) * c.Cin + ci] = xv;
                    }
                }
        } else {
            const float* ar = &d.a[(size_t)m * K];
            const float* sr = c.HW ? &d.sc[(size_t)(m / HW) * K] : nullptr;
            for (int k = 0; k < K; k++) {
                const float xs = sr ? ar[k] * sr[k] : ar[k];                   // the fp32 product every kernel forms
                if (one) { x32[k] = bf16_round(xs); xd[k] = x32[k]; d.xr[(size_t)m * K + k] = x32[k]; }
                else { x32[k] = xs; xd[k] = sr ? (double)ar[k] * (double)sr[k] : (double)ar[k]; }
            }
        }
        for (int n = 0; n < N; n++) {
            const double* wn = &wd[(size_t)n * K]; const float* wf = &w32[(size_t)n * K];
            double acc = 0, ab = 0; float a32 = 0.f;
            for (int k = 0; k < K; k++) { const double t = xd[k] * wn[k]; acc += t; ab += std::fabs(t); a32 += x32[k] * wf[k]; }
            d.sabs = std::max(d.sabs, ab);
            acc += d.bias[n];
            if (c.act == ACT_RELU6 && (acc < 0 || acc > 6)) clipped++;
            const size_t o = (size_t)m * N + n;
            d.y64[o] = act64(acc, c.act) + (c.res ? (double)d.res[o] : 0.0);
            float v32 = act32(a32 + d.bias[n], c.act);
            if (c.res) v32 += d.res[o];
            d.y32[o] = v32;
        }
    }
    if (c.act == ACT_RELU6) d.clip = (double)clipped / ((double)M * N);
}

// ------------------------------------------------------------------------------------------ device buffers
static const unsigned kPat = 0xffc0de5au;                 // a NaN payload no kernel arithmetic produces
static const unsigned kNaN = 0x7fc07fc0u;                 // a NaN as fp32 and as two bf16 values
static const size_t kGuard = 4096;                        // words on each side

static std::string cur_case = "(setup)";
#define HIPCHK(expr, what)                                                                                        \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) { printf("HIP ERROR %s at %s: %s\n", hipGetErrorString(e_), what, cur_case.c_str()); fflush(stdout); _Exit(3); } \
    } while (0)
// an input or parameter: [NaNs][exactly the bytes][NaNs] - a load beyond the tensor that meets a zero weight still shows
struct InBuf {
    char* d = nullptr;
    InBuf(const void* h, size_t bytes) {
        std::vector<unsigned> all(kGuard * 2 + (bytes + 3) / 4, kNaN);
        memcpy((char*)all.data() + kGuard * 4, h, bytes);
        if (bytes & 3) memset((char*)all.data() + kGuard * 4 + bytes, 0xff, 4 - (bytes & 3));      // (0xffff.. : a NaN too)
        HIPCHK(hipMalloc(&d, all.size() * 4), "hipMalloc");
        HIPCHK(hipMemcpy(d, all.data(), all.size() * 4, hipMemcpyHostToDevice), "hipMemcpy");
    }
    ~InBuf() { (void)hipFree(d); }
    InBuf(const InBuf&) = delete;
    const float* f() const { return reinterpret_cast<const float*>(d + kGuard * 4); }
};
static InBuf* in_f32(const std::vector<float>& v) { return new InBuf(v.data(), v.size() * 4); }
static InBuf* in_bf16(const std::vector<float>& v) {
    std::vector<uint16_t> h(v.size());
    for (size_t i = 0; i < v.size(); i++) h[i] = bf16_rne(v[i]);
    return new InBuf(h.data(), h.size() * 2);
}
// the output: [pattern][exactly the bytes][pattern]; bad() counts the guard bytes that changed
struct OutBuf {
    char* d = nullptr; size_t bytes, all; std::vector<unsigned> h;
    explicit OutBuf(size_t bytes_) : bytes(bytes_), all(kGuard * 8 + (bytes_ + 3) / 4 * 4), h(all / 4) { HIPCHK(hipMalloc(&d, all), "hipMalloc"); }
    ~OutBuf() { (void)hipFree(d); }
    OutBuf(const OutBuf&) = delete;
    void fill(hipStream_t st) { HIPCHK(hipMemsetD32Async((hipDeviceptr_t)d, (int)kPat, all / 4, st), "fill"); }
    void fetch() { HIPCHK(hipMemcpy(h.data(), d, all, hipMemcpyDeviceToHost), "copy back"); }
    float* dev() const { return reinterpret_cast<float*>(d + kGuard * 4); }
    const float* f() const { return reinterpret_cast<const float*>(h.data() + kGuard); }
    const uint16_t* h16() const { return reinterpret_cast<const uint16_t*>(h.data() + kGuard); }
    size_t bad() const {
        size_t n = 0;
        for (size_t i = 0; i < kGuard; i++) n += h[i] != kPat;
        const unsigned char* p = reinterpret_cast<const unsigned char*>(h.data());
        const unsigned char pb[4] = {0x5a, 0xde, 0xc0, 0xff};
        for (size_t i = kGuard * 4 + bytes; i < all; i++) n += p[i] != pb[i & 3];
        return n;
    }
};

struct Stat { int cases = 0; double ratio = 0, ek = 0, eh = 0; };
static std::map<std::string, Stat> forms;
static double absdiff(double a, double b) { double d = std::fabs(a - b); return (d == d && !std::isinf(d)) ? d : 1e30; }

static void wr(const std::string& dir, const char* fn, const void* p, size_t n) {
    FILE* f = fopen((dir + "/" + fn).c_str(), "wb");
    if (!f || fwrite(p, 1, n, f) != n) { printf("cannot write %s\n", fn); exit(2); }
    fclose(f);
}

int main(int argc, char** argv) {
    bool list = false; const char* only = nullptr; const char* dump = nullptr; const char* dump_dir = nullptr;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--list")) list = true;
        else if (!strcmp(argv[i], "--only") && i + 1 < argc) only = argv[++i];
        else if (!strcmp(argv[i], "--ref-dump") && i + 2 < argc) { dump = argv[++i]; dump_dir = argv[++i]; }
        else { printf("usage: pw64_lab [--list | --ref-dump NAME DIR | --only SUBSTR]\n"); return 2; }
    }
    // pw_fill_grid reads the switch once per process, so does the lab: with 0 no tile shrinks and the cases of pass 1 run, without
    // it the cases of pass 2
    const bool fill0 = getenv("BNHIP_PW_FILL") && atoi(getenv("BNHIP_PW_FILL")) == 0;
    const int pass = fill0 ? 1 : 2;
    const bool device = !list && !dump;
    if (device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { printf("no HIP device\n"); return 3; }
    }
    const std::vector<Case> cases = build_cases();
    printf("pw64_lab: %zu cases in two passes; this process: pass %d (%s)%s\n", cases.size(), pass, fill0 ? "BNHIP_PW_FILL=0: every tile as requested" : "the grid-fill shrink",
           device ? "" : " (no device touched)");
    printf("PASS %d\n", pass);
    int failures = 0, ran = 0, ncases = 0;
    hipStream_t st = nullptr;
    if (device) HIPCHK(hipStreamCreate(&st), "hipStreamCreate");

    for (const Case& c : cases) {
        if (dump ? c.name != dump : c.pass != pass) continue;
        const Pred pr = predict(c);
        const bool one = pr.one;
        if (list) {
            Data d; if (c.act == ACT_RELU6) gen(c, one, d);
            printf("CASE %s kind=%s form=%s M=%d N=%d K=%d HW=%d wm=%d nt=%d prec=%d sw=%d a16=%d o16=%d r16=%d scale=%d bias=%d res=%d act=%s slabs=%d req_rows=%d req_nt=%d run_rows=%d run_nt=%d tiled=%d", c.name.c_str(),
                   c.entry == E_IGEMM ? "ig" : "pw", pr.form.c_str(), c.M, c.N, c.K, c.HW, c.wm, c.nt, c.prec, c.sw, c.a16, c.o16, c.r16, c.HW ? 1 : 0, c.bias, c.res, act_name(c.act),
                   (c.K + 31) / 32, pr.tiled ? req_rows(c) : 0, c.nt, pr.rows, pr.nt, (int)pr.tiled);
            if (pr.tiled) { const PwGrid g = pw_grid(c.M, c.N, pr.nt, pr.rows / 64); printf(" mblk=%u nblk_n=%d", g.nblk / (unsigned)g.nblk_n, g.nblk_n); }
            if (c.entry == E_IGEMM) printf(" kh=%d kw=%d stride=%d dil=%d valid=%d B=%d H=%d W=%d Cin=%d Ho=%d Wo=%d pt=%d pl=%d", c.kh, c.kw, c.st, c.dil, c.valid, c.B, c.H, c.W, c.Cin, c.Ho, c.Wo, c.pt, c.pl);
            printf(" clip=%.4f\n", d.clip);
            ncases++;
            continue;
        }
        if (dump) {
            Data d; gen(c, one, d);
            wr(dump_dir, "a.f32", d.a.data(), d.a.size() * 4); wr(dump_dir, "w.f32", d.w.data(), d.w.size() * 4); wr(dump_dir, "b.f32", d.bias.data(), d.bias.size() * 4);
            wr(dump_dir, "scale.f32", d.sc.data(), d.sc.size() * 4); wr(dump_dir, "res.f32", d.res.data(), d.res.size() * 4);
            wr(dump_dir, "xr.f32", d.xr.data(), d.xr.size() * 4); wr(dump_dir, "wr.f32", d.wr.data(), d.wr.size() * 4);
            wr(dump_dir, "y.f64", d.y64.data(), d.y64.size() * 8);
            FILE* f = fopen((std::string(dump_dir) + "/meta.txt").c_str(), "w");
            fprintf(f, "kind=%s\nform=%s\nM=%d\nN=%d\nK=%d\nHW=%d\none=%d\nbias=%d\nres=%d\nact=%s\n", c.entry == E_IGEMM ? "ig" : "pw", pr.form.c_str(), c.M, c.N, c.K, c.HW, (int)one, c.bias, c.res,
                    act_name(c.act));
            if (c.entry == E_IGEMM) fprintf(f, "B=%d\nH=%d\nW=%d\nCin=%d\nkh=%d\nkw=%d\nstride=%d\ndil=%d\nvalid=%d\nHo=%d\nWo=%d\n", c.B, c.H, c.W, c.Cin, c.kh, c.kw, c.st, c.dil, c.valid, c.Ho, c.Wo);
            fclose(f);
            printf("dumped %s\n", c.name.c_str());
            return 0;
        }
        if (only && !strstr(c.name.c_str(), only)) continue;
        ncases++;
        cur_case = c.name + " [" + pr.form + (pr.tiled ? " " + std::to_string(pr.rows) + "x" + std::to_string(16 * pr.nt) : std::string()) + "]";
        printf("RUN %s\n", cur_case.c_str()); fflush(stdout);
        Data d; gen(c, one, d);
        const size_t nout = d.y64.size();
        double scale = 0, eh = 0;
        for (size_t i = 0; i < nout; i++) scale = std::max(scale, std::fabs(d.y64[i]));
        for (size_t i = 0; i < nout; i++) eh = std::max(eh, std::fabs((double)d.y32[i] - d.y64[i]));
        eh /= scale;
        // err <= 4 err_f32host + 2^-22, err = max|got - ref64| / max|ref64|.  Six-product forms: plus the split terms they drop, at most
        // 2^-23 of every |a scale w| (pw_bx3.hip), 2^-23 max sum_k |a scale w| / max|ref64|.  One-product forms: the reference was taken
        // on the operands the kernel rounds (a scale multiplied in fp32, then RNE to bf16; weights RNE to bf16, the image's hi plane)
        // and their products are exact in fp32 as in fp64, so the plain gate holds.
        double gate = 4.0 * eh + std::ldexp(1.0, -22);
        if (c.entry == E_BX3 && pr.six) gate += std::ldexp(1.0, -23) * d.sabs / scale;
        InBuf* dA = c.a16 ? in_bf16(d.a) : in_f32(d.a);
        InBuf* dW = in_f32(d.w);
        InBuf* db = c.bias ? in_f32(d.bias) : nullptr;
        InBuf* ds = c.HW ? in_f32(d.sc) : nullptr;
        InBuf* dr = c.res ? (c.r16 ? in_bf16(d.res) : in_f32(d.res)) : nullptr;
        InBuf* dimg = nullptr;
        if (c.entry == E_BX3) { const std::vector<uint16_t> img = pw_bx3_image(d.w.data(), c.N, c.K); dimg = new InBuf(img.data(), img.size() * 2); }
        OutBuf y(nout * (c.o16 ? 2 : 4));
        y.fill(st);
        PwParams p = params_of(c);
        p.A = dA->f(); p.W = dW->f(); p.bias = db ? db->f() : nullptr; p.ascale = ds ? ds->f() : nullptr; p.res = dr ? dr->f() : nullptr; p.out = y.dev();
        const long ws0 = bnhip_debug_pw_ws_launches(), lat0 = bnhip_debug_pw_lat_launches(), b0 = bnhip_debug_pw_b16_launches();
        if (c.entry == E_GEMM) launch_pw_gemm(p, st);
        else if (c.entry == E_BX3) launch_pw_bx3(p, reinterpret_cast<const uint16_t*>(dimg->f()), st);
        else launch_conv_igemm(p.A, p.W, p.bias, p.out, c.B, c.H, c.W, c.Cin, c.Ho, c.Wo, c.N, c.kh, c.kw, c.st, c.st, c.dil, c.dil, c.pt, c.pl, c.act, c.nt, c.wm, st);
        HIPCHK(hipGetLastError(), "launch");
        HIPCHK(hipStreamSynchronize(st), "synchronize");
        y.fetch();
        ran++;
        bool ok = true; std::string why;
        const long dws = bnhip_debug_pw_ws_launches() - ws0, dlat = bnhip_debug_pw_lat_launches() - lat0, db16 = bnhip_debug_pw_b16_launches() - b0;
        if (dws != (pr.ws ? 1 : 0) || dlat != (pr.lat ? 1 : 0) || db16 != (pr.b16 ? 1 : 0)) {
            ok = false;
            why += " form:predicted_" + pr.form + "_but_counters_ws" + std::to_string(dws) + "_lat" + std::to_string(dlat) + "_b16_" + std::to_string(db16);
        }
        const size_t gbad = y.bad();
        if (gbad) { ok = false; why += " guard:" + std::to_string(gbad) + "_bytes_overwritten"; }
        double ek = 0, ratio = 0; size_t worst = 0;
        for (size_t i = 0; i < nout; i++) {
            double got, ref = d.y64[i], allow = gate * scale;
            if (c.o16) {       // compare with the rounded reference, one bf16 ulp of the element on top
                got = bf16_widen(y.h16()[i]);
                const float rr = bf16_round((float)ref); int ex; (void)std::frexp(rr == 0.f ? std::ldexp(1.0, -126) : (double)rr, &ex);
                ref = rr; allow += std::ldexp(1.0, ex - 8);
            } else got = y.f()[i];
            const double df = absdiff(got, ref);
            ek = std::max(ek, df / scale);
            if (df / allow > ratio) { ratio = df / allow; worst = i; }
        }
        if (ratio > 1.0) {
            ok = false;
            char buf[120]; snprintf(buf, sizeof buf, " y:ratio=%.3g_at_m%zu_n%zu", ratio, worst / c.N, worst % c.N);
            why += buf;
        }
        printf("%s %s err=%.3e host32=%.3e gate=%.3e ratio=%.3f%s\n", ok ? "ok  " : "FAIL", cur_case.c_str(), ek, eh, gate, ratio, why.c_str());
        if (!ok) failures++;
        Stat& s = forms[pr.form];
        s.cases++; s.ek = std::max(s.ek, ek); s.eh = std::max(s.eh, eh); s.ratio = std::max(s.ratio, ratio);
        delete dA; delete dW; delete db; delete ds; delete dr; delete dimg;
    }
    if (dump) { printf("no such case: %s\n", dump); return 2; }
    for (auto& kv : forms) printf("FORM %s | cases=%d worst_err=%.3e worst_host32=%.3e worst_ratio=%.3f\n", kv.first.c_str(), kv.second.cases, kv.second.ek, kv.second.eh, kv.second.ratio);
    printf("SUMMARY {\"cases\": %d, \"ran\": %d, \"failures\": %d, \"pass\": %d}\n", ncases, ran, failures, pass);
    return failures ? 1 : 0;
}
