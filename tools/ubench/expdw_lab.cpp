// Fused expand + depthwise lab: every compiled form of k_expand_dw / k_expand_dw_sk / the COPY form, through the library's own
// launchers (launch_expand_dw, launch_dwconv_lds) WITH AN EXPLICIT SHAPE INDEX, on synthetic layers and without a model.  Every
// output element and every per-tile squeeze-excite sum is held to a plain fp64 loop nest on the host; a plain fp32 evaluation of the
// same case next to it sizes the tolerance (gate = 4 x its error + 2^-22).  Guard regions around y and the sums
// prove that nothing else is written.  The case list is fixed (seeded in this file).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I birdnet-go_amd/csrc -o expdw_lab tools/ubench/expdw_lab.cpp \
//         -L birdnet-go_amd/lib -lbnhip -Wl,-rpath,birdnet-go_amd/lib
//   expdw_lab                    run every case on the current device; exit status 1 on any failed check, 3 on a HIP error
//   expdw_lab --list             print layers, cases and the covered (shape, form) pairs; touches no device (assumes 256 CUs)
//   expdw_lab --ref-dump L DIR   write the inputs, parameters and fp64 result of layer L as raw arrays (no device)
//   expdw_lab --only SUBSTR      run the layers whose name contains SUBSTR
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "kernels.h"
using namespace bnhip;

// ---- the tile-shape table, restated (toh, tow per index modulo n; indices >= n: rows and columns swapped).  The library keeps its
// own private; the lab needs the tile extents to attribute output pixels to slabs, and checks its copy against expdw_shape_slabs.
struct TileShape { int k, s, toh, tow, trh, nw; };
static const TileShape kTiles[] = {
    {3, 1, 8, 16, 10, 4}, {3, 1, 4, 16, 6, 4}, {3, 1, 8, 32, 6, 4}, {3, 1, 8, 32, 10, 4},
    {5, 1, 8, 16, 12, 4}, {5, 1, 4, 16, 8, 4}, {5, 1, 8, 32, 6, 4}, {5, 1, 12, 16, 12, 4},
    {3, 2, 4, 8, 9, 4},   {3, 2, 8, 8, 12, 4}, {3, 2, 8, 8, 17, 4},
    {5, 2, 4, 8, 11, 4},  {5, 2, 4, 16, 6, 4}, {5, 2, 8, 8, 19, 4},
    {3, 1, 8, 16, 10, 8}, {3, 1, 8, 32, 6, 8}, {3, 1, 8, 32, 10, 8}, {5, 1, 8, 16, 12, 8}, {5, 1, 8, 32, 6, 8},
    {3, 2, 8, 8, 12, 8},  {3, 2, 8, 8, 17, 8}, {5, 2, 8, 8, 19, 8},
};
static const int kNT = (int)(sizeof(kTiles) / sizeof(kTiles[0]));

static uint16_t bf16_rne(float f) {                      // the rounding of expdw_bx_image's first plane
    unsigned u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static float bf16_widen(uint16_t h) { unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }
static float bf16_round(float f) { return bf16_widen(bf16_rne(f)); }

static double act64(double v, int act) {
    switch (act) {
        case ACT_SWISH: return v / (1.0 + std::exp(-v));
        case ACT_RELU6: return std::min(std::max(v, 0.0), 6.0);
        default: return v;
    }
}
static float act32(float v, int act) {
    switch (act) {
        case ACT_SWISH: return v / (1.0f + expf(-v));
        case ACT_RELU6: return fminf(fmaxf(v, 0.0f), 6.0f);
        default: return v;
    }
}
static const char* act_name(int a) { return a == ACT_SWISH ? "swish" : a == ACT_RELU6 ? "relu6" : "none"; }

// ---- geometries: H, W are the depthwise input (= expand output) size; SAME padding by TensorFlow's rule.  Stem: Hin, Win the raw image.
struct Geo { const char* name; int k, s, H, W; bool stem; int Hin, Win; const char* why; };
static const Geo kGeos[] = {
    {"k3s1_ragged", 3, 1, 19, 37, false, 0, 0, "Ho, Wo no multiple of any tile: ragged last tile row and column"},
    {"k3s1_flat", 3, 1, 6, 70, false, 0, 0, "wide-flat; the whole height is exactly TRH = 6 footprint rows of the 8-row tiles"},
    {"k3s1_tall", 3, 1, 70, 6, false, 0, 0, "tall-narrow: the transposed shapes' home"},
    {"k3s1_tiny", 3, 1, 5, 7, false, 0, 0, "smaller than one tile in both directions"},
    {"k3s1_onetile", 3, 1, 8, 16, false, 0, 0, "exactly one 8 x 16 tile: no vertical halo (compacted footprint rows)"},
    {"k5s1_ragged", 5, 1, 17, 35, false, 0, 0, "ragged; 12-row tile cut at 5 rows"},
    {"k5s1_flat", 5, 1, 6, 44, false, 0, 0, "wide-flat, exactly TRH = 6"},
    {"k5s1_tall", 5, 1, 44, 6, false, 0, 0, "tall-narrow"},
    {"k5s1_twelve", 5, 1, 12, 20, false, 0, 0, "exactly one 12-row tile high, in-image footprint = TRH = 12"},
    {"k5s1_twelve_t", 5, 1, 20, 12, false, 0, 0, "the same, transposed"},
    {"k3s2_oddeven", 3, 2, 31, 34, false, 0, 0, "stride 2, odd H (pt == pb) and even W (pl = 0 != pr = 1)"},
    {"k3s2_evenodd", 3, 2, 12, 45, false, 0, 0, "stride 2, even H = 12: one 8-row tile whose in-image footprint is exactly TRH = 12"},
    {"k3s2_tall", 3, 2, 45, 12, false, 0, 0, "the same, transposed"},
    {"k5s2_oddeven", 5, 2, 29, 32, false, 0, 0, "stride 2, 5 x 5: odd H, even W (pl = 1, pr = 2)"},
    {"k5s2_flat", 5, 2, 6, 50, false, 0, 0, "H = 6 = TRH of the 4 x 16 tile"},
    {"k5s2_tall", 5, 2, 50, 6, false, 0, 0, "the same, transposed"},
    {"stem_ragged", 3, 1, 19, 33, true, 37, 66, "stem: odd raw height, even raw width"},
    {"stem_flat", 3, 1, 6, 40, true, 12, 79, "stem: flat image for the TRH = 6 tile"},
};
static const int kNG = (int)(sizeof(kGeos) / sizeof(kGeos[0]));

// ---- channel / activation / form configurations
enum Mode { M_F32 = 0, M_BX, M_P1, M_P1X /* prec = 1 with x stored as bf16 */, M_COPY, M_STEM };
struct Cfg { const char* name; int Cin, Cmid, act_e, act_d, mode; int out_bf16; int copy_xbf16; int copy_bias; int bsel /* 0: B = 2; 1: B = 1, 3 and the large B (chunk loop whole); 2: B = 2 and the large B; 3: only the B that cut the loop into parts of several chunks */; int nosums; };
static const Cfg kCfgs[] = {
    // f32 MFMA: chunk loop Kw = 16 / 24 / 32 (and the eight-wave shapes), half slab, full slabs
    {"c16x64", 16, 64, ACT_SWISH, ACT_SWISH, M_F32, 0, 0, 0, 1, 0},
    {"c20x36", 20, 36, ACT_SWISH, ACT_SWISH, M_F32, 0, 0, 0, 1, 0},      // K tail of Kw = 24, single tail quad
    {"c24x60", 24, 60, ACT_SWISH, ACT_RELU6, M_F32, 0, 0, 0, 0, 0},      // tail chunk of 7 quads
    {"c32x100", 32, 100, ACT_SWISH, ACT_SWISH, M_F32, 0, 0, 0, 1, 1},
    {"c32x100_obf", 32, 100, ACT_SWISH, ACT_NONE, M_F32, 1, 0, 0, 0, 0},
    {"c36x36", 36, 36, ACT_SWISH, ACT_NONE, M_F32, 0, 0, 0, 0, 0},       // Kw = 40: K tail of the half slab
    {"c40x96", 40, 96, ACT_SWISH, ACT_SWISH, M_F32, 0, 0, 0, 0, 0},
    {"c48x60", 48, 60, ACT_SWISH, ACT_SWISH, M_F32, 0, 0, 0, 0, 1},
    {"c48x60_obf", 48, 60, ACT_SWISH, ACT_SWISH, M_F32, 1, 0, 0, 0, 0},
    {"c64x160", 64, 160, ACT_SWISH, ACT_RELU6, M_F32, 0, 0, 0, 0, 0},    // five chunks
    {"c96x100", 96, 100, ACT_SWISH, ACT_SWISH, M_F32, 0, 0, 0, 0, 0},
    {"c128x64", 128, 64, ACT_SWISH, ACT_NONE, M_F32, 0, 0, 0, 0, 0},
    // non-swish expand activation: leaves the chunk loop for k_expand_dw
    {"c32x64_er6", 32, 64, ACT_RELU6, ACT_SWISH, M_F32, 0, 0, 0, 0, 0},
    {"c24x36_en", 24, 36, ACT_NONE, ACT_RELU6, M_F32, 0, 0, 0, 0, 0},
    {"c16x32_er6", 16, 32, ACT_RELU6, ACT_NONE, M_F32, 0, 0, 0, 0, 0},
    // split-bf16 phase 1 (six products)
    {"c40x96_bx", 40, 96, ACT_SWISH, ACT_SWISH, M_BX, 0, 0, 0, 0, 0},
    {"c48x60_bx", 48, 60, ACT_SWISH, ACT_RELU6, M_BX, 0, 0, 0, 0, 0},
    {"c96x100_bx", 96, 100, ACT_SWISH, ACT_SWISH, M_BX, 0, 0, 0, 0, 0},
    {"c128x64_bx", 128, 64, ACT_SWISH, ACT_SWISH, M_BX, 1, 0, 0, 0, 0},
    {"c32x64_er6_bx", 32, 64, ACT_RELU6, ACT_SWISH, M_BX, 0, 0, 0, 0, 0},
    // one-product bf16 pipe: Kw = 24, 32 and NS = 2, 3, 5 resident slabs; x as fp32 and as bf16
    {"c24x60_p1", 24, 60, ACT_SWISH, ACT_SWISH, M_P1, 0, 0, 0, 1, 0},
    {"c24x60_p1x", 24, 60, ACT_SWISH, ACT_SWISH, M_P1X, 0, 0, 0, 2, 0},
    {"c32x100_p1", 32, 100, ACT_SWISH, ACT_RELU6, M_P1, 0, 0, 0, 2, 0},
    {"c32x100_p1x", 32, 100, ACT_SWISH, ACT_SWISH, M_P1X, 1, 0, 0, 2, 0},
    {"c48x36_p1", 48, 36, ACT_SWISH, ACT_SWISH, M_P1, 0, 0, 0, 2, 0},
    {"c64x64_p1x", 64, 64, ACT_SWISH, ACT_SWISH, M_P1X, 0, 0, 0, 2, 0},
    {"c96x100_p1", 96, 100, ACT_SWISH, ACT_SWISH, M_P1, 0, 0, 0, 2, 1},
    {"c96x100_p1x", 96, 100, ACT_SWISH, ACT_NONE, M_P1X, 0, 0, 0, 2, 0},
    {"c160x160_p1", 160, 160, ACT_SWISH, ACT_SWISH, M_P1, 0, 0, 0, 2, 0},
    {"c160x160_p1x", 160, 160, ACT_SWISH, ACT_SWISH, M_P1X, 0, 0, 0, 2, 0},
    {"c128x64_bx1", 128, 64, ACT_SWISH, ACT_SWISH, M_P1, 0, 0, 0, 0, 0},   // four slabs: no resident form -> k_expand_dw BX with one product
    // small calls whose chunk loop is cut into parts of SEVERAL chunks with a ragged last part (five chunks: 2 + 2 + 1)
    {"c32x160_parts", 32, 160, ACT_SWISH, ACT_SWISH, M_F32, 0, 0, 0, 3, 0},
    {"c24x160_parts", 24, 160, ACT_SWISH, ACT_SWISH, M_F32, 0, 0, 0, 3, 0},
    {"c16x160_parts", 16, 160, ACT_SWISH, ACT_SWISH, M_F32, 0, 0, 0, 3, 0},
    {"c96x160_p1_parts", 96, 160, ACT_SWISH, ACT_SWISH, M_P1, 0, 0, 0, 3, 0},
    {"c160x160_p1x_parts", 160, 160, ACT_SWISH, ACT_SWISH, M_P1X, 0, 0, 0, 3, 0},
    // plain depthwise through the same kernel (COPY), unpadded parameters, C % 32 != 0
    {"copy36", 36, 36, ACT_NONE, ACT_SWISH, M_COPY, 0, 0, 1, 0, 0},
    {"copy100_r6", 100, 100, ACT_NONE, ACT_RELU6, M_COPY, 0, 0, 1, 0, 1},
    {"copy60_nob", 60, 60, ACT_NONE, ACT_NONE, M_COPY, 0, 0, 0, 0, 0},
    {"copy100_bf", 100, 100, ACT_NONE, ACT_SWISH, M_COPY, 1, 1, 1, 0, 0},
    // stem (3 x 3 stride 2 on a two-channel image) + 3 x 3 depthwise
    {"stem32", 32, 32, ACT_SWISH, ACT_SWISH, M_STEM, 0, 0, 0, 0, 0},
    {"stem64_r6", 32, 64, ACT_RELU6, ACT_RELU6, M_STEM, 0, 0, 0, 0, 1},
};
static const int kNC = (int)(sizeof(kCfgs) / sizeof(kCfgs[0]));

struct Layer {
    std::string name;
    Geo g; Cfg c;
    int B, Ho, Wo, pt, pl, pts, pls;
    bool bf16_ops;                                        // x and We rounded to bf16 (prec = 1 forms)
    // data (filled by gen)
    std::vector<float> x, we, be, wd, bd;                 // we: [Cmid][Cin] (stem: [Cmid][3][3][2]); wd: [k*k][Cmid]
    std::vector<double> y64, bxabs;                       // reference, and sum_taps |wd| sum_k |we x| per output (BX bound)
    std::vector<float> y32;
    double clip_e = -1, clip_d = -1;                      // share of elements the ReLU6 changes (-1: no ReLU6 there)
};
static int same_out(int H, int s) { return (H + s - 1) / s; }
static int same_pad(int H, int Ho, int k, int s) { return std::max((Ho - 1) * s + k - H, 0) / 2; }

static ExpDwGeo geo_of(const Layer& L, bool pipe16) {
    ExpDwGeo g{L.g.k, L.g.s, L.g.H, L.g.W, L.Ho, L.Wo, L.pt, L.pl, L.g.stem, 0};
    if (L.c.mode != M_COPY && !pipe16) g.skw = expdw_skw(L.c.Cin, L.c.act_e, L.g.stem);
    return g;
}
static bool layer_pipe16(const Layer& L) {
    const bool img = L.c.mode == M_BX || L.c.mode == M_P1 || L.c.mode == M_P1X;
    return L.c.mode != M_COPY && expdw_sk_pipe16(L.c.Cin, L.c.act_e, L.g.stem, (L.c.mode == M_P1 || L.c.mode == M_P1X) ? 1 : 0, img);
}

// pixels of the expanded tensor as the reference sees them: E[b][h][w][n], fp64 and fp32
static void gen(Layer& L, bool want32) {
    const Geo& g = L.g; const Cfg& c = L.c;
    const int B = L.B, H = g.H, W = g.W, Cin = c.Cin, Cm = c.Cmid, k = g.k, s = g.s, Ho = L.Ho, Wo = L.Wo;
    unsigned seed = 2166136261u;                          // FNV-1a of the layer's name: the same data on every run and machine
    for (char ch : L.name) seed = (seed ^ (unsigned char)ch) * 16777619u;
    std::mt19937 rng(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    const bool copy = c.mode == M_COPY, stem = c.mode == M_STEM;
    const int K = stem ? 18 : Cin;
    L.x.resize(stem ? (size_t)B * g.Hin * g.Win * 2 : (size_t)B * H * W * Cin);
    for (auto& v : L.x) v = nd(rng);
    // ReLU6 layers: pre-activations N(1.5, 3) so that both clips bite on a visible share (~31 % below 0, ~7 % above 6)
    const float ge = c.act_e == ACT_RELU6 ? 3.f : 1.f, se = c.act_e == ACT_RELU6 ? 1.5f : 0.f;
    if (!copy) {
        L.we.resize((size_t)Cm * K);
        for (auto& v : L.we) v = nd(rng) * ge / std::sqrt((float)K);
        L.be.resize(Cm);
        for (auto& v : L.be) v = 0.1f * nd(rng) + se;
    }
    L.wd.resize((size_t)k * k * Cm);
    for (auto& v : L.wd) v = nd(rng) / (float)k;
    L.bd.assign(Cm, 0.f);
    if (!copy || c.copy_bias) for (auto& v : L.bd) v = 0.1f * nd(rng);
    if (L.bf16_ops) { for (auto& v : L.x) v = bf16_round(v); for (auto& v : L.we) v = bf16_round(v); }
    if (copy && c.copy_xbf16) for (auto& v : L.x) v = bf16_round(v);

    // ---- expand (fp64, |.| sums for the BX bound, and fp32 sequential)
    const size_t npx = (size_t)B * H * W;
    std::vector<double> E(npx * Cm), A(npx * Cm, 0.0);
    std::vector<float> E32(want32 ? npx * Cm : 0);
    size_t clipped = 0;
    std::vector<float> win(18);
    for (int b = 0; b < B; b++)
        for (int h = 0; h < H; h++)
            for (int w = 0; w < W; w++) {
                const size_t px = ((size_t)b * H + h) * W + w;
                const float* xp;
                if (stem) {
                    for (int i = 0; i < 3; i++)
                        for (int j = 0; j < 3; j++)
                            for (int ic = 0; ic < 2; ic++) {
                                const int r = 2 * h - L.pts + i, q = 2 * w - L.pls + j;
                                win[(i * 3 + j) * 2 + ic] = (r >= 0 && r < g.Hin && q >= 0 && q < g.Win) ? L.x[(((size_t)b * g.Hin + r) * g.Win + q) * 2 + ic] : 0.f;
                            }
                    xp = win.data();
                } else xp = &L.x[px * Cin];
                for (int n = 0; n < Cm; n++) {
                    if (copy) { E[px * Cm + n] = xp[n]; if (want32) E32[px * Cm + n] = xp[n]; continue; }
                    const float* wr = &L.we[(size_t)n * K];
                    double acc = 0, ab = 0;
                    for (int q = 0; q < K; q++) { const double t = (double)xp[q] * (double)wr[q]; acc += t; ab += std::fabs(t); }
                    acc += L.be[n];
                    if (c.act_e == ACT_RELU6 && (acc < 0 || acc > 6)) clipped++;
                    E[px * Cm + n] = act64(acc, c.act_e); A[px * Cm + n] = ab + std::fabs((double)L.be[n]);
                    if (want32) {
                        float a32 = 0.f;
                        for (int q = 0; q < K; q++) a32 += xp[q] * wr[q];
                        E32[px * Cm + n] = act32(a32 + L.be[n], c.act_e);
                    }
                }
            }
    if (c.act_e == ACT_RELU6) L.clip_e = (double)clipped / (double)(npx * Cm);
    if (c.act_d == ACT_RELU6) {
        // taps scaled so that the depthwise pre-activation has a standard deviation of about 3 around 1.5 (as above)
        double ss = 0; for (double v : E) ss += v * v;
        const float gd = 3.f / (float)std::sqrt(ss / (double)E.size() + 1e-30);
        for (auto& v : L.wd) v *= gd;
        for (auto& v : L.bd) v += 1.5f;
    }
    // ---- depthwise, SAME padding = zero padding of the expanded tensor
    const size_t nout = (size_t)B * Ho * Wo * Cm;
    L.y64.resize(nout); L.bxabs.resize(nout); if (want32) L.y32.resize(nout);
    clipped = 0;
    for (int b = 0; b < B; b++)
        for (int oh = 0; oh < Ho; oh++)
            for (int ow = 0; ow < Wo; ow++)
                for (int n = 0; n < Cm; n++) {
                    double acc = 0, ab = 0; float a32 = 0.f;
                    for (int i = 0; i < k; i++)
                        for (int j = 0; j < k; j++) {
                            const int h = oh * s - L.pt + i, w = ow * s - L.pl + j;
                            if (h < 0 || h >= H || w < 0 || w >= W) continue;
                            const size_t e = (((size_t)b * H + h) * W + w) * Cm + n;
                            const float t = L.wd[(size_t)(i * k + j) * Cm + n];
                            acc += E[e] * (double)t; ab += A[e] * std::fabs((double)t);
                            if (want32) a32 += E32[e] * t;
                        }
                    acc += L.bd[n];
                    if (c.act_d == ACT_RELU6 && (acc < 0 || acc > 6)) clipped++;
                    const size_t o = (((size_t)b * Ho + oh) * Wo + ow) * Cm + n;
                    L.y64[o] = act64(acc, c.act_d); L.bxabs[o] = ab;
                    if (want32) L.y32[o] = act32(a32 + L.bd[n], c.act_d);
                }
    if (c.act_d == ACT_RELU6) L.clip_d = (double)clipped / (double)nout;
}

// ---- one case = layer x shape index x (sums given or not)
struct Case { int layer, shape; bool sums; std::vector<std::string> forms; int parted /* 0: whole chunk loop, 1: one chunk per part, 2: several */; };

// the dispatcher's branch, from the launcher's public predicates
static std::string branch_of(const Layer& L, int shape, int cus, int* parted) {
    const Cfg& c = L.c;
    *parted = 0;
    if (c.mode == M_COPY) return "copy";
    if (c.mode == M_STEM) return "stem";
    const bool img = c.mode != M_F32, p1 = c.mode == M_P1 || c.mode == M_P1X;
    const bool pipe16 = expdw_sk_pipe16(c.Cin, c.act_e, false, p1 ? 1 : 0, img);
    const int skw = pipe16 ? 0 : expdw_skw(c.Cin, c.act_e, false);
    const bool sk = pipe16 || skw != 0;
    std::string br;
    const int kw = expdw_kw(c.Cin);
    if (kTiles[shape % kNT].nw == 8) br = "sk" + std::to_string(skw) + "_nw8";
    else if (pipe16) {
        const int kp = (c.Cin + 31) / 32 * 32;
        br = kp == 64 ? "pipe16_ns2" : kp == 96 ? "pipe16_ns3" : kp == 160 ? "pipe16_ns5" : kw == 24 ? "pipe16_kw24" : "pipe16_kw32";
        if (c.mode == M_P1X) br += "_xbf16";
    } else if (skw) br = "sk" + std::to_string(skw);
    else if (img && expdw_bx_ok(c.Cin)) br = p1 ? "bx1" : "bx";
    else br = (kw & 8) ? "f32_h8" : "f32_full";
    if (sk) {
        const int cch = (c.Cmid + 31) / 32;
        const long bt = (long)L.B * expdw_shape_slabs(shape, geo_of(L, pipe16));
        if (cch > 1 && bt < cus / 2) {
            const int want = (int)std::min<long>(cch, (cus + bt - 1) / bt);
            const int cpp = (cch + want - 1) / want;
            if ((cch + cpp - 1) / cpp > 1) *parted = cpp > 1 ? 2 : 1;
        }
    }
    return br;
}

static const unsigned kPat = 0xffc0de5au;                 // a NaN payload no kernel arithmetic produces
static const size_t kGuard = 4096;                        // floats on each side

static std::string cur_case = "(setup)";
#define HIPCHK(expr, what)                                                                                        \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) { printf("HIP ERROR %s at %s: %s\n", hipGetErrorString(e_), what, cur_case.c_str()); fflush(stdout); _Exit(3); } \
    } while (0)
template <typename T>
static T* dev_guarded(const std::vector<T>& h, bool nan_guard) {
    // [guard][data][guard]; the guards of an INPUT hold NaNs: a load beyond the tensor that meets a zero weight still shows
    const size_t gb = kGuard * 4, nb = h.size() * sizeof(T);
    std::vector<unsigned> all((gb * 2 + nb + 3) / 4 + 1, nan_guard ? 0x7fc00000u : 0u);
    memcpy((char*)all.data() + gb, h.data(), nb);
    char* d; HIPCHK(hipMalloc(&d, all.size() * 4), "hipMalloc");
    HIPCHK(hipMemcpy(d, all.data(), all.size() * 4, hipMemcpyHostToDevice), "hipMemcpy");
    return reinterpret_cast<T*>(d + gb);
}
template <typename T> static void dev_free_guarded(T* p) { if (p) (void)hipFree((char*)p - kGuard * 4); }

struct Stat { int cases = 0; double ratio = 0, ek = 0, eh = 0; };

int main(int argc, char** argv) {
    bool list = false; const char* only = nullptr; const char* dump_layer = nullptr; const char* dump_dir = nullptr;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--list")) list = true;
        else if (!strcmp(argv[i], "--only") && i + 1 < argc) only = argv[++i];
        else if (!strcmp(argv[i], "--ref-dump") && i + 2 < argc) { dump_layer = argv[++i]; dump_dir = argv[++i]; }
        else { printf("usage: expdw_lab [--list | --ref-dump LAYER DIR | --only SUBSTR]\n"); return 2; }
    }
    if (expdw_num_shapes() != 2 * kNT) { printf("FAIL: the library has %d shape indices, the lab's table %d\n", expdw_num_shapes(), 2 * kNT); return 1; }
    int cus = 256;
    if (!list && !dump_layer) {
        int nd = 0;
        if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) { printf("no HIP device\n"); return 3; }
        cus = device_cus();
    }
    printf("expdw_lab: %d shape indices, %d CUs%s\n", 2 * kNT, cus, list || dump_layer ? " (assumed: no device touched)" : "");

    if (list)
        for (int i = 0; i < kNT; i++) printf("SHAPE %d k=%d s=%d toh=%d tow=%d trh=%d nw=%d\n", i, kTiles[i].k, kTiles[i].s, kTiles[i].toh, kTiles[i].tow, kTiles[i].trh, kTiles[i].nw);
    if (list)
        for (const Geo& g : kGeos) printf("GEO %s k=%d s=%d H=%d W=%d: %s\n", g.name, g.k, g.s, g.H, g.W, g.why);
    // ---- layers
    std::vector<Layer> layers;
    for (int gi = 0; gi < kNG; gi++)
        for (int ci = 0; ci < kNC; ci++) {
            const Geo& g = kGeos[gi]; const Cfg& c = kCfgs[ci];
            if ((c.mode == M_STEM) != g.stem) continue;
            Layer L; L.g = g; L.c = c;
            L.Ho = same_out(g.H, g.s); L.Wo = same_out(g.W, g.s);
            L.pt = same_pad(g.H, L.Ho, g.k, g.s); L.pl = same_pad(g.W, L.Wo, g.k, g.s);
            L.pts = g.stem ? same_pad(g.Hin, g.H, 3, 2) : 0; L.pls = g.stem ? same_pad(g.Win, g.W, 3, 2) : 0;
            if (g.stem && (same_out(g.Hin, 2) != g.H || same_out(g.Win, 2) != g.W)) { printf("FAIL: stem geometry %s\n", g.name); return 1; }
            L.bf16_ops = c.mode == M_P1 || c.mode == M_P1X;
            const bool pipe16 = layer_pipe16(L);
            const ExpDwGeo eg = geo_of(L, pipe16);
            int min_tiles = 1 << 30, nfit = 0;
            for (int s = 0; s < 2 * kNT; s++)
                if (expdw_shape_fits(s, eg, false)) { min_tiles = std::min(min_tiles, expdw_shape_slabs(s, eg)); nfit++; }
            if (!nfit) continue;
            std::vector<int> Bs;
            const int big = (cus / 2 + min_tiles - 1) / min_tiles;
            if (c.bsel == 1) Bs = {1, 3, big};
            else if (c.bsel == 2) Bs = {2, big};
            else if (c.bsel == 3) {                       // B * tiles of about 3 / 8 of the CUs: three or four parts wanted of five chunks
                for (int s = 0; s < 2 * kNT; s++)
                    if (expdw_shape_fits(s, eg, false)) {
                        const int B = (cus * 3 / 8 + expdw_shape_slabs(s, eg) - 1) / expdw_shape_slabs(s, eg);
                        if (std::find(Bs.begin(), Bs.end(), B) == Bs.end()) Bs.push_back(B);
                    }
            } else Bs = {2};
            for (int B : Bs) {
                L.B = B;
                L.name = std::string(g.name) + "/" + c.name + "/B" + std::to_string(B);
                layers.push_back(L);
            }
        }
    // ---- cases
    std::vector<Case> cases;
    for (int li = 0; li < (int)layers.size(); li++) {
        const Layer& L = layers[li];
        const bool pipe16 = layer_pipe16(L);
        const ExpDwGeo eg = geo_of(L, pipe16);
        for (int s = 0; s < 2 * kNT; s++) {
            if (!expdw_shape_fits(s, eg, false)) continue;
            const TileShape& t = kTiles[s % kNT];
            const int oHo = s >= kNT ? L.Wo : L.Ho, oWo = s >= kNT ? L.Ho : L.Wo;
            if (expdw_shape_slabs(s, eg) != ((oHo + t.toh - 1) / t.toh) * ((oWo + t.tow - 1) / t.tow)) { printf("FAIL: tile table differs from the library's at index %d\n", s); return 1; }
            for (int sums = 1; sums >= (L.c.nosums && L.B <= 2 ? 0 : 1); sums--) {
                Case cs{li, s, sums != 0, {}, 0};
                const std::string br = branch_of(L, s, cus, &cs.parted);
                if (L.c.bsel == 3 && cs.parted != 2) continue;      // (these layers exist for that path only)
                cs.forms.push_back(br);
                if (L.c.mode != M_COPY && L.c.act_e != ACT_SWISH) cs.forms.push_back(std::string("acte_") + act_name(L.c.act_e));
                cs.forms.push_back(std::string("actd_") + act_name(L.c.act_d));
                if (L.c.out_bf16) cs.forms.push_back("out_bf16");
                if (L.c.mode == M_COPY && L.c.copy_xbf16) cs.forms.push_back("copy_xbf16");
                if (!sums) cs.forms.push_back("nosums");
                if (br.compare(0, 2, "sk") == 0 || br.compare(0, 6, "pipe16") == 0) {
                    if ((L.c.Cmid + 31) / 32 > 1) cs.forms.push_back(br + (cs.parted == 2 ? "+parts" : cs.parted ? "+parted" : "+whole"));   // the chunk loop whole, one chunk per part, several per part
                }
                cases.push_back(cs);
            }
        }
    }

    if (dump_layer) {
        for (Layer& L : layers) {
            if (L.name != dump_layer) continue;
            gen(L, false);
            const std::string d = dump_dir;
            auto wr = [&](const char* fn, const void* p, size_t n) {
                FILE* f = fopen((d + "/" + fn).c_str(), "wb");
                if (!f || fwrite(p, 1, n, f) != n) { printf("cannot write %s\n", fn); exit(2); }
                fclose(f);
            };
            wr("x.f32", L.x.data(), L.x.size() * 4); wr("we.f32", L.we.data(), L.we.size() * 4); wr("be.f32", L.be.data(), L.be.size() * 4);
            wr("wd.f32", L.wd.data(), L.wd.size() * 4); wr("bd.f32", L.bd.data(), L.bd.size() * 4); wr("y.f64", L.y64.data(), L.y64.size() * 8);
            FILE* f = fopen((d + "/meta.txt").c_str(), "w");
            fprintf(f, "B=%d\nH=%d\nW=%d\nCin=%d\nCmid=%d\nk=%d\ns=%d\nHo=%d\nWo=%d\npt=%d\npl=%d\nact_e=%s\nact_d=%s\nstem=%d\nHin=%d\nWin=%d\npts=%d\npls=%d\ncopy=%d\n", L.B,
                    L.g.H, L.g.W, L.c.Cin, L.c.Cmid, L.g.k, L.g.s, L.Ho, L.Wo, L.pt, L.pl, act_name(L.c.act_e), act_name(L.c.act_d), (int)L.g.stem, L.g.Hin,
                    L.g.Win, L.pts, L.pls, (int)(L.c.mode == M_COPY));
            fclose(f);
            printf("dumped %s\n", L.name.c_str());
            return 0;
        }
        printf("no such layer: %s\n", dump_layer);
        return 2;
    }

    std::map<std::pair<int, std::string>, Stat> pairs;     // (shape index, form) -> cases, worst figures
    std::map<std::string, Stat> forms;                     // dispatcher branch -> the same (the DESIGN.md table)
    hipStream_t st = nullptr;
    if (!list) HIPCHK(hipStreamCreate(&st), "hipStreamCreate");
    int failures = 0, ran = 0;
    size_t ci = 0;
    for (int li = 0; li < (int)layers.size(); li++) {
        Layer& L = layers[li];
        size_t ce = ci;
        while (ce < cases.size() && cases[ce].layer == li) ce++;
        const size_t c0 = ci; ci = ce;
        const bool sel = !only || L.name.find(only) != std::string::npos;
        const Cfg& c = L.c; const Geo& g = L.g;
        if (list) {
            const bool r6 = c.act_e == ACT_RELU6 || c.act_d == ACT_RELU6;
            if (r6) gen(L, false);
            printf("LAYER %s k=%d s=%d H=%d W=%d Ho=%d Wo=%d pt=%d pl=%d Cin=%d Cmid=%d act_e=%s act_d=%s B=%d clip_e=%.4f clip_d=%.4f\n", L.name.c_str(), g.k, g.s, g.H, g.W,
                   L.Ho, L.Wo, L.pt, L.pl, c.Cin, c.Cmid, act_name(c.act_e), act_name(c.act_d), L.B, L.clip_e, L.clip_d);
            L.x = {}; L.we = {}; L.y64 = {}; L.bxabs = {};
        }
        if (list || !sel) {
            for (size_t q = c0; q < ce; q++) {
                if (list) {
                    std::string fl; for (auto& f : cases[q].forms) fl += (fl.empty() ? "" : ",") + f;
                    printf("CASE %zu %s shape=%d sums=%d forms=%s\n", q, L.name.c_str(), cases[q].shape, (int)cases[q].sums, fl.c_str());
                    for (auto& f : cases[q].forms) pairs[{cases[q].shape, f}].cases++;
                }
            }
            continue;
        }
        if (c0 == ce) continue;
        gen(L, true);
        const int B = L.B, Cm = c.Cmid, Ho = L.Ho, Wo = L.Wo, k = g.k;
        const size_t nout = L.y64.size();
        double scale = 0, eh = 0, bxmax = 0;
        for (size_t i = 0; i < nout; i++) { scale = std::max(scale, std::fabs(L.y64[i])); bxmax = std::max(bxmax, L.bxabs[i]); }
        for (size_t i = 0; i < nout; i++) eh = std::max(eh, std::fabs((double)L.y32[i] - L.y64[i]));
        eh /= scale;
        double gate = 4.0 * eh + std::ldexp(1.0, -22);
        if (c.mode == M_BX) gate += std::ldexp(1.0, -23) * bxmax / scale;
        // ---- device images
        const bool copy = c.mode == M_COPY, stem = c.mode == M_STEM;
        const bool xbf = c.mode == M_P1X || (copy && c.copy_xbf16);
        float* dx = nullptr; uint16_t* dxh = nullptr;
        if (xbf) { std::vector<uint16_t> xh(L.x.size()); for (size_t i = 0; i < xh.size(); i++) xh[i] = bf16_rne(L.x[i]); dxh = dev_guarded(xh, true); }
        else dx = dev_guarded(L.x, true);
        const int Cp = expdw_cp(Cm), Kw = stem ? 24 : expdw_kw(c.Cin);
        float *dwe = nullptr, *dbe = nullptr, *dwd = nullptr, *dbd = nullptr; uint16_t* dimg = nullptr;
        if (copy) { dwd = dev_guarded(L.wd, true); if (c.copy_bias) dbd = dev_guarded(L.bd, true); }
        else {
            std::vector<float> wep((size_t)Cp * Kw, 0.f), bep(Cp, 0.f), wdp((size_t)k * k * Cp, 0.f), bdp(Cp, 0.f);
            for (int n = 0; n < Cm; n++) {
                if (stem) {                                // column = window row * 8 + window column * 2 + channel (the MFMA stem image, first 24 columns)
                    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) for (int ic = 0; ic < 2; ic++)
                        wep[(size_t)n * 24 + i * 8 + j * 2 + ic] = L.we[(size_t)n * 18 + (i * 3 + j) * 2 + ic];
                } else memcpy(&wep[(size_t)n * Kw], &L.we[(size_t)n * c.Cin], (size_t)c.Cin * 4);
            }
            memcpy(bep.data(), L.be.data(), (size_t)Cm * 4); memcpy(bdp.data(), L.bd.data(), (size_t)Cm * 4);
            for (int t = 0; t < k * k; t++) memcpy(&wdp[(size_t)t * Cp], &L.wd[(size_t)t * Cm], (size_t)Cm * 4);
            dwe = dev_guarded(wep, true); dbe = dev_guarded(bep, true); dwd = dev_guarded(wdp, true); dbd = dev_guarded(bdp, true);
            if (c.mode != M_F32 && !stem) dimg = dev_guarded(expdw_bx_image(L.we.data(), Cm, c.Cin), true);
        }
        const size_t ybytes = nout * (c.out_bf16 ? 2 : 4), yall = kGuard * 8 + (ybytes + 3) / 4 * 4;
        const ExpDwGeo eg = geo_of(L, layer_pipe16(L));
        int max_slabs = 0;
        for (size_t q = c0; q < ce; q++) max_slabs = std::max(max_slabs, expdw_shape_slabs(cases[q].shape, eg));
        const size_t pall = kGuard * 2 + (size_t)B * max_slabs * Cm;
        char* dy; float* dp;
        HIPCHK(hipMalloc(&dy, yall), "hipMalloc"); HIPCHK(hipMalloc(&dp, pall * 4), "hipMalloc");
        std::vector<unsigned> hy(yall / 4), hp(pall);
        for (size_t q = c0; q < ce; q++) {
            const Case& cs = cases[q];
            std::string fl; for (auto& f : cs.forms) fl += (fl.empty() ? "" : ",") + f;
            cur_case = "case " + std::to_string(q) + " " + L.name + " shape=" + std::to_string(cs.shape) + " sums=" + std::to_string((int)cs.sums) + " forms=" + fl;
            printf("RUN %s\n", cur_case.c_str()); fflush(stdout);
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)dy, (int)kPat, yall / 4, st), "fill y");
            HIPCHK(hipMemsetD32Async((hipDeviceptr_t)dp, (int)kPat, pall, st), "fill sums");
            float* y = reinterpret_cast<float*>(dy + kGuard * 4);
            float* part = cs.sums ? dp + kGuard : nullptr;
            const int tiles = expdw_shape_slabs(cs.shape, eg);
            if (copy) {
                DwParams p{xbf ? reinterpret_cast<const float*>(dxh) : dx, dwd, dbd, y, B, g.H, g.W, Cm, Ho, Wo, k, k, g.s, g.s, L.pt, L.pl, c.act_d};
                p.in_bf16 = xbf; p.out_bf16 = c.out_bf16;
                if (!dwconv_lds_supported(p)) { printf("FAIL %s: dwconv_lds_supported is false\n", cur_case.c_str()); failures++; continue; }
                launch_dwconv_lds(p, part, cs.shape, st);
            } else {
                StemGeom sg{g.Hin, g.Win, L.pts, L.pls};
                const int prec = (c.mode == M_P1 || c.mode == M_P1X) ? 1 : 0;
                launch_expand_dw(xbf ? reinterpret_cast<const float*>(dxh) : dx, dwe, dbe, dwd, dbd, y, part, B, g.H, g.W, c.Cin, Cm, Ho, Wo, k, g.s, L.pt, L.pl, c.act_e,
                                 c.act_d, cs.shape, stem ? &sg : nullptr, st, dimg, prec, c.out_bf16, c.mode == M_P1X ? 1 : 0);
            }
            HIPCHK(hipGetLastError(), "launch");
            HIPCHK(hipStreamSynchronize(st), "synchronize");
            HIPCHK(hipMemcpy(hy.data(), dy, yall, hipMemcpyDeviceToHost), "copy y");
            HIPCHK(hipMemcpy(hp.data(), dp, pall * 4, hipMemcpyDeviceToHost), "copy sums");
            ran++;
            bool ok = true;
            std::string why;
            // 3. guards
            size_t gbad = 0;
            for (size_t i = 0; i < kGuard; i++) gbad += hy[i] != kPat;
            {
                const unsigned char* yb = reinterpret_cast<const unsigned char*>(hy.data()) + kGuard * 4 + ybytes;
                const unsigned char pb[4] = {0x5a, 0xde, 0xc0, 0xff};
                for (size_t i = 0; i < yall - kGuard * 4 - ybytes; i++) gbad += yb[i] != pb[(ybytes + i) & 3];
            }
            const size_t pn = cs.sums ? (size_t)B * tiles * Cm : 0;
            for (size_t i = 0; i < pall; i++) if (i < kGuard || i >= kGuard + pn) gbad += hp[i] != kPat;
            if (gbad) { ok = false; why += " guard:" + std::to_string(gbad) + "_words_overwritten"; }
            // 1. every element of y
            double ek = 0, ratio = 0; size_t worst = 0;
            const float* yf = reinterpret_cast<const float*>(hy.data() + kGuard);
            const uint16_t* yh = reinterpret_cast<const uint16_t*>(hy.data() + kGuard);
            for (size_t i = 0; i < nout; i++) {
                double got, ref = L.y64[i], allow = gate * scale;
                if (c.out_bf16) {
                    got = bf16_widen(yh[i]);
                    const float rr = bf16_round((float)ref); int ex; (void)std::frexp(rr == 0.f ? std::ldexp(1.0, -126) : (double)rr, &ex);
                    ref = rr; allow += std::ldexp(1.0, ex - 8);          // one ulp of a bf16 value with exponent ex - 1
                } else got = yf[i];
                double d = std::fabs(got - ref);
                if (!(d == d) || std::isinf(d)) d = 1e30;
                if (d / scale > ek) ek = d / scale;
                if (d / allow > ratio) { ratio = d / allow; worst = i; }
            }
            if (ratio > 1.0) {
                ok = false;
                const size_t px = worst / Cm;
                char buf[200]; snprintf(buf, sizeof buf, " y:ratio=%.3g_at_b%zu_oh%zu_ow%zu_c%zu", ratio, px / ((size_t)Ho * Wo), px / Wo % Ho, px % Wo, worst % Cm);
                why += buf;
            }
            // 2. the sums: per slab in the kernel's tile order, and the totals per (clip, channel)
            double es = 0, et = 0, rs = 0, rt = 0;
            if (cs.sums) {
                const TileShape& t = kTiles[cs.shape % kNT];
                const bool tr = cs.shape >= kNT;
                const int oHo = tr ? Wo : Ho, oWo = tr ? Ho : Wo, tw = (oWo + t.tow - 1) / t.tow;
                std::vector<double> ref((size_t)B * tiles * Cm, 0.0), tot((size_t)B * Cm, 0.0), gtot((size_t)B * Cm, 0.0);
                std::vector<int> npx(tiles, 0);
                for (int b = 0; b < B; b++)
                    for (int r = 0; r < oHo; r++)
                        for (int q2 = 0; q2 < oWo; q2++) {
                            const int tile = (r / t.toh) * tw + q2 / t.tow, oh = tr ? q2 : r, ow = tr ? r : q2;
                            if (b == 0) npx[tile]++;
                            for (int n = 0; n < Cm; n++) ref[((size_t)b * tiles + tile) * Cm + n] += L.y64[(((size_t)b * Ho + oh) * Wo + ow) * Cm + n];
                        }
                double ss = 0, ts = 0;
                const float* pf = reinterpret_cast<const float*>(hp.data() + kGuard);
                for (size_t i = 0; i < ref.size(); i++) {
                    ss = std::max(ss, std::fabs(ref[i]));
                    tot[i / ((size_t)tiles * Cm) * Cm + i % Cm] += ref[i]; gtot[i / ((size_t)tiles * Cm) * Cm + i % Cm] += (double)pf[i];
                }
                for (double v : tot) ts = std::max(ts, std::fabs(v));
                // Allowed per slab: n (gate + 2^-24) scale, n = pixels summed.  The first term is the y gate on each of the n terms.  The
                // second is NOT the whole gamma_n bound of an fp32 sum (gamma_n sum|terms| <= n^2 2^-24 scale): it is one rounding per
                // term at the scale of y - what a pairwise / random-walk accumulation leaves - and so stricter than the derived bound.
                // Stated in units of the y scale; the printed figures are in units of the sums' own scale.
                const double gy = gate + std::ldexp(1.0, -24);
                for (size_t i = 0; i < ref.size(); i++) {
                    double d = std::fabs((double)pf[i] - ref[i]); if (!(d == d)) d = 1e30;
                    const double allow = npx[i / Cm % tiles] * gy * scale;
                    es = std::max(es, d / ss); rs = std::max(rs, d / allow);
                }
                for (size_t i = 0; i < tot.size(); i++) {
                    double d = std::fabs(gtot[i] - tot[i]); if (!(d == d)) d = 1e30;
                    et = std::max(et, d / ts); rt = std::max(rt, d / ((double)Ho * Wo * gy * scale));
                }
                char buf[120];
                if (rs > 1.0) { ok = false; snprintf(buf, sizeof buf, " slab_sums:ratio=%.3g", rs); why += buf; }
                if (rt > 1.0) { ok = false; snprintf(buf, sizeof buf, " total_sums:ratio=%.3g", rt); why += buf; }
            }
            printf("%s %s err=%.3e host32=%.3e gate=%.3e ratio=%.3f sums: slab=%.3e total=%.3e%s\n", ok ? "ok  " : "FAIL", cur_case.c_str(), ek, eh, gate, ratio, es, et, why.c_str());
            if (!ok) failures++;
            const double rr = std::max(ratio, std::max(rs, rt));
            for (auto& f : cs.forms) { Stat& s = pairs[{cs.shape, f}]; s.cases++; s.ratio = std::max(s.ratio, rr); s.ek = std::max(s.ek, ek); s.eh = std::max(s.eh, eh); }
            {   // (bf16 storage apart: its error is the rounding of y, not the kernel's arithmetic)
                Stat& s = forms[cs.forms[0] + (c.out_bf16 ? ",out_bf16" : "")];
                s.cases++; s.ratio = std::max(s.ratio, ratio); s.ek = std::max(s.ek, ek); s.eh = std::max(s.eh, eh);
            }
        }
        (void)hipFree(dy); (void)hipFree(dp);
        dev_free_guarded(dx); dev_free_guarded(dxh); dev_free_guarded(dwe); dev_free_guarded(dbe); dev_free_guarded(dwd); dev_free_guarded(dbd); dev_free_guarded(dimg);
        L.x = {}; L.we = {}; L.y64 = {}; L.y32 = {}; L.bxabs = {};
    }
    for (auto& kv : pairs) printf("PAIR %d %s cases=%d worst_ratio=%.3f err=%.3e host32=%.3e\n", kv.first.first, kv.first.second.c_str(), kv.second.cases, kv.second.ratio, kv.second.ek, kv.second.eh);
    for (auto& kv : forms) printf("FORM %s cases=%d worst_err=%.3e worst_host32=%.3e worst_ratio=%.3f\n", kv.first.c_str(), kv.second.cases, kv.second.ek, kv.second.eh, kv.second.ratio);
    printf("SUMMARY {\"layers\": %zu, \"cases\": %zu, \"ran\": %d, \"failures\": %d, \"pairs\": %zu, \"cus\": %d}\n", layers.size(), cases.size(), ran, failures, pairs.size(), cus);
    return failures ? 1 : 0;
}
