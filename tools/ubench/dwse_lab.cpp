// Plain depthwise, pooling and squeeze-excite lab: every kernel of csrc/dwconv.hip - k_dwconv_t<K,S,TH,TW,IN16>, k_dwconv<4>, k_dwconv<1>,
// k_mean_partial, k_mean_finish, k_se - through the library's own launchers (launch_dwconv, launch_mean_partial / launch_mean_finish,
// launch_se) on synthetic layers, without a model.  Every output element, every slab sum in the kernel's own slab order and the totals
// per (clip, channel) are held to a plain fp64 loop nest on the host; a plain sequential fp32 evaluation of the same case next to it
// sizes the tolerance (gates: below, and DESIGN.md).  Output buffers are sized exactly and lie between guard words that must stay
// intact; inputs and parameters are sized exactly and lie between NaNs.  The case list is fixed (seeded by the case names).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I birdnet-go_amd/csrc -o dwse_lab tools/ubench/dwse_lab.cpp \
//         -L birdnet-go_amd/lib -lbnhip -Wl,-rpath,birdnet-go_amd/lib
//   dwse_lab                     run every case on the current device; exit status 1 on any failed check, 3 on a HIP error.
//                                With BNHIP_DW_PREFETCH=0 in the environment (the switch is read once per process): only the
//                                bf16-input cases of k_dwconv_t, which then load row by row
//   dwse_lab --list              print the cases with their restated geometry; touches no device
//   dwse_lab --ref-dump NAME DIR write the inputs, parameters and fp64 result of one case as raw arrays (no device)
//   dwse_lab --only SUBSTR       run the cases whose name contains SUBSTR
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
static std::mt19937 rng_of(const std::string& name) {      // FNV-1a of the case's name: the same data on every run and machine
    unsigned seed = 2166136261u;
    for (char ch : name) seed = (seed ^ (unsigned char)ch) * 16777619u;
    return std::mt19937(seed);
}

// ------------------------------------------------------------------------------------------ depthwise cases
struct DwCase {
    const char* name; int kh, kw, sh, sw, H, W, C, B; int valid, in16, out16, act, bias, part;
};
static const int N = ACT_NONE, R6 = ACT_RELU6, SW = ACT_SWISH;
static const DwCase kDw[] = {
    // ---- k_dwconv_t: the four (K, S) forms x the four storages, on ragged odd / even sizes, three clips, sums given
    {"t_k3s1_ff", 3, 3, 1, 1, 13, 19, 20, 3, 0, 0, 0, SW, 1, 1},  {"t_k3s1_bf", 3, 3, 1, 1, 13, 19, 20, 3, 0, 1, 0, R6, 1, 1},
    {"t_k3s1_fb", 3, 3, 1, 1, 13, 19, 20, 3, 0, 0, 1, N, 1, 1},   {"t_k3s1_bb", 3, 3, 1, 1, 13, 19, 20, 3, 0, 1, 1, SW, 1, 1},
    {"t_k3s2_ff", 3, 3, 2, 2, 13, 18, 20, 3, 0, 0, 0, R6, 1, 1},  {"t_k3s2_bf", 3, 3, 2, 2, 13, 18, 20, 3, 0, 1, 0, SW, 1, 1},
    {"t_k3s2_fb", 3, 3, 2, 2, 13, 18, 20, 3, 0, 0, 1, SW, 1, 1},  {"t_k3s2_bb", 3, 3, 2, 2, 13, 18, 20, 3, 0, 1, 1, N, 1, 1},
    {"t_k5s1_ff", 5, 5, 1, 1, 11, 17, 20, 3, 0, 0, 0, N, 1, 1},   {"t_k5s1_bf", 5, 5, 1, 1, 11, 17, 20, 3, 0, 1, 0, SW, 1, 1},
    {"t_k5s1_fb", 5, 5, 1, 1, 11, 17, 20, 3, 0, 0, 1, R6, 1, 1},  {"t_k5s1_bb", 5, 5, 1, 1, 11, 17, 20, 3, 0, 1, 1, SW, 1, 1},
    {"t_k5s2_ff", 5, 5, 2, 2, 14, 15, 20, 3, 0, 0, 0, SW, 1, 1},  {"t_k5s2_bf", 5, 5, 2, 2, 14, 15, 20, 3, 0, 1, 0, N, 1, 1},
    {"t_k5s2_fb", 5, 5, 2, 2, 14, 15, 20, 3, 0, 0, 1, SW, 1, 1},  {"t_k5s2_bb", 5, 5, 2, 2, 14, 15, 20, 3, 0, 1, 1, R6, 1, 1},
    // ---- images smaller than one tile, a kernel larger than the image
    {"t_1x1_c4", 3, 3, 1, 1, 1, 1, 4, 1, 0, 0, 0, N, 1, 1},             // one block of 64 threads, one live; nblk = 1
    {"t_1x3_c12_s2", 3, 3, 2, 2, 1, 3, 12, 1, 0, 0, 0, SW, 1, 1},
    {"t_1x3_k5_bf", 5, 5, 1, 1, 1, 3, 4, 3, 0, 1, 0, N, 0, 1},
    {"t_1x5_c4_2live", 3, 3, 1, 1, 1, 5, 4, 1, 0, 0, 0, SW, 1, 1},      // two tiles, CX = 1: a block floored to 64 threads with 2 live
    {"t_h2k5", 5, 5, 1, 1, 2, 7, 20, 3, 0, 0, 0, N, 1, 1},
    {"t_h2k5_s2_bb", 5, 5, 2, 2, 2, 2, 4, 1, 0, 1, 1, N, 1, 1},
    // ---- stride 2 on even sizes (pads bottom and right only) and on odd sizes
    {"t_k3s2_even", 3, 3, 2, 2, 12, 16, 64, 1, 0, 0, 0, R6, 1, 1},
    {"t_k5s2_even_bf", 5, 5, 2, 2, 16, 12, 64, 3, 0, 1, 0, SW, 1, 1},
    {"t_k3s2_odd_bf", 3, 3, 2, 2, 15, 9, 12, 1, 0, 1, 0, R6, 1, 1},
    {"t_k5s2_odd", 5, 5, 2, 2, 15, 13, 64, 1, 0, 0, 0, N, 0, 0},
    // ---- VALID padding
    {"t_k3s1_valid", 3, 3, 1, 1, 9, 12, 20, 3, 1, 0, 0, SW, 1, 1},
    {"t_k3s2_valid_bf", 3, 3, 2, 2, 12, 11, 12, 1, 1, 1, 0, N, 1, 1},
    {"t_k5s1_valid", 5, 5, 1, 1, 9, 14, 64, 1, 1, 0, 0, R6, 1, 0},
    {"t_k5s2_valid_bb", 5, 5, 2, 2, 13, 16, 12, 3, 1, 1, 1, SW, 0, 1},
    // ---- block geometry: C = 12 -> blocks of 255 threads (CX = 3, PY = 85), 200 tiles = 85 + 85 + 30
    {"t_c12_255thr", 3, 3, 1, 1, 40, 40, 12, 1, 0, 0, 0, SW, 1, 1},
    {"t_c12_255thr_bb", 5, 5, 1, 1, 40, 39, 12, 3, 0, 1, 1, N, 1, 1},
    // C = 64 (CX = 16, PY = 16): 200 tiles = 12 full chunks + 8 -> nblk = 13
    {"t_c64_nblk13", 3, 3, 1, 1, 40, 40, 64, 1, 0, 0, 0, N, 1, 1},
    {"t_c64_nblk13_bf", 3, 3, 1, 1, 40, 40, 64, 1, 0, 1, 0, SW, 0, 1},
    // C = 256 (CX = 64, PY = 4): 20 tiles -> nblk = 5; 2 tiles < PY; 15 tiles = 3 PY + 3
    {"t_c256_nblk5", 3, 3, 1, 1, 10, 14, 256, 1, 0, 0, 0, SW, 1, 1},
    {"t_c256_tiny", 3, 3, 1, 1, 3, 3, 256, 3, 0, 0, 0, N, 1, 1},
    {"t_c256_ragged_bf", 5, 5, 2, 2, 5, 19, 256, 1, 0, 1, 0, SW, 1, 1},
    // C = 260: a second channel chunk with one live quad; nblk = 8 and nblk = 18
    {"t_c260_nblk8", 3, 3, 2, 2, 15, 14, 260, 1, 0, 0, 0, SW, 1, 1},
    {"t_c260_bb", 5, 5, 1, 1, 6, 9, 260, 3, 0, 1, 1, R6, 1, 1},
    {"t_c260_bf_nopart", 3, 3, 1, 1, 5, 6, 260, 1, 0, 1, 0, N, 0, 0},
    // ---- k_dwconv<4> / k_dwconv<1>: kh != kw, sh != sw, C % 4 != 0, kernels without a tiled form
    {"g_3x1_c8", 3, 1, 1, 1, 9, 11, 8, 3, 0, 0, 0, ACT_RELU, 1, 0},
    {"g_1x5_s12_c6", 1, 5, 1, 2, 9, 11, 6, 1, 0, 0, 0, R6, 1, 0},
    {"g_2x2_s21_c8", 2, 2, 2, 1, 10, 7, 8, 1, 0, 0, 0, SW, 1, 0},
    {"g_7x7_s33_c1", 7, 7, 3, 3, 17, 20, 1, 3, 0, 0, 0, ACT_SIGMOID, 1, 0},
    {"g_3x3_s12_c8", 3, 3, 1, 2, 8, 9, 8, 1, 0, 0, 0, ACT_HARD_SWISH, 1, 0},
    {"g_3x3_c6_nobias", 3, 3, 1, 1, 9, 11, 6, 3, 0, 0, 0, N, 0, 0},
    {"g_7x7_c8_valid", 7, 7, 1, 1, 9, 12, 8, 1, 1, 0, 0, R6, 1, 0},
    {"g_2x2_s33_c1_nobias", 2, 2, 3, 3, 11, 13, 1, 1, 0, 0, 0, SW, 0, 0},
    {"g_5x5_s11_c6", 5, 5, 1, 1, 7, 40, 6, 1, 0, 0, 0, ACT_RELU, 1, 0},       // 1680 threads: more than one block, a ragged last one
};
static const int kNDw = (int)(sizeof(kDw) / sizeof(kDw[0]));

struct DwGeo { int Ho, Wo, pt, pl; bool tiled; int TH, TW, CX, PY, tiles_w, tiles, tchunks, cchunks, nblk, block, live; };
static DwGeo dw_geo(const DwCase& c) {
    DwGeo g{};
    if (c.valid) { g.Ho = (c.H - c.kh) / c.sh + 1; g.Wo = (c.W - c.kw) / c.sw + 1; }
    else {   // SAME, TensorFlow's rule: the smaller half of the padding in front
        g.Ho = (c.H + c.sh - 1) / c.sh; g.Wo = (c.W + c.sw - 1) / c.sw;
        g.pt = std::max((g.Ho - 1) * c.sh + c.kh - c.H, 0) / 2; g.pl = std::max((g.Wo - 1) * c.sw + c.kw - c.W, 0) / 2;
    }
    // the register-tiled kernel's geometry, restated (dw_tiled_shape / dw_geometry of dwconv.hip are private; checked against
    // dwconv_sum_slabs and dwconv_tile_geometry on every case)
    g.tiled = c.C % 4 == 0 && c.kh == c.kw && c.sh == c.sw && (c.kh == 3 || c.kh == 5) && (c.sh == 1 || c.sh == 2);
    if (g.tiled) {
        g.TH = (c.kh == 5 && c.sh == 2) ? 1 : 2; g.TW = c.sh == 1 ? 4 : 2;
        const int C4 = c.C / 4;
        g.CX = std::min(C4, 64); g.PY = 256 / g.CX;
        g.tiles_w = (g.Wo + g.TW - 1) / g.TW; g.tiles = g.tiles_w * ((g.Ho + g.TH - 1) / g.TH);
        g.PY = std::min(g.PY, g.tiles);
        g.tchunks = (g.tiles + g.PY - 1) / g.PY; g.cchunks = (C4 + g.CX - 1) / g.CX;
        g.nblk = c.B * g.tchunks * g.cchunks; g.block = std::max(64, g.CX * g.PY);
        g.live = std::min(C4 - (g.cchunks - 1) * g.CX, g.CX) * (g.tiles - (g.tchunks - 1) * g.PY);   // live threads of the last block
    }
    return g;
}
struct DwData { std::vector<float> x, w, b; std::vector<double> y64; std::vector<float> y32; double clip = -1; };
static void dw_gen(const DwCase& c, const DwGeo& g, DwData& d, bool want32) {
    std::mt19937 rng = rng_of(c.name);
    std::normal_distribution<float> nd(0.f, 1.f);
    d.x.resize((size_t)c.B * c.H * c.W * c.C);
    for (auto& v : d.x) v = nd(rng);
    if (c.in16) for (auto& v : d.x) v = bf16_round(v);      // the reference is evaluated on the bf16 values
    d.w.resize((size_t)c.kh * c.kw * c.C);
    // ReLU6: pre-activations of about N(1.5, 3) in the interior, so that both clips bite on a visible share
    const float gain = (c.act == ACT_RELU6 ? 3.f : 1.f) / std::sqrt((float)(c.kh * c.kw));
    for (auto& v : d.w) v = nd(rng) * gain;
    d.b.assign(c.C, 0.f);
    if (c.bias) for (auto& v : d.b) v = 0.1f * nd(rng) + (c.act == ACT_RELU6 ? 1.5f : 0.f);
    const size_t nout = (size_t)c.B * g.Ho * g.Wo * c.C;
    d.y64.resize(nout); if (want32) d.y32.resize(nout);
    size_t clipped = 0;
    for (int b = 0; b < c.B; b++)
        for (int oh = 0; oh < g.Ho; oh++)
            for (int ow = 0; ow < g.Wo; ow++)
                for (int n = 0; n < c.C; n++) {
                    double acc = 0; float a32 = 0.f;
                    for (int i = 0; i < c.kh; i++)
                        for (int j = 0; j < c.kw; j++) {
                            const int h = oh * c.sh - g.pt + i, w = ow * c.sw - g.pl + j;
                            if (h < 0 || h >= c.H || w < 0 || w >= c.W) continue;
                            const float xv = d.x[(((size_t)b * c.H + h) * c.W + w) * c.C + n], t = d.w[(size_t)(i * c.kw + j) * c.C + n];
                            acc += (double)xv * (double)t;
                            a32 += xv * t;
                        }
                    acc += d.b[n];
                    if (c.act == ACT_RELU6 && (acc < 0 || acc > 6)) clipped++;
                    const size_t o = (((size_t)b * g.Ho + oh) * g.Wo + ow) * c.C + n;
                    d.y64[o] = act64(acc, c.act);
                    if (want32) d.y32[o] = act32(a32 + d.b[n], c.act);
                }
    if (c.act == ACT_RELU6) d.clip = (double)clipped / (double)nout;
}
static std::string dw_form(const DwCase& c, const DwGeo& g, bool pre16) {
    if (!g.tiled) return c.C % 4 == 0 ? "k_dwconv<4>" : "k_dwconv<1>";
    std::string f = "k_dwconv_t<" + std::to_string(c.kh) + "," + std::to_string(c.sh) + ">";
    f += c.in16 ? (pre16 ? " bf16-prefetched" : " bf16-rowwise") : " f32";
    f += c.out16 ? "->bf16" : "->f32";
    return f;
}

// ------------------------------------------------------------------------------------------ mean cases
struct MeanCase { const char* name; int HW, C, B; };
static const MeanCase kMean[] = {
    {"m_hw1_c1", 1, 1, 1},       {"m_hw1_c64", 1, 64, 3},      {"m_hw511_c3", 511, 3, 3},   {"m_hw512_c63", 512, 63, 1},
    {"m_hw513_c64", 513, 64, 3}, {"m_hw513_c130", 513, 130, 1}, {"m_hw1500_c65", 1500, 65, 1}, {"m_hw1500_c130", 1500, 130, 3},
};
static const int kNMean = (int)(sizeof(kMean) / sizeof(kMean[0]));
static const int kMeanSlab = 512;                        // MEAN_SLAB of dwconv.hip, restated (checked against mean_splits)

// ------------------------------------------------------------------------------------------ squeeze-excite cases
// probe: FC1 and FC2 are identity matrices without bias or activation (Cr = C), so the scale IS the kernel's mean stage, bit for bit
// (fmaf(1, m, 0) and sums with zeros are exact): the only way to hold that stage to its own gate from outside the kernel.
struct SeCase { const char* name; int threads, C, Cr, S, act1, act2, b1, b2, B, probe; };
static const int RL = ACT_RELU, SG = ACT_SIGMOID;
static const SeCase kSe[] = {
    {"se_c4_cr1_s1", 0, 4, 1, 1, SW, SG, 1, 1, 1, 0},                // P = 1 (S = 1), G = 1
    {"se_c6_cr3_s2_scalar", 64, 6, 3, 2, SW, N, 1, 1, 3, 0},           // scalar path, P = 2
    {"se_c24_cr4_s3", 256, 24, 4, 3, RL, SG, 0, 0, 1, 0},              // P = 2 with S = 3, G = 4
    {"se_c96_cr17_s96", 1024, 96, 17, 96, SW, SG, 1, 1, 3, 0},         // P = 8, G = 16, FC1 rows clamped at 16
    {"se_c1152_cr48_s130", 256, 1152, 48, 130, SW, SG, 1, 1, 1, 0},    // the block doubles to 512; P = 1 with S > 1, G = 1
    {"se_c2048_cr48_s2", 64, 2048, 48, 2, RL, SG, 1, 0, 3, 0},         // the block doubles three times
    {"se_c4096_cr17_s3", 0, 4096, 17, 3, SW, SG, 1, 1, 1, 0},          // C / 4 = threads exactly
    {"se_c4098_cr4_s2_scalar", 1024, 4098, 4, 2, RL, N, 1, 1, 1, 0},   // scalar path beyond 4096 channels
    {"se_c4100_cr3_s1", 256, 4100, 3, 1, SW, SG, 1, 1, 3, 0},          // C / 4 = 1025 > 1024 threads: FC2 loops the quad index
    {"se_c24_cr48_s96_w1", 64, 24, 48, 96, SW, SG, 1, 1, 1, 0},        // one wave: FC1 takes rows j0 .. j0 + 3; P = 2, G = 8
    {"se_c96_cr3_s130", 256, 96, 3, 130, RL, N, 0, 1, 3, 0},           // P = 2 by the thread count, G = 1 by Cr
    {"se_probe_c24_s1", 0, 24, 24, 1, N, N, 0, 0, 1, 1},
    {"se_probe_c24_s3", 1024, 24, 24, 3, N, N, 0, 0, 3, 1},            // P = 2, S = 3
    {"se_probe_c96_s130", 64, 96, 96, 130, N, N, 0, 0, 1, 1},          // P = 1: 130 serial additions
    {"se_probe_c6_s96_scalar", 1024, 6, 6, 96, N, N, 0, 0, 3, 1},      // P = 64: interleaved subsets of 2 and 1 slabs, a 64-way fold
};
static const int kNSe = (int)(sizeof(kSe) / sizeof(kSe[0]));
struct SeGeo { int thr, P, G, v4, doubled; size_t lds; };
static SeGeo se_geo(const SeCase& c) {                   // launch_se and k_se, restated (BNHIP_SE_THREADS unset)
    SeGeo g{};
    int thr = c.threads ? c.threads : 1024;
    thr = std::max(64, std::min(1024, thr / 64 * 64));
    const int thr0 = thr;
    while (thr < 1024 && (c.C + 3) / 4 > thr) thr *= 2;
    g.thr = thr; g.doubled = thr != thr0;
    g.P = 1; while (g.P * 2 * c.C <= thr && g.P * 2 <= c.S) g.P *= 2;
    g.v4 = c.C % 4 == 0;
    g.G = 1;
    if (g.v4) while (g.G * 2 * (c.C / 4) <= thr && g.G * 2 <= c.Cr) g.G *= 2;
    g.lds = (size_t)(c.C + c.Cr + 4 * thr + 16) * 4;
    return g;
}
struct SeData { std::vector<float> part, w1, b1, w2t, b2; std::vector<double> s64, mean64, sabs; std::vector<float> s32; int HW; double live = -1; /* share of FC1 outputs a ReLU lets through */ };
static void se_gen(const SeCase& c, SeData& d) {
    std::mt19937 rng = rng_of(c.name);
    std::normal_distribution<float> nd(0.f, 1.f);
    d.HW = c.S * 32;                                      // (HW / S a power of two: the oracle graph of the test feeds partial / 32 to a MEAN over S, exactly)
    d.part.resize((size_t)c.B * c.S * c.C);
    for (auto& v : d.part) v = (0.5f + nd(rng)) * (float)d.HW / (float)c.S;
    d.w1.assign((size_t)c.Cr * c.C, 0.f); d.w2t.assign((size_t)c.Cr * c.C, 0.f);
    d.b1.assign(c.Cr, 0.f); d.b2.assign(c.C, 0.f);
    if (c.probe) { for (int i = 0; i < c.C; i++) d.w1[(size_t)i * c.C + i] = d.w2t[(size_t)i * c.C + i] = 1.f; }
    else {
        // (the means are about 0.5: the offset puts FC1's outputs at about 0.25 +- 0.5, so that a ReLU passes some and stops some)
        for (auto& v : d.w1) v = nd(rng) / std::sqrt((float)c.C) + 0.5f / (float)c.C;
        for (auto& v : d.w2t) v = nd(rng) / std::sqrt((float)c.Cr);
        if (c.b1) for (auto& v : d.b1) v = 0.1f * nd(rng);
        if (c.b2) for (auto& v : d.b2) v = 0.1f * nd(rng);
    }
    if (c.act1 == ACT_RELU)                               // a ReLU must not stop every row (four rows do that once in 16 draws): the even rows pass on clip 0
        for (int j = 0; j < c.Cr; j += 2) {
            double a = d.b1[j];
            for (int ch = 0; ch < c.C; ch++) {
                double m0 = 0;
                for (int s = 0; s < c.S; s++) m0 += d.part[(size_t)s * c.C + ch];
                a += (double)d.w1[(size_t)j * c.C + ch] * m0 / d.HW;
            }
            if (a <= 0) { for (int ch = 0; ch < c.C; ch++) d.w1[(size_t)j * c.C + ch] = -d.w1[(size_t)j * c.C + ch]; d.b1[j] = -d.b1[j]; }
        }
    d.s64.resize((size_t)c.B * c.C); d.s32.resize(d.s64.size()); d.mean64.resize(d.s64.size()); d.sabs.resize(d.s64.size());
    std::vector<double> m(c.C), r(c.Cr); std::vector<float> m32(c.C), r32(c.Cr);
    size_t nlive = 0;
    for (int b = 0; b < c.B; b++) {
        for (int ch = 0; ch < c.C; ch++) {
            double a = 0, ab = 0; float a32 = 0.f;
            for (int s = 0; s < c.S; s++) { const float v = d.part[((size_t)b * c.S + s) * c.C + ch]; a += v; ab += std::fabs((double)v); a32 += v; }
            m[ch] = a / d.HW; m32[ch] = a32 / (float)d.HW;
            d.mean64[(size_t)b * c.C + ch] = m[ch]; d.sabs[(size_t)b * c.C + ch] = ab;
        }
        for (int j = 0; j < c.Cr; j++) {
            double a = 0; float a32 = 0.f;
            for (int ch = 0; ch < c.C; ch++) { a += (double)d.w1[(size_t)j * c.C + ch] * m[ch]; a32 += d.w1[(size_t)j * c.C + ch] * m32[ch]; }
            r[j] = act64(a + d.b1[j], c.act1); r32[j] = act32(a32 + d.b1[j], c.act1);
            if (r[j] > 0) nlive++;
        }
        for (int ch = 0; ch < c.C; ch++) {
            double a = 0; float a32 = 0.f;
            for (int j = 0; j < c.Cr; j++) { a += (double)d.w2t[(size_t)j * c.C + ch] * r[j]; a32 += d.w2t[(size_t)j * c.C + ch] * r32[j]; }
            d.s64[(size_t)b * c.C + ch] = act64(a + d.b2[ch], c.act2); d.s32[(size_t)b * c.C + ch] = act32(a32 + d.b2[ch], c.act2);
        }
    }
    if (c.act1 == ACT_RELU) d.live = (double)nlive / (double)(c.B * c.Cr);
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
// an output: [pattern][exactly the bytes][pattern]; bad() counts the guard bytes that changed
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
static void note(const std::string& form, double ek, double eh, double ratio) {
    Stat& s = forms[form];
    s.cases++; s.ek = std::max(s.ek, ek); s.eh = std::max(s.eh, eh); s.ratio = std::max(s.ratio, ratio);
}
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
        else { printf("usage: dwse_lab [--list | --ref-dump NAME DIR | --only SUBSTR]\n"); return 2; }
    }
    // the load form of bf16 inputs in k_dwconv_t: launch_dwconv reads the switch once per process, so does the lab
    const bool pre16 = !(getenv("BNHIP_DW_PREFETCH") && atoi(getenv("BNHIP_DW_PREFETCH")) == 0);
    const bool device = !list && !dump;
    if (device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { printf("no HIP device\n"); return 3; }
    }
    printf("dwse_lab: %d depthwise, %d mean, %d squeeze-excite cases; bf16 inputs of k_dwconv_t load %s%s\n", kNDw, kNMean, kNSe,
           pre16 ? "prefetched" : "row by row (only those cases run)", device ? "" : " (no device touched)");
    printf("LOADFORM %s\n", pre16 ? "prefetched" : "rowwise");
    int failures = 0, ran = 0, ncases = 0;
    hipStream_t st = nullptr;
    if (device) HIPCHK(hipStreamCreate(&st), "hipStreamCreate");
    auto selected = [&](const char* name) { return !only || strstr(name, only); };

    // ---------------------------------------------------------------------------------- depthwise
    for (int ci = 0; ci < kNDw; ci++) {
        const DwCase& c = kDw[ci];
        const DwGeo g = dw_geo(c);
        DwParams p{nullptr, nullptr, nullptr, nullptr, c.B, c.H, c.W, c.C, g.Ho, g.Wo, c.kh, c.kw, c.sh, c.sw, g.pt, g.pl, c.act};
        p.in_bf16 = c.in16; p.out_bf16 = c.out16;
        // the lab's slab count against the library's, and the tile geometry the GEMM tail indexes by
        const int slabs = g.tiled ? g.tchunks : 0;
        bool geo_ok = dwconv_sum_slabs(p) == slabs && g.Ho > 0 && g.Wo > 0 && (g.tiled || (!c.in16 && !c.out16 && !c.part));
        int lPY, ltw, lt, ltc;
        const bool lg = dwconv_tile_geometry(p, &lPY, &ltw, &lt, &ltc);
        if (lg != (g.tiled && g.TH == 2 && g.TW == 4)) geo_ok = false;
        if (lg && (lPY != g.PY || ltw != g.tiles_w || lt != g.tiles || ltc != g.tchunks)) geo_ok = false;
        if (!geo_ok) { printf("FAIL %s: the restated geometry differs from the library's (slabs %d vs %d)\n", c.name, slabs, dwconv_sum_slabs(p)); failures++; continue; }
        const std::string form = dw_form(c, g, pre16);
        if (list) {
            DwData d; if (c.act == ACT_RELU6) dw_gen(c, g, d, false);
            printf("CASE %s kind=%s form=%s kh=%d kw=%d sh=%d sw=%d H=%d W=%d C=%d B=%d Ho=%d Wo=%d pt=%d pl=%d valid=%d in16=%d out16=%d act=%s bias=%d part=%d", c.name,
                   g.tiled ? "dwt" : "dwg", form.substr(0, form.find(' ')).c_str(), c.kh, c.kw, c.sh, c.sw, c.H, c.W, c.C, c.B, g.Ho, g.Wo, g.pt, g.pl, c.valid, c.in16, c.out16,
                   act_name(c.act), c.bias, c.part);
            if (g.tiled) printf(" TH=%d TW=%d CX=%d PY=%d tiles=%d tchunks=%d cchunks=%d nblk=%d block=%d live_last=%d", g.TH, g.TW, g.CX, g.PY, g.tiles, g.tchunks, g.cchunks, g.nblk, g.block, g.live);
            printf(" clip=%.4f\n", d.clip);
            ncases++;
            continue;
        }
        if (dump) {
            if (strcmp(dump, c.name)) continue;
            DwData d; dw_gen(c, g, d, false);
            wr(dump_dir, "x.f32", d.x.data(), d.x.size() * 4); wr(dump_dir, "w.f32", d.w.data(), d.w.size() * 4); wr(dump_dir, "b.f32", d.b.data(), d.b.size() * 4);
            wr(dump_dir, "y.f64", d.y64.data(), d.y64.size() * 8);
            FILE* f = fopen((std::string(dump_dir) + "/meta.txt").c_str(), "w");
            fprintf(f, "kind=dw\nB=%d\nH=%d\nW=%d\nC=%d\nkh=%d\nkw=%d\nsh=%d\nsw=%d\nHo=%d\nWo=%d\nvalid=%d\nact=%s\n", c.B, c.H, c.W, c.C, c.kh, c.kw, c.sh, c.sw, g.Ho, g.Wo, c.valid, act_name(c.act));
            fclose(f);
            printf("dumped %s\n", c.name);
            return 0;
        }
        if (!selected(c.name) || (!pre16 && !(g.tiled && c.in16))) continue;
        ncases++;
        cur_case = std::string(c.name) + " [" + form + "]";
        printf("RUN %s\n", cur_case.c_str()); fflush(stdout);
        DwData d; dw_gen(c, g, d, true);
        const size_t nout = d.y64.size();
        double scale = 0, eh = 0;
        for (size_t i = 0; i < nout; i++) scale = std::max(scale, std::fabs(d.y64[i]));
        for (size_t i = 0; i < nout; i++) eh = std::max(eh, std::fabs((double)d.y32[i] - d.y64[i]));
        eh /= scale;
        // y: err <= 4 err_f32host + 2^-22, err = max|got - ref64| / max|ref64|.  bf16 input: the reference is evaluated on the bf16
        // values and their products with fp32 taps are exact in the kernel's fmaf as in fp64's product, so the gate is the same.
        const double gate = 4.0 * eh + std::ldexp(1.0, -22);
        InBuf* dx = c.in16 ? in_bf16(d.x) : in_f32(d.x);
        InBuf* dw = in_f32(d.w);
        InBuf* db = c.bias ? in_f32(d.b) : nullptr;
        OutBuf y(nout * (c.out16 ? 2 : 4));
        OutBuf sums((size_t)c.B * slabs * c.C * 4 * (c.part ? 1 : 0));       // (no sums asked for: guards only, nothing may be written)
        y.fill(st); sums.fill(st);
        p.in = dx->f(); p.w = dw->f(); p.bias = db ? db->f() : nullptr; p.out = y.dev();
        launch_dwconv(p, c.part ? sums.dev() : nullptr, st);
        HIPCHK(hipGetLastError(), "launch");
        HIPCHK(hipStreamSynchronize(st), "synchronize");
        y.fetch(); sums.fetch();
        ran++;
        bool ok = true; std::string why;
        const size_t gbad = y.bad() + sums.bad();
        if (gbad) { ok = false; why += " guard:" + std::to_string(gbad) + "_bytes_overwritten"; }
        double ek = 0, ratio = 0; size_t worst = 0;
        for (size_t i = 0; i < nout; i++) {
            double got, ref = d.y64[i], allow = gate * scale;
            if (c.out16) {     // compare with the rounded reference, one bf16 ulp of the element on top
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
            const size_t px = worst / c.C;
            char buf[200]; snprintf(buf, sizeof buf, " y:ratio=%.3g_at_b%zu_oh%zu_ow%zu_c%zu", ratio, px / ((size_t)g.Ho * g.Wo), px / g.Wo % g.Ho, px % g.Wo, worst % c.C);
            why += buf;
        }
        // the sums, slab by slab in the kernel's order: tile (oh / TH) * tiles_w + ow / TW, slab = tile / PY; partial[b][slab][c].
        // With y stored as bf16 the kernel still sums its UNROUNDED fp32 values, so the sums are pinned to the reference of the
        // unrounded tensor (y64), not to the sums of what was stored.
        double es = 0, et = 0, rs = 0, rt = 0;
        if (c.part) {
            std::vector<double> ref((size_t)c.B * slabs * c.C, 0.0), tot((size_t)c.B * c.C, 0.0), gtot((size_t)c.B * c.C, 0.0);
            std::vector<int> npx(slabs, 0);
            for (int b = 0; b < c.B; b++)
                for (int oh = 0; oh < g.Ho; oh++)
                    for (int ow = 0; ow < g.Wo; ow++) {
                        const int slab = ((oh / g.TH) * g.tiles_w + ow / g.TW) / g.PY;
                        if (b == 0) npx[slab]++;
                        for (int n = 0; n < c.C; n++) ref[((size_t)b * slabs + slab) * c.C + n] += d.y64[(((size_t)b * g.Ho + oh) * g.Wo + ow) * c.C + n];
                    }
            double ss = 0, ts = 0;
            for (size_t i = 0; i < ref.size(); i++) {
                ss = std::max(ss, std::fabs(ref[i]));
                const size_t t = i / ((size_t)slabs * c.C) * c.C + i % c.C;
                tot[t] += ref[i]; gtot[t] += (double)sums.f()[i];
            }
            for (double v : tot) ts = std::max(ts, std::fabs(v));
            // allowed per slab: pixels of the slab x (gate + 2^-24), in units of the y scale (the y gate on each term, one rounding per
            // term for the accumulation - stricter than the gamma_n bound of an fp32 sum; as in the expdw lab)
            const double gy = gate + std::ldexp(1.0, -24);
            for (size_t i = 0; i < ref.size(); i++) {
                const double df = absdiff((double)sums.f()[i], ref[i]);
                es = std::max(es, df / std::max(ss, 1e-300)); rs = std::max(rs, df / (npx[i / c.C % slabs] * gy * scale));
            }
            for (size_t i = 0; i < tot.size(); i++) {
                const double df = absdiff(gtot[i], tot[i]);
                et = std::max(et, df / std::max(ts, 1e-300)); rt = std::max(rt, df / ((double)g.Ho * g.Wo * gy * scale));
            }
            char buf[120];
            if (rs > 1.0) { ok = false; snprintf(buf, sizeof buf, " slab_sums:ratio=%.3g", rs); why += buf; }
            if (rt > 1.0) { ok = false; snprintf(buf, sizeof buf, " total_sums:ratio=%.3g", rt); why += buf; }
        }
        printf("%s %s err=%.3e host32=%.3e gate=%.3e ratio=%.3f sums: slab=%.3e total=%.3e slab_ratio=%.3f total_ratio=%.3f%s\n", ok ? "ok  " : "FAIL", cur_case.c_str(), ek, eh, gate, ratio, es,
               et, rs, rt, why.c_str());
        if (!ok) failures++;
        note(form, ek, eh, std::max(ratio, std::max(rs, rt)));
        delete dx; delete dw; delete db;
    }

    // ---------------------------------------------------------------------------------- mean
    for (int ci = 0; ci < kNMean; ci++) {
        const MeanCase& c = kMean[ci];
        const int S = (c.HW + kMeanSlab - 1) / kMeanSlab, PY = std::max(1, 256 / std::min(c.C, 64));
        if (S != mean_splits(c.HW) || PY != mean_partial_py(c.C)) { printf("FAIL %s: the restated geometry differs from the library's\n", c.name); failures++; continue; }
        if (list) { printf("CASE %s kind=mean form=k_mean HW=%d C=%d B=%d S=%d PY=%d\n", c.name, c.HW, c.C, c.B, S, PY); ncases++; continue; }
        if (dump && strcmp(dump, c.name)) continue;
        if (!dump && (!selected(c.name) || !pre16)) continue;
        std::mt19937 rng = rng_of(c.name);
        std::normal_distribution<float> nd(0.f, 1.f);
        std::vector<float> x((size_t)c.B * c.HW * c.C);
        for (auto& v : x) v = 0.25f + nd(rng);
        std::vector<double> p64((size_t)c.B * S * c.C, 0.0), pabs(p64.size(), 0.0), m64((size_t)c.B * c.C, 0.0), mabs(m64.size(), 0.0);
        for (int b = 0; b < c.B; b++)
            for (int px = 0; px < c.HW; px++)
                for (int n = 0; n < c.C; n++) {
                    const double v = x[((size_t)b * c.HW + px) * c.C + n];
                    p64[((size_t)b * S + px / kMeanSlab) * c.C + n] += v; pabs[((size_t)b * S + px / kMeanSlab) * c.C + n] += std::fabs(v);
                    m64[(size_t)b * c.C + n] += v; mabs[(size_t)b * c.C + n] += std::fabs(v);
                }
        for (auto& v : m64) v /= c.HW;
        if (dump) {
            wr(dump_dir, "x.f32", x.data(), x.size() * 4); wr(dump_dir, "y.f64", m64.data(), m64.size() * 8);
            FILE* f = fopen((std::string(dump_dir) + "/meta.txt").c_str(), "w");
            fprintf(f, "kind=mean\nB=%d\nHW=%d\nC=%d\n", c.B, c.HW, c.C);
            fclose(f);
            printf("dumped %s\n", c.name);
            return 0;
        }
        ncases++;
        cur_case = std::string(c.name) + " [k_mean_partial + k_mean_finish]";
        printf("RUN %s\n", cur_case.c_str()); fflush(stdout);
        InBuf* dx = in_f32(x);
        OutBuf part((size_t)c.B * S * c.C * 4), mean((size_t)c.B * c.C * 4);
        part.fill(st); mean.fill(st);
        launch_mean_partial(dx->f(), part.dev(), c.B, c.HW, c.C, S, st);
        launch_mean_finish(part.dev(), mean.dev(), c.B, c.HW, c.C, S, st);
        HIPCHK(hipGetLastError(), "launch");
        HIPCHK(hipStreamSynchronize(st), "synchronize");
        part.fetch(); mean.fetch();
        ran++;
        bool ok = true; std::string why;
        const size_t gbad = part.bad() + mean.bad();
        if (gbad) { ok = false; why += " guard:" + std::to_string(gbad) + "_bytes_overwritten"; }
        // Gate |got - ref64| <= d 2^-24 sum|x|, d = the longest chain of additions a term passes through in the kernel's order.
        // k_mean_partial: a thread adds every PY-th pixel of the slab to its accumulator - at most ceil(512 / PY) additions - and
        // thread row 0 then folds the PY accumulators serially: PY more.  Each addition rounds its result by a factor (1 + e),
        // |e| <= 2^-24, and a term x carries the factors of the additions behind it: |error| <= ((1 + 2^-24)^d - 1) sum|x|.  Two
        // of the d counted additions add to an exact zero (the first of the run, the first of the fold) and round nothing, and
        // (1 + u)^(d - 2) - 1 <= d u for every d u < 1/2 here (d <= 600), so the first-order form holds as stated.
        // k_mean_finish: the slab loop adds S more, and the division by HW rounds once more: d + S + 1, on sum|x| / HW.
        const int dp = (std::min(c.HW, kMeanSlab) + PY - 1) / PY + PY, dm = dp + S + 1;
        double rp = 0, rm = 0, ep = 0, em = 0;
        for (size_t i = 0; i < p64.size(); i++) {
            const double df = absdiff((double)part.f()[i], p64[i]);
            rp = std::max(rp, df / (dp * std::ldexp(1.0, -24) * pabs[i])); ep = std::max(ep, df / pabs[i]);
        }
        for (size_t i = 0; i < m64.size(); i++) {
            const double df = absdiff((double)mean.f()[i], m64[i]);
            rm = std::max(rm, df / (dm * std::ldexp(1.0, -24) * mabs[i] / c.HW)); em = std::max(em, df / (mabs[i] / c.HW));
        }
        char buf[120];
        if (rp > 1.0) { ok = false; snprintf(buf, sizeof buf, " partials:ratio=%.3g", rp); why += buf; }
        if (rm > 1.0) { ok = false; snprintf(buf, sizeof buf, " mean:ratio=%.3g", rm); why += buf; }
        printf("%s %s partial_err=%.3e (d=%d) mean_err=%.3e (d=%d) of sum|x|; ratio=%.3f / %.3f%s\n", ok ? "ok  " : "FAIL", cur_case.c_str(), ep, dp, em, dm, rp, rm, why.c_str());
        if (!ok) failures++;
        note("k_mean_partial", ep, dp * std::ldexp(1.0, -24), rp);
        note("k_mean_finish", em, dm * std::ldexp(1.0, -24), rm);
        delete dx;
    }

    // ---------------------------------------------------------------------------------- squeeze-excite
    for (int ci = 0; ci < kNSe; ci++) {
        const SeCase& c = kSe[ci];
        const SeGeo g = se_geo(c);
        if (g.lds != se_lds_bytes(c.C, c.Cr, g.thr) || !se_supported(c.C, c.Cr) || g.lds > 64 * 1024) { printf("FAIL %s: LDS request %zu\n", c.name, g.lds); failures++; continue; }
        if (list) {
            SeData dl; if (c.act1 == ACT_RELU) se_gen(c, dl);
            printf("CASE %s kind=se form=k_se threads=%d C=%d Cr=%d S=%d act1=%s act2=%s b1=%d b2=%d B=%d probe=%d thr=%d P=%d G=%d path=%s doubled=%d quads_over=%d lds=%zu relu_live=%.3f\n", c.name, c.threads, c.C,
                   c.Cr, c.S, act_name(c.act1), act_name(c.act2), c.b1, c.b2, c.B, c.probe, g.thr, g.P, g.G, g.v4 ? "v4" : "scalar", g.doubled, (int)(g.v4 && c.C / 4 > g.thr), g.lds, dl.live);
            ncases++;
            continue;
        }
        if (dump && strcmp(dump, c.name)) continue;
        if (!dump && (!selected(c.name) || !pre16)) continue;
        SeData d; se_gen(c, d);
        if (dump) {
            wr(dump_dir, "partial.f32", d.part.data(), d.part.size() * 4); wr(dump_dir, "w1.f32", d.w1.data(), d.w1.size() * 4); wr(dump_dir, "b1.f32", d.b1.data(), d.b1.size() * 4);
            wr(dump_dir, "w2t.f32", d.w2t.data(), d.w2t.size() * 4); wr(dump_dir, "b2.f32", d.b2.data(), d.b2.size() * 4); wr(dump_dir, "y.f64", d.s64.data(), d.s64.size() * 8);
            FILE* f = fopen((std::string(dump_dir) + "/meta.txt").c_str(), "w");
            fprintf(f, "kind=se\nB=%d\nS=%d\nHW=%d\nC=%d\nCr=%d\nact1=%s\nact2=%s\n", c.B, c.S, d.HW, c.C, c.Cr, act_name(c.act1), act_name(c.act2));
            fclose(f);
            printf("dumped %s\n", c.name);
            return 0;
        }
        ncases++;
        const std::string form = c.probe ? "k_se mean stage" : g.v4 ? (g.G > 1 ? "k_se v4 G>1" : "k_se v4 G=1") : "k_se scalar";
        cur_case = std::string(c.name) + " [" + form + ", " + std::to_string(g.thr) + " threads, P=" + std::to_string(g.P) + " G=" + std::to_string(g.G) + "]";
        printf("RUN %s\n", cur_case.c_str()); fflush(stdout);
        InBuf* dpart = in_f32(d.part); InBuf* dw1 = in_f32(d.w1); InBuf* dw2 = in_f32(d.w2t);
        InBuf* db1 = c.b1 ? in_f32(d.b1) : nullptr; InBuf* db2 = c.b2 ? in_f32(d.b2) : nullptr;
        OutBuf sc((size_t)c.B * c.C * 4);
        sc.fill(st);
        SeParams p{dpart->f(), c.S, d.HW, dw1->f(), db1 ? db1->f() : nullptr, dw2->f(), db2 ? db2->f() : nullptr, sc.dev(), c.B, c.C, c.Cr, c.act1, c.act2};
        p.threads = c.threads;
        launch_se(p, st);
        HIPCHK(hipGetLastError(), "launch");
        HIPCHK(hipStreamSynchronize(st), "synchronize");
        sc.fetch();
        ran++;
        bool ok = true; std::string why;
        const size_t gbad = sc.bad();
        if (gbad) { ok = false; why += " guard:" + std::to_string(gbad) + "_bytes_overwritten"; }
        double scale = 0, eh = 0, ek = 0, ratio = 0;
        for (double v : d.s64) scale = std::max(scale, std::fabs(v));
        for (size_t i = 0; i < d.s64.size(); i++) eh = std::max(eh, std::fabs((double)d.s32[i] - d.s64[i]) / scale);
        if (c.probe) {
            // the mean stage: a thread's interleaved slab subset is at most ceil(S / P) additions, the fold P more (P = 1: the subset
            // is the whole loop and there is no fold), then the product with the rounded 1 / HW: two more roundings.  The bound and
            // its first-order form as for k_mean_partial above.
            const int dd = (c.S + g.P - 1) / g.P + (g.P > 1 ? g.P : 0) + 2;
            for (size_t i = 0; i < d.s64.size(); i++) {
                const double df = absdiff((double)sc.f()[i], d.mean64[i]), allow = dd * std::ldexp(1.0, -24) * d.sabs[i] / d.HW;
                ek = std::max(ek, df / (d.sabs[i] / d.HW)); ratio = std::max(ratio, df / allow);
            }
            eh = dd * std::ldexp(1.0, -24);
        } else {
            const double gate = 4.0 * eh + std::ldexp(1.0, -22);       // the y gate, on the scale
            for (size_t i = 0; i < d.s64.size(); i++) {
                const double df = absdiff((double)sc.f()[i], d.s64[i]);
                ek = std::max(ek, df / scale); ratio = std::max(ratio, df / (gate * scale));
            }
        }
        if (ratio > 1.0) { ok = false; char buf[80]; snprintf(buf, sizeof buf, " scale:ratio=%.3g", ratio); why += buf; }
        printf("%s %s err=%.3e host32=%.3e ratio=%.3f%s\n", ok ? "ok  " : "FAIL", cur_case.c_str(), ek, eh, ratio, why.c_str());
        if (!ok) failures++;
        note(form, ek, eh, ratio);
        delete dpart; delete dw1; delete dw2; delete db1; delete db2;
    }
    if (dump) { printf("no such case: %s\n", dump); return 2; }
    for (auto& kv : forms) printf("FORM %s | cases=%d worst_err=%.3e worst_host32=%.3e worst_ratio=%.3f\n", kv.first.c_str(), kv.second.cases, kv.second.ek, kv.second.eh, kv.second.ratio);
    printf("SUMMARY {\"cases\": %d, \"ran\": %d, \"failures\": %d, \"prefetch\": %d}\n", ncases, ran, failures, (int)pre16);
    return failures ? 1 : 0;
}
