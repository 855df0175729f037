// Full-width form of k_expand_dw (csrc/expdw.hip): a fixed list of the smallest layers at which the in-image
// column mapping can go wrong, through launch_expand_dw WITH AN EXPLICIT SHAPE INDEX.  Per case: a digest of the output tensor and
// of the per-tile sums (to compare a run under BNHIP_EXPDW_FULLW=0 bit for bit), the max error against a plain
// fp64 loop nest and the error of a plain fp32 evaluation of the same case (both in units of the output scale), and whether guard
// words around y and the sums were overwritten.  The gate itself (4 x the fp32 error + 2^-22) is applied by tests/test_expdw_fullwidth.py.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I birdnet-go_amd/csrc -o expdw_fullw_check tools/ubench/expdw_fullw_check.cpp \
//         -L birdnet-go_amd/lib -lbnhip -Wl,-rpath,birdnet-go_amd/lib
//   expdw_fullw_check            run every case on the current device; exit status 1 on an overwritten guard, 3 on a HIP error
//   expdw_fullw_check --list     print the cases and whether each takes the full-width form; touches no device
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "kernels.h"
using namespace bnhip;

// the three tile shapes of the 6 x 32 layers, by their index in the library's table (checked against expdw_shape_slabs below)
struct TileShape { int idx, k, s, toh, tow; };
static const TileShape kTiles[] = {{2, 3, 1, 8, 32}, {6, 5, 1, 8, 32}, {12, 5, 2, 4, 16}};
// depthwise input sizes: the image as wide as the tile column (6, 5 and 3 rows: all, some and few of the 12 MFMA tiles valid), the
// same transposed (for the transposed shape indices), and the neighbours that must keep the footprint mapping: one column short,
// one column more (a second, ragged tile column), two full tile columns
struct Geo { int H, W; bool eligible; };
static const Geo kGeos[] = {{6, 32, true}, {5, 32, true}, {3, 32, true}, {32, 6, true}, {32, 5, true}, {32, 3, true},
                            {6, 31, false}, {6, 33, false}, {6, 64, false}, {31, 6, false}, {33, 6, false}, {64, 6, false}};
static const int kCins[] = {40, 48, 112};                 // Kw = 40: half slab (H8); 48, 112: full slabs
static const int kCmids[] = {36, 96};                     // a ragged second chunk (one quad); three full chunks

static int same_out(int H, int s) { return (H + s - 1) / s; }
static int same_pad(int H, int Ho, int k, int s) { return std::max((Ho - 1) * s + k - H, 0) / 2; }
static double swish64(double v) { return v / (1.0 + std::exp(-v)); }
static float swish32(float v) { return v / (1.0f + expf(-v)); }
static unsigned long long fnv(const void* p, size_t n, unsigned long long h = 1469598103934665603ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

static const unsigned kPat = 0xffc0de5au;                 // a NaN payload no kernel arithmetic produces
static const size_t kGuard = 4096;                        // words on each side
static std::string cur_case = "(setup)";
#define HIPCHK(expr, what)                                                                                        \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) { printf("HIP ERROR %s at %s: %s\n", hipGetErrorString(e_), what, cur_case.c_str()); fflush(stdout); _Exit(3); } \
    } while (0)
template <typename T>
static T* dev_guarded(const std::vector<T>& h) {          // [NaN guard][data][NaN guard]: a load beyond an input shows even under a zero weight
    const size_t gb = kGuard * 4, nb = h.size() * sizeof(T);
    std::vector<unsigned> all((gb * 2 + nb + 3) / 4 + 1, 0x7fc00000u);
    memcpy((char*)all.data() + gb, h.data(), nb);
    char* d; HIPCHK(hipMalloc(&d, all.size() * 4), "hipMalloc");
    HIPCHK(hipMemcpy(d, all.data(), all.size() * 4, hipMemcpyHostToDevice), "hipMemcpy");
    return reinterpret_cast<T*>(d + gb);
}
template <typename T> static void dev_free_guarded(T* p) { if (p) (void)hipFree((char*)p - kGuard * 4); }

int main(int argc, char** argv) {
    const bool list = argc > 1 && !strcmp(argv[1], "--list");
    if (argc > 1 && !list) { printf("usage: expdw_fullw_check [--list]\n"); return 2; }
    const int N = expdw_num_shapes() / 2, B = 2;
    if (!list) {
        int nd = 0;
        if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) { printf("no HIP device\n"); return 3; }
    }
    hipStream_t st = nullptr;
    if (!list) HIPCHK(hipStreamCreate(&st), "hipStreamCreate");
    int ncases = 0, bad = 0;
    for (const TileShape& t : kTiles)
        for (const Geo& g : kGeos)
            for (int Cin : kCins)
                for (int Cm : kCmids) {
                    const int k = t.k, s = t.s, H = g.H, W = g.W, Ho = same_out(H, s), Wo = same_out(W, s);
                    const int pt = same_pad(H, Ho, k, s), pl = same_pad(W, Wo, k, s);
                    const ExpDwGeo eg{k, s, H, W, Ho, Wo, pt, pl, false, 0};
                    if (expdw_skw(Cin, ACT_SWISH, false) != 0) { printf("FAIL: Cin %d takes the small-K form\n", Cin); return 1; }
                    std::vector<int> shapes;
                    for (int idx : {t.idx, t.idx + N})
                        if (expdw_shape_fits(idx, eg, false)) shapes.push_back(idx);
                    if (shapes.empty()) { printf("FAIL: no orientation of shape %d fits %dx%d\n", t.idx, H, W); return 1; }
                    // ---- data and references (seeded by the layer's name: the same on every run and machine)
                    char lname[96]; snprintf(lname, sizeof lname, "k%ds%d_%dx%d/c%dx%d", k, s, H, W, Cin, Cm);
                    std::vector<float> x, we, be, wd, bd, y32; std::vector<double> y64;
                    double scale = 0, eh = 0;
                    if (!list) {
                        unsigned seed = 2166136261u;
                        for (const char* c = lname; *c; c++) seed = (seed ^ (unsigned char)*c) * 16777619u;
                        std::mt19937 rng(seed);
                        std::normal_distribution<float> nd(0.f, 1.f);
                        x.resize((size_t)B * H * W * Cin); we.resize((size_t)Cm * Cin); be.resize(Cm); wd.resize((size_t)k * k * Cm); bd.resize(Cm);
                        for (auto& v : x) v = nd(rng);
                        for (auto& v : we) v = nd(rng) / std::sqrt((float)Cin);
                        for (auto& v : be) v = 0.1f * nd(rng);
                        for (auto& v : wd) v = nd(rng) / (float)k;
                        for (auto& v : bd) v = 0.1f * nd(rng);
                        const size_t npx = (size_t)B * H * W;
                        std::vector<double> E(npx * Cm); std::vector<float> E32(npx * Cm);
                        for (size_t px = 0; px < npx; px++)
                            for (int n = 0; n < Cm; n++) {
                                double a = 0; float a32 = 0.f;
                                for (int q = 0; q < Cin; q++) { a += (double)x[px * Cin + q] * (double)we[(size_t)n * Cin + q]; a32 += x[px * Cin + q] * we[(size_t)n * Cin + q]; }
                                E[px * Cm + n] = swish64(a + be[n]); E32[px * Cm + n] = swish32(a32 + be[n]);
                            }
                        y64.resize((size_t)B * Ho * Wo * Cm); y32.resize(y64.size());
                        for (int b = 0; b < B; b++)
                            for (int oh = 0; oh < Ho; oh++)
                                for (int ow = 0; ow < Wo; ow++)
                                    for (int n = 0; n < Cm; n++) {
                                        double a = 0; float a32 = 0.f;
                                        for (int i = 0; i < k; i++)
                                            for (int j = 0; j < k; j++) {
                                                const int h = oh * s - pt + i, w = ow * s - pl + j;
                                                if (h < 0 || h >= H || w < 0 || w >= W) continue;
                                                const size_t e = (((size_t)b * H + h) * W + w) * Cm + n;
                                                a += E[e] * (double)wd[(size_t)(i * k + j) * Cm + n]; a32 += E32[e] * wd[(size_t)(i * k + j) * Cm + n];
                                            }
                                        const size_t o = (((size_t)b * Ho + oh) * Wo + ow) * Cm + n;
                                        y64[o] = swish64(a + bd[n]); y32[o] = swish32(a32 + bd[n]);
                                    }
                        for (double v : y64) scale = std::max(scale, std::fabs(v));
                        for (size_t i = 0; i < y64.size(); i++) eh = std::max(eh, std::fabs((double)y32[i] - y64[i]));
                        eh /= scale;
                    }
                    // ---- device images (the planner's padded parameter copies)
                    const int Cp = expdw_cp(Cm), Kw = expdw_kw(Cin);
                    float *dx = nullptr, *dwe = nullptr, *dbe = nullptr, *dwd = nullptr, *dbd = nullptr; uint16_t* dimg = nullptr;
                    if (!list) {
                        std::vector<float> wep((size_t)Cp * Kw, 0.f), bep(Cp, 0.f), wdp((size_t)k * k * Cp, 0.f), bdp(Cp, 0.f);
                        for (int n = 0; n < Cm; n++) memcpy(&wep[(size_t)n * Kw], &we[(size_t)n * Cin], (size_t)Cin * 4);
                        memcpy(bep.data(), be.data(), (size_t)Cm * 4); memcpy(bdp.data(), bd.data(), (size_t)Cm * 4);
                        for (int q = 0; q < k * k; q++) memcpy(&wdp[(size_t)q * Cp], &wd[(size_t)q * Cm], (size_t)Cm * 4);
                        dx = dev_guarded(x); dwe = dev_guarded(wep); dbe = dev_guarded(bep); dwd = dev_guarded(wdp); dbd = dev_guarded(bdp);
                        dimg = dev_guarded(expdw_bx_image(we.data(), Cm, Cin));
                    }
                    for (int shape : shapes) {
                        const bool tr = shape >= N, fullw = expdw_fullwidth(shape, eg);
                        const int oHo = tr ? Wo : Ho, oWo = tr ? Ho : Wo, tw = (oWo + t.tow - 1) / t.tow, tiles = expdw_shape_slabs(shape, eg);
                        if (tiles != ((oHo + t.toh - 1) / t.toh) * tw) { printf("FAIL: tile table differs from the library's at index %d\n", shape); return 1; }
                        for (int bx = 0; bx < 2; bx++)
                            for (int sums = 1; sums >= 0; sums--) {
                                char cname[160];
                                snprintf(cname, sizeof cname, "%s%s/shape%d/%s", lname, bx ? "_bx" : "", shape, sums ? "sums" : "nosums");
                                cur_case = cname;
                                ncases++;
                                if (list) { printf("CASE %s eligible=%d fullw=%d\n", cname, (int)g.eligible, (int)fullw); continue; }
                                const size_t nout = y64.size(), yall = kGuard * 2 + nout, pn = sums ? (size_t)B * tiles * Cm : 0, pall = kGuard * 2 + (size_t)B * tiles * Cm;
                                unsigned *dy, *dp;
                                HIPCHK(hipMalloc(&dy, yall * 4), "hipMalloc"); HIPCHK(hipMalloc(&dp, pall * 4), "hipMalloc");
                                HIPCHK(hipMemsetD32Async((hipDeviceptr_t)dy, (int)kPat, yall, st), "fill y");
                                HIPCHK(hipMemsetD32Async((hipDeviceptr_t)dp, (int)kPat, pall, st), "fill sums");
                                launch_expand_dw(dx, dwe, dbe, dwd, dbd, reinterpret_cast<float*>(dy + kGuard), sums ? reinterpret_cast<float*>(dp + kGuard) : nullptr, B, H, W, Cin, Cm,
                                                 Ho, Wo, k, s, pt, pl, ACT_SWISH, ACT_SWISH, shape, nullptr, st, bx ? dimg : nullptr, 0, 0, 0);
                                HIPCHK(hipGetLastError(), "launch");
                                HIPCHK(hipStreamSynchronize(st), "synchronize");
                                std::vector<unsigned> hy(yall), hp(pall);
                                HIPCHK(hipMemcpy(hy.data(), dy, yall * 4, hipMemcpyDeviceToHost), "copy y");
                                HIPCHK(hipMemcpy(hp.data(), dp, pall * 4, hipMemcpyDeviceToHost), "copy sums");
                                (void)hipFree(dy); (void)hipFree(dp);
                                size_t gbad = 0;
                                for (size_t i = 0; i < yall; i++) if (i < kGuard || i >= kGuard + nout) gbad += hy[i] != kPat;
                                for (size_t i = 0; i < pall; i++) if (i < kGuard || i >= kGuard + pn) gbad += hp[i] != kPat;
                                const float* yf = reinterpret_cast<const float*>(hy.data() + kGuard);
                                const float* pf = reinterpret_cast<const float*>(hp.data() + kGuard);
                                double ek = 0;
                                for (size_t i = 0; i < nout; i++) { double d = std::fabs((double)yf[i] - y64[i]); if (!(d == d)) d = 1e30; ek = std::max(ek, d / scale); }
                                // the sums per tile, in the kernel's tile order, in units of (pixels summed) x (output scale)
                                double es = 0;
                                if (sums) {
                                    std::vector<double> ref((size_t)B * tiles * Cm, 0.0); std::vector<int> npx(tiles, 0);
                                    for (int b = 0; b < B; b++)
                                        for (int r = 0; r < oHo; r++)
                                            for (int q = 0; q < oWo; q++) {
                                                const int tile = (r / t.toh) * tw + q / t.tow, oh = tr ? q : r, ow = tr ? r : q;
                                                if (b == 0) npx[tile]++;
                                                for (int n = 0; n < Cm; n++) ref[((size_t)b * tiles + tile) * Cm + n] += y64[(((size_t)b * Ho + oh) * Wo + ow) * Cm + n];
                                            }
                                    for (size_t i = 0; i < ref.size(); i++) { double d = std::fabs((double)pf[i] - ref[i]); if (!(d == d)) d = 1e30; es = std::max(es, d / (npx[i / Cm % tiles] * scale)); }
                                }
                                printf("CASE %s eligible=%d fullw=%d y=%016llx sums=%016llx err=%.4e host32=%.4e sums_err=%.4e guard=%zu\n", cname, (int)g.eligible, (int)fullw,
                                       fnv(yf, nout * 4), fnv(pf, pn * 4), ek, eh, es, gbad);
                                if (gbad) bad++;
                            }
                    }
                    dev_free_guarded(dx); dev_free_guarded(dwe); dev_free_guarded(dbe); dev_free_guarded(dwd); dev_free_guarded(dbd); dev_free_guarded(dimg);
                }
    printf("SUMMARY cases=%d guard_failures=%d\n", ncases, bad);
    return bad ? 1 : 0;
}
