// gfx950 convolutions with a small Cin: the direct (VALU) forms and the 3x3 stride-2 stem as an implicit GEMM on the f32 MFMA.
// Stem weights are re-laid to [kh][kw][Cin][Cout] at plan time.  (General convolutions: launch_conv_igemm in pw_gemm.hip.)
#include "kernels.h"
#include "pw_common.h"

#include <algorithm>
#include <cstdlib>

namespace bnhip {

// ------------------------------------------------------------------------------------------ direct conv (stem)
// thread = (output pixel, group of 4 output channels); weights [kh][kw][Cin][Cout].
__global__ __launch_bounds__(256) void k_conv_direct(ConvParams p) {
    const int C4 = p.Cout >> 2;
    size_t total = (size_t)p.B * p.Ho * p.Wo * C4;
    size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    int c4 = (int)(idx % C4);
    size_t pix = idx / C4;
    int wo = (int)(pix % p.Wo);
    int ho = (int)((pix / p.Wo) % p.Ho);
    int b = (int)(pix / ((size_t)p.Wo * p.Ho));
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* w4 = reinterpret_cast<const float4*>(p.w);
    for (int i = 0; i < p.kh; i++) {
        int hi = ho * p.sh - p.pt + i;
        if (hi < 0 || hi >= p.H) continue;
        for (int j = 0; j < p.kw; j++) {
            int wi = wo * p.sw - p.pl + j;
            if (wi < 0 || wi >= p.W) continue;
            const float* ip = p.in + (((size_t)b * p.H + hi) * p.W + wi) * p.Cin;
            const float4* wp = w4 + (size_t)((i * p.kw + j) * p.Cin) * C4 + c4;
            for (int ci = 0; ci < p.Cin; ci++) {
                float x = ip[ci];
                float4 w = wp[(size_t)ci * C4];
                acc.x = fmaf(x, w.x, acc.x); acc.y = fmaf(x, w.y, acc.y);
                acc.z = fmaf(x, w.z, acc.z); acc.w = fmaf(x, w.w, acc.w);
            }
        }
    }
    if (p.bias) {
        float4 bv = reinterpret_cast<const float4*>(p.bias)[c4];
        acc.x += bv.x; acc.y += bv.y; acc.z += bv.z; acc.w += bv.w;
    }
    acc.x = apply_act(acc.x, p.act); acc.y = apply_act(acc.y, p.act);
    acc.z = apply_act(acc.z, p.act); acc.w = apply_act(acc.w, p.act);
    reinterpret_cast<float4*>(p.out)[idx] = acc;
}
// Compile-time (KH, KW, CIN) variant: every tap load is issued up front (the generic loop above is a chain of
// dependent L1/L2 round trips: 18 serial loads per thread for the 3x3x2 stem made it latency-bound at 1 TB/s).
template <int KH, int KW, int CIN>
__global__ __launch_bounds__(256) void k_conv_direct_t(ConvParams p) {
    const int C4 = p.Cout >> 2;
    size_t total = (size_t)p.B * p.Ho * p.Wo * C4;
    size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    int c4 = (int)(idx % C4);
    size_t pix = idx / C4;
    int wo = (int)(pix % p.Wo);
    int ho = (int)((pix / p.Wo) % p.Ho);
    int b = (int)(pix / ((size_t)p.Wo * p.Ho));
    float x[KH][KW][CIN];
#pragma unroll
    for (int i = 0; i < KH; i++) {
        int hi = ho * p.sh - p.pt + i;
#pragma unroll
        for (int j = 0; j < KW; j++) {
            int wi = wo * p.sw - p.pl + j;
            bool ok = hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
            const float* ip = p.in + (((size_t)b * p.H + (ok ? hi : 0)) * p.W + (ok ? wi : 0)) * CIN;
#pragma unroll
            for (int ci = 0; ci < CIN; ci++) x[i][j][ci] = ok ? ip[ci] : 0.f;
        }
    }
    float4 acc = p.bias ? reinterpret_cast<const float4*>(p.bias)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 a2 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* w4 = reinterpret_cast<const float4*>(p.w) + c4;
#pragma unroll
    for (int i = 0; i < KH; i++)
#pragma unroll
        for (int j = 0; j < KW; j++)
#pragma unroll
            for (int ci = 0; ci < CIN; ci++) {
                float4 w = w4[(size_t)((i * KW + j) * CIN + ci) * C4];
                float xv = x[i][j][ci];
                a2.x = fmaf(xv, w.x, a2.x); a2.y = fmaf(xv, w.y, a2.y); a2.z = fmaf(xv, w.z, a2.z); a2.w = fmaf(xv, w.w, a2.w);
            }
    // same association as the generic kernel: sum of products first, bias added last
    with_act(p.act, [&](auto f) {
        acc.x = f(a2.x + acc.x); acc.y = f(a2.y + acc.y); acc.z = f(a2.z + acc.z); acc.w = f(a2.w + acc.w);
    });
    reinterpret_cast<float4*>(p.out)[idx] = acc;
}
// PX consecutive output columns per thread (same 4 output channels): the weight quad is loaded once per tap for
// PX pixels and the overlapping input columns once per thread.  PMC on the one-pixel version of the 3x3x2 stem:
// 329 VALU instructions per thread for 72 FMAs - address arithmetic and 72 scalar loads dominated.
template <int KH, int KW, int CIN, int S, int PX>
__global__ __launch_bounds__(256) void k_conv_direct_px(ConvParams p, int wgroups) {
    constexpr int NCOL = (PX - 1) * S + KW;
    const int C4 = p.Cout >> 2;
    size_t total = (size_t)p.B * p.Ho * wgroups * C4;
    size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    int c4 = (int)(idx % C4);
    size_t g = idx / C4;
    int wg = (int)(g % wgroups);
    int ho = (int)((g / wgroups) % p.Ho);
    int b = (int)(g / ((size_t)wgroups * p.Ho));
    const int wo0 = wg * PX, wi0 = wo0 * S - p.pl;
    float x[KH][NCOL][CIN];
#pragma unroll
    for (int i = 0; i < KH; i++) {
        int hi = ho * S - p.pt + i;
        bool rok = hi >= 0 && hi < p.H;
        const float* rp = p.in + ((size_t)b * p.H + (rok ? hi : 0)) * p.W * CIN;
#pragma unroll
        for (int c = 0; c < NCOL; c++) {
            int wi = wi0 + c;
            bool ok = rok && wi >= 0 && wi < p.W;
            const float* ip = rp + (size_t)(ok ? wi : 0) * CIN;
#pragma unroll
            for (int ci = 0; ci < CIN; ci++) x[i][c][ci] = ok ? ip[ci] : 0.f;
        }
    }
    const float4 bv = p.bias ? reinterpret_cast<const float4*>(p.bias)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 a2[PX];
#pragma unroll
    for (int q = 0; q < PX; q++) a2[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* w4 = reinterpret_cast<const float4*>(p.w) + c4;
#pragma unroll
    for (int i = 0; i < KH; i++)
#pragma unroll
        for (int j = 0; j < KW; j++)
#pragma unroll
            for (int ci = 0; ci < CIN; ci++) {
                float4 w = w4[(size_t)((i * KW + j) * CIN + ci) * C4];
#pragma unroll
                for (int q = 0; q < PX; q++) {
                    float xv = x[i][q * S + j][ci];
                    a2[q].x = fmaf(xv, w.x, a2[q].x); a2[q].y = fmaf(xv, w.y, a2[q].y);
                    a2[q].z = fmaf(xv, w.z, a2[q].z); a2[q].w = fmaf(xv, w.w, a2[q].w);
                }
            }
    // same association as the generic kernel: sum of products first, bias added last
    with_act(p.act, [&](auto f) {
#pragma unroll
        for (int q = 0; q < PX; q++) {
            a2[q].x = f(a2[q].x + bv.x); a2[q].y = f(a2[q].y + bv.y); a2[q].z = f(a2[q].z + bv.z); a2[q].w = f(a2[q].w + bv.w);
        }
    });
    const size_t o0 = (((size_t)b * p.Ho + ho) * p.Wo + wo0) * C4 + c4;
    float4* op = reinterpret_cast<float4*>(p.out) + o0;
#pragma unroll
    for (int q = 0; q < PX; q++)
        if (wo0 + q < p.Wo) {
            if (p.out_bf16) bf16x4_store(p.out, o0 + (size_t)q * C4, a2[q]);
            else op[(size_t)q * C4] = a2[q];
        }
}
// (bf16 activation storage: only the 4-pixel kernels below write bf16)
bool conv_direct_bf16_ok(const ConvParams& p) {
    return p.kh == 3 && p.kw == 3 && (p.Cin == 1 || p.Cin == 2) && p.sh == 2 && p.sw == 2 && (p.Cout & 3) == 0;
}
void launch_conv_direct(const ConvParams& p, hipStream_t s) {
    if (p.kh == 3 && p.kw == 3 && p.Cin == 2 && p.sh == 2 && p.sw == 2 && (p.Cout & 3) == 0) {
        constexpr int PX = 4;
        int wgroups = (p.Wo + PX - 1) / PX;
        size_t tot = (size_t)p.B * p.Ho * wgroups * (p.Cout >> 2);
        hipLaunchKernelGGL((k_conv_direct_px<3, 3, 2, 2, PX>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p, wgroups);
        return;
    }
    if (p.kh == 3 && p.kw == 3 && p.Cin == 1 && p.sh == 2 && p.sw == 2 && (p.Cout & 3) == 0) {      // one-channel image (log-mel stem)
        constexpr int PX = 4;
        int wgroups = (p.Wo + PX - 1) / PX;
        size_t tot = (size_t)p.B * p.Ho * wgroups * (p.Cout >> 2);
        hipLaunchKernelGGL((k_conv_direct_px<3, 3, 1, 2, PX>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, p, wgroups);
        return;
    }
    size_t total = (size_t)p.B * p.Ho * p.Wo * (p.Cout >> 2);
    dim3 grid((unsigned)((total + 255) / 256));
    if (p.kh == 3 && p.kw == 3 && p.Cin == 2) hipLaunchKernelGGL((k_conv_direct_t<3, 3, 2>), grid, dim3(256), 0, s, p);
    else if (p.kh == 3 && p.kw == 3 && p.Cin == 1) hipLaunchKernelGGL((k_conv_direct_t<3, 3, 1>), grid, dim3(256), 0, s, p);
    else if (p.kh == 3 && p.kw == 3 && p.Cin == 3) hipLaunchKernelGGL((k_conv_direct_t<3, 3, 3>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_conv_direct, grid, dim3(256), 0, s, p);
}

// Stem as an implicit GEMM on the f32 MFMA (3x3 stride-2 conv, Cin = 2): out[pixel][n] = sum_kk A[pixel][kk] W[n][kk]
// with kk = i*8 + jj*2 + ch over a 3 x 4 x 2 window (the fourth column is a zero-weight pad, so a k-group of 4 is two
// adjacent input pixels x 2 channels = 4 contiguous floats).  K = 24 -> two 16-wide slabs in the fragment order of
// k_expand_dw (lane kq of slab s holds k = 16 s + 4 kq .. +3).  The VALU version above spends 288 FMAs + addressing per
// 4 pixels x 4 channels (58 % VALU-busy at 188 us); here the FMAs move to the matrix pipe.
struct StemParams {
    const float* in; const float* wm /*[Cout][32]*/; const float* bias /*[Cout], zeros if absent*/; float* out;
    int B, H, W, Ho, Wo, Cout, pt, pl, act;
    unsigned total_px, tiles_per_wave;
};
template <int NTILES>
__global__ __launch_bounds__(256) void k_stem_mfma(StemParams p) {
    constexpr int CS = NTILES * 16 + 4;                          // staging row stride (floats)
    __shared__ __attribute__((aligned(16))) float stage[4 * 16 * CS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, kq = lane >> 4;
    // weight fragments + bias of this lane (constant for the block)
    f32x4 wf[2][NTILES];
    float4 bq[NTILES];
#pragma unroll
    for (int t = 0; t < NTILES; t++) {
#pragma unroll
        for (int sl = 0; sl < 2; sl++) {
            float4 w = *reinterpret_cast<const float4*>(p.wm + (size_t)(16 * t + li) * 32 + 16 * sl + 4 * kq);
            wf[sl][t] = (f32x4){w.x, w.y, w.z, w.w};
        }
        bq[t] = *reinterpret_cast<const float4*>(p.bias + 16 * t + 4 * kq);
    }
    // window position of this lane's k-groups: slab 0 -> row i = kq >> 1, slab 1 -> row 2 (kq >= 2: zero weights)
    const int i0 = kq >> 1, j0 = (kq & 1) * 2;
    const unsigned tile0 = (blockIdx.x * 4u + wave) * p.tiles_per_wave;
    const unsigned hw = (unsigned)p.Ho * p.Wo;
    // pixel coordinates of this lane: decoded once, then advanced by 16 columns per tile (carry into row / clip)
    unsigned px = tile0 * 16u + li;
    int b, oh, ow;
    {
        const unsigned pc = min(px, p.total_px - 1);
        b = pc / hw;
        const unsigned rem = pc - (unsigned)b * hw;
        oh = rem / p.Wo; ow = rem - oh * p.Wo;
    }
    for (unsigned tt = 0; tt < p.tiles_per_wave; tt++, px += 16u) {
        if ((tile0 + tt) * 16u >= p.total_px) break;                    // wave-uniform
        if (tt) {
            ow += 16;
            while (ow >= p.Wo) { ow -= p.Wo; if (++oh == p.Ho) { oh = 0; b++; } }
            if (b >= p.B) { b = p.B - 1; oh = p.Ho - 1; ow = p.Wo - 1; }  // lanes past the end: any valid pixel
        }
        const float* xb = p.in + (size_t)b * p.H * p.W * 2;
        f32x4 xf[2];
        const int r0 = oh * 2 - p.pt, c0 = ow * 2 - p.pl + j0;
        // interior pixels (all but the image border) need neither clamps nor masks: one wave-uniform test
        const bool inner = r0 >= 0 && r0 + 2 < p.H && c0 >= 0 && c0 + 1 < p.W;
        if (__builtin_amdgcn_ballot_w64(!inner) == 0) {
#pragma unroll
            for (int sl = 0; sl < 2; sl++) {
                const float* q = xb + ((size_t)(r0 + (sl == 0 ? i0 : 2)) * p.W + c0) * 2;
                const float2 a = *reinterpret_cast<const float2*>(q), c = *reinterpret_cast<const float2*>(q + 2);
                xf[sl] = (f32x4){a.x, a.y, c.x, c.y};
            }
        } else {
#pragma unroll
            for (int sl = 0; sl < 2; sl++) {
                const int row = r0 + (sl == 0 ? i0 : 2), col = c0;
                const bool rv = row >= 0 && row < p.H;
                const bool v0 = rv && col >= 0 && col < p.W, v1 = rv && col + 1 >= 0 && col + 1 < p.W;
                const int rc = min(max(row, 0), p.H - 1);
                const float2 a = *reinterpret_cast<const float2*>(xb + ((size_t)rc * p.W + min(max(col, 0), p.W - 1)) * 2);
                const float2 c = *reinterpret_cast<const float2*>(xb + ((size_t)rc * p.W + min(max(col + 1, 0), p.W - 1)) * 2);
                xf[sl] = (f32x4){v0 ? a.x : 0.f, v0 ? a.y : 0.f, v1 ? c.x : 0.f, v1 ? c.y : 0.f};
            }
        }
        f32x4 acc[NTILES];
#pragma unroll
        for (int t = 0; t < NTILES; t++) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sl = 0; sl < 2; sl++)
#pragma unroll
            for (int sidx = 0; sidx < 4; sidx++)
#pragma unroll
                for (int t = 0; t < NTILES; t++)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[sl][t][sidx], xf[sl][sidx], acc[t], 0, 0, 0);
        with_act(p.act, [&](auto f) {
#pragma unroll
            for (int t = 0; t < NTILES; t++) {
                acc[t][0] = f(acc[t][0] + bq[t].x); acc[t][1] = f(acc[t][1] + bq[t].y);
                acc[t][2] = f(acc[t][2] + bq[t].z); acc[t][3] = f(acc[t][3] + bq[t].w);
            }
        });
        // the lane holds 4 channels of one pixel per n-tile: stage the 16 x Cout tile through this wave's LDS slice and write
        // it out as one contiguous run (16 pixels x Cout floats) instead of 64-byte pieces
        float* stg = stage + wave * (16 * CS);
#pragma unroll
        for (int t = 0; t < NTILES; t++) *reinterpret_cast<f32x4*>(&stg[li * CS + 16 * t + 4 * kq]) = acc[t];
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        const unsigned px0 = (tile0 + tt) * 16u;
#pragma unroll
        for (int q = 0; q < (16 * NTILES * 4) / 64; q++) {
            const int idx = lane + 64 * q;                       // float4 index inside the 16 x Cout tile
            const int row = idx / (NTILES * 4), c4 = idx % (NTILES * 4);
            if (px0 + row < p.total_px)
                *reinterpret_cast<f32x4*>(p.out + (size_t)(px0 + row) * p.Cout + 4 * c4) = *reinterpret_cast<const f32x4*>(&stg[row * CS + 4 * c4]);
        }
        __builtin_amdgcn_wave_barrier();
    }
}
bool stem_mfma_supported(const ConvParams& p) {
    return p.kh == 3 && p.kw == 3 && p.sh == 2 && p.sw == 2 && p.Cin == 2 && (p.Cout == 32 || p.Cout == 64);
}
void launch_stem_mfma(const ConvParams& c, const float* wm, const float* bias_p, hipStream_t s) {
    static const int stem_tpw = getenv("BNHIP_STEM_TPW") ? std::max(atoi(getenv("BNHIP_STEM_TPW")), 1) : 8;   // tiles per wave
    StemParams p{c.in, wm, bias_p, c.out, c.B, c.H, c.W, c.Ho, c.Wo, c.Cout, c.pt, c.pl, c.act,
                 (unsigned)((size_t)c.B * c.Ho * c.Wo), (unsigned)stem_tpw};
    unsigned tiles = (p.total_px + 15) / 16;
    unsigned blocks = (tiles + 4 * p.tiles_per_wave - 1) / (4 * p.tiles_per_wave);
    if (c.Cout == 32) hipLaunchKernelGGL((k_stem_mfma<2>), dim3(blocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_stem_mfma<4>), dim3(blocks), dim3(256), 0, s, p);
}

}  // namespace bnhip
