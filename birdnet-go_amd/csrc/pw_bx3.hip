// gfx950 split-bf16 pointwise GEMM: k_pw_bx3, its software-pipelined form k_pw_bx3p, the plan-time weight image and the launcher
// that hands a call to the streamed-operand forms (pw_b16.hip, pw_ws.hip) where they apply.
#include "kernels.h"
#include "pw_common.h"

#include <algorithm>
#include <type_traits>
#include <vector>

namespace bnhip {

// ------------------------------------------------------------------------------------------ split-bf16 pointwise GEMM
// The same GEMM on the bf16 matrix pipe with fp32-equivalent products.  The f32-input MFMA runs at the vector rate (157 TF);
// v_mfma_f32_16x16x32_bf16 is 16x faster per MAC, and an fp32 value splits EXACTLY into three bf16 pieces by truncation:
//     x = hi + mid + lo,   hi = bf16(x), mid = bf16(x - hi), lo = x - hi - mid      (round to nearest even)
// (each subtraction is exact in fp32: the remainder of an 8-significant-bit rounding has at most 16 significant bits, the
// next one at most 8, so lo is a bf16 too; |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|).  Then
//     x * w = hi*whi + (hi*wmid + mid*whi) + (hi*wlo + mid*wmid + lo*whi)  +  [mid*wlo + lo*wmid + lo*wlo]
// where every bf16 x bf16 product is exact in the MFMA's fp32 accumulator and the bracketed terms are <= 2^-23 |x w|
// (the rounding of an fp32 product itself is <= 2^-24 |x w|): six products per k instead of one reproduce the fp32 product
// to within two units of its own rounding.  Accumulation stays fp32.  (|x| above the largest bf16, 3.39e38, is the one
// range the split cannot represent: hi overflows to infinity.)  The weights are split once at plan time (pw_bx3_image); activations are split in registers right after the
// fragment read - every activation row belongs to exactly one wave, so nothing is split twice, and the f32 operand tile in
// LDS (and the squeeze-excite multiply at store time) stays as in k_pw_gemm.
// K order: lane kq of a 32-wide slab holds k = 4kq..4kq+3 and 16+4kq..16+4kq+3 (the two conflict-free b128 slots of the
// f32 tile); the weight image uses the same order.
template <int NT, bool SC, int WM>
__global__ __launch_bounds__(256) void k_pw_bx3(PwParams p, const uint16_t* __restrict__ Wimg, int Npad, int nblk_n, unsigned nblk,
                                                 FDiv dn, FDiv dhw) {
    constexpr int BM = 64 * WM;
    constexpr int XQ = BM * PW_C4 / 256;
    constexpr int WSLOTS = 12 * NT * 16;                   // 16-byte slots of the weight tile: [plane 3][kq 4][row NT*16]
    constexpr int WQ = (WSLOTS + 255) / 256;
    constexpr int TILE_F = BM * PW_LS + WSLOTS * 4;        // floats
    constexpr int STG = 4 * 16 * (NT * 16 + 4);
    constexpr int LDSN = TILE_F > STG ? TILE_F : STG;
    __shared__ __attribute__((aligned(16))) float lds[LDSN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const unsigned L = xcd_remap(blockIdx.x, nblk);
    const int mblk = (int)fdiv(L, dn);
    const int m0 = mblk * BM;
    const int n0 = ((int)L - mblk * nblk_n) * (NT * 16);
    const int K = p.K;

    unsigned xoff[XQ], soff[SC ? XQ : 1], woff[WQ];
    const bool one = p.prec == 1;                          // plain bf16: only the hi plane of the weights, one product
    const int wslots = one ? WSLOTS / 3 : WSLOTS;
    const int kc4 = 4 * (tid % PW_C4);                     // this thread's column inside a slab (the same for every q: 256 % PW_C4 == 0)
    const int lbase = (tid / PW_C4) * PW_LS + 4 * (tid % PW_C4);
    constexpr int LQ = (256 / PW_C4) * PW_LS;
#pragma unroll
    for (int q = 0; q < XQ; q++) {
        const int idx = tid + 256 * q, row = idx / PW_C4, c4 = idx % PW_C4;
        const int m = min(m0 + row, p.M - 1);
        xoff[q] = (unsigned)m * (unsigned)K + 4 * c4;
        if (SC) soff[SC ? q : 0] = fdiv((unsigned)m, dhw) * (unsigned)K + 4 * c4;
    }
#pragma unroll
    for (int q = 0; q < WQ; q++) {
        const int slot = min(tid + 256 * q, WSLOTS - 1);
        const int plkq = slot / (NT * 16), r = slot - plkq * (NT * 16);
        woff[q] = (unsigned)plkq * (unsigned)Npad + (unsigned)min(n0 + r, Npad - 1);          // in 16-byte units
    }
    float4 xreg[XQ], sreg[SC ? XQ : 1];
    u32x4 wreg[WQ];
    const u32x4* W16 = reinterpret_cast<const u32x4*>(Wimg);
    // bf16 activation storage (p.a_bf16, K % 8 == 0): a thread fetches 8 channels = the same 16 bytes per load instruction as
    // the fp32 path, in half as many instructions (4 threads per 32-wide row instead of 8; the first XQ / 2 entries of the
    // same offset / register arrays, so the fp32 path pays nothing for it).  The first form of this path kept the fp32 thread
    // mapping with 8-byte loads and made every projection 20-30 % SLOWER: these layers are bound by loads in flight per wave,
    // not by bytes.
    constexpr int XH = XQ / 2;
    constexpr int LQH = 64 * PW_LS;
    if (p.a_bf16) {
#pragma unroll
        for (int q = 0; q < XH; q++) {
            const int row = (tid >> 2) + 64 * q;
            const int m = min(m0 + row, p.M - 1);
            xoff[q] = (unsigned)m * (unsigned)K + 8u * (unsigned)(tid & 3);
            if (SC) soff[SC ? q : 0] = fdiv((unsigned)m, dhw) * (unsigned)K + 8u * (unsigned)(tid & 3);
        }
    }
    auto gload = [&](int sl) {
        const float* Ak = p.A + sl * PW_BK;
        const bool kin = sl * PW_BK + kc4 < K;             // K tail (K % 32 != 0): columns beyond K are zeros (their weights too)
        if (p.a_bf16) {
            const bool kinh = sl * PW_BK + 8 * (tid & 3) < K;
            const uint16_t* A16 = reinterpret_cast<const uint16_t*>(p.A) + sl * PW_BK;
#pragma unroll
            for (int q = 0; q < XH; q++) {
                xreg[q] = kinh ? *reinterpret_cast<const float4*>(A16 + xoff[q]) : make_float4(0.f, 0.f, 0.f, 0.f);   // (8 raw bf16)
                if (SC) {
                    const float* sp = p.ascale + sl * PW_BK + soff[SC ? q : 0];
                    sreg[SC ? 2 * q : 0] = kinh ? *reinterpret_cast<const float4*>(sp) : make_float4(0.f, 0.f, 0.f, 0.f);
                    sreg[SC ? 2 * q + 1 : 0] = kinh ? *reinterpret_cast<const float4*>(sp + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < XQ; q++) {
                xreg[q] = kin ? *reinterpret_cast<const float4*>(Ak + xoff[q]) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (SC) sreg[SC ? q : 0] = kin ? *reinterpret_cast<const float4*>(p.ascale + sl * PW_BK + soff[SC ? q : 0]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        const u32x4* Ws = W16 + (size_t)sl * 12 * Npad;
#pragma unroll
        for (int q = 0; q < WQ; q++)
            if (tid + 256 * q < wslots) wreg[q] = Ws[woff[q]];
    };
    u32x4* Wl = reinterpret_cast<u32x4*>(lds + BM * PW_LS);
    auto lstore = [&]() {
        if (p.a_bf16) {
#pragma unroll
            for (int q = 0; q < XH; q++) {
                const unsigned r[4] = {__float_as_uint(xreg[q].x), __float_as_uint(xreg[q].y), __float_as_uint(xreg[q].z), __float_as_uint(xreg[q].w)};
                float4 v0 = make_float4(__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16), __uint_as_float(r[1] & 0xffff0000u));
                float4 v1 = make_float4(__uint_as_float(r[2] << 16), __uint_as_float(r[2] & 0xffff0000u), __uint_as_float(r[3] << 16), __uint_as_float(r[3] & 0xffff0000u));
                if (SC) {
                    const float4 s0 = sreg[SC ? 2 * q : 0], s1 = sreg[SC ? 2 * q + 1 : 0];
                    v0.x *= s0.x; v0.y *= s0.y; v0.z *= s0.z; v0.w *= s0.w; v1.x *= s1.x; v1.y *= s1.y; v1.z *= s1.z; v1.w *= s1.w;
                }
                *reinterpret_cast<float4*>(&lds[((tid >> 2) * PW_LS + 8 * (tid & 3)) + q * LQH]) = v0;
                *reinterpret_cast<float4*>(&lds[((tid >> 2) * PW_LS + 8 * (tid & 3)) + q * LQH + 4]) = v1;
            }
        } else {
#pragma unroll
        for (int q = 0; q < XQ; q++) {
            float4 v = xreg[q];
            if (SC) { const float4 sc = sreg[SC ? q : 0]; v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
            *reinterpret_cast<float4*>(&lds[lbase + q * LQ]) = v;
        }
        }
#pragma unroll
        for (int q = 0; q < WQ; q++)
            if (tid + 256 * q < wslots) Wl[tid + 256 * q] = wreg[q];
    };

    f32x4 acc[NT][WM];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int mt = 0; mt < WM; mt++) acc[t][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nslab = (K + PW_BK - 1) / PW_BK;
    gload(0);
    lstore();
    if (nslab > 1) gload(1);
    __syncthreads();
    for (int sl = 0; sl < nslab; sl++) {
        bf16x8 ah[WM], am[WM], al[WM];
        if (one) {
#pragma unroll
            for (int mt = 0; mt < WM; mt++) {
                const float* xr = &lds[(16 * WM * wave + 16 * mt + li) * PW_LS + 4 * kq];
                ah[mt] = bx1_cvt8(*reinterpret_cast<const f32x4*>(xr), *reinterpret_cast<const f32x4*>(xr + 16));
            }
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const bf16x8 wh = __builtin_bit_cast(bf16x8, Wl[kq * (NT * 16) + 16 * t + li]);
#pragma unroll
                for (int mt = 0; mt < WM; mt++) acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, ah[mt], acc[t][mt], 0, 0, 0);
            }
        } else {
#pragma unroll
        for (int mt = 0; mt < WM; mt++) {
            const float* xr = &lds[(16 * WM * wave + 16 * mt + li) * PW_LS + 4 * kq];
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(xr), x1 = *reinterpret_cast<const f32x4*>(xr + 16);
            bx3_split8(x0, x1, &ah[mt], &am[mt], &al[mt]);
        }
        // weight fragments of tile t + 1 are requested before the MFMAs of tile t (the ISA of the first version waited a full
        // LDS round trip in front of every tile: with ~2 waves per SIMD on the late layers nothing else covered it)
        u32x4 wfr[2][3];
#pragma unroll
        for (int pl3 = 0; pl3 < 3; pl3++) wfr[0][pl3] = Wl[(pl3 * 4 + kq) * (NT * 16) + li];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (t + 1 < NT) {
#pragma unroll
                for (int pl3 = 0; pl3 < 3; pl3++) wfr[(t + 1) & 1][pl3] = Wl[(pl3 * 4 + kq) * (NT * 16) + 16 * (t + 1) + li];
            }
            const bf16x8 wh = __builtin_bit_cast(bf16x8, wfr[t & 1][0]);
            const bf16x8 wm = __builtin_bit_cast(bf16x8, wfr[t & 1][1]);
            const bf16x8 wl = __builtin_bit_cast(bf16x8, wfr[t & 1][2]);
#pragma unroll
            for (int mt = 0; mt < WM; mt++) acc[t][mt] = bx3_mfma6(acc[t][mt], wh, wm, wl, ah[mt], am[mt], al[mt]);
        }
        }
        if (sl + 1 < nslab) {
            __syncthreads();                 // everyone is done reading the single operand buffer
            lstore();
            if (sl + 2 < nslab) gload(sl + 2);
        }
        __syncthreads();
    }
    pw_epilogue<NT, WM>(p, acc, lds, m0, n0);
}

// Software-pipelined form (the k_pw_pipe structure): the late layers have M = 12 288 rows at batch 256, i.e. only ~2 blocks
// per CU and 1-2 waves per SIMD, so nothing hides a wave's own global -> LDS refill; with the bf16 MFMA phase 2.5x shorter
// than the fp32 one that refill dominated the slab period of k_pw_bx3.  Here it rides in the wave's MFMA shadow: two LDS
// operand buffers (dynamic LDS: up to 80 KB), slab s+1 is stored while slab s computes, slab s+2 is in flight in registers,
// one barrier per slab.
template <int NT, bool SC, int WM>
__global__ __launch_bounds__(256) void k_pw_bx3p(PwParams p, const uint16_t* __restrict__ Wimg, int Npad, int nblk_n, unsigned nblk,
                                                  FDiv dn, FDiv dhw) {
    constexpr int BM = 64 * WM;
    constexpr int XQ = BM * PW_C4 / 256;
    constexpr int WSLOTS = 12 * NT * 16;
    constexpr int WQ = (WSLOTS + 255) / 256;
    constexpr int TILE_F = BM * PW_LS + WSLOTS * 4;
    extern __shared__ __attribute__((aligned(16))) float bx3p_lds[];  // 2 * TILE_F floats (>= the epilogue staging area)
    float* lds = bx3p_lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const unsigned L = xcd_remap(blockIdx.x, nblk);
    const int mblk = (int)fdiv(L, dn);
    const int m0 = mblk * BM;
    const int n0 = ((int)L - mblk * nblk_n) * (NT * 16);
    const int K = p.K;

    unsigned xoff[XQ], soff[SC ? XQ : 1], woff[WQ];
    const bool one = p.prec == 1;                          // plain bf16: only the hi plane of the weights, one product
    const int wslots = one ? WSLOTS / 3 : WSLOTS;
    const int kc4 = 4 * (tid % PW_C4);                     // this thread's column inside a slab (the same for every q: 256 % PW_C4 == 0)
    const int lbase = (tid / PW_C4) * PW_LS + 4 * (tid % PW_C4);
    constexpr int LQ = (256 / PW_C4) * PW_LS;
#pragma unroll
    for (int q = 0; q < XQ; q++) {
        const int idx = tid + 256 * q, row = idx / PW_C4, c4 = idx % PW_C4;
        const int m = min(m0 + row, p.M - 1);
        xoff[q] = (unsigned)m * (unsigned)K + 4 * c4;
        if (SC) soff[SC ? q : 0] = fdiv((unsigned)m, dhw) * (unsigned)K + 4 * c4;
    }
#pragma unroll
    for (int q = 0; q < WQ; q++) {
        const int slot = min(tid + 256 * q, WSLOTS - 1);
        const int plkq = slot / (NT * 16), r = slot - plkq * (NT * 16);
        woff[q] = (unsigned)plkq * (unsigned)Npad + (unsigned)min(n0 + r, Npad - 1);
    }
    float4 xreg[XQ], sreg[SC ? XQ : 1];
    u32x4 wreg[WQ];
    const u32x4* W16 = reinterpret_cast<const u32x4*>(Wimg);
    // bf16 activation storage (p.a_bf16, K % 8 == 0): a thread fetches 8 channels = the same 16 bytes per load instruction as
    // the fp32 path, in half as many instructions (4 threads per 32-wide row instead of 8; the first XQ / 2 entries of the
    // same offset / register arrays, so the fp32 path pays nothing for it).  The first form of this path kept the fp32 thread
    // mapping with 8-byte loads and made every projection 20-30 % SLOWER: these layers are bound by loads in flight per wave,
    // not by bytes.
    constexpr int XH = XQ / 2;
    constexpr int LQH = 64 * PW_LS;
    if (p.a_bf16) {
#pragma unroll
        for (int q = 0; q < XH; q++) {
            const int row = (tid >> 2) + 64 * q;
            const int m = min(m0 + row, p.M - 1);
            xoff[q] = (unsigned)m * (unsigned)K + 8u * (unsigned)(tid & 3);
            if (SC) soff[SC ? q : 0] = fdiv((unsigned)m, dhw) * (unsigned)K + 8u * (unsigned)(tid & 3);
        }
    }
    auto gload = [&](int sl) {
        const float* Ak = p.A + sl * PW_BK;
        const bool kin = sl * PW_BK + kc4 < K;             // K tail (K % 32 != 0): columns beyond K are zeros (their weights too)
        if (p.a_bf16) {
            const bool kinh = sl * PW_BK + 8 * (tid & 3) < K;
            const uint16_t* A16 = reinterpret_cast<const uint16_t*>(p.A) + sl * PW_BK;
#pragma unroll
            for (int q = 0; q < XH; q++) {
                xreg[q] = kinh ? *reinterpret_cast<const float4*>(A16 + xoff[q]) : make_float4(0.f, 0.f, 0.f, 0.f);   // (8 raw bf16)
                if (SC) {
                    const float* sp = p.ascale + sl * PW_BK + soff[SC ? q : 0];
                    sreg[SC ? 2 * q : 0] = kinh ? *reinterpret_cast<const float4*>(sp) : make_float4(0.f, 0.f, 0.f, 0.f);
                    sreg[SC ? 2 * q + 1 : 0] = kinh ? *reinterpret_cast<const float4*>(sp + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < XQ; q++) {
                xreg[q] = kin ? *reinterpret_cast<const float4*>(Ak + xoff[q]) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (SC) sreg[SC ? q : 0] = kin ? *reinterpret_cast<const float4*>(p.ascale + sl * PW_BK + soff[SC ? q : 0]) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        const u32x4* Ws = W16 + (size_t)sl * 12 * Npad;
#pragma unroll
        for (int q = 0; q < WQ; q++)
            if (tid + 256 * q < wslots) wreg[q] = Ws[woff[q]];
    };
    auto lstore = [&](float* buf) {
        if (p.a_bf16) {
#pragma unroll
            for (int q = 0; q < XH; q++) {
                const unsigned r[4] = {__float_as_uint(xreg[q].x), __float_as_uint(xreg[q].y), __float_as_uint(xreg[q].z), __float_as_uint(xreg[q].w)};
                float4 v0 = make_float4(__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16), __uint_as_float(r[1] & 0xffff0000u));
                float4 v1 = make_float4(__uint_as_float(r[2] << 16), __uint_as_float(r[2] & 0xffff0000u), __uint_as_float(r[3] << 16), __uint_as_float(r[3] & 0xffff0000u));
                if (SC) {
                    const float4 s0 = sreg[SC ? 2 * q : 0], s1 = sreg[SC ? 2 * q + 1 : 0];
                    v0.x *= s0.x; v0.y *= s0.y; v0.z *= s0.z; v0.w *= s0.w; v1.x *= s1.x; v1.y *= s1.y; v1.z *= s1.z; v1.w *= s1.w;
                }
                *reinterpret_cast<float4*>(&buf[((tid >> 2) * PW_LS + 8 * (tid & 3)) + q * LQH]) = v0;
                *reinterpret_cast<float4*>(&buf[((tid >> 2) * PW_LS + 8 * (tid & 3)) + q * LQH + 4]) = v1;
            }
        } else {
#pragma unroll
        for (int q = 0; q < XQ; q++) {
            float4 v = xreg[q];
            if (SC) { const float4 sc = sreg[SC ? q : 0]; v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
            *reinterpret_cast<float4*>(&buf[lbase + q * LQ]) = v;
        }
        }
        u32x4* Wl = reinterpret_cast<u32x4*>(buf + BM * PW_LS);
#pragma unroll
        for (int q = 0; q < WQ; q++)
            if (tid + 256 * q < wslots) Wl[tid + 256 * q] = wreg[q];
    };

    f32x4 acc[NT][WM];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int mt = 0; mt < WM; mt++) acc[t][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nslab = (K + PW_BK - 1) / PW_BK;
    gload(0);
    lstore(lds);
    if (nslab > 1) gload(1);
    __syncthreads();
    auto slab = [&](int sl, auto DS, auto DL) {
        const float* Xs = lds + (sl & 1) * TILE_F;
        const u32x4* Wl = reinterpret_cast<const u32x4*>(Xs + BM * PW_LS);
        float* nxt = lds + ((sl + 1) & 1) * TILE_F;
        bf16x8 ah[WM], am[WM], al[WM];
        if (one) {
#pragma unroll
            for (int mt = 0; mt < WM; mt++) {
                const float* xr = &Xs[(16 * WM * wave + 16 * mt + li) * PW_LS + 4 * kq];
                ah[mt] = bx1_cvt8(*reinterpret_cast<const f32x4*>(xr), *reinterpret_cast<const f32x4*>(xr + 16));
            }
            bf16x8 wh1[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) wh1[t] = __builtin_bit_cast(bf16x8, Wl[kq * (NT * 16) + 16 * t + li]);
            if (decltype(DS)::value) lstore(nxt);
            if (decltype(DL)::value) gload(sl + 2);
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int mt = 0; mt < WM; mt++) acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh1[t], ah[mt], acc[t][mt], 0, 0, 0);
            __syncthreads();
            return;
        }
#pragma unroll
        for (int mt = 0; mt < WM; mt++) {
            const float* xr = &Xs[(16 * WM * wave + 16 * mt + li) * PW_LS + 4 * kq];
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(xr), x1 = *reinterpret_cast<const f32x4*>(xr + 16);
            bx3_split8(x0, x1, &ah[mt], &am[mt], &al[mt]);
        }
        u32x4 wfr[2][3];
#pragma unroll
        for (int pl3 = 0; pl3 < 3; pl3++) wfr[0][pl3] = Wl[(pl3 * 4 + kq) * (NT * 16) + li];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (t + 1 < NT) {
#pragma unroll
                for (int pl3 = 0; pl3 < 3; pl3++) wfr[(t + 1) & 1][pl3] = Wl[(pl3 * 4 + kq) * (NT * 16) + 16 * (t + 1) + li];
            }
            const bf16x8 wh = __builtin_bit_cast(bf16x8, wfr[t & 1][0]);
            const bf16x8 wm = __builtin_bit_cast(bf16x8, wfr[t & 1][1]);
            const bf16x8 wl = __builtin_bit_cast(bf16x8, wfr[t & 1][2]);
            if (t == 0 && decltype(DS)::value) lstore(nxt);
            if (t == NT - 1 && decltype(DL)::value) gload(sl + 2);
#pragma unroll
            for (int mt = 0; mt < WM; mt++) acc[t][mt] = bx3_mfma6(acc[t][mt], wh, wm, wl, ah[mt], am[mt], al[mt]);
        }
        __syncthreads();
    };
    int sl = 0;
    for (; sl + 2 < nslab; sl++) slab(sl, std::true_type{}, std::true_type{});
    if (nslab >= 2) { slab(sl, std::true_type{}, std::false_type{}); sl++; }
    slab(sl, std::false_type{}, std::false_type{});

    pw_epilogue<NT, WM>(p, acc, lds, m0, n0);
}
static size_t bx3p_lds_bytes(int nt, int wm) { return 2 * ((size_t)64 * wm * PW_LS + (size_t)12 * nt * 16 * 4) * sizeof(float); }
bool pw_bx3p_ok(int nt, int wm, int K) { return pw_bx3_ok(K) && K > PW_BK && bx3p_lds_bytes(nt, wm) <= 80 * 1024; }

// Plan-time weight image for k_pw_bx3: W [N][K] fp32 -> uint16 [ceil(K/32) slabs][3 planes][4 kq][Npad rows][8], Npad = N rounded
// up to 16 (rows beyond N are zeros), the 8 values of a (row, kq) slot being k = 32 s + 4 kq + (0..3) and 32 s + 16 + 4 kq + (0..3);
// a K tail (K % 32 != 0, K % 4 == 0) is zero weights against zero-filled operand columns.
bool pw_bx3_ok(int K) { return K >= 16 && K % 4 == 0; }
int pw_bx3_npad(int N) { return (N + 15) / 16 * 16; }
std::vector<uint16_t> pw_bx3_image(const float* W, int N, int K) {
    const int Npad = pw_bx3_npad(N), nslab = (K + PW_BK - 1) / PW_BK;
    std::vector<uint16_t> img((size_t)nslab * 12 * Npad * 8, 0);
    for (int n = 0; n < N; n++)
        for (int k = 0; k < K; k++) {
            uint16_t piece[3];
            bx3_split_host(W[(size_t)n * K + k], piece);
            const int s = k / PW_BK, kk = k % PW_BK, half = kk / 16, kq = (kk % 16) / 4, j = half * 4 + (kk % 4);
            for (int pl = 0; pl < 3; pl++)
                img[((((size_t)s * 3 + pl) * 4 + kq) * Npad + n) * 8 + j] = piece[pl];
        }
    return img;
}

void launch_pw_bx3(const PwParams& p, const uint16_t* Wimg, hipStream_t s) {
    if (!(p.sw & (PW_SW_B16_FORCE | PW_SW_B16S_FORCE | PW_SW_WS_FORCE)) && pw_lat_ok(p)) { launch_pw_lat(p, Wimg, pw_bx3_npad(p.N), s); return; }   // small calls, long K (same bits; a parity test's forced kernel goes first)
    if ((p.wm == 11 || (p.sw & PW_SW_B16S_FORCE)) && pw_b16s_ok(p)) { launch_pw_b16s(p, Wimg, pw_bx3_npad(p.N), s); return; }   // skinny layers: weights in registers
    if (((p.wm == 12 && pw_ws_fills(p)) || (p.sw & PW_SW_WS_FORCE)) && pw_ws_ok(p)) { launch_pw_ws(p, Wimg, pw_bx3_npad(p.N), s); return; }   // short K, wide N: weight columns in LDS
    // (a layer tuned onto one of those forms whose call is too small for it - a few clips - takes a tiled kernel: same bits)
    int nt = (p.nt >= 1 && p.nt <= 8) ? p.nt : pw_default_nt(p.M, p.N);
    int wm = (p.wm == 5 || p.wm == 7 || p.wm == 10) ? 1 : 2;   // PwParams::wm 5 / 6: 64- / 128-row tiles on the split-bf16 kernel, 7 / 8: pipelined,
                                                           // 10 / 9: 64- / 128-row tiles on k_pw_b16 (pw_b16.hip; one-product engines: 128 only)
    bool pipe = (p.wm == 7 || p.wm == 8) && pw_bx3p_ok(nt, wm, p.K);
    PwGrid g = pw_grid(p.M, p.N, nt, wm);
    if (pw_fill_grid(p.M, p.N, &nt, &wm, &g)) pipe = false;
    const int Npad = pw_bx3_npad(p.N);
    // "precision":"bf16" engines: 128-row tiles run on the kernel built for one product per operand fragment (pw_b16.hip) -
    // the same arithmetic, A straight from global memory into fragments
    if ((p.wm == 9 || p.wm == 10 || (p.sw & PW_SW_B16_FORCE)) && (wm == 2 || p.prec == 0) && pw_b16_ok(p.prec, p.K, p.sw, p.a_bf16)) {
        launch_pw_b16(p, Wimg, nt, wm, Npad, g.nblk_n, g.nblk, s);
        return;
    }
    const FDiv dn = make_fdiv((unsigned)g.nblk_n), dhw = make_fdiv((unsigned)std::max(p.HW, 1));
    const size_t ldsb = bx3p_lds_bytes(nt, wm);
    pw_dispatch<8, true>(nt, p.ascale != nullptr, wm, [&](auto NT, auto SC, auto WM) {
        constexpr int NT_ = decltype(NT)::value, WM_ = decltype(WM)::value;
        constexpr bool SC_ = decltype(SC)::value;
        if (pipe) {
            lds_limit_once<&k_pw_bx3p<NT_, SC_, WM_>>(80 * 1024);
            hipLaunchKernelGGL((k_pw_bx3p<NT_, SC_, WM_>), dim3(g.nblk), dim3(256), ldsb, s, p, Wimg, Npad, g.nblk_n, g.nblk, dn, dhw);
        } else {
            hipLaunchKernelGGL((k_pw_bx3<NT_, SC_, WM_>), dim3(g.nblk), dim3(256), 0, s, p, Wimg, Npad, g.nblk_n, g.nblk, dn, dhw);
        }
    });
}

}  // namespace bnhip
