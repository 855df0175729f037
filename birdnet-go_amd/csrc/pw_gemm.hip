// gfx950 pointwise / dense GEMM in fp32 on the f32-input MFMA (k_pw_gemm, its software-pipelined form k_pw_pipe, the implicit-GEMM
// convolution, the scalar fallback), the tile choice and the grid-fill rule of the whole pointwise family.
#include "kernels.h"
#include "pw_common.h"

#include <algorithm>
#include <type_traits>
#include <cstdlib>

namespace bnhip {

// ------------------------------------------------------------------------------------------ pointwise GEMM
// out[M,N] = act(A[M,K] * W[N,K]^T + bias[N]) (+ res[M,N]); optional per-(batch,k) scale on A (squeeze-excite
// MUL folded into the consumer's operand load).  f32 MFMA 16x16x4 with the roles swapped (W rows feed
// the MFMA "A" side, activation rows the "B" side) so each lane ends up holding 4 consecutive output
// channels of one row -> one 16-byte store per tile.
// Block 128 rows x (16*NT) cols, 4 waves, wave w owns rows [32w,32w+32).  BK = 32, LDS row stride 40 floats:
// with ds_read_b128 fragment loads the (row*10 + kq) 16-byte slot pattern is conflict-free for every
// 16-lane service group.  K is consumed in permuted order inside each 16-wide slab (lane kq holds
// k = 4kq..4kq+3, MFMA step s pairs element s of both operands) - a fixed reordering of the fp32 sum.
// PW_TRACE (tools/ubench/pw_trace.hip only): lane 0 of every wave of the first 64 logical blocks stamps the shader clock at
// the phase boundaries of each K slab, to see where a wave's time goes.  Compiled out of the library.
#ifdef PW_TRACE
__device__ long long* g_pw_trace = nullptr;      // [64 blocks][4 waves][PW_TRACE_SLOTS]
#define PW_TRACE_SLOTS 128
#define PW_T(i) do { if (lane == 0 && L < 64u && (i) < PW_TRACE_SLOTS && !((i) >= 60 && (i) < 64)) g_pw_trace[((size_t)L * 4 + wave) * PW_TRACE_SLOTS + (i)] = clock64(); } while (0)
#else
#define PW_T(i) do { } while (0)
#endif
// IM (implicit GEMM): the same kernel as a general convolution.  A is never materialised: row m is output pixel
// (b, oh, ow), column k = (i * kw + j) * Cin + ci is input value x[b][oh s - pt + i d][ow s - pl + j d][ci] (zero outside the
// image), and the file's OHWI weights are already the [N][K] matrix.  Cin % 4 == 0, so a float4 of K never straddles a tap.
struct ImGeo {
    int H, W, Cin, kw, sh, sw, dh, dw, pt, pl, Wo;
    FDiv d_cin, d_kw, d_wo, d_howo;      // k -> tap, tap -> row, pixel -> (oh, ow), m -> clip
};
template <int NT, bool SC, int WM, bool IM = false>
__global__ __launch_bounds__(256) void k_pw_gemm(PwParams p, int nblk_n, unsigned nblk, FDiv dn, FDiv dhw, ImGeo g) {
    constexpr int BM = 64 * WM;                  // rows per block: 4 waves x (16*WM) rows
    constexpr int XQ = BM * PW_C4 / 256;         // float4 per thread for the activation tile
    // operand tiles (the epilogue re-uses the array as per-wave output staging).  SC: squeeze-excite scale on A.
    constexpr int TILE = (BM + NT * 16) * PW_LS;
    // the epilogue stages 4 waves x 16 rows x (16 NT + 4) floats through the same array: with 64-row tiles and NT >= 7
    // that is MORE than the operand tile (found by bench.py's batch-vs-small-batch check when the work-based tuner first
    // picked <7, *, 1>: rows of neighbouring waves overwrote each other)
    constexpr int STG = 4 * 16 * (NT * 16 + 4);
    constexpr int LDSN = TILE > STG ? TILE : STG;
    __shared__ __attribute__((aligned(16))) float lds[LDSN];
    constexpr int WQ = (NT * 16 * PW_C4 + 255) / 256;   // float4 per thread for the W tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    // XCD-aware order: N-blocks fastest so the blocks that share an activation tile sit on one XCD's L2
    const unsigned L = xcd_remap(blockIdx.x, nblk);
    const int mblk = (int)fdiv(L, dn);
    const int m0 = mblk * BM;
    const int n0 = ((int)L - mblk * nblk_n) * (NT * 16);
    const int K = p.K;

    float4 xreg[XQ], wreg[WQ], sreg[SC ? XQ : 1];
    int srow[SC ? XQ : 1];                        // batch index of each staged row (for the per-(batch,k) scale)
    if (SC) {
#pragma unroll
        for (int q = 0; q < XQ; q++) {
            int m = m0 + ((tid + 256 * q) / PW_C4);
            srow[SC ? q : 0] = (int)fdiv((unsigned)(m < p.M ? m : 0), dhw);
        }
    }
    // IM: top-left input coordinate and image base of each staged row (fixed for the block)
    int ih0[IM ? XQ : 1], iw0[IM ? XQ : 1]; unsigned ibase[IM ? XQ : 1];
    if (IM) {
#pragma unroll
        for (int q = 0; q < XQ; q++) {
            const unsigned m = (unsigned)min(m0 + (tid + 256 * q) / PW_C4, p.M - 1);
            const unsigned b = fdiv(m, g.d_howo), pix = m - b * g.d_howo.d;
            const unsigned oh = fdiv(pix, g.d_wo), ow = pix - oh * (unsigned)g.Wo;
            ih0[IM ? q : 0] = (int)oh * g.sh - g.pt; iw0[IM ? q : 0] = (int)ow * g.sw - g.pl;
            ibase[IM ? q : 0] = b * (unsigned)(g.H * g.W);
        }
    }
    // all global loads of a slab are issued back-to-back (scale included); the multiply happens at LDS-store time
    auto gload = [&](int k0) {
#pragma unroll
        for (int q = 0; q < XQ; q++) {
            int idx = tid + 256 * q;
            int row = idx / PW_C4, c4 = idx % PW_C4;
            int m = m0 + row, k = k0 + 4 * c4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f), sc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (IM) {
                if (m < p.M && k < K) {
                    const unsigned tap = fdiv((unsigned)k, g.d_cin), ci = (unsigned)k - tap * (unsigned)g.Cin;
                    const unsigned ti = fdiv(tap, g.d_kw), tj = tap - ti * (unsigned)g.kw;
                    const int ih = ih0[IM ? q : 0] + (int)ti * g.dh, iw = iw0[IM ? q : 0] + (int)tj * g.dw;
                    if (ih >= 0 && ih < g.H && iw >= 0 && iw < g.W)
                        v = *reinterpret_cast<const float4*>(p.A + ((size_t)ibase[IM ? q : 0] + (size_t)ih * g.W + iw) * g.Cin + ci);
                }
            } else if (m < p.M && k < K) {
                v = *reinterpret_cast<const float4*>(p.A + (size_t)m * K + k);
                if (SC) sc = *reinterpret_cast<const float4*>(p.ascale + (size_t)srow[SC ? q : 0] * K + k);
            }
            xreg[q] = v;
            if (SC) sreg[SC ? q : 0] = sc;
        }
#pragma unroll
        for (int q = 0; q < WQ; q++) {
            int idx = tid + 256 * q;
            int row = idx / PW_C4, c4 = idx % PW_C4;
            int n = n0 + row, k = k0 + 4 * c4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < NT * 16 && n < p.N && k < K) v = *reinterpret_cast<const float4*>(p.W + (size_t)n * K + k);
            wreg[q] = v;
        }
    };
    auto lstore = [&]() {
        float* Xs = lds;
        float* Ws = Xs + BM * PW_LS;
#pragma unroll
        for (int q = 0; q < XQ; q++) {
            int idx = tid + 256 * q;
            float4 v = xreg[q];
            if (SC) { float4 sc = sreg[SC ? q : 0]; v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
            *reinterpret_cast<float4*>(&Xs[(idx / PW_C4) * PW_LS + 4 * (idx % PW_C4)]) = v;
        }
#pragma unroll
        for (int q = 0; q < WQ; q++) {
            int idx = tid + 256 * q;
            if ((idx / PW_C4) < NT * 16) *reinterpret_cast<float4*>(&Ws[(idx / PW_C4) * PW_LS + 4 * (idx % PW_C4)]) = wreg[q];
        }
    };

    f32x4 acc[NT][WM];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int mt = 0; mt < WM; mt++) acc[t][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // one operand buffer (double-buffering measured neutral on this chip for these shapes; the pipelined form is k_pw_pipe):
    // slab s computes from LDS while slab s+1's global loads are in flight in registers; two barriers per slab.
    const int nslab = (K + PW_BK - 1) / PW_BK;
    PW_T(0);
    gload(0);
    lstore();
    if (nslab > 1) gload(PW_BK);
    __syncthreads();
    PW_T(1);
    for (int sl = 0; sl < nslab; sl++) {
        PW_T(4 + 4 * sl);
        const float* Xs = lds;
        const float* Ws = Xs + BM * PW_LS;
#pragma unroll
        for (int t16 = 0; t16 < PW_BK / 16; t16++) {
            f32x4 xf[WM], wf[NT];
#pragma unroll
            for (int mt = 0; mt < WM; mt++)
                xf[mt] = *reinterpret_cast<const f32x4*>(&Xs[(16 * WM * wave + 16 * mt + li) * PW_LS + 16 * t16 + 4 * kq]);
#pragma unroll
            for (int t = 0; t < NT; t++)
                wf[t] = *reinterpret_cast<const f32x4*>(&Ws[(16 * t + li) * PW_LS + 16 * t16 + 4 * kq]);
#pragma unroll
            for (int sidx = 0; sidx < 4; sidx++) {
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int mt = 0; mt < WM; mt++)
                        acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[t][sidx], xf[mt][sidx], acc[t][mt], 0, 0, 0);
            }
        }
        PW_T(5 + 4 * sl);                      // MFMAs issued
        if (sl + 1 < nslab) {
            __syncthreads();                   // single buffer: everyone must be done reading it
            PW_T(6 + 4 * sl);                  // all waves done with the slab
#ifdef PW_TRACE
            __builtin_amdgcn_s_waitcnt(0x0f70);    // vmcnt(0): the next slab's global loads have landed
            PW_T(64 + 2 * sl);
#endif
            lstore();
#ifdef PW_TRACE
            __builtin_amdgcn_s_waitcnt(0xc07f);    // lgkmcnt(0): LDS stores done
            PW_T(65 + 2 * sl);
#endif
            if (sl + 2 < nslab) gload((sl + 2) * PW_BK);
            PW_T(7 + 4 * sl);                  // next slab stored (its global loads had landed), slab + 2 requested
        }
        __syncthreads();
    }
    PW_T(2);

    pw_epilogue<NT, WM>(p, acc, lds, m0, n0);
    PW_T(3);
}

// Software-pipelined variant for K % PW_BK == 0.  The phase trace of k_pw_gemm (tools/ubench/pw_trace.hip) shows a wave
// spending only ~1/3 of a slab period issuing MFMAs: the rest is two barrier waits and the refill of the single operand
// buffer, whose address VALU, LDS stores and global-load issue crawl because they compete with the other waves' MFMAs
// for issue slots.  Here the refill rides in the wave's OWN MFMA shadow instead: two LDS operand buffers, the stores of
// slab s+1 are interleaved with the MFMAs of the first half of slab s and the global loads of slab s+2 with those of the
// second half (sched_group_barrier), one barrier per slab.  All per-slab address arithmetic is gone: loads use per-thread
// offsets computed once (rows clamped into range: out-of-range rows produce values the epilogue never stores) plus k0.
template <int NT, bool SC, int WM>
__global__ __launch_bounds__(256) void k_pw_pipe(PwParams p, int nblk_n, unsigned nblk, FDiv dn, FDiv dhw) {
    constexpr int BM = 64 * WM;
    constexpr int XQ = BM * PW_C4 / 256, WQ = (NT * 16 * PW_C4 + 255) / 256;
    constexpr int TILE = (BM + NT * 16) * PW_LS;
    __shared__ __attribute__((aligned(16))) float lds[2 * TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const unsigned L = xcd_remap(blockIdx.x, nblk);
    const int mblk = (int)fdiv(L, dn);
    const int m0 = mblk * BM;
    const int n0 = ((int)L - mblk * nblk_n) * (NT * 16);
    const int K = p.K;

    unsigned xoff[XQ], soff[SC ? XQ : 1], woff[WQ];
    // LDS store slots: thread idx = tid + 256 q -> row idx / PW_C4, k-quad idx % PW_C4 (256 / PW_C4 rows further per q)
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
        const int idx = tid + 256 * q, row = min(idx / PW_C4, NT * 16 - 1), c4 = idx % PW_C4;
        woff[q] = (unsigned)min(n0 + row, p.N - 1) * (unsigned)K + 4 * c4;
    }
    float4 xreg[XQ], wreg[WQ], sreg[SC ? XQ : 1];
    auto gload = [&](int k0) {
        const float* Ak = p.A + k0;
        const float* Wk = p.W + k0;
#pragma unroll
        for (int q = 0; q < XQ; q++) {
            xreg[q] = *reinterpret_cast<const float4*>(Ak + xoff[q]);
            if (SC) sreg[SC ? q : 0] = *reinterpret_cast<const float4*>(p.ascale + k0 + soff[SC ? q : 0]);
        }
#pragma unroll
        for (int q = 0; q < WQ; q++) wreg[q] = *reinterpret_cast<const float4*>(Wk + woff[q]);
    };
    auto lstore = [&](float* buf) {
#pragma unroll
        for (int q = 0; q < XQ; q++) {
            float4 v = xreg[q];
            if (SC) { const float4 sc = sreg[SC ? q : 0]; v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
            *reinterpret_cast<float4*>(&buf[lbase + q * LQ]) = v;
        }
#pragma unroll
        for (int q = 0; q < WQ; q++)
            if ((NT * 16 * PW_C4) % 256 == 0 || (tid + 256 * q) / PW_C4 < NT * 16)
                *reinterpret_cast<float4*>(&buf[BM * PW_LS + lbase + q * LQ]) = wreg[q];
    };

    f32x4 acc[NT][WM];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int mt = 0; mt < WM; mt++) acc[t][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nslab = K / PW_BK;
    gload(0);
    lstore(lds);
    if (nslab > 1) gload(PW_BK);
    __syncthreads();
    // one slab: DS = also store slab sl + 1 (held in registers) into the other buffer, DL = also request slab sl + 2
    auto slab = [&](int sl, auto DS, auto DL) {
        const float* Xs = lds + (sl & 1) * TILE;
        const float* Ws = Xs + BM * PW_LS;
        float* nxt = lds + ((sl + 1) & 1) * TILE;
#pragma unroll
        for (int t16 = 0; t16 < PW_BK / 16; t16++) {
            f32x4 xf[WM], wf[NT];
#pragma unroll
            for (int mt = 0; mt < WM; mt++)
                xf[mt] = *reinterpret_cast<const f32x4*>(&Xs[(16 * WM * wave + 16 * mt + li) * PW_LS + 16 * t16 + 4 * kq]);
#pragma unroll
            for (int t = 0; t < NT; t++)
                wf[t] = *reinterpret_cast<const f32x4*>(&Ws[(16 * t + li) * PW_LS + 16 * t16 + 4 * kq]);
            if (t16 == 0 && decltype(DS)::value) lstore(nxt);
            if (t16 == PW_BK / 16 - 1 && decltype(DL)::value) gload((sl + 2) * PW_BK);
#pragma unroll
            for (int sidx = 0; sidx < 4; sidx++) {
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int mt = 0; mt < WM; mt++)
                        acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[t][sidx], xf[mt][sidx], acc[t][mt], 0, 0, 0);
            }
            // interleave: fragment reads first, then the refill instructions spread between the MFMAs
            constexpr int NMF = 4 * NT * WM, NREF = XQ + WQ, STEP = NMF / (NREF + 1) > 0 ? NMF / (NREF + 1) : 1;
            __builtin_amdgcn_sched_group_barrier(0x100, WM + NT, 0);
            if (t16 == 0 && decltype(DS)::value) {
#pragma unroll
                for (int r = 0; r < NREF; r++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, STEP, 0);
                    if (SC) __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                }
            }
            if (t16 == PW_BK / 16 - 1 && decltype(DL)::value) {
#pragma unroll
                for (int r = 0; r < NREF + (SC ? XQ : 0); r++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, SC ? 1 : STEP, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
            }
        }
        __syncthreads();
    };
    int sl = 0;
    for (; sl + 2 < nslab; sl++) slab(sl, std::true_type{}, std::true_type{});
    if (nslab >= 2) { slab(sl, std::true_type{}, std::false_type{}); sl++; }
    slab(sl, std::false_type{}, std::false_type{});

    pw_epilogue<NT, WM>(p, acc, lds, m0, n0);
}

// scalar fallback for K not a multiple of 4 (never hit by EfficientNet-style graphs; kept for drop-in safety)
__global__ void k_pw_naive(PwParams p) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)p.M * p.N) return;
    int n = (int)(idx % p.N);
    size_t m = idx / p.N;
    float acc = 0.f;
    for (int k = 0; k < p.K; k++) {
        float a = p.A[m * p.K + k];
        if (p.ascale) a *= p.ascale[(m / p.HW) * p.K + k];
        acc = fmaf(a, p.W[(size_t)n * p.K + k], acc);
    }
    if (p.bias) acc += p.bias[n];
    acc = apply_act(acc, p.act);
    if (p.res) acc += p.res[idx];
    p.out[idx] = acc;
}

// Tile-width choice.  Measured on MI355X (tests/micro sweep, late-layer shapes at batch 256): NT <= 4 keeps
// the kernel at <= 112 VGPRs (4 waves/SIMD) and beats the wider tiles (134-158 VGPRs, 2 waves/SIMD) by
// 10-45 % even where they pad less, so: widest NT in 1..4 whose padded width is within 15 % of the best.
// k_pw_pipe needs whole K slabs and both operand buffers inside the 64 KB of static LDS
bool pw_pipe_ok(int nt, int wm, int K) { return K % PW_BK == 0 && nt >= 1 && nt <= 4 && 2 * (64 * wm + 16 * nt) * PW_LS * 4 <= 64 * 1024; }
static int pick_nt(int M, int N) {
    (void)M;
    long best_cols = -1;
    for (int nt = 1; nt <= 4; nt++) {
        long cols = (long)((N + nt * 16 - 1) / (nt * 16)) * nt * 16;
        if (best_cols < 0 || cols < best_cols) best_cols = cols;
    }
    int best = 1;
    for (int nt = 1; nt <= 4; nt++) {
        long cols = (long)((N + nt * 16 - 1) / (nt * 16)) * nt * 16;
        if (cols * 100 <= best_cols * 115) best = nt;
    }
    static const int ov = getenv("BNHIP_PW_NT") ? atoi(getenv("BNHIP_PW_NT")) : 0;      // experiment switch
    if (ov >= 1 && ov <= 8) best = ov;
    return best;
}

int pw_default_nt(int M, int N) { return pick_nt(M, N); }

// The tile of a contraction is tuned at batch size.  A call with fewer clips (one clip per Predict; the 64-clip chunks of a
// blocking 256-clip host call) can leave most of the 256 CUs without a workgroup with that tile: shrink it - 64-row tiles first,
// then narrower column tiles - until the grid has at least one workgroup per CU or the smallest tile is reached.  Pipelined
// kernel forms keep their own constraints, so they fall back to the plain form when the tile changes.
bool pw_fill_grid(int M, int N, int* nt, int* wm, PwGrid* g) {
    static const int target_env = getenv("BNHIP_PW_FILL") ? atoi(getenv("BNHIP_PW_FILL")) : -1;
    const int target = target_env >= 0 ? target_env : device_cus();
    bool changed = false;
    while ((int)g->nblk < target && (*wm > 1 || *nt > 1)) {
        if (*wm > 1) *wm = 1;
        else *nt = (*nt + 1) / 2;
        changed = true;
        *g = pw_grid(M, N, *nt, *wm);
    }
    return changed;
}

void launch_pw_gemm(const PwParams& p, hipStream_t s) {
    if ((p.K & 3) != 0) {
        size_t total = (size_t)p.M * p.N;
        hipLaunchKernelGGL(k_pw_naive, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
        return;
    }
    int nt = (p.nt >= 1 && p.nt <= 8) ? p.nt : pick_nt(p.M, p.N);
    // wm 3 / 4 = the software-pipelined kernel with 64 / 128-row tiles (needs whole K slabs and nt <= 4)
    static const int wm_env = getenv("BNHIP_PW_WM") ? atoi(getenv("BNHIP_PW_WM")) : 0;      // test switch: force the row tile / kernel
    const int wm_req = wm_env >= 1 && wm_env <= 4 ? wm_env : p.wm;
    bool pipe = (wm_req == 3 || wm_req == 4) && pw_pipe_ok(nt, wm_req - 2, p.K);
    int wm = (wm_req == 1 || wm_req == 3) ? 1 : 2;
    PwGrid g = pw_grid(p.M, p.N, nt, wm);
    // the tile was tuned at batch size; a call with a handful of clips would leave most CUs idle with it (one clip:
    // 1-5 workgroups each walking the whole K loop): fall back to the smallest tile to get workgroups
    static const bool forced = getenv("BNHIP_PW_NT") != nullptr || getenv("BNHIP_PW_WM") != nullptr;   // tests pin the tile
    if (!forced && pw_fill_grid(p.M, p.N, &nt, &wm, &g)) pipe = false;
    const FDiv dn = make_fdiv((unsigned)g.nblk_n), dhw = make_fdiv((unsigned)std::max(p.HW, 1));
    const bool sc = p.ascale != nullptr;
    if (pipe) {
        pw_dispatch<4, true>(nt, sc, wm, [&](auto NT, auto SC, auto WM) {
            hipLaunchKernelGGL((k_pw_pipe<decltype(NT)::value, decltype(SC)::value, decltype(WM)::value>), dim3(g.nblk), dim3(256), 0, s, p, g.nblk_n,
                               g.nblk, dn, dhw);
        });
        return;
    }
    pw_dispatch<8, true>(nt, sc, wm, [&](auto NT, auto SC, auto WM) {
        hipLaunchKernelGGL((k_pw_gemm<decltype(NT)::value, decltype(SC)::value, decltype(WM)::value>), dim3(g.nblk), dim3(256), 0, s, p, g.nblk_n,
                           g.nblk, dn, dhw, ImGeo{});
    });
}

// General convolution as an implicit GEMM on the f32 MFMA (k_pw_gemm<.., IM = true>): any kernel size, stride, dilation and
// explicit top / left padding, Cin % 4 == 0.  Weights are the file's OHWI tensor as it is.  Bias, activation and the output
// burst are the pointwise kernel's epilogue.
bool conv_igemm_supported(int Cin, int Cout, int kh, int kw) { return (Cin & 3) == 0 && Cin >= 4 && kh * kw * Cin >= 32 && Cout >= 1; }
void launch_conv_igemm(const float* in, const float* w_ohwi, const float* bias, float* out, int B, int H, int W, int Cin, int Ho, int Wo,
                       int Cout, int kh, int kw, int sh, int sw, int dh, int dw, int pt, int pl, int act, int nt_req, int wm_req,
                       hipStream_t s) {
    PwParams p{in, w_ohwi, bias, nullptr, nullptr, out, B * Ho * Wo, Cout, kh * kw * Cin, Ho * Wo, act, nt_req, wm_req};
    int nt = (p.nt >= 1 && p.nt <= 8) ? p.nt : pick_nt(p.M, p.N);
    int wm = p.wm == 1 ? 1 : 2;
    PwGrid gr = pw_grid(p.M, p.N, nt, wm);
    if (gr.nblk < 64 && (nt > 1 || wm > 1)) {
        nt = 1; wm = 1;
        gr = pw_grid(p.M, p.N, nt, wm);
    }
    ImGeo g{H, W, Cin, kw, sh, sw, dh, dw, pt, pl, Wo, make_fdiv((unsigned)Cin), make_fdiv((unsigned)kw), make_fdiv((unsigned)Wo),
            make_fdiv((unsigned)(Ho * Wo))};
    const FDiv dn = make_fdiv((unsigned)gr.nblk_n), dhw = make_fdiv((unsigned)std::max(p.HW, 1));
    pw_dispatch<8, false>(nt, false, wm, [&](auto NT, auto, auto WM) {
        hipLaunchKernelGGL((k_pw_gemm<decltype(NT)::value, false, decltype(WM)::value, true>), dim3(gr.nblk), dim3(256), 0, s, p, gr.nblk_n, gr.nblk,
                           dn, dhw, g);
    });
}

}  // namespace bnhip
