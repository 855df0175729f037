// gfx950 depthwise convolution (register-tiled, with the fused squeeze-excite sums), spatial mean and the squeeze-excite block.
#include "kernels.h"
#include "pw_common.h"

#include <algorithm>
#include <cstdlib>

namespace bnhip {

// ------------------------------------------------------------------------------------------ depthwise conv
// Register-tiled depthwise conv: a thread owns 4 channels x (TH x TW) output pixels, so each input
// row segment it loads is reused across the TW horizontal and up to K vertical taps (HBM/L2 traffic per
// output drops from K*K loads to ~((TH-1)S+K)((TW-1)S+K)/(TH*TW)).  Threads are laid out channel-fastest
// (coalesced float4), tiles row-major; blocks are XCD-remapped so vertically adjacent tiles of a clip share an
// L2.  Optionally emits deterministic per-block channel sums for the squeeze-excite mean (no second pass over
// the tensor, no float atomics): partial[b][tile_chunk][c].
// IN16 (bf16 activation storage on the input): the thread's whole input patch - RH x RW quads of 8 bytes - is requested before
// the first tap is applied, so a block pays one memory round trip instead of one per input row (the row loop otherwise issues
// RW loads, waits, multiplies, and only then issues the next row's: b1 / b2 of the Perch stack ran at 2.0 / 3.2 TB/s).
template <int K, int S, int TH, int TW, bool IN16 = false>
__global__ __launch_bounds__(256) void k_dwconv_t(DwParams p, int CX, int PY, int tiles_w, int tiles, int tchunks,
                                                  int cchunks, unsigned nblk, float* __restrict__ partial) {
    __shared__ float red[256 * 4];
    const unsigned L = xcd_remap(blockIdx.x, nblk);
    const int bpc = tchunks * cchunks;
    const int b = L / bpc;
    const int rest = L % bpc;
    const int tc = rest / cchunks, cc = rest % cchunks;
    const int tx = threadIdx.x % CX, ty = threadIdx.x / CX;
    const int c4 = cc * CX + tx;
    const int C4 = p.C >> 2;
    const int tile = tc * PY + ty;
    const bool live = c4 < C4 && tile < tiles && ty < PY;
    float4 acc[TH][TW];
#pragma unroll
    for (int a = 0; a < TH; a++)
#pragma unroll
        for (int c = 0; c < TW; c++) acc[a][c] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int th0 = live ? (tile / tiles_w) * TH : 0, tw0 = live ? (tile % tiles_w) * TW : 0;
    if (live) {
        constexpr int RW = (TW - 1) * S + K;       // input columns per row segment
        constexpr int RH = (TH - 1) * S + K;       // input rows
        const int hi0 = th0 * S - p.pt, wi0 = tw0 * S - p.pl;
        const float4* in4 = reinterpret_cast<const float4*>(p.in) + (size_t)b * p.H * p.W * C4 + c4;
        const float4* w4 = reinterpret_cast<const float4*>(p.w) + c4;
        uint2 raw[IN16 ? RH : 1][IN16 ? RW : 1];
        if constexpr (IN16) {
            const uint2* in2 = reinterpret_cast<const uint2*>(p.in) + (size_t)b * p.H * p.W * C4 + c4;
#pragma unroll
            for (int r = 0; r < RH; r++)
#pragma unroll
                for (int c = 0; c < RW; c++) {
                    const int hi = hi0 + r, wi = wi0 + c;
                    const bool in = hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
                    raw[r][c] = in ? in2[((size_t)hi * p.W + wi) * C4] : make_uint2(0u, 0u);
                }
        }
#pragma unroll
        for (int r = 0; r < RH; r++) {
            const int hi = hi0 + r;
            if (hi < 0 || hi >= p.H) continue;
            float4 x[RW];
#pragma unroll
            for (int c = 0; c < RW; c++) {
                int wi = wi0 + c;
                if constexpr (IN16) {
                    const uint2 rr = raw[r][c];
                    x[c] = make_float4(__uint_as_float(rr.x << 16), __uint_as_float(rr.x & 0xffff0000u), __uint_as_float(rr.y << 16), __uint_as_float(rr.y & 0xffff0000u));
                } else if (!(wi >= 0 && wi < p.W)) x[c] = make_float4(0.f, 0.f, 0.f, 0.f);
                else if (p.in_bf16) x[c] = bf16x4_load(p.in, ((size_t)b * p.H * p.W + (size_t)hi * p.W + wi) * C4 + c4);
                else x[c] = in4[((size_t)hi * p.W + wi) * C4];
            }
#pragma unroll
            for (int a = 0; a < TH; a++) {
                const int i = r - a * S;            // kernel row feeding output row a from input row r
                if (i < 0 || i >= K) continue;
#pragma unroll
                for (int j = 0; j < K; j++) {
                    const float4 w = w4[(size_t)(i * K + j) * C4];
#pragma unroll
                    for (int c = 0; c < TW; c++) {
                        const float4 xv = x[c * S + j];
                        acc[a][c].x = fmaf(xv.x, w.x, acc[a][c].x); acc[a][c].y = fmaf(xv.y, w.y, acc[a][c].y);
                        acc[a][c].z = fmaf(xv.z, w.z, acc[a][c].z); acc[a][c].w = fmaf(xv.w, w.w, acc[a][c].w);
                    }
                }
            }
        }
    }
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        float4 bv = p.bias ? reinterpret_cast<const float4*>(p.bias)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
        float4* out4 = reinterpret_cast<float4*>(p.out) + (size_t)b * p.Ho * p.Wo * C4 + c4;
        if (p.act == ACT_SWISH) {
#pragma unroll
            for (int a = 0; a < TH; a++)
#pragma unroll
                for (int c = 0; c < TW; c++) {
                    float4& v = acc[a][c];
                    const f32x4 r = swish4((f32x4){v.x + bv.x, v.y + bv.y, v.z + bv.z, v.w + bv.w});
                    v = make_float4(r[0], r[1], r[2], r[3]);
                }
        } else {
            with_act(p.act, [&](auto f) {
#pragma unroll
                for (int a = 0; a < TH; a++)
#pragma unroll
                    for (int c = 0; c < TW; c++) {
                        float4& v = acc[a][c];
                        v.x = f(v.x + bv.x); v.y = f(v.y + bv.y); v.z = f(v.z + bv.z); v.w = f(v.w + bv.w);
                    }
            });
        }
#pragma unroll
        for (int a = 0; a < TH; a++) {
            int ho = th0 + a;
            if (ho >= p.Ho) continue;
#pragma unroll
            for (int c = 0; c < TW; c++) {
                int wo = tw0 + c;
                if (wo >= p.Wo) continue;
                float4 v = acc[a][c];
                if (p.out_bf16) bf16x4_store(p.out, ((size_t)b * p.Ho * p.Wo + (size_t)ho * p.Wo + wo) * C4 + c4, v);
                else out4[((size_t)ho * p.Wo + wo) * C4] = v;
                sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
            }
        }
    }
    if (partial) {
        reinterpret_cast<float4*>(red)[threadIdx.x] = sum;
        __syncthreads();
        if (ty == 0 && c4 < C4) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int y = 0; y < PY; y++) {
                float4 v = reinterpret_cast<float4*>(red)[y * CX + tx];
                t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
            }
            reinterpret_cast<float4*>(partial)[((size_t)b * tchunks + tc) * C4 + c4] = t;
        }
    }
}

// generic fallback: thread = (output pixel, 4 or 1 channels)
template <int VEC>
__global__ __launch_bounds__(256) void k_dwconv(DwParams p) {
    const int CV = p.C / VEC;
    size_t total = (size_t)p.B * p.Ho * p.Wo * CV;
    size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    int cv = (int)(idx % CV);
    size_t pix = idx / CV;
    int wo = (int)(pix % p.Wo);
    int ho = (int)((pix / p.Wo) % p.Ho);
    int b = (int)(pix / ((size_t)p.Wo * p.Ho));
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; v++) acc[v] = 0.f;
    for (int i = 0; i < p.kh; i++) {
        int hi = ho * p.sh - p.pt + i;
        if (hi < 0 || hi >= p.H) continue;
        for (int j = 0; j < p.kw; j++) {
            int wi = wo * p.sw - p.pl + j;
            if (wi < 0 || wi >= p.W) continue;
            const float* ip = p.in + (((size_t)b * p.H + hi) * p.W + wi) * p.C + (size_t)cv * VEC;
            const float* wp = p.w + (size_t)(i * p.kw + j) * p.C + (size_t)cv * VEC;
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[v] = fmaf(ip[v], wp[v], acc[v]);
        }
    }
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        float x = acc[v];
        if (p.bias) x += p.bias[cv * VEC + v];
        p.out[idx * VEC + v] = apply_act(x, p.act);
    }
}

static void dw_geometry(const DwParams& p, int TH, int TW, int* CX, int* PY, int* tiles_w, int* tiles, int* tchunks,
                        int* cchunks) {
    int C4 = p.C / 4;
    *CX = C4 < 64 ? C4 : 64;
    *PY = 256 / *CX;
    *tiles_w = (p.Wo + TW - 1) / TW;
    *tiles = *tiles_w * ((p.Ho + TH - 1) / TH);
    if (*PY > *tiles) *PY = *tiles;
    *tchunks = (*tiles + *PY - 1) / *PY;
    *cchunks = (C4 + *CX - 1) / *CX;
}
static bool dw_tiled_shape(const DwParams& p, int* TH, int* TW) {
    if ((p.C & 3) || p.kh != p.kw || p.sh != p.sw) return false;
    if (p.kh == 3 && p.sh == 1) { *TH = 2; *TW = 4; return true; }
    if (p.kh == 3 && p.sh == 2) { *TH = 2; *TW = 2; return true; }
    if (p.kh == 5 && p.sh == 1) { *TH = 2; *TW = 4; return true; }
    if (p.kh == 5 && p.sh == 2) { *TH = 1; *TW = 2; return true; }
    return false;
}
int dwconv_sum_slabs(const DwParams& p) {
    int TH, TW, CX, PY, tw, t, tch, cch;
    if (!dw_tiled_shape(p, &TH, &TW)) return 0;
    dw_geometry(p, TH, TW, &CX, &PY, &tw, &t, &tch, &cch);
    return tch;
}
bool dwconv_tile_geometry(const DwParams& p, int* PY, int* tiles_w, int* tiles, int* tchunks) {
    int TH, TW, CX, cch;
    if (!dw_tiled_shape(p, &TH, &TW) || TH != 2 || TW != 4) return false;
    dw_geometry(p, TH, TW, &CX, PY, tiles_w, tiles, tchunks, &cch);
    return true;
}
void launch_dwconv(const DwParams& p, float* partial, hipStream_t s) {
    int TH, TW;
    if (dw_tiled_shape(p, &TH, &TW)) {
        int CX, PY, tiles_w, tiles, tchunks, cchunks;
        dw_geometry(p, TH, TW, &CX, &PY, &tiles_w, &tiles, &tchunks, &cchunks);
        unsigned nblk = (unsigned)p.B * tchunks * cchunks;
        dim3 block(CX * PY < 64 ? 64 : CX * PY);
        static const bool pre16 = !(getenv("BNHIP_DW_PREFETCH") && atoi(getenv("BNHIP_DW_PREFETCH")) == 0);
#define DW_LAUNCH(K_, S_, TH_, TW_) do { if (p.in_bf16 && pre16) hipLaunchKernelGGL((k_dwconv_t<K_, S_, TH_, TW_, true>), dim3(nblk), block, 0, s, p, CX, PY, \
                                                       tiles_w, tiles, tchunks, cchunks, nblk, partial); \
                                         else hipLaunchKernelGGL((k_dwconv_t<K_, S_, TH_, TW_>), dim3(nblk), block, 0, s, p, CX, PY, \
                                                       tiles_w, tiles, tchunks, cchunks, nblk, partial); } while (0)
        if (p.kh == 3 && p.sh == 1) DW_LAUNCH(3, 1, 2, 4);
        else if (p.kh == 3) DW_LAUNCH(3, 2, 2, 2);
        else if (p.sh == 1) DW_LAUNCH(5, 1, 2, 4);
        else DW_LAUNCH(5, 2, 1, 2);
#undef DW_LAUNCH
        return;
    }
    if ((p.C & 3) == 0) {
        size_t total = (size_t)p.B * p.Ho * p.Wo * (p.C / 4);
        hipLaunchKernelGGL(k_dwconv<4>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
    } else {
        size_t total = (size_t)p.B * p.Ho * p.Wo * p.C;
        hipLaunchKernelGGL(k_dwconv<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
    }
}

// ------------------------------------------------------------------------------------------ spatial mean
// Deterministic two-stage reduction (no float atomics): partial[b][s][c] = sum over the s-th pixel slab.
#define MEAN_SLAB 512
int mean_splits(int HW) { return (HW + MEAN_SLAB - 1) / MEAN_SLAB; }

__global__ __launch_bounds__(256) void k_mean_partial(const float* __restrict__ in, float* __restrict__ partial,
                                                      int HW, int C, int S) {
    __shared__ float red[256];
    const int b = blockIdx.z, sp = blockIdx.y;
    const int CW = blockDim.x, PY = blockDim.y;
    const int c = blockIdx.x * CW + threadIdx.x;
    const int p0 = sp * MEAN_SLAB, p1 = min(HW, p0 + MEAN_SLAB);
    float acc = 0.f;
    if (c < C)
        for (int px = p0 + threadIdx.y; px < p1; px += PY) acc += in[((size_t)b * HW + px) * C + c];
    red[threadIdx.y * CW + threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.y == 0 && c < C) {
        float sum = 0.f;
        for (int y = 0; y < PY; y++) sum += red[y * CW + threadIdx.x];
        partial[((size_t)b * S + sp) * C + c] = sum;
    }
}
int mean_partial_py(int C) {
    int CW = C < 64 ? C : 64;
    int PY = 256 / CW; if (PY < 1) PY = 1;
    return PY;
}
void launch_mean_partial(const float* in, float* partial, int B, int HW, int C, int S, hipStream_t s) {
    int CW = C < 64 ? C : 64;
    int PY = mean_partial_py(C);
    dim3 grid((C + CW - 1) / CW, S, B);
    hipLaunchKernelGGL(k_mean_partial, grid, dim3(CW, PY), 0, s, in, partial, HW, C, S);
}
__global__ void k_mean_finish(const float* __restrict__ partial, float* __restrict__ out, int B, int HW, int C, int S) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * C) return;
    int c = (int)(idx % C); size_t b = idx / C;
    float sum = 0.f;
    for (int sidx = 0; sidx < S; sidx++) sum += partial[(b * S + sidx) * C + c];
    out[idx] = sum / (float)HW;
}
void launch_mean_finish(const float* partial, float* out, int B, int HW, int C, int S, hipStream_t s) {
    size_t total = (size_t)B * C;
    hipLaunchKernelGGL(k_mean_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, partial, out, B, HW, C, S);
}

// ------------------------------------------------------------------------------------------ squeeze-excite
// One block (16 waves) per clip: mean -> FC(Cr)+act1 -> FC(C)+act2 -> scale[b][c].
// w1 [Cr][C] is read wave-per-output with coalesced rows; w2t is the second FC transposed to [Cr][C] at plan
// time so thread c reads it coalesced.  (Splitting a clip over 4 blocks that each redo mean+FC1 measured 2x slower:
// the pass over the per-slab sums dominates.)
__global__ __launch_bounds__(1024) void k_se(SeParams p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* mean = sm;            // [C]
    float* r = sm + p.C;         // [Cr]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NTHR = blockDim.x, NW = NTHR >> 6;      // block size is a launch parameter (see launch_se)
    const float inv = 1.0f / (float)p.HW;
    // the per-slab sums: P threads per channel walk interleaved slab subsets (a 96-slab layer with 96 channels used to
    // be 96 threads x 96 serial loads), then fold through LDS in a fixed order
    int P = 1;
    while (P * 2 * p.C <= NTHR && P * 2 <= p.S) P *= 2;
    float* part = sm + ((p.C + p.Cr + 3) & ~3);      // [P][C] / float4 [G][C/4] scratch, 16-byte aligned
    if (P > 1) {
        const int c = tid % p.C, q = tid / p.C;
        if (q < P) {
            float sum = 0.f;
#pragma unroll 4
            for (int sidx = q; sidx < p.S; sidx += P) sum += p.partial[((size_t)b * p.S + sidx) * p.C + c];
            part[q * p.C + c] = sum;
        }
        __syncthreads();
        for (int c2 = tid; c2 < p.C; c2 += NTHR) {
            float sum = 0.f;
            for (int q2 = 0; q2 < P; q2++) sum += part[q2 * p.C + c2];
            mean[c2] = sum * inv;
        }
    } else {
        for (int c = tid; c < p.C; c += NTHR) {
            float sum = 0.f;
#pragma unroll 4
            for (int sidx = 0; sidx < p.S; sidx++) sum += p.partial[((size_t)b * p.S + sidx) * p.C + c];
            mean[c] = sum * inv;
        }
    }
    __syncthreads();
    const bool v4 = (p.C & 3) == 0;
    // FC1: one wave per output, 16-byte loads (the scalar form was ~54 dependent 4-byte loads per thread per FC).  A wave takes
    // its outputs four at a time: the kernel is bound by round trips to the weights, so four rows' loads are in flight together
    // (one clip: 21.7 -> 15.7 us on a 1152-channel layer, 11.9 -> 8.3 us on the first); each output's own sum keeps its order
    // (a lane's columns ascending, then the butterfly), so no bit changes.
    for (int j0 = wave; j0 < p.Cr; j0 += 4 * NW) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (v4) {
            const float4* m4 = reinterpret_cast<const float4*>(mean);
            const float4* w4 = reinterpret_cast<const float4*>(p.w1);
            const int C4 = p.C / 4;
#pragma unroll 2
            for (int c = lane; c < C4; c += 64) {
                const float4 mv = m4[c];
                float4 w[4];
#pragma unroll
                for (int u = 0; u < 4; u++) w[u] = w4[(size_t)min(j0 + u * NW, p.Cr - 1) * C4 + c];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    acc[u] = fmaf(w[u].x, mv.x, acc[u]); acc[u] = fmaf(w[u].y, mv.y, acc[u]);
                    acc[u] = fmaf(w[u].z, mv.z, acc[u]); acc[u] = fmaf(w[u].w, mv.w, acc[u]);
                }
            }
        } else {
            for (int c = lane; c < p.C; c += 64) {
                const float mv = mean[c];
#pragma unroll
                for (int u = 0; u < 4; u++) acc[u] = fmaf(p.w1[(size_t)min(j0 + u * NW, p.Cr - 1) * p.C + c], mv, acc[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            float a = acc[u];
            for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
            const int j = j0 + u * NW;
            if (lane == 0 && j < p.Cr) r[j] = apply_act(a + (p.b1 ? p.b1[j] : 0.f), p.act1);
        }
    }
    __syncthreads();
    // FC2: a thread owns 4 channels; G thread groups split the Cr range and fold through LDS in a fixed order
    if (v4) {
        const int C4 = p.C / 4;
        int G = 1;
        while (G * 2 * C4 <= NTHR && G * 2 <= p.Cr) G *= 2;
        if (G > 1) {
            float4* part4 = reinterpret_cast<float4*>(part);       // [G][C4]: G * C4 <= NTHR float4, the scratch launch_se sizes
            const int c4 = tid % C4, g = tid / C4;
            if (g < G) {
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4* w4 = reinterpret_cast<const float4*>(p.w2) + c4;
#pragma unroll 8
                for (int j = g; j < p.Cr; j += G) {
                    float4 w = w4[(size_t)j * C4];
                    float rj = r[j];
                    acc.x = fmaf(w.x, rj, acc.x); acc.y = fmaf(w.y, rj, acc.y); acc.z = fmaf(w.z, rj, acc.z); acc.w = fmaf(w.w, rj, acc.w);
                }
                part4[g * C4 + c4] = acc;
            }
            __syncthreads();
            for (int c = tid; c < C4; c += NTHR) {
                float4 acc = part4[c];
                for (int g2 = 1; g2 < G; g2++) { float4 v = part4[g2 * C4 + c]; acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
                float4 bb = p.b2 ? reinterpret_cast<const float4*>(p.b2)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
                float4 o = make_float4(apply_act(acc.x + bb.x, p.act2), apply_act(acc.y + bb.y, p.act2),
                                       apply_act(acc.z + bb.z, p.act2), apply_act(acc.w + bb.w, p.act2));
                reinterpret_cast<float4*>(p.scale + (size_t)b * p.C)[c] = o;
            }
        } else {
            // G == 1: a thread walks the quads tid, tid + NTHR, ...  launch_se doubles the block only up to 1024 threads, so a layer of
            // more than 4096 channels has more quads than the block has threads (one trip of this loop everywhere else)
            for (int c4 = tid; c4 < C4; c4 += NTHR) {
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4* w4 = reinterpret_cast<const float4*>(p.w2) + c4;
#pragma unroll 8
                for (int j = 0; j < p.Cr; j++) {
                    float4 w = w4[(size_t)j * C4];
                    float rj = r[j];
                    acc.x = fmaf(w.x, rj, acc.x); acc.y = fmaf(w.y, rj, acc.y); acc.z = fmaf(w.z, rj, acc.z); acc.w = fmaf(w.w, rj, acc.w);
                }
                float4 bb = p.b2 ? reinterpret_cast<const float4*>(p.b2)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
                float4 o = make_float4(apply_act(acc.x + bb.x, p.act2), apply_act(acc.y + bb.y, p.act2),
                                       apply_act(acc.z + bb.z, p.act2), apply_act(acc.w + bb.w, p.act2));
                reinterpret_cast<float4*>(p.scale + (size_t)b * p.C)[c4] = o;
            }
        }
    } else {
        for (int c = tid; c < p.C; c += NTHR) {
            float acc = 0.f;
#pragma unroll 8
            for (int j = 0; j < p.Cr; j++) acc = fmaf(p.w2[(size_t)j * p.C + c], r[j], acc);
            p.scale[(size_t)b * p.C + c] = apply_act(acc + (p.b2 ? p.b2[c] : 0.f), p.act2);
        }
    }
}
// Dynamic LDS of k_se for a block of thr threads: mean [C], r [Cr], and the fold scratch - [P][C] floats with P C <= threads, or
// [G][C / 4] float4 with G C / 4 <= threads, i.e. at most one float4 per thread.  k_se raises no limit of its own, so a launch may
// ask for 64 KB; se_supported: the largest block's request stays within that (the planner refuses the block otherwise).
size_t se_lds_bytes(int C, int Cr, int thr) { return (size_t)(C + Cr + 4 * thr + 16) * sizeof(float); }
bool se_supported(int C, int Cr) { return C > 0 && Cr > 0 && se_lds_bytes(C, Cr, 1024) <= 64 * 1024; }
void launch_se(const SeParams& p, hipStream_t s) {
    // Block size: 1024 threads finish a clip fastest when the kernel owns the GPU, but a 16-wave workgroup needs a whole
    // CU's worth of free wave slots and, beside another context's kernels, waited for one 5-30x its own run time
    // (rocprofv3, timed window: avg 50 us, max 330 us against 6-18 us alone) - stalling the dependent projection GEMM.
    // A pipelined engine therefore launches 4-wave blocks that slot in anywhere (BNHIP_SE_THREADS overrides).
    static const int env = getenv("BNHIP_SE_THREADS") ? atoi(getenv("BNHIP_SE_THREADS")) : 0;
    int thr = env ? env : (p.threads ? p.threads : 1024);
    thr = std::max(64, std::min(1024, thr / 64 * 64));
    while (thr < 1024 && (p.C + 3) / 4 > thr) thr *= 2;              // FC2 maps one thread to a channel quad (beyond 4096 channels: k_se loops)
    // (Sized for 1024 threads whatever the block, a 4-wave block asked for 16 KB more LDS than it can use and,
    // beside another context's LDS-heavy kernels, waited for it: rocprofv3, Perch bf16 pipelined: avg 62 us, max 777 us.)
    const size_t lds = se_lds_bytes(p.C, p.Cr, thr);
    hipLaunchKernelGGL(k_se, dim3(p.B), dim3(thr), lds, s, p);
}

}  // namespace bnhip
