// gfx950 ingest and the fp64-MFMA mel front end: PCM -> fp32, per-clip min / range, k_frontend (normalise -> frame -> window ->
// real-DFT * mel -> power law -> NHWC store in one kernel).  The FFT-based front end is stft.hip.
#include "kernels.h"
#include "ragged.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>

namespace bnhip {

// ------------------------------------------------------------------------------------------ ingest
// internal/analysis/process.go:491-495: float32(int16)/32768
__global__ void k_pcm16_to_f32(const int16_t* __restrict__ pcm, float* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = (float)pcm[i] / 32768.0f;
}
// internal/audiocore/convert/pcm.go:242-268: 24-bit little-endian with two's-complement sign extension / 8388608,
// 32-bit / 2147483648 (float32(int32) rounds to nearest even in Go and here; the divisors are powers of two)
__global__ void k_pcm24_to_f32(const uint8_t* __restrict__ pcm, float* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int32_t v = (int32_t)pcm[3 * i] | ((int32_t)pcm[3 * i + 1] << 8) | ((int32_t)pcm[3 * i + 2] << 16);
        if (v & 0x00800000) v |= ~0x00FFFFFF;
        out[i] = (float)v / 8388608.0f;
    }
}
__global__ void k_pcm32_to_f32(const int32_t* __restrict__ pcm, float* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = (float)pcm[i] / 2147483648.0f;
}
void launch_pcm_to_f32(const void* pcm, int bits, float* out, size_t n, hipStream_t s) {
    int blocks = (int)((n + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    if (bits == 16) hipLaunchKernelGGL(k_pcm16_to_f32, dim3(blocks), dim3(256), 0, s, static_cast<const int16_t*>(pcm), out, n);
    else if (bits == 24) hipLaunchKernelGGL(k_pcm24_to_f32, dim3(blocks), dim3(256), 0, s, static_cast<const uint8_t*>(pcm), out, n);
    else hipLaunchKernelGGL(k_pcm32_to_f32, dim3(blocks), dim3(256), 0, s, static_cast<const int32_t*>(pcm), out, n);
}

// ------------------------------------------------------------------------------------------ front-end
// One block per clip: min(x) and fl(max(x)-min)+eps, i.e. REDUCE_MIN -> SUB -> REDUCE_MAX -> ADD eps.
__global__ __launch_bounds__(1024) void k_clip_minmax(const float* __restrict__ x, int n_samples, float eps,
                                                      float2* __restrict__ mm) {
    const float* xc = x + (size_t)blockIdx.x * n_samples;
    float mn = INFINITY, mx = -INFINITY;
    if ((n_samples & 3) == 0 && ((((size_t)blockIdx.x * n_samples) & 3) == 0)) {
        const float4* x4 = reinterpret_cast<const float4*>(xc);
        // batches of 8 independent loads: a rolled loop walks the clip one L2/HBM round trip at a time (24 us for one clip)
        const int n4 = n_samples / 4;
        for (int i0 = threadIdx.x; i0 < n4; i0 += 8 * blockDim.x) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                int i = i0 + u * blockDim.x;
                v[u] = i < n4 ? x4[i] : x4[i0];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                mn = fminf(fminf(mn, v[u].x), fminf(v[u].y, fminf(v[u].z, v[u].w)));
                mx = fmaxf(fmaxf(mx, v[u].x), fmaxf(v[u].y, fmaxf(v[u].z, v[u].w)));
            }
        }
    } else {
        for (int i = threadIdx.x; i < n_samples; i += blockDim.x) { float v = xc[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    }
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_down(mn, o, 64)); mx = fmaxf(mx, __shfl_down(mx, o, 64)); }
    __shared__ float smn[16], smx[16];
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smn[w] = mn; smx[w] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int nw = blockDim.x >> 6;
        for (int i = 1; i < nw; i++) { mn = fminf(mn, smn[i]); mx = fmaxf(mx, smx[i]); }
        float range = mx - mn;          // == max_i fl(x_i - mn): rounding is monotone
        mm[blockIdx.x] = make_float2(mn, range + eps);
    }
}
// Small calls (one clip per Predict is the product's call pattern): one block walks a 576 KB clip in ~5 dependent round trips
// (17-20 us at one clip).  G blocks per clip take a contiguous part each, publish (min, max) with agent-scope atomic stores, and the
// block that arrives last at the clip's counter combines the G pairs - min / max are exact whatever the grouping, so the result
// is the one-block kernel's bit for bit.  scratch: [clip][2 G + 2] floats of the plan's arena that nothing else ever uses, zeroed
// once (the counter resets itself).  Cross-XCD visibility: payload and counter are agent-scope atomics on both sides
// (MI355X_MICROARCH.md, "valid forms").
__global__ __launch_bounds__(1024) void k_clip_minmax_parts(const float* __restrict__ x, int n_samples, float eps, int G, float* __restrict__ scratch,
                                                            float2* __restrict__ mm) {
    const int clip = blockIdx.x / G, part = blockIdx.x - clip * G;
    const float4* x4 = reinterpret_cast<const float4*>(x + (size_t)clip * n_samples);
    const int n4 = n_samples / 4, per = (n4 + G - 1) / G, lo = part * per, hi = min(lo + per, n4);
    float mn = INFINITY, mx = -INFINITY;
    for (int i0 = lo + threadIdx.x; i0 < hi; i0 += 4 * blockDim.x) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int i = i0 + u * blockDim.x; v[u] = i < hi ? x4[i] : x4[i0]; }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            mn = fminf(fminf(mn, v[u].x), fminf(v[u].y, fminf(v[u].z, v[u].w)));
            mx = fmaxf(fmaxf(mx, v[u].x), fmaxf(v[u].y, fmaxf(v[u].z, v[u].w)));
        }
    }
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_down(mn, o, 64)); mx = fmaxf(mx, __shfl_down(mx, o, 64)); }
    __shared__ float smn[16], smx[16];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { smn[w] = mn; smx[w] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < (int)(blockDim.x >> 6); i++) { mn = fminf(mn, smn[i]); mx = fmaxf(mx, smx[i]); }
        float* sc = scratch + (size_t)clip * (2 * G + 2);
        __hip_atomic_store(sc + 2 * part, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(sc + 2 * part + 1, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        unsigned* cnt = reinterpret_cast<unsigned*>(sc + 2 * G);
        if (atomicAdd(cnt, 1u) == (unsigned)(G - 1)) {           // every other part of this clip is published
            __threadfence();
            for (int g = 0; g < G; g++) {
                mn = fminf(mn, __hip_atomic_load(sc + 2 * g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                mx = fmaxf(mx, __hip_atomic_load(sc + 2 * g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
            mm[clip] = make_float2(mn, (mx - mn) + eps);
            __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next call on this arena
        }
    }
}
void launch_clip_minmax(const float* x, int n_clips, int n_samples, float eps, float2* mm, float* scratch, hipStream_t s) {
    // (the parts kernel needs whole, aligned quads; above 16 clips one block per clip already fills enough of the chip)
    if (scratch && n_clips <= 16 && (n_samples & 3) == 0 && n_samples >= 16 * 4096) {
        hipLaunchKernelGGL(k_clip_minmax_parts, dim3(n_clips * kMinMaxParts), dim3(1024), 0, s, x, n_samples, eps, kMinMaxParts, scratch, mm);
        return;
    }
    hipLaunchKernelGGL(k_clip_minmax, dim3(n_clips), dim3(1024), 0, s, x, n_samples, eps, mm);
}

// ------------------------------------------------------------------------------------------ resident min/max + normalise
// k_clip_minmax followed by k_normalize (stft.hip) reads the clip from HBM twice: the second kernel cannot start before the first
// has seen the clip's last sample.  A v2.4 clip is 576 KB and one CU has 512 KB of vector registers and 160 KB of LDS, so one
// 1024-thread block (16 waves at 128 VGPRs) keeps the whole clip on chip between the two passes: thread t holds quads
// t + 1024 r, r < kNormR, in registers, the quads from 1024 kNormR on sit in dynamic LDS (each thread reads back only what it wrote
// itself, so the data needs no barrier).  One read of x, one write of xn, one launch.  The arithmetic is the pair's: min / max are
// exact whatever the grouping (v_min_f32 / v_max_f32 order -0 below +0), so every thread folds the 16 wave partials for itself, and the four normalise operations are k_normalize's in its order under the same -ffp-contract=off, IEEE division
// included - xn and mm are the pair's bit for bit.  PCM input (int16, packed 24-bit, int32) is converted in the load exactly as
// k_pcm*_to_f32 convert it.  No block waits for another one.
// Addressing: every round of 1024 quads reads and writes through a buffer descriptor of its own that starts at the round's first quad
// and ends with the clip, built with scalar arithmetic; the thread's one byte offset serves all of them, and the hardware range
// check stands in for the end-of-clip test: a quad past the end loads as zeros (and is kept out of min / max) and is not stored.
// With a selected index per load the 28 offsets of the register part were live at once and the kernel spilled.
struct Pcm24 {};                                  // sample-type tag: 3 bytes little-endian, two's complement
constexpr int kNormR = 28;                        // quads per thread in registers (112 of the 128 VGPRs)
constexpr int kNormRegQuads = 1024 * kNormR;
constexpr int kNormLdsBytes = 160 * 1024 - 256;   // dynamic part; the static part is the 2 x 16 wave partials
constexpr int kNormLdsQuads = kNormLdsBytes / 16;

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t ClipBuf;
// bytes [off, bytes) of a clip as a raw buffer (stride 0): a thread offset at or past the end is out of range.  The range check
// covers the VGPR offset only, never the instruction's scalar offset - so a block-uniform displacement goes into the descriptor
// (scalar arithmetic), not into the access.
__device__ __forceinline__ ClipBuf clip_buf(const void* base, int bytes, int off) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(static_cast<const char*>(base)) + off, 0, max(bytes - off, 0), 0x00020000);
}
// quad q of the buffer as four floats
template <typename T> struct ClipIn;
template <> struct ClipIn<float> {
    static constexpr int kBytes = 4;
    static __device__ __forceinline__ float4 quad(ClipBuf b, int q) {
        const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(b, q * 16, 0, 0);
        return make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
    }
};
template <> struct ClipIn<int16_t> {
    static constexpr int kBytes = 2;
    static __device__ __forceinline__ float s16(uint32_t v) { return (float)(int16_t)v / 32768.0f; }
    static __device__ __forceinline__ float4 quad(ClipBuf b, int q) {
        const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(b, q * 8, 0, 0);
        return make_float4(s16(w.x), s16(w.x >> 16), s16(w.y), s16(w.y >> 16));
    }
};
template <> struct ClipIn<Pcm24> {
    static constexpr int kBytes = 3;
    static __device__ __forceinline__ float s24(uint32_t v) { return (float)((int32_t)(v << 8) >> 8) / 8388608.0f; }
    static __device__ __forceinline__ float4 quad(ClipBuf b, int q) {       // four samples = three aligned words
        const u32x3 w = __builtin_amdgcn_raw_buffer_load_b96(b, q * 12, 0, 0);
        return make_float4(s24(w.x), s24((w.x >> 24) | (w.y << 8)), s24((w.y >> 16) | (w.z << 16)), s24(w.z >> 8));
    }
};
template <> struct ClipIn<int32_t> {
    static constexpr int kBytes = 4;
    static __device__ __forceinline__ float4 quad(ClipBuf b, int q) {
        const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(b, q * 16, 0, 0);
        return make_float4((float)(int32_t)w.x / 2147483648.0f, (float)(int32_t)w.y / 2147483648.0f, (float)(int32_t)w.z / 2147483648.0f,
                           (float)(int32_t)w.w / 2147483648.0f);
    }
};
__device__ __forceinline__ void quad_minmax(const float4& v, bool in_clip, float& mn, float& mx) {
    const float a = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
    const float b = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    mn = in_clip ? a : mn;
    mx = in_clip ? b : mx;
}
__device__ __forceinline__ float norm1(float x, float mn, float d, float sub, float mul) {      // k_normalize, operation for operation
    float t = x - mn;
    t = t / d;
    t = t - sub;
    return t * mul;
}
__device__ __forceinline__ void store_norm4(ClipBuf o, int q, const float4& v, float mn, float d, float sub, float mul) {
    u32x4 w;
    w.x = __float_as_uint(norm1(v.x, mn, d, sub, mul)); w.y = __float_as_uint(norm1(v.y, mn, d, sub, mul));
    w.z = __float_as_uint(norm1(v.z, mn, d, sub, mul)); w.w = __float_as_uint(norm1(v.w, mn, d, sub, mul));
    __builtin_amdgcn_raw_buffer_store_b128(w, o, q * 16, 0, 0);
}
// The framed form (FRAMED, file analysis: analyze.h): x is the block of recordings and block b takes window wv.w0 + b of the burst
// instead of clip b of a batch.  It finds its recording in the window prefix table (ragged_clip), and its input descriptors start
// at the window's first sample and end with the window's valid samples, rounded up to a whole quad - the slot's zero fill; hop is
// a multiple of 4, so every quad is aligned and wholly inside or wholly outside that extent.  The quads behind it load as zeros and,
// unlike quads behind the clip, take part in min / max: they are the zero padding wav.frame_clips gives a recording's last window.
// All of it is block-uniform scalar arithmetic in front of the first load; the other form never reads wv.
template <typename T, bool FRAMED>
__global__ __launch_bounds__(1024) void k_clip_norm_resident(const void* __restrict__ x, int n_samples, float eps, float norm_sub, float norm_mul,
                                                             float2* __restrict__ mm, float* __restrict__ out, WinView wv) {
    extern __shared__ float4 lq[];                // quads kNormRegQuads .. n4 - 1 of the clip
    __shared__ float smn[16], smx[16];
    constexpr int kIn = ClipIn<T>::kBytes * 4;     // bytes of an input quad
    const float* oc = out + (size_t)blockIdx.x * n_samples;
    const int n4 = n_samples / 4, nl = max(n4 - kNormRegQuads, 0), tid = threadIdx.x;
    const char* xc;
    int xbytes;                                   // where the input ends, from xc
    if constexpr (FRAMED) {
        const long long w = (long long)wv.w0 + blockIdx.x;
        const int rec = ragged_clip(wv.first, wv.n_rec, w);
        const long long s0 = (w - wv.first[rec]) * wv.hop;
        const int valid = (int)min((long long)n_samples, wv.slot[2 * rec + 1] - s0);
        xc = static_cast<const char*>(x) + wv.slot[2 * rec] + s0 * ClipIn<T>::kBytes;
        xbytes = ((valid + 3) >> 2) * kIn;
    } else {
        xc = static_cast<const char*>(x) + (size_t)blockIdx.x * n_samples * ClipIn<T>::kBytes;
        xbytes = n4 * kIn;
    }
    float mn = INFINITY, mx = -INFINITY;
    // the LDS part first, while the registers are free: 8 independent loads per thread and round
    for (int j0 = 0; j0 < nl; j0 += 8 * 1024) {
        float4 t[8];
#pragma unroll
        for (int u = 0; u < 8; u++) t[u] = ClipIn<T>::quad(clip_buf(xc, xbytes, (kNormRegQuads + j0 + u * 1024) * kIn), tid);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int j = j0 + u * 1024 + tid;
            quad_minmax(t[u], j < nl, mn, mx);
            if (j < nl) lq[j] = t[u];
        }
    }
    // the register part: kNormR independent loads per thread
    float4 v[kNormR];
#pragma unroll
    for (int r = 0; r < kNormR; r++) v[r] = ClipIn<T>::quad(clip_buf(xc, xbytes, 1024 * r * kIn), tid);
#pragma unroll
    for (int r = 0; r < kNormR; r++) {            // (in source order: the scheduler's interleaving of the rounds costs registers, which spill)
        quad_minmax(v[r], tid + 1024 * r < n4, mn, mx);
        __builtin_amdgcn_sched_barrier(0);
    }
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_down(mn, o, 64)); mx = fmaxf(mx, __shfl_down(mx, o, 64)); }
    if ((tid & 63) == 0) { smn[tid >> 6] = mn; smx[tid >> 6] = mx; }
    __syncthreads();
    // every thread needs the clip's pair: lane l takes partial l % 16 and a butterfly over 16 lanes folds them (two registers; 16
    // partials read by every thread at once cost 20 and spilled the resident quads)
    mn = smn[tid & 15]; mx = smx[tid & 15];
    for (int o = 8; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 16)); mx = fmaxf(mx, __shfl_xor(mx, o, 16)); }
    const float d = (mx - mn) + eps;
    if (tid == 0) mm[blockIdx.x] = make_float2(mn, d);
#pragma unroll
    for (int r = 0; r < kNormR; r++) {
        store_norm4(clip_buf(oc, n4 * 16, 1024 * r * 16), tid, v[r], mn, d, norm_sub, norm_mul);
        __builtin_amdgcn_sched_barrier(0);
    }
    const ClipBuf ol = clip_buf(oc, n4 * 16, kNormRegQuads * 16);
    for (int j = tid; j < nl; j += 1024) store_norm4(ol, j, lq[j], mn, d, norm_sub, norm_mul);
}
bool clip_norm_resident_fits(int n_samples) {
    return n_samples > 0 && (n_samples & 3) == 0 && n_samples / 4 <= kNormRegQuads + kNormLdsQuads;
}
template <typename T, bool FRAMED>
static void launch_cnr_form(const void* x, int n_clips, int n_samples, float eps, float norm_sub, float norm_mul, float2* mm, float* out, hipStream_t s,
                            const WinView& wv) {
    lds_limit_once<&k_clip_norm_resident<T, FRAMED>>(kNormLdsBytes);
    const int nl = std::max(n_samples / 4 - kNormRegQuads, 0);
    hipLaunchKernelGGL((k_clip_norm_resident<T, FRAMED>), dim3(n_clips), dim3(1024), (size_t)nl * 16, s, x, n_samples, eps, norm_sub, norm_mul, mm, out, wv);
}
template <typename T>
static void launch_cnr(const void* x, int n_clips, int n_samples, float eps, float norm_sub, float norm_mul, float2* mm, float* out, hipStream_t s,
                       const WinView* win) {
    if (win) launch_cnr_form<T, true>(x, n_clips, n_samples, eps, norm_sub, norm_mul, mm, out, s, *win);
    else launch_cnr_form<T, false>(x, n_clips, n_samples, eps, norm_sub, norm_mul, mm, out, s, WinView{});
}
bool clip_norm_framed_ok(const void* block, const WinView& v) {
    return v.first && v.slot && v.n_rec > 0 && v.hop > 0 && (v.hop & 3) == 0 && !(reinterpret_cast<uintptr_t>(block) & 15);
}
bool launch_clip_norm_resident(const void* x, int bits, int n_clips, int n_samples, float eps, float norm_sub, float norm_mul, float2* mm, float* out,
                               hipStream_t s, const WinView* win) {
    // whole quads, loaded and stored at their natural alignment (a clip is a whole number of quads, so every clip's base is aligned
    // when the first one is: 16 bytes for float32 / int32, 8 for int16, 4 for the three words of a 24-bit quad; a window of the
    // framed form starts a multiple of 4 samples into a 16-byte aligned slot)
    const uintptr_t in_align = bits == 16 ? 8 : bits == 24 ? 4 : 16;
    if (n_clips <= 0 || !clip_norm_resident_fits(n_samples) || (reinterpret_cast<uintptr_t>(x) & (in_align - 1)) || (reinterpret_cast<uintptr_t>(out) & 15))
        return false;
    if (win && !clip_norm_framed_ok(x, *win)) return false;
    if (bits == 0) launch_cnr<float>(x, n_clips, n_samples, eps, norm_sub, norm_mul, mm, out, s, win);
    else if (bits == 16) launch_cnr<int16_t>(x, n_clips, n_samples, eps, norm_sub, norm_mul, mm, out, s, win);
    else if (bits == 24) launch_cnr<Pcm24>(x, n_clips, n_samples, eps, norm_sub, norm_mul, mm, out, s, win);
    else if (bits == 32) launch_cnr<int32_t>(x, n_clips, n_samples, eps, norm_sub, norm_mul, mm, out, s, win);
    else return false;
    return true;
}

// Fused normalise -> frame -> window -> (real-DFT * mel) -> x^p1 -> x^p2 -> NHWC store.
// Because the graph keeps only the REAL part of the STFT (CAST complex64->float32) and applies the
// mel matrix before squaring, everything between the window multiply and the first POW is linear:
//   mel[f, m] = sum_n fl32(xn[f*hop + n] * w[n]) * G[n, m],   G[n, m] = sum_k cos(2*pi*k*n/N) * Mel[k, m]
// TFLite evaluates RFFT2D in double precision (rfft2d.cc runs Ooura fft2d on doubles), so bins that
// cancel to ~0 really are ~0 there; the subsequent power-law compression (x^0.45) amplifies any
// accumulation noise in such bins by orders of magnitude (digital silence - the reference benchmark's
// own input, cmd/benchmark/benchmark.go:99-101 - is the extreme case).  The contraction therefore
// runs on the f64 MFMA (v_mfma_f64_16x16x4_f64) with G held in fp64, while the window product is
// rounded to fp32 first exactly as the graph's MUL does.  A rows are overlapping windows of the
// LDS-resident clip segment (never materialised), B = G streamed from L2 in 32-row chunks.
// cos(2*pi*k*(N-n)/N) = cos(2*pi*k*n/N) makes G symmetric in n, so the windowed frame is folded first,
//   a[n'] = double(fl32(x[n']*w[n'])) + double(fl32(x[N-n']*w[N-n']))   (exact in fp64), n' = 0..N/2,
// halving the contraction length (K = N/2+1) at no cost in accuracy.
// Block: 64 frames x (16*NT) mel columns, 4 waves, wave w owns frames [16w,16w+16) x all NT tiles.
typedef double f64x4 __attribute__((ext_vector_type(4)));
// Tile parameters: FT frames x all mel tiles per block, waves = (FT/16 frame groups) x (WN mel groups), G streamed
// in KC-row chunks.  Two shapes are instantiated:
//   <FT 32, KC 16>: ~80 KB of LDS -> two blocks per CU (measured 3 % faster than the 64-frame shape);
//   <FT 64, KC 32|16>: fallback when the smaller shape's LDS does not allow two blocks anyway.
// Measured ceilings on MI355X (tools/ubench/mfma_f64*.hip): the f64 MFMA sustains 68 TF with two waves per SIMD and
// nothing else; FP VALU work does NOT overlap it (2 v_mul_f32 per MFMA -> 54 TF, 8 -> 49 TF; integer VALU is free) and
// an LDS read consumed right away costs far more (1 per MFMA -> 57 TF, 4 -> 38 TF).  This kernel needs 5 FP ops per
// 3 MFMAs to build the folded A operand, which bounds it near 55 TF; it reaches 39 TF (ch0) / 33 TF (ch1).
template <int NT, int WN, int FT, int KC>
__global__ __launch_bounds__(64 * (FT / 16) * WN) void k_frontend(FrontendParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NTP = NT * 16;
    constexpr int NTW = NT / WN;                 // mel tiles per wave
    constexpr int FG = FT / 16;                  // frame groups
    constexpr int NTHR = 64 * FG * WN;
    constexpr int GS = NTP + 16;                 // LDS row stride (doubles): k-rows land 32 banks apart for ds_read_b64
    constexpr int GQ = (KC * (NTP / 4) + NTHR - 1) / NTHR;   // double4 (32 B) per thread per chunk
    const int seg_len = (FT - 1) * p.hop + p.Lfft + 4;      // +4: the n'=0 mirror reads one past the frame (weight 0)
    float* seg = smem;
    float* win = smem + ((seg_len + 3) & ~3);                // [Kp] window at n'
    float* win2 = win + p.Kp;                                // [Kp] window at the mirror index (0 where there is none)
    double* Gs = reinterpret_cast<double*>(win2 + p.Kp);     // Kp is a multiple of 16 -> 16-byte aligned

    const int b = blockIdx.y;
    const int f0 = blockIdx.x * FT;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = (tid >> 6) % FG, nh = (tid >> 6) / FG;
    const int li = lane & 15, kq = lane >> 4;

    // ---- stage + normalise the clip segment ((x - min) / (range+eps) - 0.5) * 2, exactly the graph's op order
    {
        const float2 mm = p.mm[b];
        const float* xc = p.x + (size_t)b * p.n_samples;
        const int s0 = f0 * p.hop;
        // all of this thread's loads are issued before the first use (a rolled one-load-per-iteration loop exposes
        // the global latency once per element)
        auto norm = [&](float x) { float t = x - mm.x; t = t / mm.y; t = t - p.norm_sub; return t * p.norm_mul; };
        const int lim = min(seg_len - 4, p.n_samples - s0);      // samples of this segment that exist
        if ((((size_t)xc & 15) | (s0 & 3)) == 0) {
            constexpr int UN = 10;
            const int nq = (seg_len + 3) >> 2;
            for (int q0 = tid; q0 < nq; q0 += NTHR * UN) {
                float4 v[UN];
#pragma unroll
                for (int u = 0; u < UN; u++) {
                    int q = q0 + u * NTHR;
                    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (4 * q + 3 < lim) v[u] = *reinterpret_cast<const float4*>(xc + s0 + 4 * q);
                    else if (4 * q < lim) {
                        v[u].x = xc[s0 + 4 * q];
                        if (4 * q + 1 < lim) v[u].y = xc[s0 + 4 * q + 1];
                        if (4 * q + 2 < lim) v[u].z = xc[s0 + 4 * q + 2];
                    }
                }
#pragma unroll
                for (int u = 0; u < UN; u++) {
                    int q = q0 + u * NTHR;
                    if (q < nq) {
                        float4 o;
                        o.x = 4 * q < lim ? norm(v[u].x) : 0.f; o.y = 4 * q + 1 < lim ? norm(v[u].y) : 0.f;
                        o.z = 4 * q + 2 < lim ? norm(v[u].z) : 0.f; o.w = 4 * q + 3 < lim ? norm(v[u].w) : 0.f;
                        *reinterpret_cast<float4*>(seg + 4 * q) = o;
                    }
                }
            }
        } else {
            for (int i = tid; i < seg_len; i += NTHR) seg[i] = i < lim ? norm(xc[s0 + i]) : 0.0f;
        }
        for (int i = tid; i < p.Kp; i += NTHR) { win[i] = p.window[i]; win2[i] = p.window[p.Kp + i]; }
    }

    // G chunks travel global -> registers (two stages: the load for chunk c+3 is issued while chunk c computes, so it
    // has two full iterations to arrive; one iteration is shorter than the L2 latency under load) -> LDS (2 buffers)
    const double4* G4 = reinterpret_cast<const double4*>(p.G);
    double4 greg[2][GQ];
    auto gload = [&](int chunk, double4 (&gr)[GQ]) {
#pragma unroll
        for (int q = 0; q < GQ; q++) {
            int idx = tid + NTHR * q;
            double4 v = make_double4(0., 0., 0., 0.);
            if (idx < KC * (NTP / 4)) v = G4[(size_t)chunk * KC * (NTP / 4) + idx];
            gr[q] = v;
        }
    };
    auto gstore = [&](int buf, const double4 (&gr)[GQ]) {
#pragma unroll
        for (int q = 0; q < GQ; q++) {
            int idx = tid + NTHR * q;
            if (idx < KC * (NTP / 4)) {
                int r = idx / (NTP / 4), c4 = idx % (NTP / 4);
                *reinterpret_cast<double4*>(&Gs[buf * KC * GS + r * GS + 4 * c4]) = gr[q];
            }
        }
    };

    f64x4 acc[NTW];
#pragma unroll
    for (int t = 0; t < NTW; t++) acc[t] = (f64x4){0., 0., 0., 0.};

    // Register pipeline, one chunk deep: while the KS*NTW MFMAs of chunk ch run from registers, the operands of
    // chunk ch+1 are fetched from LDS (folded window products + G fragments) and G(ch+2) travels global -> regs ->
    // LDS.  (ISA of the first version: every k-step was ds_read -> s_waitcnt lgkmcnt(0) -> mfma, i.e. the LDS
    // latency was exposed once per k-step with only two waves per SIMD to cover it.)
    constexpr int KS = KC / 4;
    const int nchunks = p.Kp / KC;
    const float* arow = seg + (16 * wave + li) * p.hop + kq;                 // x[f*hop + n']
    const float* mrow = seg + (16 * wave + li) * p.hop + p.Lfft - kq;        // x[f*hop + N - n']
    auto fetch = [&](int ch, double (&av)[KS], double (&bm)[KS][NTW]) {
        const double* gb = Gs + (ch & 1) * KC * GS + kq * GS + nh * NTW * 16 + li;
        const float* ab = arow + ch * KC;
        const float* mb = mrow - ch * KC;
        const float* wb = win + ch * KC + kq;
        const float* wb2 = win2 + ch * KC + kq;
#pragma unroll
        for (int kk = 0; kk < KS; kk++) {
            float xw = ab[kk * 4] * wb[kk * 4];          // fp32 products, rounded like the graph's window MUL
            float xm = mb[-kk * 4] * wb2[kk * 4];
            av[kk] = (double)xw + (double)xm;            // exact fold in fp64
#pragma unroll
            for (int t = 0; t < NTW; t++) bm[kk][t] = gb[kk * 4 * GS + t * 16];
        }
    };
    auto mma = [&](const double (&av)[KS], const double (&bm)[KS][NTW]) {
#pragma unroll
        for (int kk = 0; kk < KS; kk++)
#pragma unroll
            for (int t = 0; t < NTW; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], bm[kk][t], acc[t], 0, 0, 0);
    };
    double a0[KS], b0[KS][NTW], a1[KS], b1[KS][NTW];
    gload(0, greg[0]);
    if (nchunks > 1) gload(1, greg[1]);
    gstore(0, greg[0]);
    if (nchunks > 2) gload(2, greg[0]);
    __syncthreads();
    fetch(0, a0, b0);
    if (nchunks > 1) gstore(1, greg[1]);
    __syncthreads();
    // iteration invariant: (ac,bc) = chunk ch in registers, LDS buffer (ch+1)&1 = G(ch+1) visible to all
    // (ac,bc) = chunk ch in registers, LDS buffer (ch+1)&1 = G(ch+1) visible to all, gc = G(ch+2) in flight/registers
    auto iter = [&](int ch, double (&ac)[KS], double (&bc)[KS][NTW], double (&an)[KS], double (&bn)[KS][NTW],
                    double4 (&gc)[GQ], double4 (&gn)[GQ]) {
        if (ch + 3 < nchunks) gload(ch + 3, gn);
        // unconditional (the last iteration re-reads its own chunk, unused) so that fetch and the MFMA burst share a
        // basic block; the group barriers then interleave them: each 64-cycle f64 MFMA leaves 15 issue slots
        fetch(min(ch + 1, nchunks - 1), an, bn);
        mma(ac, bc);
#pragma unroll
        for (int i = 0; i < KS * NTW; i++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // 2 LDS reads
            __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);   // 3 VALU
        }
        if (ch + 2 < nchunks) gstore(ch & 1, gc);   // buffer ch&1 was last read (chunk ch) before the previous barrier
        __syncthreads();
    };
    for (int ch = 0; ch < nchunks; ch += 2) {
        iter(ch, a0, b0, a1, b1, greg[0], greg[1]);
        if (ch + 1 < nchunks) iter(ch + 1, a1, b1, a0, b0, greg[1], greg[0]);
    }

    // ---- epilogue: f64 C/D layout D[row = kq + 4*r][col = li]  (row = frame, col = mel)
#pragma unroll
    for (int t = 0; t < NTW; t++) {
        int m = (nh * NTW + t) * 16 + li;
        if (m >= p.n_mels) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            int f = f0 + 16 * wave + kq + 4 * r;
            if (f >= p.F) continue;
            float v = (float)acc[t][r];
            float y = (p.p1 == 2.0f) ? v * v : powf(v, p.p1);
            if (p.p2 != 1.0f) y = powf(y, p.p2);
            p.out[(((size_t)b * p.n_mels + m) * p.F + f) * p.C + p.c] = y;
        }
    }
}

static size_t fe_lds_bytes(int FT, int KC, int Lfft, int Kp, int hop, int NTP) {
    int seg_len = (FT - 1) * hop + Lfft + 4;
    return (size_t)(((seg_len + 3) & ~3) + 2 * Kp) * sizeof(float) + (size_t)2 * KC * (NTP + 16) * sizeof(double);
}
// two blocks of the 32-frame shape must fit in the CU's 160 KB, otherwise the 64-frame shape is used
static bool fe_small_shape(int Lfft, int Kp, int hop, int NTP) {
    return 2 * (fe_lds_bytes(32, 16, Lfft, Kp, hop, NTP) + 512) <= 160 * 1024;
}
int frontend_kc(int Lfft, int hop, int NTP) {
    int Kp16 = (Lfft / 2 + 1 + 15) / 16 * 16;
    return fe_small_shape(Lfft, Kp16, hop, NTP) ? 16 : 32;
}
size_t frontend_lds_bytes(int Lfft, int Kp, int hop, int NTP) {
    return fe_small_shape(Lfft, Kp, hop, NTP) ? fe_lds_bytes(32, 16, Lfft, Kp, hop, NTP) : fe_lds_bytes(64, Kp % 32 ? 16 : 32, Lfft, Kp, hop, NTP);
}

template <int NT, int WN, int FT, int KC>
static void launch_frontend_shape(const FrontendParams& p, hipStream_t s) {
    size_t lds = fe_lds_bytes(FT, KC, p.Lfft, p.Kp, p.hop, p.NTP);
    // (per launch: the limit is an attribute of the function on the CURRENT device - see launch_stft_bins)
    lds_limit_once<&k_frontend<NT, WN, FT, KC>>(160 * 1024);
    dim3 grid((p.F + FT - 1) / FT, p.n_clips);
    hipLaunchKernelGGL((k_frontend<NT, WN, FT, KC>), grid, dim3(64 * (FT / 16) * WN), lds, s, p);
}
template <int NT, int WN>
static void launch_frontend_nt(const FrontendParams& p, hipStream_t s) {
    static const char* force = getenv("BNHIP_FE_SHAPE");       // experiment switch: "64" forces the large shape
    bool small = fe_small_shape(p.Lfft, p.Kp, p.hop, p.NTP) && p.Kp % 16 == 0 && !(force && atoi(force) == 64);
    if (small) launch_frontend_shape<NT, WN, 32, 16>(p, s);
    else if (p.Kp % 32 == 0) launch_frontend_shape<NT, WN, 64, 32>(p, s);
    else launch_frontend_shape<NT, WN, 64, 16>(p, s);
}
void launch_frontend(const FrontendParams& p, hipStream_t s) {
    // even tile counts run 8 waves (two mel halves): two waves per SIMD keep the f64 matrix pipe fed while the
    // partner waits on LDS
    switch (p.NTP / 16) {
        case 1: launch_frontend_nt<1, 1>(p, s); break; case 2: launch_frontend_nt<2, 2>(p, s); break;
        case 3: launch_frontend_nt<3, 1>(p, s); break; case 4: launch_frontend_nt<4, 2>(p, s); break;
        case 5: launch_frontend_nt<5, 1>(p, s); break; case 6: launch_frontend_nt<6, 2>(p, s); break;
        case 7: launch_frontend_nt<7, 1>(p, s); break; case 8: launch_frontend_nt<8, 2>(p, s); break;
        default: break;
    }
}

}  // namespace bnhip
