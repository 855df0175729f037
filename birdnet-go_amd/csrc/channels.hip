// The per-channel energy measurement behind BNHIP_CHANNEL_AUTO (channels.h): exact 128-bit sums of squares, integer arithmetic
// throughout - an integer sum is the same number whatever the tiling, the thread that took a sample or the order of the adds, so
// the result depends neither on launch geometry nor on arrival order, and no atomic is needed: every partial has one writer.
//
// k_channel_energy: one block per tile of ENERGY_TILE frames of one recording.  It is a read-once reduction, bound by bytes:
//   - 16- and 32-bit recordings whose channel count divides the samples of a 16-byte vector (8 / 4) are read as 16-byte vectors -
//     a recording starts on a 16-byte line of the raw block and a tile holds whole vectors - and lane j of a vector is always
//     channel j mod C, so a thread keeps one sum per lane;
//   - every other shape (packed 24-bit, 3 / 5 / 6 ... channels) is read sample by sample, thread t on channel t mod C of frames
//     t / C, t / C + G, ... (G = 256 / C frames a pass), consecutive threads on consecutive samples.
// k_channel_decide: one block per recording adds its tiles' partials per channel, writes the sums and - one thread, in fp64 with
// every operation rounded - the decision of channels.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "channels.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace bnhip {

namespace {

struct U128 { unsigned long long lo, hi; };
__host__ __device__ __forceinline__ void add128(U128& a, unsigned long long lo, unsigned long long hi) {
    a.lo += lo;
    a.hi += hi + (a.lo < lo ? 1ull : 0ull);
}
__device__ __forceinline__ void add_square(U128& a, int32_t v) {
    const long long w = v;
    add128(a, (unsigned long long)(w * w), 0ull);                     // v^2 <= 2^62
}

// the decision of channels.h over a recording's sums e[channels][2]
__device__ inline int channel_decide_rule(const unsigned long long* e, int channels, int bits, long long length) {
#pragma clang fp contract(off)
    if (channels == 1) return 0;
    const double quiet = (1073.741824 * (double)(1ull << (2 * (bits - 16)))) * (double)length;
    double ed[CHANNELS_MAX];
    bool all_quiet = true;
    int top = 0;
    for (int c = 0; c < channels; c++) {
        ed[c] = (double)e[2 * c + 1] * 18446744073709551616.0 + (double)e[2 * c];
        all_quiet = all_quiet && ed[c] < quiet;
        if (ed[c] > ed[top]) top = c;
    }
    if (all_quiet) return CHANNEL_MIX;
    int second = top == 0 ? 1 : 0;
    for (int c = 0; c < channels; c++)
        if (c != top && ed[c] > ed[second]) second = c;
    return ed[top] > 3.9810717055349722 * ed[second] ? top : CHANNEL_MIX;
}

// acc[t] (t < n_slots * groups, slot = t % n_slots) summed over the groups into acc[slot]; every thread of the block calls it
__device__ __forceinline__ void fold_groups(U128* acc, int n_slots, int groups) {
    int half = 1;
    while (half < groups) half <<= 1;
    for (half >>= 1; half > 0; half >>= 1) {
        __syncthreads();
        const int t = threadIdx.x, g = t / n_slots;
        if (g < half && g + half < groups && t < n_slots * groups) {
            const U128 o = acc[t + half * n_slots];
            add128(acc[t], o.lo, o.hi);
        }
    }
    __syncthreads();
}

// the vector form: BITS 16 (8 lanes) or 32 (4 lanes), C divides the lanes; in points at the tile, n its samples
template <int BITS>
__device__ __forceinline__ void energy_tile_vec(const char* __restrict__ in, long long n, int C, U128* acc, unsigned long long* __restrict__ out) {
    constexpr int LANES = BITS == 16 ? 8 : 4;
    U128 a[LANES];
#pragma unroll
    for (int j = 0; j < LANES; j++) a[j] = U128{0ull, 0ull};
    const long long n_vec = n / LANES;
    const int4* v4 = reinterpret_cast<const int4*>(in);
    for (long long k = threadIdx.x; k < n_vec; k += 256) {
        const int4 q = v4[k];
        const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (BITS == 16) {
                add_square(a[2 * j], (int32_t)(int16_t)(w[j] & 0xFFFF));
                add_square(a[2 * j + 1], w[j] >> 16);
            } else {
                add_square(a[j], w[j]);
            }
        }
    }
    // what is left of the tile behind its last whole vector: fewer than LANES samples, sample e on lane e mod LANES
    const long long e = n_vec * LANES + threadIdx.x;
    if (e < n) {
        const int32_t v = pcm_int<BITS>(in, e);
#pragma unroll
        for (int j = 0; j < LANES; j++) if (j == (int)threadIdx.x) add_square(a[j], v);
    }
    // lane j over the block's threads, then the lanes of a channel
#pragma unroll
    for (int j = 0; j < LANES; j++) {
        __syncthreads();
        acc[threadIdx.x] = a[j];
        fold_groups(acc, 1, 256);
        if (threadIdx.x == 0) acc[256 + j] = acc[0];
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        U128 s{0ull, 0ull};
        for (int j = threadIdx.x; j < LANES; j += C) add128(s, acc[256 + j].lo, acc[256 + j].hi);
        out[2 * threadIdx.x] = s.lo;
        out[2 * threadIdx.x + 1] = s.hi;
    }
}

// the sample form: any depth and channel count; in points at the recording, frames [f0, f1) are the tile's
template <int BITS>
__device__ __forceinline__ void energy_tile_any(const char* __restrict__ in, long long f0, long long f1, int C, U128* acc,
                                                unsigned long long* __restrict__ out) {
    const int G = 256 / C;
    const int t = threadIdx.x, c = t % C, g = t / C;
    U128 a{0ull, 0ull};
    if (g < G)
        for (long long f = f0 + g; f < f1; f += G) add_square(a, pcm_int<BITS>(in, f * C + c));
    acc[t] = a;
    fold_groups(acc, C, G);
    if (t < C) {
        out[2 * t] = acc[t].lo;
        out[2 * t + 1] = acc[t].hi;
    }
}

__global__ __launch_bounds__(256) void k_channel_energy(const char* __restrict__ raw, const EnergyDesc* __restrict__ desc,
                                                        const long long* __restrict__ tile0, int n, unsigned long long* __restrict__ partials) {
    __shared__ U128 acc[256 + 8];
    const int r = ragged_clip(tile0, n, (long long)blockIdx.x);
    const EnergyDesc d = desc[r];
    const long long f0 = ((long long)blockIdx.x - tile0[r]) * ENERGY_TILE;
    const long long f1 = min((long long)d.n_in, f0 + ENERGY_TILE);
    const char* in = raw + d.in_off;
    unsigned long long* out = partials + (size_t)blockIdx.x * (2 * CHANNELS_MAX);
    const int C = d.channels;
    if (d.bits == 16 && 8 % C == 0) energy_tile_vec<16>(in + f0 * C * 2, (f1 - f0) * C, C, acc, out);
    else if (d.bits == 32 && 4 % C == 0) energy_tile_vec<32>(in + f0 * C * 4, (f1 - f0) * C, C, acc, out);
    else if (d.bits == 16) energy_tile_any<16>(in, f0, f1, C, acc, out);
    else if (d.bits == 24) energy_tile_any<24>(in, f0, f1, C, acc, out);
    else energy_tile_any<32>(in, f0, f1, C, acc, out);
}

__global__ __launch_bounds__(256) void k_channel_decide(const EnergyDesc* __restrict__ desc, const long long* __restrict__ tile0,
                                                        const unsigned long long* __restrict__ partials, unsigned long long* __restrict__ energy,
                                                        int* __restrict__ sel) {
    __shared__ U128 acc[256];
    __shared__ unsigned long long e[2 * CHANNELS_MAX];
    const int r = blockIdx.x;
    const EnergyDesc d = desc[r];
    const long long t0 = tile0[r], t1 = tile0[r + 1];
    for (int c = 0; c < d.channels; c++) {
        U128 a{0ull, 0ull};
        for (long long t = t0 + threadIdx.x; t < t1; t += 256) {
            const unsigned long long* p = partials + (size_t)t * (2 * CHANNELS_MAX) + 2 * c;
            add128(a, p[0], p[1]);
        }
        __syncthreads();                          // the channel in front has been read out of acc[0]
        acc[threadIdx.x] = a;
        fold_groups(acc, 1, 256);
        if (threadIdx.x == 0) { e[2 * c] = acc[0].lo; e[2 * c + 1] = acc[0].hi; }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * d.channels) energy[(size_t)r * (2 * CHANNELS_MAX) + threadIdx.x] = e[threadIdx.x];
    if (threadIdx.x == 0) sel[d.rec] = channel_decide_rule(e, d.channels, d.bits, d.n_in);
}

}  // namespace

void launch_channel_energy(const void* d_raw, const EnergyDesc* d_desc, const long long* d_tile0, int n, long long n_tiles,
                           unsigned long long* d_partials, unsigned long long* d_energy, int* d_sel, hipStream_t s) {
    if (n <= 0 || n_tiles <= 0) return;
    hipLaunchKernelGGL(k_channel_energy, dim3((unsigned)n_tiles), dim3(256), 0, s, static_cast<const char*>(d_raw), d_desc, d_tile0, n, d_partials);
    hipLaunchKernelGGL(k_channel_decide, dim3((unsigned)n), dim3(256), 0, s, d_desc, d_tile0, d_partials, d_energy, d_sel);
}

}  // namespace bnhip
