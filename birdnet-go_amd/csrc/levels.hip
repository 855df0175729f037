// The kernel of levels.h: ragged frames of packed PCM -> {sum of squares, full-scale samples} per frame, one pass.
#include "levels.h"

#include "pcm_sample.h"
#include "ragged.h"

namespace bnhip {

namespace {

// one sample of the meter into the lane's counters; the square of an int16 is at most 2^30, and the sum is 64-bit from here on
__device__ __forceinline__ void level_take(int q, unsigned long long& sum, unsigned& clipped) {
    sum += (unsigned long long)(unsigned)(q * q);
    clipped += (q == 32767 || q == -32768) ? 1u : 0u;
}

// the sum of v over the wave's 64 lanes, in lane 0: lane moves, no LDS
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

}  // namespace

// A flat grid over the tile prefix of the call's frames, a block finds its frame with the search of ragged.h (as k_capture_write
// and k_cut_clips do), and a lane takes LEVEL_LINES steps of level_step(BITS) samples, the block's lanes side by side in each step.
// A frame begins at a 16-byte line, so a step of a 16- or 32-bit frame that lies whole inside the frame is one 16-byte load; a
// 24-bit frame's steps, and every frame's ragged last step, are read per sample - never a byte beyond the frame's last sample, so
// never a neighbouring frame's.  The lane's sum is 64-bit (eight squares already reach 2^33); the wave's comes by lane moves, the
// block's four through LDS, and the block adds its two integers to the frame's zeroed record with integer atomics: integer adds
// commute, so the record's bits do not depend on the order the tiles finish in.  The sums are integer arithmetic throughout; the
// only float operations are pcm_sample.h's own conversion of a 24- or 32-bit sample to the int16 the capture ring stores.
template <int BITS>
__global__ __launch_bounds__(256) void k_frame_levels(const char* __restrict__ pcm, long long pcm_bytes, const LevelFrame* __restrict__ frames,
                                                      const long long* __restrict__ tile0, int n_frames, LevelRecord* __restrict__ rec) {
    constexpr int STEP = level_step(BITS), BYTES = BITS / 8;
    __shared__ unsigned long long s_sum[4], s_clip[4];
    const long long b = blockIdx.x;
    const int c = ragged_clip(tile0, n_frames, b);
    const LevelFrame fr = frames[c];
    // (the host has checked the frames; a lane never reads outside the call's PCM whatever the table says)
    const bool sane = fr.off >= 0 && (fr.off & 15) == 0 && fr.off <= pcm_bytes;
    const long long n = sane ? min(fr.n, (pcm_bytes - fr.off) / BYTES) : 0;
    const char* base = pcm + (sane ? fr.off : 0);
    const long long t0 = (b - tile0[c]) * level_tile(BITS);
    unsigned long long sum = 0;
    unsigned clipped = 0;                               // at most LEVEL_LINES * 8 per lane
#pragma unroll
    for (int k = 0; k < LEVEL_LINES; k++) {
        const long long i = t0 + ((long long)k * 256 + threadIdx.x) * STEP;
        if (i >= n) break;
        if (BITS != 24 && i + STEP <= n) {
            union { int4 v; int16_t h[8]; char c[16]; } u;
            u.v = *reinterpret_cast<const int4*>(base + i * BYTES);
#pragma unroll
            for (int j = 0; j < STEP; j++) level_take(BITS == 16 ? (int)u.h[j] : (int)sample_pcm16(frame_sample<BITS>(u.c, j)), sum, clipped);
        } else {
            const int m = (int)min(n - i, (long long)STEP);
            for (int j = 0; j < m; j++)
                level_take(BITS == 16 ? (int)reinterpret_cast<const int16_t*>(base)[i + j] : (int)sample_pcm16(frame_sample<BITS>(base, i + j)), sum,
                           clipped);
        }
    }
    sum = wave_sum(sum);
    const unsigned long long clip = wave_sum((unsigned long long)clipped);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_sum[wave] = sum; s_clip[wave] = clip; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long S = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3], C = s_clip[0] + s_clip[1] + s_clip[2] + s_clip[3];
        if (S) atomicAdd(&rec[c].sum_squares, S);
        if (C) atomicAdd(&rec[c].clipped_samples, C);
    }
}

void launch_frame_levels(const void* pcm, long long pcm_bytes, int bits, const LevelFrame* frames, const long long* tile0, int n_frames,
                         long long n_tiles, LevelRecord* rec, hipStream_t s) {
    if (n_frames <= 0 || n_tiles <= 0) return;
    const dim3 grid((unsigned)n_tiles);
    const char* p = static_cast<const char*>(pcm);
    if (bits == 16) hipLaunchKernelGGL(k_frame_levels<16>, grid, dim3(256), 0, s, p, pcm_bytes, frames, tile0, n_frames, rec);
    else if (bits == 24) hipLaunchKernelGGL(k_frame_levels<24>, grid, dim3(256), 0, s, p, pcm_bytes, frames, tile0, n_frames, rec);
    else hipLaunchKernelGGL(k_frame_levels<32>, grid, dim3(256), 0, s, p, pcm_bytes, frames, tile0, n_frames, rec);
}

}  // namespace bnhip
