// Multichannel recordings (bnhip_analyze_channels_*, analyze_recordings.cpp; bnhip_channel_energy_pcm, api_channels.cpp): the frames stay interleaved as they
// are in the file, and the launch that converts and resamples fetches "channel c" or "the mean of the channels" (channel_sample,
// used by k_resample_slots_mc, resample.hip).  Which one is, where asked, decided from a measurement made on the device
// (channels.hip): the exact sum of squares of every channel as a 128-bit integer, the reference's left / right / downmix rule
// (internal/audiocore/ffmpeg/analyze.go:157-202) restated on those sums without transcendental functions:
//   Ed[c] = (double)sum_hi * 2^64 + (double)sum_lo
//   quiet(c)  : Ed[c] < (1073.741824 * 4^(bits - 16)) * (double)length              (-60 dBFS)
//   one channel -> channel 0; every channel quiet -> mix; else top = the largest Ed (ties: the lower index), second = the largest
//   of the others; top when Ed[top] > 3.9810717055349722 * Ed[second] (6 dB in power), else mix.
// Every value is reproducible bit for bit in numpy (tests/chanref.py): nothing here may contract into an fma.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pcm_sample.h"

namespace bnhip {

constexpr int CHANNEL_MIX = -1;                  // BNHIP_CHANNEL_MIX
constexpr int CHANNEL_AUTO = -2;                 // BNHIP_CHANNEL_AUTO
constexpr int CHANNELS_MAX = 16;

// element i of a block of integer PCM as the integer it is (BITS 16, 24 packed, 32)
template <int BITS> __device__ __forceinline__ int32_t pcm_int(const char* p, long long i);
template <> __device__ __forceinline__ int32_t pcm_int<16>(const char* p, long long i) { return reinterpret_cast<const int16_t*>(p)[i]; }
template <> __device__ __forceinline__ int32_t pcm_int<24>(const char* p, long long i) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(p) + 3 * i;
    int32_t v = (int32_t)b[0] | ((int32_t)b[1] << 8) | ((int32_t)b[2] << 16);
    if (v & 0x00800000) v |= ~0x00FFFFFF;
    return v;
}
template <> __device__ __forceinline__ int32_t pcm_int<32>(const char* p, long long i) { return reinterpret_cast<const int32_t*>(p)[i]; }

// Frame n of a recording of C interleaved channels as the float32 the slot launch stages.  sel >= 0: that channel's sample, as
// frame_sample converts it.  CHANNEL_MIX: integer depths (float)((double)S / (double)(C * 2^(bits - 1))) with S the exact sum of
// the frame's samples; float32 the channels added in channel order in fp64, divided by (double)C, rounded to float32.
template <int BITS>
__device__ __forceinline__ float channel_sample(const char* p, long long n, int C, int sel) {
#pragma clang fp contract(off)
    if (sel >= 0) return frame_sample<BITS>(p, n * C + sel);
    if constexpr (BITS == 0) {
        const float* f = reinterpret_cast<const float*>(p) + n * C;
        double acc = (double)f[0];
        for (int c = 1; c < C; c++) acc = acc + (double)f[c];
        return (float)(acc / (double)C);
    } else {
        long long S = 0;
        for (int c = 0; c < C; c++) S += pcm_int<BITS>(p, n * C + c);
        return (float)((double)S / ((double)C * (double)(1ll << (BITS - 1))));
    }
}

// One recording of a measurement: `n_in` frames of `channels` interleaved samples of `bits` (16 / 24 / 32) from byte in_off (a
// 16-byte line) of the raw block; rec: where its decision goes in sel[]
struct EnergyDesc {
    long long in_off;
    int n_in, bits, channels, rec;
};
static_assert(sizeof(EnergyDesc) == 24, "descriptor layout");
// frames of one block of k_channel_energy (a multiple of 8: a tile of any depth and channel count starts on a 16-byte line)
constexpr int ENERGY_TILE = 16384;
inline long long energy_tiles(long long frames) { return (frames + ENERGY_TILE - 1) / ENERGY_TILE; }
// a 128-bit sum is two uint64 (lo, hi); a tile's partials and a recording's sums are [CHANNELS_MAX] of them
constexpr size_t ENERGY_ROW_BYTES = (size_t)CHANNELS_MAX * 16;

// The measurement of n recordings in two launches on s: per-tile partial sums (d_partials: [n_tiles] rows), then one block per
// recording that adds them, writes the sums (d_energy: [n] rows) and the decision into d_sel[desc.rec].  d_tile0: the prefix table
// [n + 1] of energy_tiles(n_in); n_tiles = tile0[n] fits a 31-bit grid (2^36 samples are at most 2^22 + 65 535 tiles).
void launch_channel_energy(const void* d_raw, const EnergyDesc* d_desc, const long long* d_tile0, int n, long long n_tiles,
                           unsigned long long* d_partials, unsigned long long* d_energy, int* d_sel, hipStream_t s);

}  // namespace bnhip
