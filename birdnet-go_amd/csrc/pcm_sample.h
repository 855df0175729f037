// One sample of a block of PCM as float32, at any alignment of a packed 24-bit block: internal/analysis/process.go:491-495 and
// internal/audiocore/convert/pcm.go:242-268, as k_pcm16_to_f32 / k_pcm24_to_f32 / k_pcm32_to_f32 (frontend.hip) state them.
// BITS 0: the block is float32 and the sample is copied.  (k_frame_windows, analyze.hip; k_resample_slots, resample.hip)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bnhip {

template <int BITS> __device__ __forceinline__ float frame_sample(const char* p, long long i);
template <> __device__ __forceinline__ float frame_sample<0>(const char* p, long long i) { return reinterpret_cast<const float*>(p)[i]; }
template <> __device__ __forceinline__ float frame_sample<16>(const char* p, long long i) { return (float)reinterpret_cast<const int16_t*>(p)[i] / 32768.0f; }
template <> __device__ __forceinline__ float frame_sample<24>(const char* p, long long i) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(p) + 3 * i;
    int32_t v = (int32_t)b[0] | ((int32_t)b[1] << 8) | ((int32_t)b[2] << 16);
    if (v & 0x00800000) v |= ~0x00FFFFFF;
    return (float)v / 8388608.0f;
}
template <> __device__ __forceinline__ float frame_sample<32>(const char* p, long long i) { return (float)reinterpret_cast<const int32_t*>(p)[i] / 2147483648.0f; }

// The way back, for a clip cut out of a recording (k_cut_clips, clips.hip): x is what frame_sample answers, q = clamp(rint(x * 2^15),
// -32768, 32767) with ties to even, and a NaN gives 0.  x * 2^15 is exact (or an infinity), so the one rounding is rint's; a 16-bit
// sample comes back as itself.
__host__ __device__ __forceinline__ int16_t sample_pcm16(float x) {
    const float y = rintf(x * 32768.0f);
    if (!(y == y)) return 0;
    return (int16_t)(y < -32768.0f ? -32768.0f : y > 32767.0f ? 32767.0f : y);
}

}  // namespace bnhip
