// The saturating int16 gain (pcmgain.ApplyInt16, pcmgain.go:52-63), stated once for every kernel that applies a clip's factor
// (loudness.hip, flac.hip): a factor of exactly 1 is the identity; otherwise (double)s * factor, rounded half away from zero,
// saturated to int16.  The product is one rounded operation (nothing fused).  pcm_quantized is the rounding and saturation alone,
// for a kernel whose value is not a product (denoise.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bnhip {

__device__ __forceinline__ double pcm_quantized(double v) {
    v = round(v);
    v = v > 32767.0 ? 32767.0 : v;
    v = v < -32768.0 ? -32768.0 : v;
    return v;
}

__device__ __forceinline__ double pcm_gained(int16_t s, double f) {
#pragma clang fp contract(off)
    if (f == 1.0) return (double)s;
    return pcm_quantized((double)s * f);
}

}  // namespace bnhip
