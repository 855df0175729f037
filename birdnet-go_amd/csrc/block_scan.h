// The block-wide scan of the layout kernels (flac.hip, png.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace bnhip {

// inclusive scan over a block of 256; sh is in use until the caller's next __syncthreads
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* __restrict__ sh, int tid) {
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const T a = tid >= d ? sh[tid - d] : (T)0;
        __syncthreads();
        sh[tid] += a;
        __syncthreads();
    }
    return sh[tid];
}

}  // namespace bnhip
