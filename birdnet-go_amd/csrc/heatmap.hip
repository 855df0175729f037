// Heat-map grid kernels of bnhip_range_heatmap (HeatmapInferenceService.ComputeGridWithBinding, internal/classifier/
// heatmap_service.go:143-420): every row of a grid request is [lat, lon, week] through the range-filter meta-model, and only one
// species' output is kept.  Three small kernels around the engine's plan, enqueued per chunk of max_batch rows:
//   k_heatmap_rows    the chunk's model rows from the cell centres (on the device once per call) and the row's week index
//   k_heatmap_column  pruned tail: the plan runs without its final dense step, and this kernel computes only the wanted column -
//                     one fp32 dot product of length K per row (16 lanes per row, float4 loads of the penultimate activation,
//                     a fixed butterfly over the 16 partial sums), plus bias and the step's folded activation.  Memory-bound on
//                     the activation; no atomics.
//   k_heatmap_gather  gather tail (any other plan): column `col` of the full logits
// Every kernel writes straight into the result's [week][cell] layout at the chunk's first row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "heatmap.h"
#include "pw_common.h"

namespace bnhip {

__global__ __launch_bounds__(256) void k_heatmap_rows(const float* __restrict__ coords, int n_cells, int stride, int g0, int n,
                                                      float* __restrict__ rows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int g = g0 + r;                      // < weeks * n_cells, which the entry point checked fits an int
    const int wi = g / n_cells, c = g - wi * n_cells;
    rows[(size_t)r * 3 + 0] = coords[(size_t)c * 2 + 0];
    rows[(size_t)r * 3 + 1] = coords[(size_t)c * 2 + 1];
    rows[(size_t)r * 3 + 2] = (float)(1 + wi * stride);
}

// 16 rows per 256-thread block, 16 lanes per row.  Lane l of a row accumulates k = 4l + 64j (VEC: float4 of a and w) or
// k = l + 16j (K not a multiple of 4) in increasing j, then the 16 partial sums meet in a butterfly: the order is fixed per K.
template <bool VEC>
__global__ __launch_bounds__(256) void k_heatmap_column(const float* __restrict__ a, int K, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int act, int n, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int l = threadIdx.x & 15;
    const int r = blockIdx.x * 16 + (threadIdx.x >> 4);
    float s = 0.f;
    if (r < n) {
        const float* ar = a + (size_t)r * K;
        if (VEC) {
            for (int k = l * 4; k < K; k += 64) {
                const float4 x = *reinterpret_cast<const float4*>(ar + k);
                const float4 y = *reinterpret_cast<const float4*>(w + k);
                s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
            }
        } else {
            for (int k = l; k < K; k += 16) s = fmaf(ar[k], w[k], s);
        }
    }
    for (int o = 8; o; o >>= 1) s += __shfl_xor(s, o, 16);      // (every lane of the wave takes part)
    if (r < n && l == 0) out[r] = apply_act(s + (bias ? bias[0] : 0.f), act);
}

__global__ __launch_bounds__(256) void k_heatmap_gather(const float* __restrict__ logits, int n_classes, int col, int n,
                                                        float* __restrict__ out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n) out[r] = logits[(size_t)r * n_classes + col];
}

void launch_heatmap_rows(const float* coords, int n_cells, int stride, int g0, int n, float* rows, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_heatmap_rows, dim3((n + 255) / 256), dim3(256), 0, s, coords, n_cells, stride, g0, n, rows);
}

void launch_heatmap_column(const float* a, int K, const float* w, const float* bias, int act, int n, float* out, hipStream_t s) {
    if (n <= 0) return;
    // float4 loads need 16-byte rows: K % 4 == 0 (the activation arena and the weight rows start 256-byte aligned)
    const bool vec = (K % 4) == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w)) & 15) == 0;
    if (vec) hipLaunchKernelGGL(k_heatmap_column<true>, dim3((n + 15) / 16), dim3(256), 0, s, a, K, w, bias, act, n, out);
    else hipLaunchKernelGGL(k_heatmap_column<false>, dim3((n + 15) / 16), dim3(256), 0, s, a, K, w, bias, act, n, out);
}

void launch_heatmap_gather(const float* logits, int n_classes, int col, int n, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_heatmap_gather, dim3((n + 255) / 256), dim3(256), 0, s, logits, n_classes, col, n, out);
}

}  // namespace bnhip
