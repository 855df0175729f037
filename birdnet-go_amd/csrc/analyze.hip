// File analysis on the device (analyze.h): the general framing kernel and the detection rows.  The framed form of the resident
// min/max + normalise launch, which reads its window straight out of the recording, is in frontend.hip.
#include "analyze.h"

#include <algorithm>

#include "block_scan.h"
#include "pcm_sample.h"
#include "ragged.h"

namespace bnhip {

// ------------------------------------------------------------------------------------------ k_frame_windows
// (one sample of the block as float32: frame_sample, pcm_sample.h)
// blockIdx.y = window of the launch, blockIdx.x strides over its samples
template <int BITS>
__global__ __launch_bounds__(256) void k_frame_windows(const char* __restrict__ block, WinView v, int n_samples, float* __restrict__ out) {
    const long long w = (long long)v.w0 + blockIdx.y;
    const int r = ragged_clip(v.first, v.n_rec, w);
    const long long s0 = (w - v.first[r]) * v.hop, len = v.slot[2 * r + 1];
    const char* rec = block + v.slot[2 * r];
    const int valid = (int)min((long long)n_samples, len - s0);
    float* o = out + (size_t)blockIdx.y * n_samples;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_samples; i += gridDim.x * 256) o[i] = i < valid ? frame_sample<BITS>(rec, s0 + i) : 0.0f;
}
void launch_frame_windows(const void* block, int bits, const WinView& v, int n, int n_samples, float* out, hipStream_t s) {
    if (n <= 0 || n_samples <= 0) return;
    const dim3 grid((unsigned)std::min((n_samples + 2047) / 2048, 64), (unsigned)n);
    const char* b = static_cast<const char*>(block);
    if (bits == 0) hipLaunchKernelGGL(k_frame_windows<0>, grid, dim3(256), 0, s, b, v, n_samples, out);
    else if (bits == 16) hipLaunchKernelGGL(k_frame_windows<16>, grid, dim3(256), 0, s, b, v, n_samples, out);
    else if (bits == 24) hipLaunchKernelGGL(k_frame_windows<24>, grid, dim3(256), 0, s, b, v, n_samples, out);
    else hipLaunchKernelGGL(k_frame_windows<32>, grid, dim3(256), 0, s, b, v, n_samples, out);
}

// ------------------------------------------------------------------------------------------ k_detections
// scratch: int off[W] (a window's first row, counted from its block's first row), then, 8-byte aligned, unsigned long long
// base[ceil(W / 256)] (a block's first row).
static size_t det_off_bytes(int W) { return ((size_t)W * 4 + 7) / 8 * 8; }
size_t detections_scratch_bytes(int W) { return det_off_bytes(W) + (size_t)((W + 255) / 256) * 8; }

__device__ __forceinline__ bool det_keeps(float c, float threshold) { return c >= threshold; }      // (false for a NaN)

// thread = window: its count, scanned over the block
__global__ __launch_bounds__(256) void k_det_count(const float* __restrict__ conf, int W, int k, float threshold, int* __restrict__ off,
                                                   unsigned long long* __restrict__ base) {
    __shared__ int sh[256];
    const int w = blockIdx.x * 256 + threadIdx.x;
    int c = 0;
    if (w < W) for (int j = 0; j < k; j++) c += det_keeps(conf[(size_t)w * k + j], threshold) ? 1 : 0;
    const int incl = block_scan(c, sh, threadIdx.x);
    if (w < W) off[w] = incl - c;
    if (threadIdx.x == 255) base[blockIdx.x] = (unsigned long long)incl;
}
// one block: the block totals in place -> exclusive bases, 256 at a time with a running carry; the grand total
__global__ __launch_bounds__(256) void k_det_bases(unsigned long long* __restrict__ base, int nb, unsigned long long* __restrict__ total) {
    __shared__ unsigned long long sh[256];
    unsigned long long carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const unsigned long long c = b < nb ? base[b] : 0ull;
        const unsigned long long incl = block_scan(c, sh, threadIdx.x);
        if (b < nb) base[b] = carry + incl - c;
        const unsigned long long sum = sh[255];
        __syncthreads();                          // (sh is written again by the next round's scan)
        carry += sum;
    }
    if (threadIdx.x == 0) *total = carry;
}
// thread = window: its kept rows in rank order from its offset on, as far as the caller's rows reach
__global__ __launch_bounds__(256) void k_det_scatter(const float* __restrict__ conf, const int32_t* __restrict__ idx, int W, int k, float threshold,
                                                     WinView v, const int* __restrict__ off, const unsigned long long* __restrict__ base,
                                                     DetRow* __restrict__ rows, unsigned long long cap) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= W) return;
    unsigned long long o = base[blockIdx.x] + (unsigned long long)off[w];
    if (o >= cap) return;
    const int r = ragged_clip(v.first, v.n_rec, (long long)w);
    const int win = (int)((long long)w - v.first[r]);
    for (int j = 0; j < k && o < cap; j++) {
        const float c = conf[(size_t)w * k + j];
        if (!det_keeps(c, threshold)) continue;
        rows[o++] = DetRow{r, win, idx[(size_t)w * k + j], c};
    }
}
void launch_detections(const float* conf, const int32_t* idx, int W, int k, float threshold, const WinView& v, void* scratch, DetRow* rows,
                       unsigned long long cap, unsigned long long* d_total, hipStream_t s) {
    if (W <= 0 || k <= 0) return;
    const int nb = (W + 255) / 256;
    int* off = static_cast<int*>(scratch);
    unsigned long long* base = reinterpret_cast<unsigned long long*>(static_cast<char*>(scratch) + det_off_bytes(W));
    hipLaunchKernelGGL(k_det_count, dim3(nb), dim3(256), 0, s, conf, W, k, threshold, off, base);
    hipLaunchKernelGGL(k_det_bases, dim3(1), dim3(256), 0, s, base, nb, d_total);
    if (cap) hipLaunchKernelGGL(k_det_scatter, dim3(nb), dim3(256), 0, s, conf, idx, W, k, threshold, v, off, base, rows, cap);
}

}  // namespace bnhip
