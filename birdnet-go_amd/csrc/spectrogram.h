// Detection-clip spectrogram images (spectrogram.hip, api_spectrogram.cpp bnhip_spectrogram_*): PCM -> uint8 level indices
// [n_clips][H][W], the rendering spec of DESIGN.md §9 in fp64.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ragged.h"

namespace bnhip {

constexpr int SPEC_N_MIN = 64, SPEC_N_MAX = 4096;       // supported transform lengths N = 2 (H - 1), powers of two

// The geometry of one call: what the spec fixes (N, K) and what the mapping chooses (T, F, the LDS layout).
struct SpecPlan {
    int N = 0;             // transform length 2 (H - 1)
    int K = 1;             // frames averaged per column: max(1, ceil(n / (W N)))
    int T = 0;             // columns per block
    int F = 0;             // frames transformed per round
    int span_cap = 0;      // samples of the staged span of one round: (F - 1) ceil(n / (K W)) + N + 2
    size_t lds = 0;        // bytes of dynamic LDS
};
SpecPlan spectrogram_plan(int n, int W, int H);

// One clip of a ragged burst as the kernel reads it: its first sample in the packed buffer and its own plan.
struct SpecClip {
    long long start;       // the sum of the lengths before it
    int n, K, F, span_cap;
};
static_assert(sizeof(SpecClip) == 24, "row layout");

// [N/2] (cos, -sin)(2 pi j / N) pairs, then the N window coefficients: the table the kernel reads, uploaded once per
// (device, N, window contents)
std::vector<double> spectrogram_table(int N, const double* window);

// samples: int16 PCM or (f32) float32 [n_clips][n], or the clips of a ragged burst packed back to back; d_table: spectrogram_table on
// the device; wsum = the window's sum; image: uint8 [n_clips][H][W].  d_rows: spectrogram_table_bytes of device memory for a ragged
// burst's SpecClip rows, filled by a copy enqueued on s ahead of the kernel (a uniform batch has none: 0 bytes, not read).  The
// geometry has been validated by the caller (H = 2^k + 1, N within SPEC_N_MIN..SPEC_N_MAX).
size_t spectrogram_table_bytes(const Clips& clips);
void launch_spectrogram(const void* samples, int f32, const Clips& clips, int W, int H, const double* d_table, double wsum, double top_db,
                        double range_db, uint8_t* image, void* d_rows, hipStream_t s);

}  // namespace bnhip
