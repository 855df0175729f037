// Spectral noise reduction of detection clips, a uniform batch or a ragged burst (denoise.hip, api_denoise.cpp bnhip_denoise_* /
// bnhip_denoise_ragged_* / bnhip_process_pcm16 / bnhip_process_ragged_pcm16): int16 PCM ->
// framed, Hann-windowed real FFT -> per-bin gain against a white noise floor -> inverse FFT -> overlap-add -> int16, the spec of
// DESIGN.md §9 "Denoise" in fp64.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ragged.h"

namespace bnhip {

constexpr int DN_N_MIN = 64, DN_N_MAX = 4096;            // supported frame lengths, powers of two
constexpr double DN_NR_MIN = 0.0, DN_NR_MAX = 97.0;      // nr_db, afftdn's range for nr
constexpr double DN_NF_MIN = -80.0, DN_NF_MAX = -20.0;   // nf_db, afftdn's range for nf

// What the mapping chooses for one call (the spec fixes everything else): T output hops per block, F frames per round, the LDS.
// Neither T nor F changes a sample's bits: its four contributions are added in frame order whatever the grouping.
struct DenoisePlan {
    int T = 0, F = 0;
    size_t lds = 0;
};
// T by the call's total tile count, the sum of ceil(hops_c / T) over the clips (a uniform batch's: the product); F and the LDS
// from N and T.
DenoisePlan denoise_plan(const Clips& clips, int N);
// the device tables of a ragged launch: start | tile0, (n_clips + 1) 64-bit entries each, rounded up to 256 bytes; a uniform batch
// has none (0)
size_t denoise_table_bytes(const Clips& clips);

// [N/2] (cos, -sin)(2 pi j / N) pairs, then the N periodic Hann coefficients (spectrogram_table of that window)
std::vector<double> denoise_table(int N);

// pcm, out: int16 [n_clips][n], or the clips of a ragged burst packed back to back; distinct.  d_table: denoise_table on the device.
// d_tables: denoise_table_bytes of device memory, 8-byte aligned, which a copy enqueued on s fills before the kernel (not read for a
// uniform batch).  Arguments validated by the caller.  The bytes of clip c are those of a launch on that clip alone.
void launch_denoise(const int16_t* pcm, const Clips& clips, int N, double nr_db, double nf_db, const double* d_table, int16_t* out,
                    void* d_tables, hipStream_t s);

// out[i] = the pcmgain.h gain of pcm[i] at `factor` (in place allowed)
void launch_pcm_gain(const int16_t* pcm, size_t total, double factor, int16_t* out, hipStream_t s);

}  // namespace bnhip
