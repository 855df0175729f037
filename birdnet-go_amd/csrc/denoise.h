// Spectral noise reduction of detection clips, a uniform batch or a ragged burst (denoise.hip, api_denoise.cpp bnhip_denoise_* /
// bnhip_denoise_ragged_* / bnhip_process_pcm16 / bnhip_process_ragged_pcm16): int16 PCM ->
// framed, Hann-windowed real FFT -> per-bin gain against a white noise floor -> inverse FFT -> overlap-add -> int16, the spec of
// DESIGN.md §9 "Denoise" in fp64.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

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
DenoisePlan denoise_plan(int n_clips, int n, int N);
// The same of a ragged burst (ragged.h): lens[n_clips] >= 1 on the host.  T by the uniform rule with the burst's total tile count,
// the sum of ceil(hops_c / T) over the clips, in place of the product; F and the LDS from N and T as above.
DenoisePlan denoise_ragged_plan(int n_clips, const int* lens, int N);
// the ragged launch's device tables start | tile0, (n_clips + 1) 64-bit entries each, rounded up to 256 bytes
size_t denoise_ragged_table_bytes(int n_clips);

// [N/2] (cos, -sin)(2 pi j / N) pairs, then the N periodic Hann coefficients (spectrogram_table of that window)
std::vector<double> denoise_table(int N);

// pcm, out: int16 [n_clips][n], distinct; d_table: denoise_table on the device.  Arguments validated by the caller.
void launch_denoise(const int16_t* pcm, int n_clips, int n, int N, double nr_db, double nf_db, const double* d_table, int16_t* out,
                    hipStream_t s);

// The same of a ragged burst: pcm, out the clips packed back to back (distinct), lens on the host, d_tables
// denoise_ragged_table_bytes of device memory, 8-byte aligned, which a copy enqueued on s fills before the kernel.  The bytes of
// clip c are those of launch_denoise on that clip alone.
void launch_denoise_ragged(const int16_t* pcm, int n_clips, const int* lens, int N, double nr_db, double nf_db, const double* d_table,
                           int16_t* out, void* d_tables, hipStream_t s);

// out[i] = the pcmgain.h gain of pcm[i] at `factor` (in place allowed)
void launch_pcm_gain(const int16_t* pcm, size_t total, double factor, int16_t* out, hipStream_t s);

}  // namespace bnhip
