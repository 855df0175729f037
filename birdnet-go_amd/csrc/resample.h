// Polyphase resampler (resample.hip): the filter design, the one-shot / streaming launch and the bank launch (api_resample.cpp
// bnhip_resampler_bank_*), which resamples one call's frames of every stream of a bank that shares (rate_in, rate_out).  The
// bank's descriptor table travels in front of the packed PCM16 in one staging buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace bnhip {

// the [L][T] phase table of rate ratio L/M (filter half-length half_factor * max(L, M) taps)
void resample_design(int L, int M, double beta, int half_factor, std::vector<float>* table, int* T_out, int* half_out);
// the design every entry point uses
constexpr double RESAMPLE_BETA = 5.0;
constexpr int RESAMPLE_HALF_FACTOR = 10;

// LDS a launch of this geometry needs (phase table + worst-case input span of 256 outputs); more than RESAMPLE_LDS_MAX does not run
size_t resample_lds(int L, int M, int T);
constexpr size_t RESAMPLE_LDS_MAX = 150 * 1024;

// returns 0 on success, -1 if the geometry does not fit LDS
int launch_resample(const void* d_in, void* d_out, const float* d_table, int in_pcm16, int out_pcm16, int n_clips, int n_in,
                    int n_out, int L, int M, int T, int half, long long i_base, long long n_base, hipStream_t s);

// The one-shot PCM16 -> float32 form for a ragged burst: clip c of lens_in[c] samples packed back to back gives lens_out[c] =
// bnhip_resample_length(lens_in[c], ..) >= 1 floats, packed the same way (host arrays).  d_tables: device memory of
// resample_ragged_table_bytes(n_clips) bytes, filled by a copy enqueued on s ahead of the kernel.  One launch whatever the lengths;
// the sum of ceil(lens_out[c] / 256) must fit a 31-bit grid.  returns 0 on success, -1 if the geometry does not fit LDS
size_t resample_ragged_table_bytes(int n_clips);
int launch_resample_ragged(const int16_t* d_in, float* d_out, const float* d_table, int n_clips, const int* lens_in, const int* lens_out,
                           int L, int M, int T, int half, void* d_tables, hipStream_t s);

// One stream of one call.  Stream indices (n_base, i_next, keep_from) are positions since the stream started.
struct ResampleBankDesc {
    long long n_base;      // stream index of the first history sample
    long long i_next;      // stream index of this call's first output
    long long keep_from;   // stream index of the first sample of the new history
    int in_off;            // this stream's first input sample in the packed PCM16 (its frames of the call, back to back)
    int n_in;              // input samples of the call
    int n_hist;            // valid floats in the slab read this call
    int hist_rd;           // float offset of the slab read this call
    int hist_wr;           // float offset of the slab the new tail goes to
    int keep;              // floats of the new tail
    int cnt;               // outputs of the call
    int out_off;           // first output in the packed output
    int block0;            // first block of this stream in the flattened grid: ceil(cnt / 256) tile blocks, then one tail block
    int pad;
};
static_assert(sizeof(ResampleBankDesc) == 64, "descriptor layout");

// returns 0 on success, -1 if the geometry does not fit LDS
int launch_resample_bank(const ResampleBankDesc* d_desc, int n_desc, int n_blocks, const int16_t* d_pcm, float* d_hist,
                         int16_t* d_out, const float* d_table, int L, int M, int T, int half, hipStream_t s);

}  // namespace bnhip
