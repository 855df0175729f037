// Batched streaming resampler (api.cpp bnhip_resampler_bank_*): one launch resamples one call's frames of every stream of a
// bank that shares (rate_in, rate_out).  The descriptor table travels in front of the packed PCM16 in one staging buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bnhip {

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

// LDS a launch of this geometry needs (phase table + worst-case input span of 256 outputs), as launch_resample
size_t resample_bank_lds(int L, int M, int T);
// returns 0 on success, -1 if the geometry does not fit LDS
int launch_resample_bank(const ResampleBankDesc* d_desc, int n_desc, int n_blocks, const int16_t* d_pcm, float* d_hist,
                         int16_t* d_out, const float* d_table, int L, int M, int T, int half, hipStream_t s);

}  // namespace bnhip
