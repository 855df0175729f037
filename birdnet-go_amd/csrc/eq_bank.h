// Batched per-source equalizer (api_eq.cpp bnhip_eq_bank_*): one launch runs one call's PCM16 frames of every processed stream
// of a bank through its biquad stages, gain, clamp and truncation.  The descriptor table, the normalised coefficients and the
// packed PCM16 travel in one staging buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bnhip {

constexpr int EQ_MAX_STAGES = 16;     // one 16-lane DPP row per stream, lane s = stage s

// One stream of one call.  Its output has as many samples as its input and sits at the same offset of the packed output.
struct EqBankDesc {
    double gain;           // linear gain applied after the last stage
    int in_off;            // first sample of this stream's frames (back to back) in the packed PCM16, and of its output
    int n;                 // samples of the call
    int n_stages;          // 0..EQ_MAX_STAGES (0: gain only)
    int coef_off;          // double offset of stage 0's {b0, b1, b2, a1, a2} / a0 in the coefficient area
    int st_rd;             // double offset of the state slab read this call ([n_stages][in1, in2, out1, out2]); -1 = zero state
    int st_wr;             // double offset of the slab the new state goes to
    int blk_steps;         // (descriptor 4k only) steps every row of block k runs: max(n + max(n_stages, 1) - 1), a multiple of 16
    int pad;
};
static_assert(sizeof(EqBankDesc) == 40, "descriptor layout");

// One wave of 4 rows per 4 descriptors.  Returns 0 (nothing to do for n_desc <= 0).
int launch_eq_bank(const EqBankDesc* d_desc, int n_desc, const double* d_coef, const int16_t* d_pcm, double* d_state,
                   int16_t* d_out, hipStream_t s);

}  // namespace bnhip
