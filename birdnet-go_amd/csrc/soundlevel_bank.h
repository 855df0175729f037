// Batched 1/3-octave sound level monitor (api_soundlevel.cpp bnhip_soundlevel_bank_*): one launch runs one call's PCM16 frames of every
// stream of a bank through the bank's band-pass biquads and returns, per band, the sum of squares of every 1-second block the
// call completes.  The descriptor table, the band table and the packed PCM16 travel in one staging buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bnhip {

constexpr int SL_MAX_BANDS = 32;      // one lane per band, 32 lanes (half a wave) per stream
constexpr int SL_STATE = 5;           // doubles of one band's state: {x1, x2, y1, y2, sum}
constexpr int SL_SLAB = SL_MAX_BANDS * SL_STATE;

// One stream of one call.
struct SoundLevelDesc {
    int in_off;            // first sample of this stream's frames (back to back) in the packed PCM16
    int n;                 // samples of the call
    int fill;              // samples already in the open 1-second block (0 .. fs - 1)
    int out_off;           // double offset of this stream's first finished block: block k, band j at out_off + k * n_bands + j
    int st_rd;             // double offset of the state slab read this call; -1 = zero state
    int st_wr;             // double offset of the slab the new state goes to
    int blk_steps;         // (descriptor 2k only) steps both streams of wave k run: the longer n, rounded up to 32
    int pad;
};
static_assert(sizeof(SoundLevelDesc) == 32, "descriptor layout");

// One wave of 2 streams per 2 descriptors; d_bands holds n_bands x {b0, b1, b2, a1, a2}.  Returns 0 (nothing to do for
// n_desc <= 0).
int launch_soundlevel_bank(const SoundLevelDesc* d_desc, int n_desc, const double* d_bands, int n_bands, int fs,
                           const int16_t* d_pcm, double* d_state, double* d_out, hipStream_t s);

}  // namespace bnhip
