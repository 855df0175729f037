// Polyphase resampler (resample.hip): the filter design, the one-shot / streaming launch and the bank launch (api_resample.cpp
// bnhip_resampler_bank_*), which resamples one call's frames of every stream of a bank that shares (rate_in, rate_out).  The
// bank's descriptor table travels in front of the packed PCM16 in one staging buffer.  The slot launch (analyze_recordings.cpp) resamples
// a burst of recordings at their own rates and depths into the float32 slots that file analysis frames.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
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

// The polyphase geometry of one rate pair (resample.hip): L / M = rate_out / rate_in in lowest terms, T taps per phase and the
// filter half-length.  Output i's newest input is n0(i) = floor((i*M + half) / L); indices count from the stream start.
struct ResamplePlan {
    int L = 1, M = 1, T = 0, half = 0;
    // outputs computable once n_total inputs are known: every i whose newest tap n0(i) < n_total
    long long ready(long long n_total) const {
        const long long num = n_total * L - half;
        return num <= 0 ? 0 : (num + M - 1) / M;
    }
    // EstimateOutput analogue (resample.go:83-88): an upper bound for any call, whatever the state
    long long estimate(long long n_in) const { return n_in <= 0 ? 0 : (n_in * L + M - 1) / M + 1; }
    // outputs of n inputs followed by zeros: the one-shot length, and where a flush ends
    long long end(long long n) const { return (n * L + M - 1) / M; }
    // the first input the next call still needs once the outputs before i_end are out: n0(i_end) - (T-1), within [n_base, n_after]
    long long keep_from(long long i_end, long long n_base, long long n_after) const {
        return std::min(std::max((i_end * M + half) / L - (T - 1), n_base), n_after);
    }
    bool fits_lds() const { return resample_lds(L, M, T) <= RESAMPLE_LDS_MAX; }
};

// rate_in, rate_out > 0: L, M, and T / half as resample_design lays the filter out.  With a table the filter is designed too (the
// [L][T] phase table).
inline ResamplePlan resample_plan(int rate_in, int rate_out, std::vector<float>* table) {
    const int g = std::gcd(rate_in, rate_out);
    ResamplePlan p;
    p.L = rate_out / g;
    p.M = rate_in / g;
    // (saturated for ratios whose filter leaves an int: such a plan never fits LDS and is never designed)
    const long long half = (long long)RESAMPLE_HALF_FACTOR * std::max(p.L, p.M);
    p.half = (int)std::min<long long>(half, INT32_MAX);
    p.T = (int)std::min<long long>((2 * half + p.L) / p.L, INT32_MAX);
    if (table) resample_design(p.L, p.M, RESAMPLE_BETA, RESAMPLE_HALF_FACTOR, table, &p.T, &p.half);
    return p;
}

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

// The slot form (file analysis of recordings at their own rates and depths, analyze_recordings.cpp): recording r lies as it is in its file
// - n_in samples of `bits` (0 = float32, 16, 24 packed, 32) from byte in_off of the raw block - and becomes n_out float32 samples at
// byte out_off of the slot block, followed by zeros up to a whole quad (what analyze_slot_bytes(n_out, 0) reserves).  L == 0: the
// recording is at the model's rate and is only converted; else out[i] is resample_tile's fmaf chain over the [L][T] phase table at
// float tab_off of the call's concatenated table buffer, inputs outside the recording reading as zero.
struct ResampleSlotDesc {
    long long in_off, out_off;
    int n_in, n_out, bits;
    int L, M, T, half, tab_off;
};
static_assert(sizeof(ResampleSlotDesc) == 48, "descriptor layout");
// outputs of one block of k_resample_slots: the phase table is staged once per tile, the input span once per 256 outputs
// (a multiple of 256; -DBNHIP_RESAMPLE_SLOT_TILE=... builds another size to measure against, build.py BNHIP_EXTRA_FLAGS)
#ifndef BNHIP_RESAMPLE_SLOT_TILE
#define BNHIP_RESAMPLE_SLOT_TILE 4096
#endif
constexpr int RESAMPLE_SLOT_TILE = BNHIP_RESAMPLE_SLOT_TILE;
static_assert(RESAMPLE_SLOT_TILE >= 256 && RESAMPLE_SLOT_TILE % 256 == 0, "whole sub-tiles of 256 outputs");
inline long long resample_slot_tiles(long long n_out) { return (n_out + RESAMPLE_SLOT_TILE - 1) / RESAMPLE_SLOT_TILE; }
// One launch for the whole burst.  d_desc: [n_rec]; d_tile0: the prefix table [n_rec + 1] of resample_slot_tiles(n_out) (ragged.h);
// n_tiles = tile0[n_rec] <= INT_MAX; lds: the largest resample_lds of the call's plans (0 when every recording is convert-only),
// each <= RESAMPLE_LDS_MAX.
void launch_resample_slots(const void* d_raw, void* d_slots, const float* d_tables, const ResampleSlotDesc* d_desc, const long long* d_tile0,
                           int n_rec, long long n_tiles, size_t lds, hipStream_t s);
// The multichannel form (bnhip_analyze_channels_*): recording r is n_in FRAMES of d_channels[r] interleaved samples, and d_sel[r] (a
// channel index or CHANNEL_MIX, channels.h) says which value of a frame is staged.  The descriptor is the one above; the two
// tables [n_rec] lie beside it.  d_sel is read on the device when the launch runs: a measurement enqueued in front may write it.
void launch_resample_slots_mc(const void* d_raw, void* d_slots, const float* d_tables, const ResampleSlotDesc* d_desc, const long long* d_tile0,
                              int n_rec, long long n_tiles, size_t lds, const int* d_channels, const int* d_sel, hipStream_t s);

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
