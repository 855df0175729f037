// k_soundlevel_bank: the 1/3-octave sound level monitor's per-sample work (soundlevel.Processor, internal/audiocore/soundlevel/
// processor.go) for every stream of a bank in one launch.  Per stream, in the reference's float64 arithmetic:
//   x = float64(int16) / 32768                                          (convert.BytesToFloat64PCM16Into)
//   every band (processAudioSample :231-250):
//     y = b0*x + b1*x1 + b2*x2 - a1*y1 - a2*y2   (normalised by a0, evaluated left to right, no contraction, b1 term kept)
//     NaN, +-Inf or |y| > 100: state zeroed, y = x * 0.1
//     x2 = x1; x1 = x; y2 = y1; y1 = y
//   sum += y*y from 0.0 over every consecutive fs-sample block of the stream  (calculateRMS :427-437, before its sqrt)
// The host takes the block sums from here (sqrt, clamp, dB and the interval statistics run in api_soundlevel.cpp).
//
// Mapping: one lane per (stream, band), 32 lanes per stream, so one wave holds two streams.  The bands are independent: no
// cross-lane move sits on the recurrence.  Every lane of a stream needs the same input sample at each step: lane j of a stream
// loads sample j of the next 32-sample block one block ahead, and step j broadcasts it with v_readlane (a constant lane), off
// the recurrence.  Time is never split: a blocked IIR scan would round differently.  A stream's lanes count the samples of its
// open block (the host passes the fill it starts with) and write the block's sum as a double when it reaches fs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "soundlevel_bank.h"

namespace bnhip {

__global__ __launch_bounds__(64) void k_soundlevel_bank(const SoundLevelDesc* __restrict__ desc, int n_desc,
                                                        const double* __restrict__ bands, int n_bands, int fs,
                                                        const int16_t* __restrict__ pcm, double* __restrict__ state,
                                                        double* __restrict__ out) {
#pragma clang fp contract(off)
    const int band = threadIdx.x & 31;
    const bool upper = threadIdx.x >= 32;
    const int di = blockIdx.x * 2 + (threadIdx.x >> 5);
    const int steps = desc[blockIdx.x * 2].blk_steps;         // the same for every lane of the wave
    const bool row_live = di < n_desc;
    SoundLevelDesc d{};
    if (row_live) d = desc[di];
    const bool live = row_live && band < n_bands;
    double b0 = 0.0, b1 = 0.0, b2 = 0.0, a1 = 0.0, a2 = 0.0;
    double x1 = 0.0, x2 = 0.0, y1 = 0.0, y2 = 0.0, sum = 0.0;
    if (live) {
        const double* c = bands + band * 5;
        b0 = c[0]; b1 = c[1]; b2 = c[2]; a1 = c[3]; a2 = c[4];
        if (d.st_rd >= 0) {
            const double* st = state + d.st_rd + band * SL_STATE;
            x1 = st[0]; x2 = st[1]; y1 = st[2]; y2 = st[3]; sum = st[4];
        }
    }
    const int16_t* src = pcm + d.in_off;
    const int n = d.n;
    int pos = d.fill;                                          // samples in the open block
    double* dst = out + d.out_off + band;
    int xcur = (row_live && band < n) ? (int)src[band] : 0;
    for (int base = 0; base < steps; base += 32) {
        // the next block's 32 samples, one per lane, loaded now so that the load is off the recurrence
        const int nx = base + 32 + band;
        const int xnext = (row_live && nx < n) ? (int)src[nx] : 0;
#pragma unroll
        for (int j = 0; j < 32; j++) {
            const int lo = __builtin_amdgcn_readlane(xcur, j);
            const int hi = __builtin_amdgcn_readlane(xcur, 32 + j);
            const double x = (double)(upper ? hi : lo) / 32768.0;
            if (live && base + j < n) {
                double y = b0 * x + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2;
                if (!(__builtin_fabs(y) <= 100.0)) {           // NaN, +-Inf or |y| > maxFilterAmplitude: the filter restarts
                    x1 = 0.0; x2 = 0.0; y1 = 0.0; y2 = 0.0;
                    y = x * 0.1;
                }
                x2 = x1; x1 = x; y2 = y1; y1 = y;
                sum = sum + y * y;
                if (++pos == fs) {                             // a 1-second block is complete
                    *dst = sum;
                    dst += n_bands;
                    sum = 0.0;
                    pos = 0;
                }
            }
        }
        xcur = xnext;
    }
    if (live && n > 0) {
        double* st = state + d.st_wr + band * SL_STATE;
        st[0] = x1; st[1] = x2; st[2] = y1; st[3] = y2; st[4] = sum;
    }
}

int launch_soundlevel_bank(const SoundLevelDesc* d_desc, int n_desc, const double* d_bands, int n_bands, int fs,
                           const int16_t* d_pcm, double* d_state, double* d_out, hipStream_t s) {
    if (n_desc <= 0) return 0;
    hipLaunchKernelGGL(k_soundlevel_bank, dim3((n_desc + 1) / 2), dim3(64), 0, s, d_desc, n_desc, d_bands, n_bands, fs, d_pcm,
                       d_state, d_out);
    return 0;
}

}  // namespace bnhip
