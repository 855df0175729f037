// k_eq_bank: the analysis route's EQ + gain (AudioRouter.applyProcessing, internal/audiocore/router.go:1006-1080) for every
// processed stream of a bank in one launch.  Per stream, in the reference's float64 arithmetic:
//   x = float64(int16) / 32768                                          (convert.BytesToFloat64PCM16Into)
//   every stage (filter f, pass p, in chain order):                     (equalizer.Filter.ApplyBatch)
//     y = b0*x + b1*in1 + b2*in2 - a1*out1 - a2*out2   (normalised by a0, evaluated left to right, no contraction)
//   y *= gain; clamp to [-1, 1]; int16(y * 32767), truncated            (convert.Float64ToBytesPCM16)
//
// Mapping: one 16-lane DPP row per stream (4 streams per wave), lane s runs stage s.  At step t lane s processes sample t - s:
// its input is lane s-1's output of step t-1, moved one lane on by row_shr:1; lane 0 takes the next input sample, which a
// row_shl:1 rotation of 16 prefetched samples brings to it.  Running the stages sample by sample in a pipeline gives the same
// doubles as the reference's pass after pass over the whole batch (each stage is causal and owns its state), and only the
// out1 recurrence of a stage is serial.  Time is never split: a blocked IIR scan would round differently.  The last stage's
// lane converts to int16 and drops the value into a 16-lane row_ror:1 rotation, so after 16 steps the row holds 16
// consecutive outputs and stores them with one instruction.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "eq_bank.h"

namespace bnhip {

namespace {

constexpr int DPP_ROW_SHL1 = 0x101, DPP_ROW_SHR1 = 0x111, DPP_ROW_ROR1 = 0x121;

template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true);
}

template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = dpp_i<CTRL>((int)(b & 0xffffffffll));
    const int hi = dpp_i<CTRL>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

}  // namespace

__global__ __launch_bounds__(64) void k_eq_bank(const EqBankDesc* __restrict__ desc, int n_desc, const double* __restrict__ coef,
                                                const int16_t* __restrict__ pcm, double* __restrict__ state,
                                                int16_t* __restrict__ out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 15;
    const int di = blockIdx.x * 4 + (threadIdx.x >> 4);
    const int steps = desc[blockIdx.x * 4].blk_steps;         // the same for every lane of the wave: DPP rows stay in step
    const bool row_live = di < n_desc;
    EqBankDesc d{};
    if (row_live) d = desc[di];
    const int S = d.n_stages;
    const int last = S > 0 ? S - 1 : 0;                        // the lane whose output is the stream's
    const bool stage = lane < S;
    double b0 = 0.0, b1 = 0.0, b2 = 0.0, a1 = 0.0, a2 = 0.0;
    double in1 = 0.0, in2 = 0.0, out1 = 0.0, out2 = 0.0;
    if (stage) {
        const double* c = coef + d.coef_off + lane * 5;
        b0 = c[0]; b1 = c[1]; b2 = c[2]; a1 = c[3]; a2 = c[4];
        if (d.st_rd >= 0) {
            const double* st = state + d.st_rd + lane * 4;
            in1 = st[0]; in2 = st[1]; out1 = st[2]; out2 = st[3];
        }
    }
    const int16_t* src = pcm + d.in_off;
    int16_t* dst = out + d.in_off;
    const int n = d.n;
    const double gain = d.gain;
    double y = 0.0;
    int xin = (row_live && lane < n) ? (int)src[lane] : 0;
    for (int base = 0; base < steps; base += 16) {
        // the next 16 input samples, loaded now so that the load is off the recurrence
        const int nx = base + 16 + lane;
        const int xin_next = (row_live && nx < n) ? (int)src[nx] : 0;
        int ob = 0;
        for (int j = 0; j < 16; j++) {
            const int t = base + j;
            const double xs = dpp_d<DPP_ROW_SHR1>(y);          // lane s-1's output of step t-1 = stage s's input of sample t-s
            const double x = lane == 0 ? (double)xin / 32768.0 : xs;
            const int i = t - lane;                            // the sample this lane processes at step t
            const bool act = lane <= last && i >= 0 && i < n;
            double v;
            if (stage) {
                v = b0 * x + b1 * in1 + b2 * in2 - a1 * out1 - a2 * out2;
                if (act) { in2 = in1; in1 = x; out2 = out1; out1 = v; }
            } else {
                v = x;                                         // a gain-only stream: lane 0 passes the sample on
            }
            y = v;
            ob = dpp_i<DPP_ROW_ROR1>(ob);
            if (lane == last && act) {
                double g = v * gain;
                g = g > 1.0 ? 1.0 : (g < -1.0 ? -1.0 : g);
                ob = (int)(int16_t)(int)(g * 32767.0);        // truncation toward zero, as Go's int16(float64)
            }
            xin = dpp_i<DPP_ROW_SHL1>(xin);
        }
        // the value lane `last` produced at step j was rotated 15 - j times: lane L holds step j = (last + 15 - L) mod 16, which
        // is output o = base + j - last; the 16 lanes cover 16 consecutive outputs
        const int o = base + ((last + 15 - lane) & 15) - last;
        if (row_live && o >= 0 && o < n) dst[o] = (int16_t)ob;
        xin = xin_next;
    }
    if (stage && row_live && n > 0) {
        double* st = state + d.st_wr + lane * 4;
        st[0] = in1; st[1] = in2; st[2] = out1; st[3] = out2;
    }
}

int launch_eq_bank(const EqBankDesc* d_desc, int n_desc, const double* d_coef, const int16_t* d_pcm, double* d_state,
                   int16_t* d_out, hipStream_t s) {
    if (n_desc <= 0) return 0;
    hipLaunchKernelGGL(k_eq_bank, dim3((n_desc + 3) / 4), dim3(64), 0, s, d_desc, n_desc, d_coef, d_pcm, d_state, d_out);
    return 0;
}

}  // namespace bnhip
