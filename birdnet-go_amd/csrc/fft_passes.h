// The in-LDS forward transform of the framed fp64 kernels (spectrogram.hip, denoise.hip): F packed frames of N/2 complex points each,
// transformed together and in place by radix-8 decimation-in-frequency passes (fft_r8_dft8, one butterfly per thread and step, the
// block's threads spread over all frames of the round) closed by one radix-2 / radix-4 pass (fft_regs) when N/2 is not a power of
// 8 - the pass structure of k_us_frame_power8 with the length a parameter.  Z[k] ends up at the mixed-radix digit-reversed index
// fft_pos(k).  A frame is [re | im], FS = SPEC_PHYS(N/2) doubles each.
#pragma once
#include <hip/hip_runtime.h>

#include "fft_r8.h"

namespace bnhip {

#define SPEC_PHYS(i) ((i) + ((i) >> 3))      // one pad per 8 doubles, as US8_PHYS: the last radix-8 pass walks with stride 8

struct FftPasses {
    int log2n2, npass, lg[4];                // N/2 = 2^log2n2 = product of the passes' radices 2^lg[i]
};

inline FftPasses fft_passes_plan(int N) {
    FftPasses p{};
    while ((2 << p.log2n2) < N) p.log2n2++;
    for (int rem = p.log2n2; rem > 0;) { const int lr = rem >= 3 ? 3 : rem; p.lg[p.npass++] = lr; rem -= lr; }
    return p;
}

// where Z[k] lies after the passes: digit i of k (radix 2^lg[i], least significant first) becomes the digit of weight N/2 / (r_0 .. r_i)
__device__ __forceinline__ int fft_pos(const FftPasses& p, int k) {
    int pos = 0, rem = p.log2n2;
    for (int i = 0; i < p.npass; i++) {
        rem -= p.lg[i];
        pos |= (k & ((1 << p.lg[i]) - 1)) << rem;
        k >>= p.lg[i];
    }
    return pos;
}

// closing pass (span 1: no twiddles): R consecutive points, natural-order outputs
template <int R>
__device__ __forceinline__ void fft_pass_small(double* zr, double* zi, int base) {
    double re[R], im[R];
#pragma unroll
    for (int m = 0; m < R; m++) { const int i = SPEC_PHYS(base + m); re[m] = zr[i]; im[m] = zi[i]; }
    fft_regs<R, double>(re, im);
#pragma unroll
    for (int m = 0; m < R; m++) { const int i = SPEC_PHYS(base + m); zr[i] = re[m]; zi[i] = im[m]; }
}

// All passes over the nf frames at `work`, by the whole block (THREADS threads, every one calls it); tw: [N/2] (cos, -sin)(2 pi j / N).
// The frames are complete before the call (a barrier has passed) and after it.
template <int THREADS>
__device__ __forceinline__ void fft_passes_run(const FftPasses& p, const double2* __restrict__ tw, double* work, int nf, int tid) {
    const int N2 = 1 << p.log2n2, FS = SPEC_PHYS(N2);
    int lgL = p.log2n2;                                          // the pass splits blocks of 2^lgL points
    for (int ps = 0; ps < p.npass; ps++) {
        const int lr = p.lg[ps], sp = 1 << (lgL - lr);           // radix 2^lr, butterfly stride sp
        const int per = p.log2n2 - lr;                           // log2 butterflies per frame
        for (int u = tid; u < (nf << per); u += THREADS) {
            const int f = u >> per, t = u & ((1 << per) - 1);
            const int j = t & (sp - 1), base = ((t - j) << lr) + j;
            double* zr = work + (size_t)f * 2 * FS;
            double* zi = zr + FS;
            if (lr == 3) {
                double re[8], im[8];
#pragma unroll
                for (int m = 0; m < 8; m++) { const int i = SPEC_PHYS(base + m * sp); re[m] = zr[i]; im[m] = zi[i]; }
                fft_r8_dft8(re, im);
                const int tstep = j << (p.log2n2 + 1 - lgL);     // W_L^(j q) = W_N^(q * tstep)
#pragma unroll
                for (int sl = 0; sl < 8; sl++) {
                    const int q = kFftR8Slot[sl];
                    double yr = re[sl], yi = im[sl];
                    if (q != 0 && sp > 1) {
                        const int e = q * tstep;                 // < 7 N / 8
                        double2 w = tw[e & (N2 - 1)];
                        if (e >= N2) { w.x = -w.x; w.y = -w.y; }
                        const double tr = yr * w.x - yi * w.y, ti = yr * w.y + yi * w.x;
                        yr = tr; yi = ti;
                    }
                    const int i = SPEC_PHYS(base + q * sp);
                    zr[i] = yr; zi[i] = yi;
                }
            } else if (lr == 2) fft_pass_small<4>(zr, zi, base);
            else fft_pass_small<2>(zr, zi, base);
        }
        __syncthreads();
        lgL -= lr;
    }
}

}  // namespace bnhip
