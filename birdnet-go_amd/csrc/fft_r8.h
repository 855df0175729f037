// Register FFT building blocks.
// fft_regs<P>: radix-2 DIT on P = 2 / 4 / 8 / 16 complex values, outputs in natural order (the four-step STFT of stft.hip, the closing
// radix-2 / radix-4 pass of fft_passes.h).
// fft_r8_dft8: 8-point DFT on complex doubles in registers (decimation in frequency, three radix-2 stages with the W8 constants folded
// in).  Outputs land in bit-reversed slots: slot s holds y[kFftR8Slot[s]].  Shared by the ultrasonic power kernel
// (post.hip) and the in-LDS passes of the spectrogram and denoise kernels (fft_passes.h).
#pragma once

namespace bnhip {

// In-place radix-2 DIT on P complex doubles held in registers; every index is a compile-time constant after unrolling.
template <int P, typename R>
__device__ __forceinline__ void fft_regs(R (&re)[P], R (&im)[P]) {
    // cos / sin of 2 pi t / 16, t = 0..7 (P <= 16 uses a stride into this table)
    constexpr double C16[8] = {1.0, 0.92387953251128673848, 0.70710678118654752440, 0.38268343236508977173,
                               0.0, -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128673848};
    constexpr double S16[8] = {0.0, 0.38268343236508977173, 0.70710678118654752440, 0.92387953251128673848,
                               1.0, 0.92387953251128673848, 0.70710678118654752440, 0.38268343236508977173};
    constexpr int LOG = P == 16 ? 4 : (P == 8 ? 3 : (P == 4 ? 2 : 1));
#pragma unroll
    for (int i = 0; i < P; i++) {
        int j = 0;
#pragma unroll
        for (int bit = 0; bit < LOG; bit++) j |= ((i >> bit) & 1) << (LOG - 1 - bit);
        if (i < j) { R t = re[i]; re[i] = re[j]; re[j] = t; t = im[i]; im[i] = im[j]; im[j] = t; }
    }
#pragma unroll
    for (int len = 2; len <= P; len <<= 1) {
        const int half = len >> 1, step = 16 / len;
#pragma unroll
        for (int i = 0; i < P; i += len) {
#pragma unroll
            for (int k = 0; k < half; k++) {
                const R wr = (R)C16[k * step], wi = (R)-S16[k * step];      // e^{-2 pi i k / len}
                const R xr = re[i + k + half], xi = im[i + k + half];
                const R ur = re[i + k], ui = im[i + k];
                if (k == 0) {                                               // w = 1
                    re[i + k] = ur + xr; im[i + k] = ui + xi; re[i + k + half] = ur - xr; im[i + k + half] = ui - xi;
                } else if (2 * k == half) {                                 // w = -i
                    re[i + k] = ur + xi; im[i + k] = ui - xr; re[i + k + half] = ur - xi; im[i + k + half] = ui + xr;
                } else {                                                    // explicit FMAs (contraction is off file-wide)
                    re[i + k] = fma(xr, wr, fma(-xi, wi, ur));
                    im[i + k] = fma(xr, wi, fma(xi, wr, ui));
                    re[i + k + half] = fma(-xr, wr, fma(xi, wi, ur));
                    im[i + k + half] = fma(-xr, wi, fma(-xi, wr, ui));
                }
            }
        }
    }
}

__device__ __forceinline__ void fft_r8_dft8(double (&re)[8], double (&im)[8]) {
    constexpr double R = 0.70710678118654752440;
#pragma unroll
    for (int m = 0; m < 4; m++) {                    // stage 1: (m, m + 4), lower half times W8^m
        const double ur = re[m] + re[m + 4], ui = im[m] + im[m + 4], vr = re[m] - re[m + 4], vi = im[m] - im[m + 4];
        re[m] = ur; im[m] = ui;
        if (m == 0) { re[4] = vr; im[4] = vi; }
        else if (m == 1) { re[5] = (vr + vi) * R; im[5] = (vi - vr) * R; }       // (1 - i) / sqrt 2
        else if (m == 2) { re[6] = vi; im[6] = -vr; }                             // -i
        else { re[7] = (vi - vr) * R; im[7] = -(vr + vi) * R; }                   // (-1 - i) / sqrt 2
    }
#pragma unroll
    for (int h = 0; h < 8; h += 4)                   // stage 2: (m, m + 2) inside each half, lower element times W4^m
#pragma unroll
        for (int m = 0; m < 2; m++) {
            const int a = h + m, b = h + m + 2;
            const double ur = re[a] + re[b], ui = im[a] + im[b], vr = re[a] - re[b], vi = im[a] - im[b];
            re[a] = ur; im[a] = ui;
            if (m == 0) { re[b] = vr; im[b] = vi; } else { re[b] = vi; im[b] = -vr; }
        }
#pragma unroll
    for (int a = 0; a < 8; a += 2) {                 // stage 3: (m, m + 1)
        const double ur = re[a] + re[a + 1], ui = im[a] + im[a + 1], vr = re[a] - re[a + 1], vi = im[a] - im[a + 1];
        re[a] = ur; im[a] = ui; re[a + 1] = vr; im[a + 1] = vi;
    }
}
__device__ constexpr int kFftR8Slot[8] = {0, 4, 2, 6, 1, 5, 3, 7};

}  // namespace bnhip
