// gfx950 elementwise ops, post-processing (activation, top-k) and the ultrasonic frame-CV kernels.
#include "kernels.h"
#include "pw_common.h"
#include "fft_r8.h"

#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace bnhip {

// ------------------------------------------------------------------------------------------ generic elementwise
__global__ void k_unary(const float* __restrict__ in, float* __restrict__ out, size_t n, int act) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = apply_act(in[i], act);
}
void launch_unary(const float* in, float* out, size_t n, int act, hipStream_t s) {
    size_t blocks = (n + 255) / 256; if (blocks > 16384) blocks = 16384; if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_unary, dim3((unsigned)blocks), dim3(256), 0, s, in, out, n, act);
}
__global__ void k_binary(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, size_t n,
                         int op, int mode, int HW, int C, int act) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        float y = mode == 0 ? b[i] : (mode == 2 ? b[0] : b[(i / ((size_t)HW * C)) * C + (i % C)]);
        float x = a[i];
        float v = op == 0 ? x + y : (op == 1 ? x * y : x - y);
        out[i] = apply_act(v, act);
    }
}
void launch_binary(const float* a, const float* b, float* out, size_t n, int op, int mode, int HW, int C, int act,
                   hipStream_t s) {
    size_t blocks = (n + 255) / 256; if (blocks > 16384) blocks = 16384; if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_binary, dim3((unsigned)blocks), dim3(256), 0, s, a, b, out, n, op, mode, HW, C, act);
}

// ------------------------------------------------------------------------------------------ post-processing
// classifier/analyze.go:113-115,197-208 (mode 0); onnx/postprocess.go:8-10 (mode 2)
__global__ void k_sigmoid(const float* __restrict__ x, float* __restrict__ out, size_t n, int mode, double sens) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) out[i] = (float)(1.0 / (1.0 + exp(-sens * (double)x[i])));
    else out[i] = 1.0f / (1.0f + (float)exp((double)(-x[i])));
}
// classifier/perch_onnx.go:315-335: f32 max, e = float32(exp(float64(x - m))), f32 sum in index order, divide
__global__ __launch_bounds__(256) void k_softmax(const float* __restrict__ x, float* __restrict__ out, int n) {
    __shared__ float red[4];
    __shared__ float s_sum;
    const float* xr = x + (size_t)blockIdx.x * n;
    float* orow = out + (size_t)blockIdx.x * n;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, xr[i]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    for (int i = threadIdx.x; i < n; i += 256) orow[i] = (float)exp((double)(xr[i] - m));
    __syncthreads();
    if (threadIdx.x == 0) {          // sequential f32 sum in index order == the Go loop, bit for bit
        float sum = 0.f;
        for (int i = 0; i < n; i++) sum += orow[i];
        s_sum = sum;
    }
    __syncthreads();
    float sum = s_sum;
    for (int i = threadIdx.x; i < n; i += 256) orow[i] = orow[i] / sum;
}
void launch_activation(const float* logits, float* conf, int n_clips, int n_classes, int activation, double sens,
                       hipStream_t s) {
    if (activation == 1) {
        hipLaunchKernelGGL(k_softmax, dim3(n_clips), dim3(256), 0, s, logits, conf, n_classes);
    } else {
        size_t n = (size_t)n_clips * n_classes;
        hipLaunchKernelGGL(k_sigmoid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, logits, conf, n, activation, sens);
    }
}

// top-k by confidence, descending; ties resolved to the lower label index (the reference's order for
// ties is implementation-defined: analyze.go:120-124 uses the unstable sort.Slice).
__global__ __launch_bounds__(256) void k_topk(const float* __restrict__ conf, int n, int k, float* __restrict__ oc,
                                              int32_t* __restrict__ oi) {
    extern __shared__ float v[];
    __shared__ float rv[4];
    __shared__ int ri[4];
    const float* row = conf + (size_t)blockIdx.x * n;
    // NaN confidences (non-finite logits) rank below everything: loaded as -inf, so every emitted index is in [0, n)
    for (int i = threadIdx.x; i < n; i += 256) { float x = row[i]; v[i] = x != x ? -INFINITY : x; }
    __syncthreads();
    int kk = k < n ? k : n;
    for (int r = 0; r < kk; r++) {
        float best = -INFINITY; int bi = 0x7fffffff;
        for (int i = threadIdx.x; i < n; i += 256) {
            float x = v[i];
            if (x > best || (x == best && i < bi)) { best = x; bi = i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            float ob = __shfl_down(best, o, 64); int oidx = __shfl_down(bi, o, 64);
            if (ob > best || (ob == best && oidx < bi)) { best = ob; bi = oidx; }
        }
        if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = best; ri[threadIdx.x >> 6] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++)
                if (rv[w] > best || (rv[w] == best && ri[w] < bi)) { best = rv[w]; bi = ri[w]; }
            oc[(size_t)blockIdx.x * k + r] = best;
            oi[(size_t)blockIdx.x * k + r] = bi;
            if (bi >= 0 && bi < n) v[bi] = __builtin_nanf("");      // taken: NaN never compares > or ==, so -inf ties stay selectable
        }
        __syncthreads();
    }
}
void launch_topk(const float* conf, int n_clips, int n_classes, int k, float* out_conf, int32_t* out_idx,
                 hipStream_t s) {
    if ((size_t)n_classes * sizeof(float) > 48 * 1024)      // class counts above 12 K need more than the default dynamic LDS (per device: not cached)
        lds_limit_once<&k_topk>(160 * 1024 - 256);
    hipLaunchKernelGGL(k_topk, dim3(n_clips), dim3(256), (size_t)n_classes * sizeof(float), s, conf, n_classes, k,
                       out_conf, out_idx);
}

// ------------------------------------------------------------------------------------------ ultrasonic frame-CV
// internal/audiocore/ultrasonic/filter.go:20-66 in float64.  One block per (frame, clip); the 8192-point
// complex128 FFT lives entirely in LDS (128 KiB of the CU's 160 KiB): bit-reversed load with the symmetric
// Hann window applied, radix-2 DIT stages with directly evaluated twiddles (the Go code's w *= wn recurrence
// only adds rounding noise), then the one-sided power sum above the split bin.
// T = double (the reference's float64 samples) or int16_t (raw PCM: int16 / 32768 as float64, convert/pcm.go:108-113)
template <typename T>
__global__ __launch_bounds__(1024) void k_us_frame_power(const T* __restrict__ samples, int n, int fft, int hop,
                                                         int frames, int split_bin, int log2n,
                                                         const double2* __restrict__ tw /* [fft/2] (cos, -sin)(2 pi j / fft), then the Hann window [fft] */,
                                                         double* __restrict__ powers) {
    extern __shared__ __attribute__((aligned(16))) double lds[];   // re[fft], im[fft]
    double* re = lds; double* im = lds + fft;
    __shared__ double red[16];
    const int frame = blockIdx.x, clip = blockIdx.y;
    const T* x = samples + (size_t)clip * n + (size_t)frame * hop;
    const double* __restrict__ hann = reinterpret_cast<const double*>(tw + fft / 2);    // symmetric Hann window, filter.go:139-145
    for (int i = threadIdx.x; i < fft; i += blockDim.x) {
        double w = hann[i];
        unsigned j = __brev((unsigned)i) >> (32 - log2n);
        const double xv = std::is_same<T, int16_t>::value ? (double)x[i] / 32768.0 : (double)x[i];
        re[j] = xv * w; im[j] = 0.0;
    }
    __syncthreads();
    // twiddles from a plan-time table (L1 / L2 resident, 64 KiB for 8192 points): evaluating sincos in float64 per butterfly
    // was ~5x the butterfly arithmetic itself (2.0 ms for 256 x 34 frames; the Go code's w *= wn recurrence only adds noise)
    int shift = log2n - 1;
    for (int size = 2; size <= fft; size <<= 1, shift--) {
        int half = size >> 1;
        for (int t = threadIdx.x; t < fft / 2; t += blockDim.x) {
            int k = t & (half - 1);
            int i0 = ((t - k) << 1) + k, i1 = i0 + half;
            const double2 w = tw[k << shift];
            const double c = w.x, s = w.y;
            double vr = c * re[i1] - s * im[i1], vi = c * im[i1] + s * re[i1];
            double ur = re[i0], ui = im[i0];
            re[i0] = ur + vr; im[i0] = ui + vi; re[i1] = ur - vr; im[i1] = ui - vi;
        }
        __syncthreads();
    }
    const int nyq = fft / 2;
    double pw = 0.0;
    for (int b = split_bin + threadIdx.x; b <= nyq; b += blockDim.x) {
        double q = re[b] * re[b] + im[b] * im[b];
        if (b > 0 && b < nyq) q *= 2.0;
        pw += q;
    }
    for (int o = 32; o > 0; o >>= 1) pw += __shfl_down(pw, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = pw;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); w++) sum += red[w];
        powers[(size_t)clip * frames + frame] = sum;
    }
}
// 8192-point frames (the reference's default, filter.go:20-66) the fast way.  The frame is real: its even / odd samples are
// packed into 4096 complex points, transformed by four in-place radix-8 decimation-in-frequency passes (512 threads, one 8-point
// butterfly per thread and pass, the 8-point DFT in registers: 4 LDS round trips instead of the 13 of the radix-2 kernel above,
// on half the data), and the spectrum of the real frame is recovered on the fly in the power sum: X[k] = E[k] + W^k O[k] with
// E, O from Z[k] and conj(Z[4096 - k]).  DIF leaves Z[k] at the base-8 digit-reversed index.  LDS index i lives at i + (i >> 3)
// (one pad per 8 doubles: the last pass walks the array with stride 8).  73.7 KB of LDS per frame: two frames per CU.
#define US8_N2 4096
#define US8_PHYS(i) ((i) + ((i) >> 3))
template <typename T>
__global__ __launch_bounds__(512) void k_us_frame_power8(const T* __restrict__ samples, int n, int hop, int frames, int split_bin,
                                                         const double2* __restrict__ tw /* [4096] (cos, -sin)(2 pi j / 8192), then Hann [8192] */,
                                                         double* __restrict__ powers) {
    extern __shared__ __attribute__((aligned(16))) double us8_lds[];
    double* zr = us8_lds; double* zi = us8_lds + US8_PHYS(US8_N2);
    __shared__ double red[8];
    const int tid = threadIdx.x, frame = blockIdx.x, clip = blockIdx.y;
    const T* x = samples + (size_t)clip * n + (size_t)frame * hop;
    const double* __restrict__ hann = reinterpret_cast<const double*>(tw + US8_N2);
    auto sample = [&](int i) -> double { return std::is_same<T, int16_t>::value ? (double)x[i] / 32768.0 : (double)x[i]; };
    for (int i = tid; i < US8_N2; i += 512) {
        zr[US8_PHYS(i)] = sample(2 * i) * hann[2 * i];
        zi[US8_PHYS(i)] = sample(2 * i + 1) * hann[2 * i + 1];
    }
    __syncthreads();
#pragma unroll 1
    for (int st = 0; st < 4; st++) {
        const int L = US8_N2 >> (3 * st), span = L >> 3;
        const int j = tid & (span - 1), base = ((tid - j) << 3) + j;  // (tid / span) * L + j
        double re[8], im[8];
#pragma unroll
        for (int m = 0; m < 8; m++) { const int i = US8_PHYS(base + m * span); re[m] = zr[i]; im[m] = zi[i]; }
        fft_r8_dft8(re, im);
        const int tstep = j * (8192 / L);                            // W_L^(j q) = W_8192^(q * tstep)
#pragma unroll
        for (int sl = 0; sl < 8; sl++) {
            const int q = kFftR8Slot[sl];
            double yr = re[sl], yi = im[sl];
            if (q != 0 && st < 3) {                                  // the last pass has span 1: j = 0, no twiddles
                int e = q * tstep;                                   // < 7168
                double2 w = tw[e & 4095];
                if (e >= 4096) { w.x = -w.x; w.y = -w.y; }
                const double tr = yr * w.x - yi * w.y, ti = yr * w.y + yi * w.x;
                yr = tr; yi = ti;
            }
            const int i = US8_PHYS(base + q * span);
            zr[i] = yr; zi[i] = yi;
        }
        __syncthreads();
    }
    // power above the split bin (filter.go:48-63) from the spectrum of the real frame
    auto rev = [](int k) { return ((k & 7) << 9) | (((k >> 3) & 7) << 6) | (((k >> 6) & 7) << 3) | ((k >> 9) & 7); };
    const int nyq = US8_N2;                                          // bin index of the Nyquist frequency (fft / 2)
    double pw = 0.0;
    for (int b = split_bin + tid; b <= nyq; b += 512) {
        double xr, xi;
        if (b == nyq) { const int i0 = US8_PHYS(0); xr = zr[i0] - zi[i0]; xi = 0.0; }
        else {
            const int ia = US8_PHYS(rev(b)), ib = US8_PHYS(rev((US8_N2 - b) & (US8_N2 - 1)));
            const double ar = zr[ia], ai = zi[ia], br = zr[ib], bi = -zi[ib];      // Z[b], conj(Z[N2 - b])
            const double er = 0.5 * (ar + br), ei = 0.5 * (ai + bi);
            const double dr = ar - br, di = ai - bi;
            const double orr = 0.5 * di, oi = -0.5 * dr;                             // O = -i/2 (Z[b] - conj(Z[N2 - b]))
            const double2 w = tw[b];                                                 // W_8192^b
            xr = er + (orr * w.x - oi * w.y); xi = ei + (orr * w.y + oi * w.x);
        }
        double q = xr * xr + xi * xi;
        if (b > 0 && b < nyq) q *= 2.0;
        pw += q;
    }
    for (int o = 32; o > 0; o >>= 1) pw += __shfl_down(pw, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = pw;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int w = 0; w < 8; w++) sum += red[w];
        powers[(size_t)clip * frames + frame] = sum;
    }
}

std::vector<double> us_twiddle_table(int fft_size) {
    std::vector<double> t((size_t)2 * fft_size);             // fft/2 (cos, -sin) pairs, then the fft window coefficients
    for (int j = 0; j < fft_size / 2; j++) {
        const double a = 6.283185307179586476925286766559 * (double)j / (double)fft_size;
        t[2 * j] = std::cos(a); t[2 * j + 1] = -std::sin(a);
    }
    const double hw = 6.283185307179586476925286766559 / (double)(fft_size - 1);
    for (int i = 0; i < fft_size; i++) t[(size_t)fft_size + i] = 0.5 * (1.0 - std::cos(hw * (double)i));   // filter.go:139-145
    return t;
}
void launch_us_frame_power(const void* samples, int pcm16, int n_clips, int n, int fft_size, int hop, int frames, int split_bin,
                           const double* d_tw, double* powers, hipStream_t s) {
    const double2* tw = reinterpret_cast<const double2*>(d_tw);
    static const bool no8 = getenv("BNHIP_US_RADIX2") != nullptr;
    if (fft_size == 8192 && !no8) {
        const size_t lds8 = (size_t)2 * US8_PHYS(US8_N2) * sizeof(double);
        if (pcm16) {
            lds_limit_once<&k_us_frame_power8<int16_t>>(80 * 1024);
            hipLaunchKernelGGL(k_us_frame_power8<int16_t>, dim3(frames, n_clips), dim3(512), lds8, s, static_cast<const int16_t*>(samples), n, hop,
                               frames, split_bin, tw, powers);
        } else {
            lds_limit_once<&k_us_frame_power8<double>>(80 * 1024);
            hipLaunchKernelGGL(k_us_frame_power8<double>, dim3(frames, n_clips), dim3(512), lds8, s, static_cast<const double*>(samples), n, hop,
                               frames, split_bin, tw, powers);
        }
        return;
    }
    int log2n = 0; while ((1 << log2n) < fft_size) log2n++;
    size_t lds = (size_t)fft_size * 2 * sizeof(double);
    int threads = fft_size / 2 < 1024 ? (fft_size / 2 < 64 ? 64 : fft_size / 2) : 1024;
    if (pcm16) {
        lds_limit_once<&k_us_frame_power<int16_t>>(160 * 1024 - 256);
        hipLaunchKernelGGL(k_us_frame_power<int16_t>, dim3(frames, n_clips), dim3(threads), lds, s, static_cast<const int16_t*>(samples), n,
                           fft_size, hop, frames, split_bin, log2n, tw, powers);
    } else {
        lds_limit_once<&k_us_frame_power<double>>(160 * 1024 - 256);
        hipLaunchKernelGGL(k_us_frame_power<double>, dim3(frames, n_clips), dim3(threads), lds, s, static_cast<const double*>(samples), n,
                           fft_size, hop, frames, split_bin, log2n, tw, powers);
    }
}
// filter.go:76-97, sequential like the Go loop
__global__ void k_us_cv(const double* __restrict__ powers, int frames, double* __restrict__ cv) {
    if (threadIdx.x != 0) return;
    const double* p = powers + (size_t)blockIdx.x * frames;
    double n = (double)frames, sum = 0.0;
    if (frames < 2) { cv[blockIdx.x] = 0.0; return; }
    for (int i = 0; i < frames; i++) sum += p[i];
    double mean = sum / n;
    if (mean <= 0.0) { cv[blockIdx.x] = 0.0; return; }
    double sq = 0.0;
    for (int i = 0; i < frames; i++) { double d = p[i] - mean; sq += d * d; }
    cv[blockIdx.x] = sqrt(sq / n) / mean;
}
void launch_us_cv(const double* powers, int n_clips, int frames, double* cv, hipStream_t s) {
    hipLaunchKernelGGL(k_us_cv, dim3(n_clips), dim3(64), 0, s, powers, frames, cv);
}

}  // namespace bnhip
