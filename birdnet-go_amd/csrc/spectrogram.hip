// Detection-clip spectrogram images for gfx950: PCM -> framed, windowed real FFT (fp64) -> mean power of a column's K frames ->
// dB -> level index 0..255 -> uint8 [n_clips][H][W], Nyquist in row 0.  The rendering spec (frame centres, normalisation, level
// rule) is DESIGN.md §9; tests/specref.py restates it in numpy float64.
//
// Reference path being replaced: the `sox ... rate 24k spectrogram -x W -y H -z R -r` child process per clip of
// internal/spectrogram/generator.go:425-530.  sox is not in the reference tree: pixel values are this project's spec, not sox's.
//
// Mapping.  A block of 256 threads owns T consecutive columns of one clip (T = 32 / 16 / 8 for N <= 1024 / 2048 / 4096) and
// walks their T * K frames in rounds of up to F consecutive frames (F from the LDS budget, spectrogram_plan):
//   1. the round's sample span [centre of its first frame - N/2, centre of its last + N/2) comes from HBM once, as int16 or
//      float32, and goes to LDS as doubles (frames overlap: at "lg" with a 15 s clip the hop is 351 against N = 1024);
//   2. each frame is windowed (the caller's table; the kernel computes no window) and packed into N/2 complex points
//      z[i] = x[2i] w[2i] + i x[2i+1] w[2i+1];
//   3. the F packed frames are transformed together, in place, by the passes of fft_passes.h (shared with denoise.hip).  Z[k] ends
//      up at the mixed-radix digit-reversed index;
//   4. thread b recovers X[b] = E[b] + W_N^b O[b] from Z[b] and conj(Z[N/2 - b]), adds the K frame powers of a column in frame
//      order (a column whose K frames span several rounds carries its sum in LDS) and writes the level index into the block's
//      H x T byte tile;
//   5. the tile leaves as runs of T contiguous bytes per image row.
// A round never splits a column unless K > F, and then it holds frames of that one column only, so the sum order is k = 0..K-1.
//
// Ragged bursts (k_spectrogram<S, true>): every image of a burst is W x H, so the grid stays column tiles x clips; what a clip's
// length decides - its first sample in the packed buffer, n, K, F and span_cap - comes from row blockIdx.y of a table (SpecClip)
// instead of the launch's scalars, and the LDS carve-up follows that row.  F only groups frames into rounds and the acc carry keeps
// the sum order, so a clip's image is what the uniform launch gives that clip alone.
#include "spectrogram.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "fft_passes.h"
#include "kernels.h"

namespace bnhip {

constexpr int SPEC_THREADS = 256;
constexpr int SPEC_FMAX = 64;                // frames per round at most (the per-frame offset table's size)

struct SpecParams {
    const void* samples;
    const double2* tw;         // [N/2] (cos, -sin)(2 pi j / N)
    const double* window;      // [N]
    uint8_t* image;
    int n, W, H, N, K, T, F, span_cap;
    FftPasses fp;              // the passes of N/2 complex points
    double pscale, top_db, range_db;
    const SpecClip* clips;     // ragged: one row per clip, in place of n, K, F and span_cap above; NULL: the uniform arithmetic
};

template <typename S, bool RAGGED>
__global__ __launch_bounds__(SPEC_THREADS) void k_spectrogram(SpecParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char spec_sm[];
    const int N = p.N, N2 = N >> 1, H = p.H, FS = SPEC_PHYS(N2);
    // the clip's own geometry: its row of the table, or the launch's scalars
    SpecClip g{};
    if (RAGGED) g = p.clips[blockIdx.y];
    const int F = RAGGED ? g.F : p.F, span_cap = RAGGED ? g.span_cap : p.span_cap;
    double* work = reinterpret_cast<double*>(spec_sm);           // [F][re | im][FS]
    double* span = work + (size_t)F * 2 * FS;                    // [span_cap]
    double* acc = span + span_cap;                               // [H] power sums of a column that spans rounds
    int* foff = reinterpret_cast<int*>(acc + H);                 // [SPEC_FMAX] first sample of each frame of the round, in span
    uint8_t* img = reinterpret_cast<uint8_t*>(foff + SPEC_FMAX); // [H][T]
    const int tid = threadIdx.x, clip = blockIdx.y;
    const int c0 = blockIdx.x * p.T, ncol = min(p.T, p.W - c0);
    const int n = RAGGED ? g.n : p.n, K = RAGGED ? g.K : p.K;
    // (a packed clip starts at any sample: element loads only)
    const S* x = static_cast<const S*>(p.samples) + (RAGGED ? (size_t)g.start : (size_t)clip * n);
    const long long den = 2LL * K * p.W;
    const double2* win2 = reinterpret_cast<const double2*>(p.window);

    int c = 0, k0 = 0;
    while (c < ncol) {
        int Cr, Kr;
        if (K <= F) { Cr = min(F / K, ncol - c); Kr = K; }
        else { Cr = 1; Kr = min(F, K - k0); }
        const int nf = Cr * Kr;
        // ---- 1. the round's span: frame g = column * K + k is centred at floor((2 g + 1) n / (2 K W))
        const long long g0 = (long long)(c0 + c) * K + k0;
        const long long s_lo = ((2 * g0 + 1) * n) / den - N2;
        const long long s_hi = ((2 * (g0 + nf - 1) + 1) * n) / den + N2;
        const int len = (int)min(s_hi - s_lo, (long long)span_cap);
        if (tid < nf) foff[tid] = (int)(((2 * (g0 + tid) + 1) * n) / den - N2 - s_lo);
        for (int i = tid; i < len; i += SPEC_THREADS) {
            const long long s = s_lo + i;
            double v = 0.0;
            if (s >= 0 && s < n) v = std::is_same<S, int16_t>::value ? (double)x[s] / 32768.0 : (double)x[s];
            span[i] = v;
        }
        __syncthreads();
        // ---- 2. window and pack
        for (int idx = tid; idx < (nf << p.fp.log2n2); idx += SPEC_THREADS) {
            const int f = idx >> p.fp.log2n2, i = idx & (N2 - 1), o = foff[f] + 2 * i;
            const double2 w = win2[i];
            double* zr = work + (size_t)f * 2 * FS;
            zr[SPEC_PHYS(i)] = (o < len ? span[o] : 0.0) * w.x;
            zr[FS + SPEC_PHYS(i)] = (o + 1 < len ? span[o + 1] : 0.0) * w.y;
        }
        __syncthreads();
        // ---- 3. in-place DIF passes over all frames of the round
        fft_passes_run<SPEC_THREADS>(p.fp, p.tw, work, nf, tid);
        // ---- 4. spectrum of the real frames, power sums, level indices
        const bool first = k0 == 0, last = k0 + Kr == K;
        for (int lc = 0; lc < Cr; lc++)
            for (int b = tid; b < H; b += SPEC_THREADS) {
                double sum = first ? 0.0 : acc[b];
                const int ia = SPEC_PHYS(fft_pos(p.fp, b & (N2 - 1))), ib = SPEC_PHYS(fft_pos(p.fp, (N2 - b) & (N2 - 1)));
                const double2 w = p.tw[b & (N2 - 1)];                 // W_N^b (unused at b = N/2)
                for (int kk = 0; kk < Kr; kk++) {
                    const double* zr = work + (size_t)(lc * Kr + kk) * 2 * FS;
                    const double* zi = zr + FS;
                    double xr, xi;
                    if (b == N2) { xr = zr[0] - zi[0]; xi = 0.0; }
                    else {
                        const double ar = zr[ia], ai = zi[ia], br = zr[ib], bi = -zi[ib];     // Z[b], conj(Z[N/2 - b])
                        const double er = 0.5 * (ar + br), ei = 0.5 * (ai + bi);
                        const double dr = ar - br, di = ai - bi;
                        const double orr = 0.5 * di, oi = -0.5 * dr;                            // O = -i/2 (Z[b] - conj(Z[N/2 - b]))
                        xr = er + (orr * w.x - oi * w.y); xi = ei + (orr * w.y + oi * w.x);
                    }
                    sum += (xr * xr + xi * xi) * p.pscale;
                }
                if (!last) { acc[b] = sum; continue; }
                const double P = sum / (double)K;
                int level = 0;
                if (P > 0.0) {
                    const double db = 10.0 * log10(P);
                    const double v = (db - p.top_db + p.range_db) / p.range_db * 255.0;
                    if (v >= 255.0) level = 255;
                    else if (v > 0.0) level = (int)floor(v + 0.5);
                }
                img[(H - 1 - b) * p.T + c + lc] = (uint8_t)level;
            }
        __syncthreads();
        if (K <= F) c += Cr;
        else { k0 += Kr; if (k0 == K) { k0 = 0; c++; } }
    }
    // ---- 5. rows of ncol contiguous bytes
    uint8_t* out = p.image + (size_t)clip * H * p.W + c0;
    for (int idx = tid; idx < H * p.T; idx += SPEC_THREADS) {
        const int r = idx / p.T, j = idx - r * p.T;
        if (j < ncol) out[(size_t)r * p.W + j] = img[idx];
    }
}

static size_t spec_lds_bytes(int N, int H, int T, int F, int hop) {
    const int N2 = N / 2;
    return (size_t)F * 2 * SPEC_PHYS(N2) * 8 + ((size_t)(F - 1) * hop + N + 2) * 8 + (size_t)H * 8 + SPEC_FMAX * 4 + (size_t)H * T;
}

SpecPlan spectrogram_plan(int n, int W, int H) {
    SpecPlan q;
    q.N = 2 * (H - 1);
    const long long wn = (long long)W * q.N;
    q.K = (int)std::max<long long>(1, (n + wn - 1) / wn);
    const long long kw = (long long)q.K * W;
    const int hop = (int)((n + kw - 1) / kw);                        // <= N: centres of consecutive frames are at most this far apart
    q.T = q.N <= 1024 ? 32 : (q.N <= 2048 ? 16 : 8);
    // F: as many frames per round as leave room for two blocks per CU; one block per CU where not even two frames fit that
    const long long fcap = std::min<long long>(SPEC_FMAX, (long long)q.T * q.K);
    auto fit = [&](size_t budget) {
        int F = 1;
        while (F < fcap && spec_lds_bytes(q.N, H, q.T, F + 1, hop) <= budget) F++;
        return F;
    };
    q.F = fit(78 * 1024);
    if (q.F < 2) q.F = fit(160 * 1024 - 256);
    q.span_cap = (q.F - 1) * hop + q.N + 2;
    q.lds = spec_lds_bytes(q.N, H, q.T, q.F, hop);
    return q;
}

std::vector<double> spectrogram_table(int N, const double* window) {
    std::vector<double> t((size_t)2 * N);
    for (int j = 0; j < N / 2; j++) {
        const double a = 6.283185307179586476925286766559 * (double)j / (double)N;
        t[2 * j] = std::cos(a); t[2 * j + 1] = -std::sin(a);
    }
    for (int i = 0; i < N; i++) t[(size_t)N + i] = window[i];
    return t;
}

template <bool RAGGED>
static void spec_launch(const SpecParams& p, int f32, int n_clips, size_t lds, hipStream_t s) {
    const dim3 grid((p.W + p.T - 1) / p.T, n_clips);
    if (f32) {
        lds_limit_once<&k_spectrogram<float, RAGGED>>(160 * 1024);
        hipLaunchKernelGGL((k_spectrogram<float, RAGGED>), grid, dim3(SPEC_THREADS), lds, s, p);
    } else {
        lds_limit_once<&k_spectrogram<int16_t, RAGGED>>(160 * 1024);
        hipLaunchKernelGGL((k_spectrogram<int16_t, RAGGED>), grid, dim3(SPEC_THREADS), lds, s, p);
    }
}

size_t spectrogram_table_bytes(const Clips& clips) { return clips.lens ? ((size_t)clips.n_clips * sizeof(SpecClip) + 255) & ~(size_t)255 : 0; }

void launch_spectrogram(const void* samples, int f32, const Clips& clips, int W, int H, const double* d_table, double wsum, double top_db,
                        double range_db, uint8_t* image, void* d_rows, hipStream_t s) {
    SpecParams p{};
    p.samples = samples;
    p.N = 2 * (H - 1);
    p.tw = reinterpret_cast<const double2*>(d_table);
    p.window = d_table + p.N;
    p.image = image;
    p.W = W; p.H = H;
    p.fp = fft_passes_plan(p.N);
    p.pscale = (2.0 / wsum) * (2.0 / wsum);
    p.top_db = top_db; p.range_db = range_db;
    if (!clips.lens) {
        const SpecPlan q = spectrogram_plan(clips.n, W, H);
        p.n = clips.n; p.K = q.K; p.T = q.T; p.F = q.F; p.span_cap = q.span_cap;
        spec_launch<false>(p, f32, clips.n_clips, q.lds, s);
        return;
    }
    // the plan of every clip on the host; the launch's LDS is the largest any of them needs (T depends on N only)
    std::vector<SpecClip> rows((size_t)clips.n_clips);
    size_t lds = 0;
    long long start = 0;
    for (int c = 0; c < clips.n_clips; c++) {
        const SpecPlan q = spectrogram_plan(clips.lens[c], W, H);
        rows[c] = {start, clips.lens[c], q.K, q.F, q.span_cap};
        start += clips.lens[c];
        lds = std::max(lds, q.lds);
        p.T = q.T;
    }
    // (a pageable source is staged before hipMemcpyAsync returns, so the host rows need not outlive the call)
    (void)hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(SpecClip), hipMemcpyHostToDevice, s);
    p.clips = static_cast<const SpecClip*>(d_rows);
    spec_launch<true>(p, f32, clips.n_clips, lds, s);
}

}  // namespace bnhip
