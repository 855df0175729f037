// Spectral noise reduction of detection clips for gfx950: int16 PCM -> frames of N samples at hop h = N/4, periodic Hann window,
// real FFT -> power, smoothed over three bins -> gain max(g_min, 1 - Nz / P) against a white noise floor -> inverse FFT -> window,
// overlap-add, 2/3 -> int16 by the rule of pcmgain.h.  The spec (frame grid, smoothing, noise model, gain, synthesis scale) is
// DESIGN.md §9 "Denoise"; tests/dnref.py restates it in numpy float64.  Everything is fp64; no frame depends on another.
//
// Reference path being replaced: the `afftdn=nr=..:nf=..` stage of the FFmpeg child process that
// internal/audiocore/ffmpeg/process.go:164-251 builds for ProcessAudioByID / ProcessedSpectrogramByID
// (internal/api/v2/media/media.go:1200-1447).  FFmpeg is not in the reference tree: the sample values are this project's spec, not
// afftdn's.  Kept from the reference: the two parameters, their ranges, the presets, the chain order (api_denoise.cpp).
//
// Mapping.  A block of 512 threads owns T consecutive output hops of one clip (hop u = samples [u h, (u + 1) h)) and walks the
// T + 3 frames that cover them (frame f of the tile starts 3 hops before the tile's hop f) in rounds of up to F frames:
//   1. the round's sample span, (F + 3) h samples, comes from HBM once and stays in LDS as int16, zeros outside the clip;
//   2. each frame is windowed and packed into N/2 complex points z[i] = x[2i] w[2i] + i x[2i+1] w[2i+1];
//   3. the packed frames are transformed in place by the passes of fft_passes.h (Z[k] at its digit-reversed index);
//   4. a thread per bin pair (b, N/2 - b) recovers X[b] and X[N/2 - b] and writes them, in natural order, to a second array;
//   5. a thread per bin pair forms the smoothed powers and gains of its two bins from that array, and writes the conjugate of
//      the packed spectrum of the gained frame, Z'[k] = E'[k] + i O'[k], back over the frame in natural order;
//   6. the same passes again: conj(FFT(conj(Z'))) / (N/2) is the packed output frame y[2i] + i y[2i+1];
//   7. overlap-add: thread (c, off) owns offset `off` of every hop u = c (mod 3) of the round, in ascending u, and adds the hop's
//      covering frames of this round in frame order.  A hop whose last frame (u + 3) is in the round leaves as int16 at once;
//      otherwise its partial sum waits in carry[c][off] for the next round - read and written by that one thread, so no two
//      rounds race and there are no atomics.  The sum of a sample is ((f_u + f_u+1) + f_u+2) + f_u+3 whatever T and F are, so a
//      clip's bytes depend neither on the batch it is in nor on the plan.
// Hops outside the tile (other blocks own them) are not summed; no load leaves [0, n) of the block's clip.
//
// Bursts (ragged.h).  The kernel is stated once: a NULL tile table means the uniform arithmetic.  A uniform batch is a
// dim3(tiles, n_clips) grid: block (x, y) owns tile x of clip y, which starts at y n.  A ragged burst packs clips of lengths
// len[c] >= 1 back to back and is a flat grid of tile0[n_clips] blocks, tile0 the prefix table of the clips' tile counts
// ceil(hops_c / T), hops_c = (len_c - 1) / h + 1 >= 1: block b finds its clip by ragged_clip(tile0, n_clips, b) (a search over a
// table that stays in L2, no LDS), owns tile b - tile0[clip] of it, and reads and writes [start[clip], start[clip] + len[clip])
// only - step 1 zero-fills what lies outside the clip, step 7 writes gi < n.  Nothing else of the seven steps knows which form it
// runs in, so a clip's bytes are those of the uniform call on that clip alone.  A clip may start at an odd offset: every int16
// access to HBM is a scalar one.
// The flat grid stays inside 31 bits: h >= 16 and T >= 8, so a clip has at most len_c / 128 + 2 tiles, and with the limits of
// clips_check (at most 65535 clips, a total below 2^36) a burst has at most 2^36 / 128 + 2 * 65535 < 2^29 + 2^17 tiles.
#include "denoise.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fft_passes.h"
#include "kernels.h"
#include "pcmgain.h"
#include "ragged.h"
#include "spectrogram.h"

namespace bnhip {

constexpr int DN_THREADS = 512;
constexpr int DN_FMAX = 64;                  // frames per round at most
constexpr int DN_TMAX = 64;                  // output hops per block at most: 3 / 64 of the frames are computed twice

struct DnParams {
    const int16_t* pcm;
    int16_t* out;
    const double2* tw;         // [N/2] (cos, -sin)(2 pi j / N)
    const double* window;      // [N]
    ClipGeom g;                // the samples: n_clips clips of g.n, or start[n_clips + 1]
    const long long* tile0;    // [n_clips + 1] prefix of the clips' tile counts on a flat grid; NULL: block (tile, clip)
    int N, T, F;
    FftPasses fp;
    double nz, gmin;           // 10^(nf_db / 10) 3N/8, 10^(-nr_db / 20)
};

// the natural-order spectrum of a frame: [re | im], DN_XS(N/2) doubles each, X[0..N/2]
#define DN_XS(n2) ((n2) + 2)

__device__ __forceinline__ double dn_gain(const double* xr, const double* xi, int k, int N2, double nz, double gmin) {
    const int km = k == 0 ? 1 : k - 1, kp = k == N2 ? N2 - 1 : k + 1;
    const double pm = xr[km] * xr[km] + xi[km] * xi[km], pp = xr[kp] * xr[kp] + xi[kp] * xi[kp], pc = xr[k] * xr[k] + xi[k] * xi[k];
    const double pb = ((pm + pp) + 2.0 * pc) * 0.25;
    if (!(pb > 0.0)) return gmin;
    const double g = 1.0 - nz / pb;
    return g > gmin ? g : gmin;
}

__global__ __launch_bounds__(DN_THREADS) void k_denoise(DnParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dn_sm[];
    const int N = p.N, N2 = N >> 1, h = N >> 2, FS = SPEC_PHYS(N2), XS = DN_XS(N2), F = p.F, lg = p.fp.log2n2;
    double* work = reinterpret_cast<double*>(dn_sm);             // [F][re | im][FS]
    double* xs = work + (size_t)F * 2 * FS;                      // [F][re | im][XS]
    double* carry = xs + (size_t)F * 2 * XS;                     // [3][h] partial sums of the hops a round leaves open
    int16_t* span = reinterpret_cast<int16_t*>(carry + 3 * h);   // [(F + 3) h]
    const int tid = threadIdx.x;
    const int clip = p.tile0 ? ragged_clip(p.tile0, p.g.n_clips, blockIdx.x) : (int)blockIdx.y;
    const int tile = p.tile0 ? (int)(blockIdx.x - p.tile0[clip]) : (int)blockIdx.x;
    const int n = clip_len(p.g, clip);
    const int hops = (n - 1) / h + 1;
    const int j0 = tile * p.T, Tt = min(p.T, hops - j0), NF = Tt + 3;
    const int16_t* x = p.pcm + clip_start(p.g, clip);
    int16_t* y = p.out + clip_start(p.g, clip);
    const double2* win2 = reinterpret_cast<const double2*>(p.window);
    const int per = (N >> 2) + 1;                                // bin pairs (b, N/2 - b), b = 0..N/4
    // sample j = q h + off of a frame is half (j & 1) of packed point q (h / 2) + (off >> 1): disjoint bits, and fft_pos permutes bits
    const int pq1 = fft_pos(p.fp, 1 << (lg - 2)), pq2 = fft_pos(p.fp, 2 << (lg - 2)), pq3 = fft_pos(p.fp, 3 << (lg - 2));
    const double inv = 2.0 / (double)N, vscale = 32768.0 * (2.0 / 3.0);

    for (int f0 = 0; f0 < NF; f0 += F) {
        const int nf = min(F, NF - f0);
        // ---- 1. the round's span: frame f0 starts at hop j0 + f0 - 3
        const long long s_lo = ((long long)j0 + f0 - 3) * h;
        for (int i = tid; i < (nf + 3) * h; i += DN_THREADS) {
            const long long s = s_lo + i;
            span[i] = (s >= 0 && s < n) ? x[s] : (int16_t)0;
        }
        __syncthreads();
        // ---- 2. window and pack
        for (int idx = tid; idx < (nf << lg); idx += DN_THREADS) {
            const int f = idx >> lg, i = idx & (N2 - 1), o = f * h + 2 * i;
            const double2 w = win2[i];
            double* zr = work + (size_t)f * 2 * FS;
            zr[SPEC_PHYS(i)] = ((double)span[o] * (1.0 / 32768.0)) * w.x;
            zr[FS + SPEC_PHYS(i)] = ((double)span[o + 1] * (1.0 / 32768.0)) * w.y;
        }
        __syncthreads();
        // ---- 3. forward
        fft_passes_run<DN_THREADS>(p.fp, p.tw, work, nf, tid);
        // ---- 4. X[b] = E[b] + W^b O[b], X[N/2 - b] = conj(E[b] - W^b O[b]) from Z[b] and conj(Z[N/2 - b])
        for (int idx = tid; idx < nf * per; idx += DN_THREADS) {
            const int f = idx / per, b = idx - f * per;
            const double* zr = work + (size_t)f * 2 * FS;
            const double* zi = zr + FS;
            double* xr = xs + (size_t)f * 2 * XS;
            double* xi = xr + XS;
            if (b == 0) {
                const double a = zr[0], d = zi[0];
                xr[0] = a + d; xi[0] = 0.0; xr[N2] = a - d; xi[N2] = 0.0;
            } else {
                const int c = N2 - b, ia = SPEC_PHYS(fft_pos(p.fp, b)), ib = SPEC_PHYS(fft_pos(p.fp, c));
                const double ar = zr[ia], ai = zi[ia], br = zr[ib], bi = -zi[ib];
                const double er = 0.5 * (ar + br), ei = 0.5 * (ai + bi);
                const double dr = ar - br, di = ai - bi;
                const double orr = 0.5 * di, oi = -0.5 * dr;                                // O = -i/2 (Z[b] - conj(Z[N/2 - b]))
                const double2 w = p.tw[b];
                const double tr = orr * w.x - oi * w.y, ti = orr * w.y + oi * w.x;
                xr[b] = er + tr; xi[b] = ei + ti;
                if (c != b) { xr[c] = er - tr; xi[c] = -(ei - ti); }
            }
        }
        __syncthreads();
        // ---- 5. Y = g X; conj(Z'[k]) with Z'[k] = E'[k] + i O'[k], E' = (Y[k] + conj(Y[N/2 - k])) / 2,
        //         O' = (Y[k] - conj(Y[N/2 - k])) / 2 conj(W^k); Z'[N/2 - k] = conj(E') + i conj(O')
        for (int idx = tid; idx < nf * per; idx += DN_THREADS) {
            const int f = idx / per, b = idx - f * per;
            double* zr = work + (size_t)f * 2 * FS;
            double* zi = zr + FS;
            const double* xr = xs + (size_t)f * 2 * XS;
            const double* xi = xr + XS;
            const double gb = dn_gain(xr, xi, b, N2, p.nz, p.gmin);
            if (b == 0) {
                const double y0 = gb * xr[0], yn = dn_gain(xr, xi, N2, N2, p.nz, p.gmin) * xr[N2];
                zr[0] = 0.5 * (y0 + yn); zi[0] = -(0.5 * (y0 - yn));
            } else {
                const int c = N2 - b;
                const double gc = c != b ? dn_gain(xr, xi, c, N2, p.nz, p.gmin) : gb;
                const double ybr = gb * xr[b], ybi = gb * xi[b], ycr = gc * xr[c], yci = gc * xi[c];
                const double er = 0.5 * (ybr + ycr), ei = 0.5 * (ybi - yci);
                const double dr = 0.5 * (ybr - ycr), di = 0.5 * (ybi + yci);
                const double2 w = p.tw[b];
                const double orr = dr * w.x + di * w.y, oi = di * w.x - dr * w.y;
                zr[SPEC_PHYS(b)] = er - oi; zi[SPEC_PHYS(b)] = -(ei + orr);
                if (c != b) { zr[SPEC_PHYS(c)] = er + oi; zi[SPEC_PHYS(c)] = ei - orr; }
            }
        }
        __syncthreads();
        // ---- 6. inverse: the forward passes on conj(Z'); y[2i] = Re / (N/2), y[2i+1] = -Im / (N/2) at fft_pos(i)
        fft_passes_run<DN_THREADS>(p.fp, p.tw, work, nf, tid);
        // ---- 7. overlap-add in frame order
        const int u_end = min(f0 + nf - 1, Tt - 1);
        for (int it = tid; it < 3 * h; it += DN_THREADS) {
            const int c = it / h, off = it - c * h;
            const int po = fft_pos(p.fp, off >> 1);
            const bool odd = off & 1;
            const int u_lo = max(f0 - 3, 0);
            for (int u = u_lo + (c - u_lo % 3 + 3) % 3; u <= u_end; u += 3) {
                const int fa = max(u, f0), fb = min(u + 3, f0 + nf - 1);
                double sum = u >= f0 ? 0.0 : carry[it];
                for (int f = fa; f <= fb; f++) {
                    const int q = u - f + 3;
                    const int i = SPEC_PHYS((q == 0 ? 0 : (q == 1 ? pq1 : (q == 2 ? pq2 : pq3))) | po);
                    const double* zr = work + (size_t)(f - f0) * 2 * FS;
                    const double r = odd ? -zr[FS + i] : zr[i];
                    sum += p.window[q * h + off] * (r * inv);
                }
                if (fb == u + 3) {
                    const long long gi = ((long long)j0 + u) * h + off;
                    if (gi < n) y[gi] = (int16_t)pcm_quantized(sum * vscale);
                } else carry[it] = sum;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_pcm_gain(const int16_t* pcm, size_t total, double f, int16_t* out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) out[i] = (int16_t)pcm_gained(pcm[i], f);
}

static size_t dn_lds_bytes(int N, int F) {
    const int N2 = N / 2, h = N / 4;
    return (size_t)F * 2 * SPEC_PHYS(N2) * 8 + (size_t)F * 2 * DN_XS(N2) * 8 + (size_t)3 * h * 8 + (size_t)(F + 3) * h * 2;
}

// the blocks of one clip of n samples at T hops of N / 4 samples per block
static int dn_tiles(int n, int N, int T) { return ((n - 1) / (N / 4) + 1 + T - 1) / T; }

DenoisePlan denoise_plan(const Clips& clips, int N) {
    DenoisePlan q;
    // T: as many hops per block as leave the device a few blocks per CU
    q.T = DN_TMAX;
    while (q.T > 8 && clips.sum([&](int n) { return dn_tiles(n, N, q.T); }) < 1024) q.T >>= 1;
    // F: as many frames per round as leave room for two blocks per CU; one block per CU where not even two frames fit that
    const int fcap = std::min(DN_FMAX, q.T + 3);
    auto fit = [&](size_t budget) {
        int F = 1;
        while (F < fcap && dn_lds_bytes(N, F + 1) <= budget) F++;
        return F;
    };
    q.F = fit(78 * 1024);
    if (q.F < 2) q.F = fit(160 * 1024 - 256);
    q.lds = dn_lds_bytes(N, q.F);
    return q;
}

size_t denoise_table_bytes(const Clips& clips) { return clips.lens ? (2 * ((size_t)clips.n_clips + 1) * 8 + 255) & ~(size_t)255 : 0; }

std::vector<double> denoise_table(int N) {
    std::vector<double> w((size_t)N);
    for (int j = 0; j < N; j++) w[j] = 0.5 - 0.5 * std::cos(6.283185307179586476925286766559 * (double)j / (double)N);
    return spectrogram_table(N, w.data());
}

void launch_denoise(const int16_t* pcm, const Clips& clips, int N, double nr_db, double nf_db, const double* d_table, int16_t* out,
                    void* d_tables, hipStream_t s) {
    const int n_clips = clips.n_clips;
    const DenoisePlan q = denoise_plan(clips, N);
    DnParams p{};
    p.pcm = pcm; p.out = out;
    p.tw = reinterpret_cast<const double2*>(d_table);
    p.window = d_table + N;
    p.N = N; p.T = q.T; p.F = q.F;
    p.fp = fft_passes_plan(N);
    p.nz = std::pow(10.0, nf_db / 10.0) * (3.0 * (double)N / 8.0);
    p.gmin = std::pow(10.0, -nr_db / 20.0);
    p.g.n_clips = n_clips; p.g.n = clips.n;
    dim3 grid;
    if (!clips.lens) {
        grid = dim3(dn_tiles(clips.n, N, q.T), n_clips);
    } else {
        // start | tile0, [n_clips + 1] each
        std::vector<long long> t(2 * ((size_t)n_clips + 1));
        long long *start = t.data(), *tile0 = start + n_clips + 1;
        start[0] = tile0[0] = 0;
        for (int c = 0; c < n_clips; c++) {
            start[c + 1] = start[c] + clips.lens[c];
            tile0[c + 1] = tile0[c] + dn_tiles(clips.lens[c], N, q.T);
        }
        // (a pageable source is staged before hipMemcpyAsync returns, so the host tables need not outlive the call)
        (void)hipMemcpyAsync(d_tables, t.data(), t.size() * 8, hipMemcpyHostToDevice, s);
        p.g.start = static_cast<const long long*>(d_tables);
        p.tile0 = p.g.start + n_clips + 1;
        grid = dim3((unsigned)tile0[n_clips]);
    }
    lds_limit_once<&k_denoise>(160 * 1024);
    hipLaunchKernelGGL(k_denoise, grid, dim3(DN_THREADS), q.lds, s, p);
}

void launch_pcm_gain(const int16_t* pcm, size_t total, double factor, int16_t* out, hipStream_t s) {
    const size_t blocks = std::min<size_t>((total + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(k_pcm_gain, dim3((unsigned)blocks), dim3(256), 0, s, pcm, total, factor, out);
}

}  // namespace bnhip
