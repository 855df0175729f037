// GPU polyphase FIR resampler for the step just upstream of the classifier (reference wrapper:
// internal/audiocore/resample/resample.go:57-172; call sites analysis/buffer_consumer.go:118,192, audiocore/router.go:277).
//
// The reference delegates the filter arithmetic to github.com/tphakala/go-audio-resampler v1.7.0 (QualityMedium), which
// is NOT in the reference tree and whose sample values no reference test pins (resample_test.go checks only the output
// length within +-5 %), so the filter here is this project's own, fully specified design: rational ratio L/M after
// gcd, Kaiser-windowed sinc low-pass with cutoff 1/max(L,M) (of the up-sampled Nyquist), half-length
// 10*max(L,M) taps, beta 5.0, unit DC gain times L, zero-phase (centred), zero-padded edges, n_out = ceil(n_in*L/M)
// - i.e. exactly scipy.signal.resample_poly's default design, which is therefore the oracle.  What IS restated from the
// reference are the PCM edges: in = float32(int16)/32768, out = clamp(+-1) then int16(f*32767) truncating toward zero
// (resample.go:120-124,161-169).
//
//   out[i] = sum_n x[n] * h[i*M + half - n*L]        (h of length 2*half+1)
// as L polyphase branches of T = ceil((2*half+1)/L) taps: phase p = (i*M + half) mod L, newest input n0 = (i*M+half)/L.
// One thread per output sample; the phase table (<= 61 KiB) and the block's input span are LDS-resident.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "channels.h"
#include "kernels.h"
#include "pcm_sample.h"
#include "ragged.h"
#include "resample.h"

namespace bnhip {

static double bessel_i0(double x) {
    double sum = 1.0, term = 1.0, q = x * x / 4.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// scipy.signal.firwin(2*half+1, 1/max_rate, window=('kaiser', beta)) * L, re-laid as [L][T] polyphase rows (tap t of
// phase p = h[p + t*L]).
void resample_design(int L, int M, double beta, int half_factor, std::vector<float>* table, int* T_out, int* half_out) {
    const int max_rate = L > M ? L : M;
    const int half = half_factor * max_rate;
    const int N = 2 * half + 1;
    const double fc = 1.0 / (double)max_rate, alpha = 0.5 * (N - 1);
    std::vector<double> h(N);
    double sum = 0.0;
    const double i0b = bessel_i0(beta);
    for (int n = 0; n < N; n++) {
        double m = (double)n - alpha;
        double s = m == 0.0 ? 1.0 : std::sin(M_PI * fc * m) / (M_PI * fc * m);
        double r = m / alpha;
        double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
        h[n] = fc * s * w;
        sum += h[n];
    }
    for (int n = 0; n < N; n++) h[n] = h[n] / sum * (double)L;
    const int T = (N + L - 1) / L;
    table->assign((size_t)L * T, 0.0f);
    for (int p = 0; p < L; p++)
        for (int t = 0; t < T; t++) {
            int k = p + t * L;
            if (k < N) (*table)[(size_t)p * T + t] = (float)h[k];
        }
    *T_out = T;
    *half_out = half;
}

// One tile of 256 outputs [i0, i0 + 256) of one clip, whose first input / output sample is element in0 / out0 of in_ / out_.
// i_base / n_base (streaming form, api_resample.cpp bnhip_resampler_*): stream index of this launch's first output and of in[0]; the
// one-shot entries pass 0 / 0.  Inputs before the stream start and beyond the supplied span read as zero.
template <bool IN_PCM16, bool OUT_PCM16>
__device__ __forceinline__ void resample_tile(const void* __restrict__ in_, void* __restrict__ out_, const float* __restrict__ table,
                                              size_t in0, size_t out0, int i0, int n_in, int n_out, int L, int M, int T, int half,
                                              long long i_base, long long n_base) {
    extern __shared__ float sm[];
    float* tab = sm;                       // [L*T]
    float* xs = sm + L * T;                // input span of this block
    const int i1 = min(n_out, i0 + 256);
    for (int k = threadIdx.x; k < L * T; k += 256) tab[k] = table[k];
    // inputs touched by outputs [i0, i1): n from (i0*M+half)/L - (T-1) to ((i1-1)*M+half)/L   (stream indices)
    const long long lo = ((i_base + i0) * M + half) / L - (T - 1);
    const long long hi = ((i_base + i1 - 1) * M + half) / L;
    const int span = (int)(hi - lo + 1);
    for (int k = threadIdx.x; k < span; k += 256) {
        long long n = lo + k - n_base;     // index into this launch's input
        float v = 0.0f;
        if (lo + k >= 0 && n >= 0 && n < n_in) {
            if (IN_PCM16) v = (float)reinterpret_cast<const int16_t*>(in_)[in0 + n] / 32768.0f;
            else v = reinterpret_cast<const float*>(in_)[in0 + n];
        }
        xs[k] = v;
    }
    __syncthreads();
    const int i = i0 + threadIdx.x;
    if (i >= i1) return;
    const long long pos = (i_base + i) * M + half;
    const int p = (int)(pos % L);
    const int n0 = (int)(pos / L - lo);            // index of the newest input in xs
    const float* tp = tab + p * T;
    float acc = 0.0f;
    for (int t = 0; t < T; t++) acc = fmaf(xs[n0 - t], tp[t], acc);
    if (OUT_PCM16) {
        float f = fminf(fmaxf(acc, -1.0f), 1.0f);
        reinterpret_cast<int16_t*>(out_)[out0 + i] = (int16_t)(f * 32767.0f);     // truncation toward zero
    } else {
        reinterpret_cast<float*>(out_)[out0 + i] = acc;
    }
}

// n_clips clips of n_in samples each: block (tile, clip)
template <bool IN_PCM16, bool OUT_PCM16>
__global__ __launch_bounds__(256) void k_resample(const void* __restrict__ in_, void* __restrict__ out_, const float* __restrict__ table,
                                                  int n_in, int n_out, int L, int M, int T, int half, long long i_base, long long n_base) {
    const int clip = blockIdx.y;
    resample_tile<IN_PCM16, OUT_PCM16>(in_, out_, table, (size_t)clip * n_in, (size_t)clip * n_out, blockIdx.x * 256, n_in, n_out, L, M, T,
                                       half, i_base, n_base);
}

// A ragged burst, PCM16 in and float32 out (what the spectrogram render reads): clip c has start_in[c + 1] - start_in[c] samples at
// start_in[c] of the packed input and its outputs at start_out[c] of the packed output; the tiles of all clips are one flat list,
// clip c's from tile0[c] on (prefix tables [n_clips + 1], ragged.h).  An output is the uniform launch's fmaf chain over the same
// staged taps, so its bits are k_resample's on that clip alone.
__global__ __launch_bounds__(256) void k_resample_ragged(const int16_t* __restrict__ in, float* __restrict__ out,
                                                         const float* __restrict__ table, const long long* __restrict__ start_in,
                                                         const long long* __restrict__ start_out, const long long* __restrict__ tile0,
                                                         int n_clips, int L, int M, int T, int half) {
    const int clip = ragged_clip(tile0, n_clips, (long long)blockIdx.x);
    const long long si = start_in[clip], so = start_out[clip];
    const int tile = (int)((long long)blockIdx.x - tile0[clip]);
    resample_tile<true, false>(in, out, table, (size_t)si, (size_t)so, tile * 256, (int)(start_in[clip + 1] - si),
                               (int)(start_out[clip + 1] - so), L, M, T, half, 0, 0);
}

// returns 0 on success, -1 if the geometry does not fit LDS
int launch_resample(const void* d_in, void* d_out, const float* d_table, int in_pcm16, int out_pcm16, int n_clips, int n_in,
                    int n_out, int L, int M, int T, int half, long long i_base, long long n_base, hipStream_t s) {
    const size_t lds = resample_lds(L, M, T);
    if (lds > RESAMPLE_LDS_MAX) return -1;
    dim3 grid((n_out + 255) / 256, n_clips);
#define BN_RS(IP, OP)                                                                                                        \
    do {                                                                                                                     \
        lds_limit_once<&k_resample<IP, OP>>(160 * 1024); \
        hipLaunchKernelGGL((k_resample<IP, OP>), grid, dim3(256), lds, s, d_in, d_out, d_table, n_in, n_out, L, M, T, half, i_base, n_base); \
    } while (0)
    if (in_pcm16 && out_pcm16) BN_RS(true, true);
    else if (!in_pcm16 && out_pcm16) BN_RS(false, true);
    else if (!in_pcm16 && !out_pcm16) BN_RS(false, false);
    else BN_RS(true, false);                                        // (the spectrogram entry: PCM in, the float samples it renders out)
#undef BN_RS
    return 0;
}

size_t resample_ragged_table_bytes(int n_clips) { return (3 * ((size_t)n_clips + 1) * 8 + 255) & ~(size_t)255; }

int launch_resample_ragged(const int16_t* d_in, float* d_out, const float* d_table, int n_clips, const int* lens_in, const int* lens_out,
                           int L, int M, int T, int half, void* d_tables, hipStream_t s) {
    const size_t lds = resample_lds(L, M, T);
    if (lds > RESAMPLE_LDS_MAX) return -1;
    // start_in[n_clips + 1], then start_out[n_clips + 1], then tile0[n_clips + 1]
    std::vector<long long> t(3 * ((size_t)n_clips + 1));
    long long* start_in = t.data(), *start_out = start_in + n_clips + 1, *tile0 = start_out + n_clips + 1;
    start_in[0] = start_out[0] = tile0[0] = 0;
    for (int c = 0; c < n_clips; c++) {
        start_in[c + 1] = start_in[c] + lens_in[c]; start_out[c + 1] = start_out[c] + lens_out[c];
        tile0[c + 1] = tile0[c] + (lens_out[c] + 255) / 256;
    }
    // (a pageable source is staged before hipMemcpyAsync returns, so the host tables need not outlive the call)
    (void)hipMemcpyAsync(d_tables, t.data(), t.size() * 8, hipMemcpyHostToDevice, s);
    const long long* d = static_cast<const long long*>(d_tables);
    lds_limit_once<&k_resample_ragged>(160 * 1024);
    hipLaunchKernelGGL(k_resample_ragged, dim3((unsigned)tile0[n_clips]), dim3(256), lds, s, d_in, d_out, d_table, d, d + n_clips + 1,
                       d + 2 * ((size_t)n_clips + 1), n_clips, L, M, T, half);
    return 0;
}

// ------------------------------------------------------------------------------------------------ slot form
// Recordings at their own rates and depths -> float32 slots at the model's rate (ResampleSlotDesc, resample.h), one launch for the
// burst: a block takes one tile of RESAMPLE_SLOT_TILE outputs of one recording, found in the flat tile list as k_resample_ragged
// finds its clip.  The recording's phase table is staged once per block and serves the tile's 256-output sub-tiles one after the
// other; a sub-tile stages its input span - converted in the load, zeros outside the recording - and computes as resample_tile does:
// the same p, the same newest input and the fmaf chain over the same taps in the same order, so the bits are k_resample<false, false>'s
// on the converted recording.  The slot's tail up to a whole quad is written as zeros here (the framed min/max launch loads quads).
//
// MC (k_resample_slots_mc): the recording is frames of C interleaved channels and a staged value is channel_sample's (channels.h) -
// channel `sel` or the mean of the channels - where frame_sample stands; everything after the staged float32 is the same code.
template <int BITS, bool MC>
__device__ __forceinline__ float slot_sample(const char* __restrict__ in, long long n, int C, int sel) {
    if constexpr (MC) return channel_sample<BITS>(in, n, C, sel);
    else return frame_sample<BITS>(in, n);
}

template <int BITS, bool MC>
__device__ __forceinline__ void resample_slot_tile(const char* __restrict__ in, float* __restrict__ out, const float* __restrict__ table,
                                                   const ResampleSlotDesc& d, long long i0, int C, int sel) {
    const long long n_pad = ((long long)d.n_out + 3) & ~3ll;
    const long long i_end = min(n_pad, i0 + RESAMPLE_SLOT_TILE);
    if (d.L == 0) {                               // at the model's rate: converted only
        for (long long i = i0 + threadIdx.x; i < i_end; i += 256) out[i] = i < d.n_out ? slot_sample<BITS, MC>(in, i, C, sel) : 0.0f;
        return;
    }
    extern __shared__ float sm[];
    const int L = d.L, M = d.M, T = d.T;
    float* tab = sm;                              // [L*T]
    float* xs = sm + L * T;                       // input span of one sub-tile
    for (int k = threadIdx.x; k < L * T; k += 256) tab[k] = table[k];
    // (a sub-tile always holds an output: n_pad is the first multiple of 4 from n_out on, and s0 is one)
    for (long long s0 = i0; s0 < i_end; s0 += 256) {
        const long long s1 = min((long long)d.n_out, s0 + 256);
        const long long pos0 = s0 * M + d.half;
        const long long q0 = pos0 / L;
        const unsigned r0 = (unsigned)(pos0 % L);
        const long long lo = q0 - (T - 1);
        const int span = (int)(((s1 - 1) * M + d.half) / L - lo + 1);
        __syncthreads();                          // the sub-tile in front has read its span
        for (int k = threadIdx.x; k < span; k += 256) {
            const long long n = lo + k;
            xs[k] = n >= 0 && n < d.n_in ? slot_sample<BITS, MC>(in, n, C, sel) : 0.0f;
        }
        __syncthreads();
        const long long i = s0 + threadIdx.x;
        if (i < s1) {
            // pos = pos0 + threadIdx.x * M = q0 * L + rem; a plan that fits LDS has L <= 38 400 and 255 * M / L < 38 400, so rem < 2^31
            const unsigned rem = r0 + threadIdx.x * (unsigned)M;
            const int n0 = T - 1 + (int)(rem / (unsigned)L);      // index of the newest input in xs
            const float* tp = tab + (rem % (unsigned)L) * T;
            float acc = 0.0f;
            for (int t = 0; t < T; t++) acc = fmaf(xs[n0 - t], tp[t], acc);
            out[i] = acc;
        } else if (i < i_end) {
            out[i] = 0.0f;
        }
    }
}

template <bool MC>
__device__ __forceinline__ void resample_slots_block(const char* __restrict__ raw, char* __restrict__ slots, const float* __restrict__ tables,
                                                     const ResampleSlotDesc* __restrict__ desc, const long long* __restrict__ tile0,
                                                     int n_rec, const int* __restrict__ channels, const int* __restrict__ sel) {
    const int r = ragged_clip(tile0, n_rec, (long long)blockIdx.x);
    const ResampleSlotDesc d = desc[r];
    const long long i0 = ((long long)blockIdx.x - tile0[r]) * RESAMPLE_SLOT_TILE;
    const char* in = raw + d.in_off;
    float* out = reinterpret_cast<float*>(slots + d.out_off);
    const float* table = tables + d.tab_off;
    const int C = MC ? channels[r] : 1, sl = MC ? sel[r] : 0;
    if (d.bits == 16) resample_slot_tile<16, MC>(in, out, table, d, i0, C, sl);
    else if (d.bits == 24) resample_slot_tile<24, MC>(in, out, table, d, i0, C, sl);
    else if (d.bits == 32) resample_slot_tile<32, MC>(in, out, table, d, i0, C, sl);
    else resample_slot_tile<0, MC>(in, out, table, d, i0, C, sl);
}

__global__ __launch_bounds__(256) void k_resample_slots(const char* __restrict__ raw, char* __restrict__ slots, const float* __restrict__ tables,
                                                        const ResampleSlotDesc* __restrict__ desc, const long long* __restrict__ tile0,
                                                        int n_rec) {
    resample_slots_block<false>(raw, slots, tables, desc, tile0, n_rec, nullptr, nullptr);
}

// the multichannel form: recording r has channels[r] interleaved channels (n_in counts frames) and sel[r] - a channel or
// CHANNEL_MIX, device memory that the measurement in front of this launch may have written (channels.hip) - says what is fetched
__global__ __launch_bounds__(256) void k_resample_slots_mc(const char* __restrict__ raw, char* __restrict__ slots, const float* __restrict__ tables,
                                                           const ResampleSlotDesc* __restrict__ desc, const long long* __restrict__ tile0,
                                                           int n_rec, const int* __restrict__ channels, const int* __restrict__ sel) {
    resample_slots_block<true>(raw, slots, tables, desc, tile0, n_rec, channels, sel);
}

void launch_resample_slots(const void* d_raw, void* d_slots, const float* d_tables, const ResampleSlotDesc* d_desc, const long long* d_tile0,
                           int n_rec, long long n_tiles, size_t lds, hipStream_t s) {
    if (n_rec <= 0 || n_tiles <= 0) return;
    lds_limit_once<&k_resample_slots>(160 * 1024);
    hipLaunchKernelGGL(k_resample_slots, dim3((unsigned)n_tiles), dim3(256), lds, s, static_cast<const char*>(d_raw), static_cast<char*>(d_slots),
                       d_tables, d_desc, d_tile0, n_rec);
}

void launch_resample_slots_mc(const void* d_raw, void* d_slots, const float* d_tables, const ResampleSlotDesc* d_desc, const long long* d_tile0,
                              int n_rec, long long n_tiles, size_t lds, const int* d_channels, const int* d_sel, hipStream_t s) {
    if (n_rec <= 0 || n_tiles <= 0) return;
    lds_limit_once<&k_resample_slots_mc>(160 * 1024);
    hipLaunchKernelGGL(k_resample_slots_mc, dim3((unsigned)n_tiles), dim3(256), lds, s, static_cast<const char*>(d_raw), static_cast<char*>(d_slots),
                       d_tables, d_desc, d_tile0, n_rec, d_channels, d_sel);
}

// ------------------------------------------------------------------------------------------------ bank form
// Every stream of a bank (api_resample.cpp bnhip_resampler_bank_*) in one launch.  A stream's input is the virtual array
//   x(n) = slab[n - n_base]                     for n_base <= n < n_base + n_hist     (history, already float32)
//        = float32(pcm16) / 32768               for the next n_in samples             (this call's frames, back to back)
//        = 0                                    otherwise (before the stream start, or beyond what was supplied)
// which is exactly what k_resample reads from the single-stream resampler's [history | chunk] work buffer, and every output is
// the same fmaf chain over the same taps in the same order, so the bits are k_resample's.  Blocks are flattened over
// (stream, 256-output tile) plus one tail block per stream that writes the stream's new history into its other slab.
__device__ __forceinline__ float bank_x(const ResampleBankDesc& d, const int16_t* __restrict__ pcm, const float* __restrict__ hist,
                                        long long n) {
    long long k = n - d.n_base;
    if (n < 0 || k < 0) return 0.0f;
    if (k < d.n_hist) return hist[d.hist_rd + k];
    k -= d.n_hist;
    if (k < d.n_in) return (float)pcm[d.in_off + k] / 32768.0f;
    return 0.0f;
}

__global__ __launch_bounds__(256) void k_resample_bank(const ResampleBankDesc* __restrict__ desc, int n_desc,
                                                       const int16_t* __restrict__ pcm, float* __restrict__ hist,
                                                       int16_t* __restrict__ out, const float* __restrict__ table, int L, int M,
                                                       int T, int half) {
    extern __shared__ float sm[];
    // the stream of this block: the last descriptor whose block0 <= blockIdx.x (block0 ascends; descriptor 0 starts at 0)
    const int b = blockIdx.x;
    int lo_d = 0, hi_d = n_desc - 1;
    while (lo_d < hi_d) {
        const int mid = (lo_d + hi_d + 1) >> 1;
        if (desc[mid].block0 <= b) lo_d = mid;
        else hi_d = mid - 1;
    }
    const ResampleBankDesc d = desc[lo_d];
    const int tile = b - d.block0;
    const int n_tiles = (d.cnt + 255) >> 8;
    if (tile >= n_tiles) {                        // tail block: the inputs from keep_from on, for the next call
        for (int j = threadIdx.x; j < d.keep; j += 256) hist[d.hist_wr + j] = bank_x(d, pcm, hist, d.keep_from + j);
        return;
    }
    float* tab = sm;                              // [L*T]
    float* xs = sm + L * T;                       // input span of this block
    const int i0 = tile * 256;
    const int i1 = min(d.cnt, i0 + 256);
    for (int k = threadIdx.x; k < L * T; k += 256) tab[k] = table[k];
    const long long lo = ((d.i_next + i0) * M + half) / L - (T - 1);
    const long long hi = ((d.i_next + i1 - 1) * M + half) / L;
    const int span = (int)(hi - lo + 1);
    for (int k = threadIdx.x; k < span; k += 256) xs[k] = bank_x(d, pcm, hist, lo + k);
    __syncthreads();
    const int i = i0 + threadIdx.x;
    if (i >= i1) return;
    const long long pos = (d.i_next + i) * M + half;
    const int p = (int)(pos % L);
    const int n0 = (int)(pos / L - lo);
    const float* tp = tab + p * T;
    float acc = 0.0f;
    for (int t = 0; t < T; t++) acc = fmaf(xs[n0 - t], tp[t], acc);
    float f = fminf(fmaxf(acc, -1.0f), 1.0f);
    out[(size_t)d.out_off + i] = (int16_t)(f * 32767.0f);     // truncation toward zero
}

size_t resample_lds(int L, int M, int T) {
    const long long span = ((long long)255 * M) / L + T + 2;
    return ((size_t)L * T + (size_t)span) * sizeof(float);
}

int launch_resample_bank(const ResampleBankDesc* d_desc, int n_desc, int n_blocks, const int16_t* d_pcm, float* d_hist,
                         int16_t* d_out, const float* d_table, int L, int M, int T, int half, hipStream_t s) {
    const size_t lds = resample_lds(L, M, T);
    if (lds > RESAMPLE_LDS_MAX) return -1;
    if (n_desc <= 0 || n_blocks <= 0) return 0;
    lds_limit_once<&k_resample_bank>(160 * 1024);
    hipLaunchKernelGGL(k_resample_bank, dim3(n_blocks), dim3(256), lds, s, d_desc, n_desc, d_pcm, d_hist, d_out, d_table, L, M, T, half);
    return 0;
}

}  // namespace bnhip
