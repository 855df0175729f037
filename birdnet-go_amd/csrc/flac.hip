// FLAC encoding of a batch of clips (DESIGN.md §9 "FLAC"): integer arithmetic but for the LPC coefficients' fp64 recursion, every
// frame independent.
//
//   analyse   one block per frame: the gained samples in LDS, the residuals of FIXED orders 0..4 (one wave per order), the sums
//             S[o][p][k] = sum of (u >> k) over the frame's finest partitions; coarser partitions are exact sums of those.  Then
//             the exact choice over (o, P, k) and one record per frame.  With lpc_order > 0 eight more waves own LPC orders 1..8:
//             windowed autocorrelation (int64), Levinson-Durbin by one thread, a thread per order quantises, then the same sums.
//   layout    a scan of frame bytes per clip, then of clip bytes across the batch -> offsets[n_clips + 1]
//   headers   "fLaC", STREAMINFO and the seek points of every clip
//   emit      one block per frame: the chosen residual again, a block scan of the code lengths, the codes ORed into a zeroed LDS
//             bit buffer (the zeros of the unary parts cost nothing), CRC-8 and CRC-16, then the frame copied to its byte offset.
// A frame's absolute offset is offsets[clip] + head_bytes + rel[frame]: emit and headers add the three, which saves a pass that
// would only store the sums.  Vector stores only.
// Geometry (ragged.h): a uniform batch runs analyse and emit on a (frames, n_clips) grid and indexes by arithmetic; a ragged burst
// runs them on the flat list of all clips' frames, and a block finds (clip, frame in clip) by a search over frame0[n_clips + 1].
// Everything a clip's stream depends on - its length, frame count, seek points, head size - is derived from the clip's own length
// in both forms, so a clip's bytes do not depend on its neighbours.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "block_scan.h"
#include "flac.h"
#include "pcmgain.h"
#include "ragged.h"

namespace bnhip {

namespace {

typedef unsigned long long u64;

constexpr int AN_THREADS = 64 * (FLAC_MAX_ORDER + 1);    // analyse: wave o owns order o
constexpr int AN_THREADS_LPC = AN_THREADS + 64 * FLAC_MAX_LPC_ORDER;      // and with LPC wave 4 + m owns LPC order m
constexpr int EM_THREADS = 256;
constexpr int NK = FLAC_MAX_K + 1;
constexpr int NPART = 1 << FLAC_MAX_PORDER;              // finest partitions
constexpr int NLEVEL = 2 * NPART - 1;                    // partitions of all orders: order P starts at (1 << P) - 1
// the longest frame: 4 + 7 (frame number) + 2 (block size) + 1 (CRC-8), a VERBATIM subframe, CRC-16; words, one spare for the copy
constexpr int FRAME_MAX_BYTES = 14 + 1 + 2 * FLAC_BLOCK + 2;
constexpr int W_WORDS = (FRAME_MAX_BYTES + 3) / 4 + 1;
// the largest folded residual of the FIXED orders on int16 input: order 4 gives |r| <= 8 * 32767 + 8 * 32768 = 524280, u <= 2 |r|
constexpr unsigned long long FLAC_MAX_FOLD = 2 * 524280;

__host__ __device__ inline int frame_no_bytes(u64 v) {
    return v < 0x80ull ? 1 : v < 0x800ull ? 2 : v < 0x10000ull ? 3 : v < 0x200000ull ? 4 : v < 0x4000000ull ? 5 : v < 0x80000000ull ? 6 : 7;
}
__host__ __device__ inline int block_size_bytes(int bs) { return bs == FLAC_BLOCK ? 0 : bs <= 256 ? 1 : 2; }
__host__ __device__ inline int frame_head_bytes(u64 frame_no, int bs) { return 4 + frame_no_bytes(frame_no) + block_size_bytes(bs) + 1; }
__host__ __device__ inline int frame_block(int n, int f) {
    const long long left = (long long)n - (long long)f * FLAC_BLOCK;
    return left < FLAC_BLOCK ? (int)left : FLAC_BLOCK;
}
__host__ __device__ inline int seek_points_of(int n, int seek_interval) {
    if (seek_interval <= 0 || n < 1) return 0;
    const long long last = ((long long)(n - 1) / seek_interval) * seek_interval;       // the last multiple below n
    return seek_interval >= FLAC_BLOCK ? (int)(last / seek_interval) + 1 : (int)(last / FLAC_BLOCK) + 1;
}
// everything of a stream before its first frame
__host__ __device__ inline u64 stream_head_bytes(int seek_points) {
    return (u64)FLAC_STREAM_HEAD + (seek_points > 0 ? 4ull + (u64)FLAC_SEEK_POINT * (u64)seek_points : 0ull);
}
__host__ __device__ inline int rate_code(int rate) {
    switch (rate) {
        case 88200: return 1; case 176400: return 2; case 192000: return 3; case 8000: return 4; case 16000: return 5;
        case 22050: return 6; case 24000: return 7; case 32000: return 8; case 44100: return 9; case 48000: return 10;
        case 96000: return 11; default: return 0;
    }
}

// the residual of FIXED order o at sample i >= o
__device__ __forceinline__ int fixed_residual(const int* __restrict__ x, int i, int o) {
    switch (o) {
        case 0: return x[i];
        case 1: return x[i] - x[i - 1];
        case 2: return x[i] - 2 * x[i - 1] + x[i - 2];
        case 3: return x[i] - 3 * x[i - 1] + 3 * x[i - 2] - x[i - 3];
        default: return x[i] - 4 * x[i - 1] + 6 * x[i - 2] - 4 * x[i - 3] + x[i - 4];
    }
}
// u = 2 r for r >= 0, -2 r - 1 otherwise
__device__ __forceinline__ uint32_t rice_fold(int r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }

// A call's frames: frame0 NULL for a uniform batch of `frames` frames per clip, else the prefix table [n_clips + 1] of a ragged burst.
struct FlacGeom {
    ClipGeom c;
    int frames = 0;
    const long long* frame0 = nullptr;
};
// One clip of the call: its samples, its first sample in pcm, its frames, its first frame's index in rec / rel / lpc.
struct FlacClip { int n; long long x0; int frames; long long f0; };
__device__ __forceinline__ FlacClip flac_clip(const FlacGeom& g, int clip) {
    FlacClip k;
    k.n = clip_len(g.c, clip); k.x0 = clip_start(g.c, clip);
    k.frames = g.frame0 ? (int)(g.frame0[clip + 1] - g.frame0[clip]) : g.frames;
    k.f0 = g.frame0 ? g.frame0[clip] : (long long)clip * g.frames;
    return k;
}
// The frame of a block of analyse / emit: grid (frames, n_clips) of a uniform batch, (all frames) of a ragged burst.
__device__ __forceinline__ FlacClip block_frame(const FlacGeom& g, int* clip, int* f) {
    if (g.frame0) {
        *clip = ragged_clip(g.frame0, g.c.n_clips, (long long)blockIdx.x);
        *f = (int)((long long)blockIdx.x - g.frame0[*clip]);
    } else { *clip = blockIdx.y; *f = blockIdx.x; }
    return flac_clip(g, *clip);
}

__device__ __forceinline__ void stage_frame(const int16_t* __restrict__ pcm, const double* __restrict__ factor, const FlacClip& k, int clip, int f,
                                            int bs, int* __restrict__ xs, int tid, int threads) {
    const double fac = factor ? factor[clip] : 1.0;
    const int16_t* x = pcm + k.x0 + (long long)f * FLAC_BLOCK;                         // f * 4096 + i < n
    for (int i = tid; i < bs; i += threads) xs[i] = (int)pcm_gained(x[i], fac);
}

// the residual of LPC order m at sample i >= m: q[j] multiplies x[i - 1 - j]; |sum| <= 8 * 2048 * 32768 = 2^29
__device__ __forceinline__ int lpc_residual(const int* __restrict__ x, int i, int m, const int* __restrict__ q, int shift) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < FLAC_MAX_LPC_ORDER; j++)
        if (j < m) s += q[j] * x[i - 1 - j];
    return x[i] - (s >> shift);
}

// One candidate of a frame's list.
struct Candidate { int kind, order, porder; u64 bits; };

// What the LPC part of the analysis keeps in LDS.
struct LpcShared {
    u64 R[FLAC_MAX_LPC_ORDER + 1];
    double rd[FLAC_MAX_LPC_ORDER + 1];
    double A[FLAC_MAX_LPC_ORDER][FLAC_MAX_LPC_ORDER];       // A[m - 1][j - 1] = a_j of order m
    int qs[FLAC_MAX_LPC_ORDER][FLAC_MAX_LPC_ORDER];
    int qshift[FLAC_MAX_LPC_ORDER];
    int offered[FLAC_MAX_LPC_ORDER];
    int over[FLAC_MAX_LPC_ORDER];                           // a residual of the order broke the fold bound
    int reached;                                            // the recursion's last order
};
// The LPC candidates' coefficients (DESIGN.md §9 "FLAC", LPC candidates): xs holds the frame; xw is bs words of scratch.  On return
// qs[m - 1] / qshift[m - 1] hold order m's quantised coefficients and shift where offered[m - 1] is set.  Called by the whole
// block; it ends synchronised.
__device__ __forceinline__ void lpc_coefficients(const int* __restrict__ xs, int* __restrict__ xw, int bs, int mmax, LpcShared& S, int tid,
                                                 int threads) {
    // the window: a Welch window scaled to 2^14, non-zero at both ends; |xw| <= 2^23
    const u64 den = (u64)(bs + 1) * (u64)(bs + 1);
    for (int i = tid; i < bs; i += threads) {
        const int w = (int)((((u64)4 * (u64)(i + 1) * (u64)(bs - i)) << 14) / den);
        xw[i] = (xs[i] * w) >> 6;
    }
    if (tid <= FLAC_MAX_LPC_ORDER) S.R[tid] = 0ull;
    if (tid < FLAC_MAX_LPC_ORDER) { S.offered[tid] = 0; S.over[tid] = 0; }
    __syncthreads();
    // the lags: |R| <= 4096 * 2^46, exact in int64 in any order
    long long acc[FLAC_MAX_LPC_ORDER + 1];
#pragma unroll
    for (int l = 0; l <= FLAC_MAX_LPC_ORDER; l++) acc[l] = 0;
    for (int i = tid; i < bs; i += threads) {
        const long long a = xw[i];
#pragma unroll
        for (int l = 0; l <= FLAC_MAX_LPC_ORDER; l++)
            if (i >= l) acc[l] += a * (long long)xw[i - l];
    }
#pragma unroll
    for (int l = 0; l <= FLAC_MAX_LPC_ORDER; l++) {
        for (int d = 32; d >= 1; d >>= 1) acc[l] += __shfl_xor(acc[l], d);
        if ((tid & 63) == 0) atomicAdd(&S.R[l], (u64)acc[l]);
    }
    __syncthreads();
    if (tid == 0) {
        // Levinson-Durbin in fp64: one rounding per operation, in this order (the build forbids contraction)
        int stop = 0;
        if (S.R[0] != 0ull) {
            for (int l = 0; l <= FLAC_MAX_LPC_ORDER; l++) S.rd[l] = (double)(long long)S.R[l];
            double err = S.rd[0];
            for (int m = 1; m <= mmax; m++) {
                double a = S.rd[m];
                for (int j = 1; j < m; j++) a = a - S.A[m - 2][j - 1] * S.rd[m - j];
                const double k = a / err;
                for (int j = 1; j < m; j++) S.A[m - 1][j - 1] = S.A[m - 2][j - 1] - k * S.A[m - 2][m - j - 1];
                S.A[m - 1][m - 1] = k;
                err = err * (1.0 - k * k);
                stop = m;
                if (!(err > 0.0)) break;
            }
        }
        S.reached = stop;
    }
    __syncthreads();
    if (tid < FLAC_MAX_LPC_ORDER && tid + 1 <= S.reached) {
        // thread m - 1 quantises order m: precision 12, error feedback
        const int m = tid + 1;
        double cmax = 0.0;
        bool finite = true;
        for (int j = 0; j < m; j++) {
            const double v = fabs(S.A[m - 1][j]);
            finite = finite && isfinite(v);
            if (v > cmax) cmax = v;
        }
        if (finite && cmax > 0.0) {
            int e;
            (void)frexp(cmax, &e);
            int shift = FLAC_LPC_PRECISION - 1 - e;
            if (shift > FLAC_LPC_MAX_SHIFT) shift = FLAC_LPC_MAX_SHIFT;
            if (shift >= 0) {
                const double scale = (double)(1 << shift);
                double ef = 0.0;
                for (int j = 0; j < m; j++) {
                    ef = ef + S.A[m - 1][j] * scale;
                    double t = rint(ef);
                    t = t < -2048.0 ? -2048.0 : t > 2047.0 ? 2047.0 : t;
                    S.qs[m - 1][j] = (int)t;
                    ef = ef - t;
                }
                S.qshift[m - 1] = shift;
                S.offered[m - 1] = 1;
            }
        }
    }
    __syncthreads();
}

// Grid: block_frame's.  LPC: whether LPC orders 1..lpc_order are candidates; without, the block is five waves and the code that of
// the FIXED-only encoder.  A slot s is a predictor: FIXED order s for s <= 4, LPC order s - 4 above; wave s owns slot s.
template <bool LPC>
__global__ __launch_bounds__(LPC ? AN_THREADS_LPC : AN_THREADS) void k_flac_analyse(const int16_t* __restrict__ pcm, const double* __restrict__ factor,
                                                                                   FlacGeom g, int lpc_order, FlacRecord* __restrict__ rec,
                                                                                   FlacLpc* __restrict__ lpc) {
    constexpr int NS = FLAC_MAX_ORDER + 1 + (LPC ? FLAC_MAX_LPC_ORDER : 0);
    constexpr int THREADS = 64 * NS;
    __shared__ int xs[FLAC_BLOCK];
    // uint32 holds a finest partition's sum: u <= FLAC_MAX_FOLD = 1048560; a block of 4096 has 32 partitions of 128, and the longest
    // single partition is an odd block's 4095 samples: 4095 * 1048560 < 2^32 (by 0.03 %).
    // An LPC order with a folded residual above FLAC_MAX_FOLD is not a candidate, so the condition below covers both families.
    static_assert((unsigned long long)(FLAC_BLOCK - 1) * FLAC_MAX_FOLD <= 0xffffffffull, "finest partition sums overflow uint32");
    __shared__ uint32_t fine[NS][NPART][NK];
    static_assert(!LPC || sizeof(fine) >= sizeof(int) * FLAC_BLOCK, "the windowed samples borrow the sums' space");
    __shared__ u64 pbits[NS][NLEVEL];
    __shared__ uint8_t pk[NS][NLEVEL];
    __shared__ u64 cost[NS][FLAC_MAX_PORDER + 1];
    __shared__ Candidate chosen;
    __shared__ LpcShared S;                                         // (LPC only)
    const int tid = threadIdx.x;
    int clip, f;
    const FlacClip kc = block_frame(g, &clip, &f);
    const int bs = frame_block(kc.n, f);
    stage_frame(pcm, factor, kc, clip, f, bs, xs, tid, THREADS);
    if (!LPC)
        for (int i = tid; i < NS * NPART * NK; i += THREADS) (&fine[0][0][0])[i] = 0u;
    __syncthreads();
    int diff = 0;
    for (int i = tid; i < bs; i += THREADS) diff |= xs[i] != xs[0];
    const int differs = __syncthreads_or(diff);

    const int tz = __ffs(bs) - 1;
    const int pmax = tz < FLAC_MAX_PORDER ? tz : FLAC_MAX_PORDER;
    const int omax = bs - 1 < FLAC_MAX_ORDER ? bs - 1 : FLAC_MAX_ORDER;
    const int mmax = LPC ? (bs - 1 < lpc_order ? bs - 1 : lpc_order) : 0;
    const int np = 1 << pmax, L = bs >> pmax;                       // finest partitions and their length
    if constexpr (LPC) {
        lpc_coefficients(xs, reinterpret_cast<int*>(&fine[0][0][0]), bs, mmax, S, tid, THREADS);
        for (int i = tid; i < NS * NPART * NK; i += THREADS) (&fine[0][0][0])[i] = 0u;
        __syncthreads();
    }
    // a slot's predictor order, and whether it is a candidate at all
    auto order_of = [](int s) { return s <= FLAC_MAX_ORDER ? s : s - FLAC_MAX_ORDER; };
    auto live = [&](int s) {
        if (s <= FLAC_MAX_ORDER) return s <= omax;
        if constexpr (LPC) {
            const int m = s - FLAC_MAX_ORDER;
            return m <= mmax && S.offered[m - 1] && !S.over[m - 1];
        }
        return false;
    };
    {   // wave s, lane -> (partition, chunk of it); a lane starts `lane` samples into its chunk, so that the lanes of a wave read
        // different LDS banks when the chunk length is a multiple of 64
        const int s = tid >> 6, lane = tid & 63, o = order_of(s);
        const int cn = 64 >> pmax, lc = (L + cn - 1) / cn;
        const int part = lane / cn, c = lane % cn;
        const int start = part * L + c * lc;
        const int end = min(start + lc, (part + 1) * L);
        if (live(s) && start < end) {
            int q[FLAC_MAX_LPC_ORDER], shift = 0;
            if constexpr (LPC) {
                if (s > FLAC_MAX_ORDER) {
#pragma unroll
                    for (int j = 0; j < FLAC_MAX_LPC_ORDER; j++) q[j] = j < o ? S.qs[o - 1][j] : 0;
                    shift = S.qshift[o - 1];
                }
            }
            uint32_t acc[NK];
#pragma unroll
            for (int k = 0; k < NK; k++) acc[k] = 0u;
            bool over = false;
            int jj = lane % lc;
            for (int j = 0; j < lc; j++) {
                const int i = start + jj;
                if (i < end && i >= o) {
                    const uint32_t u = rice_fold(LPC && s > FLAC_MAX_ORDER ? lpc_residual(xs, i, o, q, shift) : fixed_residual(xs, i, s));
                    if (LPC && u > (uint32_t)FLAC_MAX_FOLD) over = true;
                    else {
#pragma unroll
                        for (int k = 0; k < NK; k++) acc[k] += u >> k;
                    }
                }
                jj = jj + 1 == lc ? 0 : jj + 1;
            }
#pragma unroll
            for (int k = 0; k < NK; k++) atomicAdd(&fine[s][part][k], acc[k]);
            if constexpr (LPC) {
                if (over) S.over[o - 1] = 1;
            }
        }
    }
    __syncthreads();
    // every partition of every slot: its sums from the finest ones, its k (ties to the lowest) and its bits
    if (tid < NS * NLEVEL) {
        const int s = tid / NLEVEL, q = tid % NLEVEL, o = order_of(s);
        const int P = 31 - __clz(q + 1), p = q + 1 - (1 << P);
        if (live(s) && P <= pmax && (bs >> P) > o) {
            const int span = 1 << (pmax - P), first = p * span;
            const u64 cnt = (u64)((bs >> P) - (p == 0 ? o : 0));
            u64 best = ~0ull; int kb = 0;
#pragma unroll 1
            for (int k = 0; k < NK; k++) {
                u64 sum = 0;
                for (int j = 0; j < span; j++) sum += fine[s][first + j][k];
                const u64 b = (u64)(1 + k) * cnt + sum;
                if (b < best) { best = b; kb = k; }
            }
            pbits[s][q] = best; pk[s][q] = (uint8_t)kb;
        }
    }
    __syncthreads();
    if (tid < NS * (FLAC_MAX_PORDER + 1)) {
        const int s = tid / (FLAC_MAX_PORDER + 1), P = tid % (FLAC_MAX_PORDER + 1), o = order_of(s);
        u64 c = ~0ull;
        if (live(s) && P <= pmax && (bs >> P) > o) {
            // FIXED: type byte, warm-up, method and partition order; LPC: also 4 bits of precision, 5 of shift, 12 per coefficient
            c = s <= FLAC_MAX_ORDER ? 8 + 16 * o + 6 : 8 + 16 * o + 4 + 5 + FLAC_LPC_PRECISION * o + 6;
            for (int p = 0; p < (1 << P); p++) c += 4 + pbits[s][(1 << P) - 1 + p];
        }
        cost[s][P] = c;
    }
    __syncthreads();
    if (tid == 0) {
        // the candidate list, in rank order: CONSTANT (when it applies), the FIXED candidates by (P, o), the LPC candidates by
        // (P, m), VERBATIM.  A predictor replaces the choice only by strictly fewer bits, and the best predictor is taken only if it
        // has strictly fewer bits than VERBATIM; CONSTANT, where it applies, is taken outright.
        Candidate best{FLAC_VERBATIM, 0, 0, (u64)(8 + 16 * bs)};
        if (!differs) best = Candidate{FLAC_CONSTANT, 0, 0, 8 + 16};
        else {
            Candidate fx{FLAC_FIXED, 0, 0, ~0ull};
            for (int P = 0; P <= pmax; P++)
                for (int o = 0; o <= omax; o++)
                    if (cost[o][P] < fx.bits) fx = Candidate{FLAC_FIXED, o, P, cost[o][P]};
            if (LPC)
                for (int P = 0; P <= pmax; P++)
                    for (int m = 1; m <= mmax; m++)
                        if (cost[FLAC_MAX_ORDER + m][P] < fx.bits) fx = Candidate{FLAC_LPC, m, P, cost[FLAC_MAX_ORDER + m][P]};
            if (fx.bits < best.bits) best = fx;
        }
        chosen = best;
    }
    __syncthreads();
    const Candidate ch = chosen;
    const bool coded = ch.kind == FLAC_FIXED || ch.kind == FLAC_LPC;
    const int slot = ch.kind == FLAC_LPC ? FLAC_MAX_ORDER + ch.order : ch.order;
    FlacRecord* r = rec + kc.f0 + f;
    if (tid < NPART) r->k[tid] = (coded && tid < (1 << ch.porder)) ? pk[slot][(1 << ch.porder) - 1 + tid] : (uint8_t)0;
    if (tid == 0) {
        r->kind = (uint8_t)ch.kind; r->order = (uint8_t)ch.order; r->porder = (uint8_t)ch.porder; r->reserved = 0;
        r->bits = (uint32_t)ch.bits;                                   // <= 8 + 16 * 4096
        r->bytes = (uint32_t)(frame_head_bytes((u64)f, bs) + (int)((ch.bits + 7) / 8) + 2);
        r->reserved2 = 0;
    }
    if constexpr (LPC) {
        FlacLpc* l = lpc + kc.f0 + f;
        const bool won = ch.kind == FLAC_LPC;
        if (tid < FLAC_MAX_LPC_ORDER) l->q[tid] = (won && tid < ch.order) ? (int16_t)S.qs[ch.order - 1][tid] : (int16_t)0;
        if (tid == 0) l->shift = won ? S.qshift[ch.order - 1] : 0;
    }
}

// One block per clip: rel[f], the clip's bytes, its smallest and largest frame.
__global__ __launch_bounds__(256) void k_flac_layout_clip(FlacGeom g, int seek_interval, const FlacRecord* __restrict__ rec, u64* __restrict__ rel,
                                                          u64* __restrict__ clip_bytes, uint32_t* __restrict__ fmin, uint32_t* __restrict__ fmax) {
    __shared__ u64 sh[256];
    __shared__ uint32_t lo, hi;
    const int clip = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { lo = 0xffffffffu; hi = 0u; }
    __syncthreads();
    const FlacClip kc = flac_clip(g, clip);
    const int frames = kc.frames;
    const long long base = kc.f0;
    const u64 head_bytes = stream_head_bytes(seek_points_of(kc.n, seek_interval));
    u64 carry = 0;
    uint32_t mn = 0xffffffffu, mx = 0u;
    for (int f0 = 0; f0 < frames; f0 += 256) {
        const int f = f0 + tid;
        const uint32_t b = f < frames ? rec[base + f].bytes : 0u;
        if (f < frames) { mn = min(mn, b); mx = max(mx, b); }
        const u64 incl = block_scan<u64>((u64)b, sh, tid);
        if (f < frames) rel[base + f] = carry + incl - b;
        carry += sh[255];
        __syncthreads();
    }
    atomicMin(&lo, mn); atomicMax(&hi, mx);
    __syncthreads();
    if (tid == 0) { clip_bytes[clip] = head_bytes + carry; fmin[clip] = lo; fmax[clip] = hi; }
}

// One block: offsets[c] = the bytes of the clips before c, offsets[n_clips] = all of them.
__global__ __launch_bounds__(256) void k_flac_layout_batch(int n_clips, const u64* __restrict__ clip_bytes, u64* __restrict__ offsets) {
    __shared__ u64 sh[256];
    const int tid = threadIdx.x;
    u64 carry = 0;
    for (int c0 = 0; c0 < n_clips; c0 += 256) {
        const int c = c0 + tid;
        const u64 b = c < n_clips ? clip_bytes[c] : 0ull;
        const u64 incl = block_scan<u64>(b, sh, tid);
        if (c < n_clips) offsets[c] = carry + incl - b;
        carry += sh[255];
        __syncthreads();
    }
    if (tid == 0) offsets[n_clips] = carry;
}

__device__ __forceinline__ void store_be(uint8_t* __restrict__ p, u64 v, int bytes) {
    for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * (bytes - 1 - i)));
}

// One block per clip: the stream marker, STREAMINFO, and with seek points the SEEKTABLE.
__global__ __launch_bounds__(256) void k_flac_headers(FlacGeom g, int rate, int seek_interval, const u64* __restrict__ offsets,
                                                      const u64* __restrict__ rel, const uint32_t* __restrict__ fmin, const uint32_t* __restrict__ fmax,
                                                      uint8_t* __restrict__ out, u64 out_cap) {
    const int clip = blockIdx.x, tid = threadIdx.x;
    const FlacClip kc = flac_clip(g, clip);
    const int n = kc.n, seek_points = seek_points_of(n, seek_interval);
    const u64 base = offsets[clip];
    const u64 head = stream_head_bytes(seek_points);
    if (base + head > out_cap) return;
    uint8_t* o = out + base;
    if (tid == 0) {
        o[0] = 'f'; o[1] = 'L'; o[2] = 'a'; o[3] = 'C';
        o[4] = seek_points > 0 ? 0x00 : 0x80;                           // last-block flag, type 0
        store_be(o + 5, 34, 3);
        store_be(o + 8, FLAC_BLOCK, 2); store_be(o + 10, FLAC_BLOCK, 2);
        store_be(o + 12, fmin[clip], 3); store_be(o + 15, fmax[clip], 3);
        // 20 bits rate, 3 bits channels - 1, 5 bits sample size - 1, 36 bits total samples
        store_be(o + 18, ((u64)rate << 44) | (0ull << 41) | (15ull << 36) | (u64)n, 8);
        for (int i = 26; i < 42; i++) o[i] = 0;                         // MD5: unknown
        if (seek_points > 0) { o[42] = 0x83; store_be(o + 43, (u64)FLAC_SEEK_POINT * (u64)seek_points, 3); }
    }
    // point q: an interval of a frame or more names another frame each time; a shorter one names every frame up to the last
    // multiple's, each once
    for (int q = tid; q < seek_points; q += 256) {
        const int f = seek_interval >= FLAC_BLOCK ? (int)(((long long)q * seek_interval) / FLAC_BLOCK) : q;
        uint8_t* p = o + FLAC_STREAM_HEAD + 4 + (u64)FLAC_SEEK_POINT * (u64)q;
        store_be(p, (u64)f * FLAC_BLOCK, 8);
        store_be(p + 8, rel[kc.f0 + f], 8);
        store_be(p + 16, (u64)frame_block(n, f), 2);
    }
}

// ORs the low `len` (1..32) bits of v into the MSB-first bit buffer at bit `pos`
__device__ __forceinline__ void put_bits(uint32_t* __restrict__ W, uint32_t pos, int len, uint32_t v) {
    const uint32_t w = pos >> 5;
    const int room = 32 - (int)(pos & 31);
    if (w + 1 >= (uint32_t)W_WORDS) return;
    if (len <= room) atomicOr(&W[w], v << (room - len));
    else { atomicOr(&W[w], v >> (len - room)); atomicOr(&W[w + 1], v << (32 - (len - room))); }
}
__device__ __forceinline__ uint32_t frame_byte(const uint32_t* __restrict__ W, int j) { return (W[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu; }

// a * b mod x^16 + x^15 + x^2 + 1
__device__ __forceinline__ uint32_t crc16_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 15; i >= 0; i--) {
        r = ((r << 1) ^ ((r & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// Grid: block_frame's.  LPC: whether a record may name an LPC subframe (then `lpc` holds its coefficients).
template <bool LPC>
__global__ __launch_bounds__(EM_THREADS) void k_flac_emit(const int16_t* __restrict__ pcm, const double* __restrict__ factor, FlacGeom g, int rate,
                                                          int seek_interval, const FlacRecord* __restrict__ rec, const FlacLpc* __restrict__ lpc,
                                                          const u64* __restrict__ rel, const u64* __restrict__ offsets, uint8_t* __restrict__ out,
                                                          u64 out_cap) {
    __shared__ int xs[FLAC_BLOCK];
    __shared__ uint32_t W[W_WORDS];
    __shared__ uint32_t sc[EM_THREADS];
    __shared__ uint32_t T[256];                                  // CRC-16 of one byte
    __shared__ uint32_t cv[EM_THREADS];
    __shared__ uint8_t ks[NPART];
    __shared__ int lq[FLAC_MAX_LPC_ORDER + 1];                  // (LPC only) the coefficients, then the shift
    const int tid = threadIdx.x;
    int clip, f;
    const FlacClip kc = block_frame(g, &clip, &f);
    const int bs = frame_block(kc.n, f);
    const FlacRecord* r = rec + kc.f0 + f;
    const int kind = r->kind, o = r->order, P = r->porder;
    const int bytes = (int)r->bytes, hb = frame_head_bytes((u64)f, bs);
    const u64 off = offsets[clip] + stream_head_bytes(seek_points_of(kc.n, seek_interval)) + rel[kc.f0 + f];
    if (bytes > FRAME_MAX_BYTES || bytes < hb + 2 || off + (u64)bytes > out_cap) return;       // (block-uniform)
    if (kind == FLAC_FIXED && (o > FLAC_MAX_ORDER || P > FLAC_MAX_PORDER || (bs >> P) <= o)) return;
    if (kind > FLAC_FIXED && (!LPC || kind != FLAC_LPC || o < 1 || o > FLAC_MAX_LPC_ORDER || P > FLAC_MAX_PORDER || (bs >> P) <= o)) return;
    if constexpr (LPC) {
        const FlacLpc* l = lpc + kc.f0 + f;
        if (kind == FLAC_LPC && (l->shift < 0 || l->shift > FLAC_LPC_MAX_SHIFT)) return;
        if (tid < FLAC_MAX_LPC_ORDER) lq[tid] = l->q[tid];
        if (tid == FLAC_MAX_LPC_ORDER) lq[tid] = l->shift;
    }
    const bool is_lpc = LPC && kind == FLAC_LPC;
    // the subframe's bits before the residual's method: the type byte, the warm-up, and for LPC precision, shift and coefficients
    const int pre = is_lpc ? 8 + 16 * o + 4 + 5 + FLAC_LPC_PRECISION * o : 8 + 16 * o;
    stage_frame(pcm, factor, kc, clip, f, bs, xs, tid, EM_THREADS);
    for (int i = tid; i < W_WORDS; i += EM_THREADS) W[i] = 0u;
    if (tid < NPART) ks[tid] = r->k[tid];
    {
        uint32_t c = (uint32_t)tid << 8;
#pragma unroll
        for (int i = 0; i < 8; i++) c = ((c << 1) ^ ((c & 0x8000u) ? 0x8005u : 0u)) & 0xffffu;
        T[tid] = c;
    }
    __syncthreads();

    const uint32_t sub = 8u * (uint32_t)hb;                      // the subframe's first bit
    if (tid == 0) {
        uint8_t h[16];
        int m = 0;
        h[m++] = 0xff; h[m++] = 0xf8;                            // sync 0x3FFE, reserved 0, fixed block size
        const int bsb = block_size_bytes(bs);
        h[m++] = (uint8_t)(((bsb == 0 ? 12 : bsb == 1 ? 6 : 7) << 4) | rate_code(rate));
        h[m++] = 0x08;                                           // mono, 16 bits, reserved 0
        const u64 v = (u64)f;
        const int nb = frame_no_bytes(v);
        if (nb == 1) h[m++] = (uint8_t)v;
        else {
            h[m++] = (uint8_t)(((0xff00u >> nb) & 0xffu) | (uint32_t)(v >> (6 * (nb - 1))));
            for (int j = nb - 2; j >= 0; j--) h[m++] = (uint8_t)(0x80u | (uint32_t)((v >> (6 * j)) & 0x3fu));
        }
        if (bsb == 1) h[m++] = (uint8_t)(bs - 1);
        else if (bsb == 2) { h[m++] = (uint8_t)((bs - 1) >> 8); h[m++] = (uint8_t)(bs - 1); }
        uint32_t c8 = 0;
        for (int j = 0; j < m; j++) {
            c8 ^= h[j];
            for (int i = 0; i < 8; i++) c8 = ((c8 << 1) ^ ((c8 & 0x80u) ? 0x07u : 0u)) & 0xffu;
        }
        h[m++] = (uint8_t)c8;
        for (int j = 0; j < m; j++) put_bits(W, 8u * j, 8, h[j]);
        // the subframe header: a zero bit, six bits of type, no wasted bits
        put_bits(W, sub, 8, kind == FLAC_CONSTANT ? 0x00u : kind == FLAC_VERBATIM ? 0x02u : is_lpc ? (uint32_t)((32 | (o - 1)) << 1)
                                                                                                   : (uint32_t)((8 | o) << 1));
        if (kind == FLAC_CONSTANT) put_bits(W, sub + 8, 16, (uint32_t)xs[0] & 0xffffu);
        if constexpr (LPC) {
            if (is_lpc) {
                put_bits(W, sub + 8 + 16 * o, 4, (uint32_t)(FLAC_LPC_PRECISION - 1));
                put_bits(W, sub + 8 + 16 * o + 4, 5, (uint32_t)lq[FLAC_MAX_LPC_ORDER]);
                for (int j = 0; j < o; j++) put_bits(W, sub + 8 + 16 * o + 9 + FLAC_LPC_PRECISION * j, FLAC_LPC_PRECISION, (uint32_t)lq[j] & 0xfffu);
            }
        }
        if (kind == FLAC_FIXED || is_lpc) put_bits(W, sub + pre, 6, (uint32_t)P);    // method 00, partition order
    }
    if (kind == FLAC_VERBATIM) {
        for (int i = tid; i < bs; i += EM_THREADS) put_bits(W, sub + 8 + 16 * i, 16, (uint32_t)xs[i] & 0xffffu);
    } else if (kind == FLAC_FIXED || is_lpc) {
        int q[FLAC_MAX_LPC_ORDER], shift = 0;
        if constexpr (LPC) {
#pragma unroll
            for (int j = 0; j < FLAC_MAX_LPC_ORDER; j++) q[j] = lq[j];
            shift = lq[FLAC_MAX_LPC_ORDER];
        }
        auto residual = [&](int i) { return is_lpc ? lpc_residual(xs, i, o, q, shift) : fixed_residual(xs, i, o); };
        if (tid < o) put_bits(W, sub + 8 + 16 * tid, 16, (uint32_t)xs[tid] & 0xffffu);
        // a thread's samples are contiguous; a code is q zeros, a one, k bits; a partition's first code follows its 4-bit k
        const int ch = (bs + EM_THREADS - 1) / EM_THREADS;
        const int i0 = max(tid * ch, o), i1 = min(tid * ch + ch, bs);
        // (the partition index and the offset in it advance with i: one division per thread, not per sample)
        const int lp = bs >> P;
        const int part0 = i0 < i1 ? i0 / lp : 0, rem0 = i0 < i1 ? i0 - part0 * lp : 0;
        uint32_t total = 0;
        for (int i = i0, part = part0, rem = rem0; i < i1; i++) {
            const int k = ks[part];
            total += (rice_fold(residual(i)) >> k) + 1u + (uint32_t)k + ((i == o || rem == 0) ? 4u : 0u);
            if (++rem == lp) { rem = 0; part++; }
        }
        const uint32_t incl = block_scan<uint32_t>(total, sc, tid);
        uint32_t pos = sub + pre + 6 + (incl - total);
        for (int i = i0, part = part0, rem = rem0; i < i1; i++) {
            const int k = ks[part];
            const uint32_t u = rice_fold(residual(i));
            if (i == o || rem == 0) { put_bits(W, pos, 4, (uint32_t)k); pos += 4; }
            const uint32_t q = u >> k;
            put_bits(W, pos + q, k + 1, (1u << k) | (u & ((1u << k) - 1u)));
            pos += q + 1u + (uint32_t)k;
            if (++rem == lp) { rem = 0; part++; }
        }
    }
    __syncthreads();

    // CRC-16 of the D bytes before it.  Both CRCs start from 0, so zero bytes in front change nothing: the frame is taken as
    // 256 chunks of C bytes with the padding in front, and crc(A || B) = crc(A) x^(8 |B|) mod P ^ crc(B) folds them in a tree.
    const int D = bytes - 2;
    const int C = (D + EM_THREADS - 1) / EM_THREADS, padding = EM_THREADS * C - D;
    uint32_t crc = 0, mul = 1;
    for (int j = 0; j < C; j++) {
        const int b = tid * C + j - padding;
        if (b >= 0) crc = ((crc << 8) ^ T[(crc >> 8) ^ frame_byte(W, b)]) & 0xffffu;
        mul = ((mul << 8) ^ T[mul >> 8]) & 0xffffu;                                  // x^(8 C)
    }
    cv[tid] = crc;
    for (int s = 1; s < EM_THREADS; s <<= 1) {
        __syncthreads();
        if ((tid & (2 * s - 1)) == 0) cv[tid] = crc16_mul(cv[tid], mul) ^ cv[tid + s];
        mul = crc16_mul(mul, mul);
    }
    if (tid == 0) put_bits(W, 8u * (uint32_t)D, 16, cv[0]);
    __syncthreads();

    // the copy: bytes up to the first 4-byte boundary of the destination, whole words, the bytes left over
    uint8_t* dst = out + off;
    int head = (int)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
    head = head < bytes ? head : bytes;
    const int nw = (bytes - head) / 4, tail = bytes - head - 4 * nw;
    if (tid < head) dst[tid] = (uint8_t)frame_byte(W, tid);
    for (int w = tid; w < nw; w += EM_THREADS) {
        const int i = head + 4 * w, sh = 8 * (i & 3);
        const uint32_t hi = W[i >> 2], lo = W[(i >> 2) + 1];                         // (the spare word)
        const uint32_t be = sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
        *reinterpret_cast<uint32_t*>(dst + i) = __builtin_bswap32(be);
    }
    if (tid < tail) dst[head + 4 * nw + tid] = (uint8_t)frame_byte(W, head + 4 * nw + tid);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

int flac_frames(int n) { return (int)(((long long)n + FLAC_BLOCK - 1) / FLAC_BLOCK); }

int flac_seek_points(int n, int seek_interval) { return seek_points_of(n, seek_interval); }

size_t flac_max_bytes(int n_clips, int n, int seek_interval) {
    size_t b = (size_t)stream_head_bytes(flac_seek_points(n, seek_interval));
    const long long full = n / FLAC_BLOCK;
    const int rem = n % FLAC_BLOCK;
    // full frames: 5 header bytes beside the frame number, the subframe byte, the samples, the CRC-16
    b += (size_t)full * (size_t)(5 + 1 + 2 * FLAC_BLOCK + 2);
    const long long lim[7] = {0x80, 0x800, 0x10000, 0x200000, 0x4000000, 0x80000000ll, 0x1000000000ll};
    long long lo = 0;
    for (int i = 0; i < 7 && lo < full; i++) {
        const long long hi = std::min(full, lim[i]);
        b += (size_t)(hi - lo) * (size_t)(i + 1);
        lo = hi;
    }
    if (rem) b += (size_t)(frame_head_bytes((u64)full, rem) + 1 + 2 * rem + 2);
    return b * (size_t)n_clips;
}

size_t flac_max_bytes(const Clips& clips, int seek_interval) {
    return clips.sum([&](int n) { return flac_max_bytes(1, n, seek_interval); });
}

namespace {

// the arrays of F frames of n_clips clips, after `tables` bytes of prefix tables
size_t work_bytes(size_t tables, size_t n_clips, size_t F, int lpc_order) {
    return tables + align256(F * sizeof(FlacRecord)) + align256(F * 8) + align256(n_clips * 8) + 2 * align256(n_clips * 4) +
           (lpc_order > 0 ? align256(F * sizeof(FlacLpc)) : 0);
}
void carve(FlacWork& w, char* p, size_t F) {
    const size_t n_clips = (size_t)w.n_clips;
    w.rec = (FlacRecord*)p; p += align256(F * sizeof(FlacRecord));
    w.rel = (u64*)p; p += align256(F * 8);
    w.clip_bytes = (u64*)p; p += align256(n_clips * 8);
    w.fmin = (uint32_t*)p; p += align256(n_clips * 4);
    w.fmax = (uint32_t*)p; p += align256(n_clips * 4);
    if (w.lpc_order > 0) w.lpc = (FlacLpc*)p;
}
size_t tables_bytes(const Clips& clips) { return clips.lens ? align256(2 * ((size_t)clips.n_clips + 1) * 8) : 0; }

}  // namespace

size_t flac_workspace_bytes(const Clips& clips, int lpc_order) {
    return work_bytes(tables_bytes(clips), (size_t)clips.n_clips, clips.sum(flac_frames), lpc_order);
}

FlacWork flac_work(const Clips& clips, int rate, int seek_interval, void* d_block, int lpc_order) {
    const int n_clips = clips.n_clips;
    FlacWork w;
    w.n_clips = n_clips; w.n = clips.n; w.rate = rate; w.seek_interval = seek_interval; w.lpc_order = lpc_order;
    if (!clips.lens) {
        w.frames = flac_frames(clips.n);
        w.total_frames = (long long)n_clips * w.frames;
    } else {
        // start[n_clips + 1], then frame0[n_clips + 1]
        w.tables.resize(2 * ((size_t)n_clips + 1));
        long long* start = w.tables.data(), *frame0 = start + n_clips + 1;
        start[0] = frame0[0] = 0;
        for (int c = 0; c < n_clips; c++) { start[c + 1] = start[c] + clips.lens[c]; frame0[c + 1] = frame0[c] + flac_frames(clips.lens[c]); }
        w.total_frames = frame0[n_clips];
        w.start = (const long long*)d_block;
        w.frame0 = w.start + n_clips + 1;
    }
    carve(w, (char*)d_block + tables_bytes(clips), (size_t)w.total_frames);
    return w;
}

void launch_flac(const int16_t* pcm, const double* factor, const FlacWork& w, uint8_t* out, size_t out_cap, unsigned long long* offsets,
                 hipStream_t s) {
    // (a pageable source is staged before hipMemcpyAsync returns, so the host tables need not outlive the call)
    if (!w.tables.empty()) (void)hipMemcpyAsync((void*)w.start, w.tables.data(), w.tables.size() * 8, hipMemcpyHostToDevice, s);
    FlacGeom g;
    g.c.n_clips = w.n_clips; g.c.n = w.n; g.c.start = w.start;
    g.frames = w.frames; g.frame0 = w.frame0;
    const dim3 grid = w.frame0 ? dim3((unsigned)w.total_frames) : dim3((unsigned)w.frames, (unsigned)w.n_clips);
    if (w.lpc_order > 0)
        hipLaunchKernelGGL(k_flac_analyse<true>, grid, dim3(AN_THREADS_LPC), 0, s, pcm, factor, g, w.lpc_order, w.rec, w.lpc);
    else
        hipLaunchKernelGGL(k_flac_analyse<false>, grid, dim3(AN_THREADS), 0, s, pcm, factor, g, 0, w.rec, (FlacLpc*)nullptr);
    hipLaunchKernelGGL(k_flac_layout_clip, dim3(w.n_clips), dim3(256), 0, s, g, w.seek_interval, (const FlacRecord*)w.rec, w.rel, w.clip_bytes,
                       w.fmin, w.fmax);
    hipLaunchKernelGGL(k_flac_layout_batch, dim3(1), dim3(256), 0, s, w.n_clips, (const u64*)w.clip_bytes, offsets);
    hipLaunchKernelGGL(k_flac_headers, dim3(w.n_clips), dim3(256), 0, s, g, w.rate, w.seek_interval, (const u64*)offsets, (const u64*)w.rel,
                       (const uint32_t*)w.fmin, (const uint32_t*)w.fmax, out, (u64)out_cap);
    if (w.lpc_order > 0)
        hipLaunchKernelGGL(k_flac_emit<true>, grid, dim3(EM_THREADS), 0, s, pcm, factor, g, w.rate, w.seek_interval, (const FlacRecord*)w.rec,
                           (const FlacLpc*)w.lpc, (const u64*)w.rel, (const u64*)offsets, out, (u64)out_cap);
    else
        hipLaunchKernelGGL(k_flac_emit<false>, grid, dim3(EM_THREADS), 0, s, pcm, factor, g, w.rate, w.seek_interval, (const FlacRecord*)w.rec,
                           (const FlacLpc*)nullptr, (const u64*)w.rel, (const u64*)offsets, out, (u64)out_cap);
}

}  // namespace bnhip
