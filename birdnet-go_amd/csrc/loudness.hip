// EBU R 128 loudness of a batch of clips, parallel in time (DESIGN.md §9 "clip loudness").
//
// The K-weighting cascade is a linear recurrence with the 4-vector state (u1, u2, y1, y2) once the input is known, so a clip
// is cut into equal segments, q per sub-block (loudness_split), and every segment is one lane's work:
//   pass A   each segment from zero state, with its true x[-1], x[-2]            -> the zero-state end state zs[k]
//   scan     start[0] = 0, start[k+1] = zs[k] + M start[k], M the homogeneous map over one segment (one lane per clip)
//   pass B   each segment again from start[k], summing y^2                        -> Ep[k]; E = the q sums of a sub-block, in order
// The true peak has no recurrence: every position is 4 x 32 products over a span staged in LDS.  One wave per clip then
// gates, plans and flags.  A clip under the absolute gate is measured a second time with its lift applied on the fly.
// All arithmetic is fp64, every operation rounded (no fused multiply-add), vector stores only.
// Geometry (ragged.h): the segments, sub-blocks and true-peak tiles of all clips are flat lists, clip after clip.  A uniform batch
// indexes them by arithmetic; a ragged burst finds a unit's clip by a search over the prefix tables sub0 / tile0 [n_clips + 1], and
// every per-clip count (sub-blocks, tiles, samples) comes from the tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "loudness.h"
#include "pcmgain.h"
#include "ragged.h"

#pragma clang fp contract(off)

namespace bnhip {

namespace {

constexpr int KW_LANES = 64;               // segments per block of the K-weighting passes: one wave
constexpr int KW_CHUNK = 64;               // samples of every segment staged per round
constexpr int KW_ROW = KW_CHUNK + 2;       // int16 row stride in LDS: 33 dwords, so 64 lanes reading one column hit 64 banks
constexpr int TP_THREADS = 256, TP_R = LOUD_TP_TILE / TP_THREADS;      // positions per thread
constexpr int TP_SPAN = LOUD_TP_TILE + LOUD_TP_TAPS - 1;

// one sample of the measured signal: s / 32768, or the saturated gain of pcmgain.h first
__device__ __forceinline__ double loud_sample(int16_t s, double f) { return pcm_gained(s, f) * (1.0 / 32768.0); }

struct KwState { double x1, x2, u1, u2, y1, y2; };

// one step of the cascade, left to right, every operation rounded (meter.go:52-57); host and device share it
__host__ __device__ __forceinline__ double kw_step(const double* __restrict__ c, KwState& s, double x) {
#pragma clang fp contract(off)
    const double u = c[0] * x + c[1] * s.x1 + c[2] * s.x2 - c[3] * s.u1 - c[4] * s.u2;
    const double y = c[5] * u + c[6] * s.u1 + c[7] * s.u2 - c[8] * s.y1 - c[9] * s.y2;
    s.x2 = s.x1; s.x1 = x;
    s.u2 = s.u1; s.u1 = u;
    s.y2 = s.y1; s.y1 = y;
    return y;
}

// A call's units: sub0 / tile0 NULL for a uniform batch of Ns sub-blocks and tp_blocks tiles per clip, else the prefix tables.
struct LoudGeom {
    ClipGeom c;
    int Ns = 0, tp_blocks = 0;
    const long long *sub0 = nullptr, *tile0 = nullptr;
};
// a clip's sub-blocks and the first of them in E / (times q) in zs, st, Ep; its tiles and the first of them in partial
__device__ __forceinline__ int clip_subs(const LoudGeom& g, int clip) { return g.sub0 ? (int)(g.sub0[clip + 1] - g.sub0[clip]) : g.Ns; }
__device__ __forceinline__ long long clip_sub0(const LoudGeom& g, int clip) { return g.sub0 ? g.sub0[clip] : (long long)clip * g.Ns; }
__device__ __forceinline__ int clip_tiles(const LoudGeom& g, int clip) { return g.tile0 ? (int)(g.tile0[clip + 1] - g.tile0[clip]) : g.tp_blocks; }
__device__ __forceinline__ long long clip_tile0(const LoudGeom& g, int clip) { return g.tile0 ? g.tile0[clip] : (long long)clip * g.tp_blocks; }

__global__ __launch_bounds__(256) void k_loud_init(int n_clips, double* __restrict__ pre, int* __restrict__ act) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_clips) { pre[i] = 1.0; act[i] = 1; }
}

// PASS_B == 0: out = zs [G][4]; PASS_B == 1: start = [G][4], out = Ep [G].  (S here: samples per segment; a clip has q segments
// per sub-block.)  Lane l of block b owns segment g = 64 b + l: of a uniform batch clip g / (q Ns), segment g % (q Ns) of it; of a
// ragged burst the clip that owns sub-block g / q, and segment g - q sub0[clip] of it.  Rounds of KW_CHUNK samples: the wave
// copies row r (segment r's next samples) with one coalesced load per row into a padded LDS tile, then every lane walks its own row.
template <int PASS_B>
__global__ __launch_bounds__(KW_LANES) void k_loud_kweight(const int16_t* __restrict__ pcm, LoudGeom geo, int S, int q, long long G,
                                                           const double* __restrict__ tab, const double* __restrict__ pre,
                                                           const int* __restrict__ act, const double* __restrict__ start,
                                                           double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ int16_t tile[KW_LANES * KW_ROW];
    __shared__ long long base[KW_LANES];
    const int lane = threadIdx.x;
    const long long g = (long long)blockIdx.x * KW_LANES + lane;
    int clip = 0, k = 0;
    if (g < G) {
        if (geo.sub0) { clip = ragged_clip(geo.sub0, geo.c.n_clips, g / q); k = (int)(g - geo.sub0[clip] * q); }
        else { const int Nq = geo.Ns * q; clip = (int)(g / Nq); k = (int)(g % Nq); }
    }
    const bool on = g < G && act[clip] != 0;
    if (!__syncthreads_or(on ? 1 : 0)) return;                 // (a block of lifted-run segments with no lifted clip)
    const long long off = clip_start(geo.c, clip) + (long long)k * S;
    base[lane] = on ? off : -1;
    const double f = on ? pre[clip] : 1.0;
    double c[10];
#pragma unroll
    for (int i = 0; i < 10; i++) c[i] = tab[i];
    KwState s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (on && k > 0) { s.x1 = loud_sample(pcm[off - 1], f); s.x2 = loud_sample(pcm[off - 2], f); }   // (S >= 100 > 2)
    if (PASS_B && on) { s.u1 = start[g * 4 + 0]; s.u2 = start[g * 4 + 1]; s.y1 = start[g * 4 + 2]; s.y2 = start[g * 4 + 3]; }
    double e = 0.0;
    for (int c0 = 0; c0 < S; c0 += KW_CHUNK) {
        __syncthreads();
        const bool col = c0 + lane < S;
#pragma unroll 8
        for (int r = 0; r < KW_LANES; r++) {
            const long long b = base[r];
            tile[r * KW_ROW + lane] = (b >= 0 && col) ? pcm[b + c0 + lane] : (int16_t)0;       // b + c0 + lane < the clip's start + (k + 1) S <= its end
        }
        __syncthreads();
        const int m = S - c0 < KW_CHUNK ? S - c0 : KW_CHUNK;
        for (int j = 0; j < m; j++) {
            const double y = kw_step(c, s, loud_sample(tile[lane * KW_ROW + j], f));
            if (PASS_B) e = e + y * y;
        }
    }
    if (!on) return;
    if (PASS_B) out[g] = e;
    else { out[g * 4 + 0] = s.u1; out[g * 4 + 1] = s.u2; out[g * 4 + 2] = s.y1; out[g * 4 + 3] = s.y2; }
}

// start[clip][0] = 0; start[k + 1] = zs[k] + M start[k], the row sums left to right.  One lane per clip.
__global__ __launch_bounds__(64) void k_loud_scan(LoudGeom geo, int q, const double* __restrict__ tab, const int* __restrict__ act,
                                                  const double* __restrict__ zs, double* __restrict__ st) {
#pragma clang fp contract(off)
    const int clip = blockIdx.x * 64 + threadIdx.x;
    if (clip >= geo.c.n_clips || !act[clip]) return;
    double M[16];
#pragma unroll
    for (int i = 0; i < 16; i++) M[i] = tab[LOUD_TAB_M + i];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    const long long g0 = clip_sub0(geo, clip) * q;
    const int Nq = clip_subs(geo, clip) * q;
    for (int k = 0; k < Nq; k++) {
        double* o = st + (g0 + k) * 4;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
        const double* z = zs + (g0 + k) * 4;
        double w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) w[i] = z[i] + (M[i * 4 + 0] * v[0] + M[i * 4 + 1] * v[1] + M[i * 4 + 2] * v[2] + M[i * 4 + 3] * v[3]);
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = w[i];
    }
}

// Block (bx, clip) of a uniform batch, the clip's tile bx = blockIdx.x - tile0[clip] of a ragged burst: positions
// k = 1024 bx .. +1023 of P = max(|x[k]|, |sum_t c[p][t] x[k - t]|), k < n + 16, each sum from 0.0 with the oldest sample first
// (t = 31 .. 0).  A thread keeps its 4 positions' 16 sums in registers.
__global__ __launch_bounds__(TP_THREADS) void k_loud_truepeak(const int16_t* __restrict__ pcm, LoudGeom geo,
                                                              const double* __restrict__ tab, const double* __restrict__ pre,
                                                              const int* __restrict__ act, double* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double xs[TP_SPAN];
    __shared__ double cs[LOUD_TP_PHASES * LOUD_TP_TAPS];
    __shared__ double red[TP_THREADS / 64];
    const int tid = threadIdx.x;
    const int clip = geo.tile0 ? ragged_clip(geo.tile0, geo.c.n_clips, (long long)blockIdx.x) : (int)blockIdx.y;
    if (!act[clip]) return;
    const double f = pre[clip];
    const long long t0 = clip_tile0(geo, clip);
    const int bx = geo.tile0 ? (int)((long long)blockIdx.x - t0) : (int)blockIdx.x;
    const int n = clip_len(geo.c, clip);
    const long long k_base = (long long)bx * LOUD_TP_TILE;
    const int16_t* x = pcm + clip_start(geo.c, clip);
    for (int i = tid; i < TP_SPAN; i += TP_THREADS) {
        const long long idx = k_base - (LOUD_TP_TAPS - 1) + i;
        xs[i] = (idx >= 0 && idx < n) ? loud_sample(x[idx], f) : 0.0;
    }
    if (tid < LOUD_TP_PHASES * LOUD_TP_TAPS) cs[tid] = tab[LOUD_TAB_TP + tid];
    __syncthreads();
    const int k0 = tid * TP_R;                                 // xs[k0 + i] = x[k_base + k0 - 31 + i]
    double acc[TP_R][LOUD_TP_PHASES];
#pragma unroll
    for (int r = 0; r < TP_R; r++)
#pragma unroll
        for (int p = 0; p < LOUD_TP_PHASES; p++) acc[r][p] = 0.0;
    // taps in TP_G groups, oldest first; a group's TP_R + 7 samples and 32 taps are re-read from LDS, which keeps the registers
    // at a few waves per SIMD (all 128 taps held at once take the whole file)
    constexpr int TP_GT = 8, TP_G = LOUD_TP_TAPS / TP_GT;
#pragma unroll 1
    for (int q = TP_G - 1; q >= 0; q--) {
        double xg[TP_R + TP_GT - 1];                           // xg[i] = x[k_base + k0 - (8 q + 7) + i]
#pragma unroll
        for (int i = 0; i < TP_R + TP_GT - 1; i++) xg[i] = xs[k0 + LOUD_TP_TAPS - TP_GT * (q + 1) + i];
#pragma unroll
        for (int tt = TP_GT - 1; tt >= 0; tt--) {
            double ct[LOUD_TP_PHASES];
#pragma unroll
            for (int p = 0; p < LOUD_TP_PHASES; p++) ct[p] = cs[(TP_GT * q + tt) * LOUD_TP_PHASES + p];
#pragma unroll
            for (int r = 0; r < TP_R; r++)
#pragma unroll
                for (int p = 0; p < LOUD_TP_PHASES; p++) acc[r][p] = acc[r][p] + ct[p] * xg[r + TP_GT - 1 - tt];
        }
    }
    double xr[TP_R];                                            // the positions' own samples
#pragma unroll
    for (int r = 0; r < TP_R; r++) xr[r] = xs[k0 + LOUD_TP_TAPS - 1 + r];
    double m = 0.0;
#pragma unroll
    for (int r = 0; r < TP_R; r++) {
        if (k_base + k0 + r >= (long long)n + LOUD_TP_DRAIN) continue;
        m = fmax(m, fabs(xr[r]));                // (0 past the clip's end)
#pragma unroll
        for (int p = 0; p < LOUD_TP_PHASES; p++) m = fmax(m, fabs(acc[r][p]));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int i = 1; i < TP_THREADS / 64; i++) m = fmax(m, red[i]);
        partial[t0 + bx] = m;
    }
}

// PlanGain (audionorm.go:181-202): -> the gain; L = -inf plans nothing
__device__ double loud_plan_gain(double L, double dbtp, double T, double C, double* target_gain, bool* limited) {
#pragma clang fp contract(off)
    *target_gain = 0.0; *limited = false;
    if (L == -HUGE_VAL) return 0.0;
    double gain = T - L;
    *target_gain = gain;
    if (dbtp != -HUGE_VAL) {
        const double head = C - dbtp;
        if (gain > head) { gain = head; *limited = true; }
    }
    return gain;
}

// FactorFromDB (pcmgain.go:27-32)
__device__ double loud_factor(double gain_db) { return gain_db == 0.0 ? 1.0 : pow(10.0, gain_db / 20.0); }

// One wave per clip.  run 1: the clip's measurement, then the plan - or, for a clip the gate fallback lifts, its lift, pre-gain
// and active flag, and the plan waits for run 2.  run 2 (lifted clips only): the lifted clip's measurement refines the lift.
__global__ __launch_bounds__(64) void k_loud_tail(int run, int S, LoudGeom geo, int q, const double* __restrict__ Ep,
                                                  double* __restrict__ E, const double* __restrict__ partial, LoudPlan pl, double* __restrict__ pre,
                                                  int* __restrict__ act, bnhip_loudness* __restrict__ out) {
#pragma clang fp contract(off)
    const int clip = blockIdx.x, lane = threadIdx.x;
    if (run == 2 && !act[clip]) return;
    const int Ns = clip_subs(geo, clip), tp_blocks = clip_tiles(geo, clip);
    const long long s0 = clip_sub0(geo, clip), t0 = clip_tile0(geo, clip);
    double P = 0.0;
    for (int i = lane; i < tp_blocks; i += 64) P = fmax(P, partial[t0 + i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) P = fmax(P, __shfl_xor(P, d));
    // E[k]: the sub-block's q segment sums, added in order
    double* e = E + s0;
    for (int k = lane; k < Ns; k += 64) {
        const double* p = Ep + (s0 + k) * q;
        double a = p[0];
        for (int i = 1; i < q; i++) a = a + p[i];
        e[k] = a;
    }
    __threadfence_block();
    __syncthreads();
    if (lane != 0) return;
    // both gates, in block order (meter.go:318-352)
    const int Nb = Ns - 3;
    const double den = 4.0 * (double)S;
    double L = -HUGE_VAL;
    double sum = 0.0; int cnt = 0;
    for (int j = 0; j < Nb; j++) {
        const double z = (e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / den;
        if (z > pl.gate_abs) { sum = sum + z; cnt++; }
    }
    if (cnt > 0) {
        const double rel = (sum / (double)cnt) * pl.gate_rel;
        double sum2 = 0.0; int cnt2 = 0;
        for (int j = 0; j < Nb; j++) {
            const double z = (e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / den;
            if (z > pl.gate_abs && z > rel) { sum2 = sum2 + z; cnt2++; }
        }
        if (cnt2 > 0) L = -0.691 + 10.0 * log10(sum2 / (double)cnt2);
    }
    const double dbtp = P > 0.0 ? 20.0 * log10(P) : -HUGE_VAL;

    bnhip_loudness o;
    o.reserved = 0;
    double planned, lift = 0.0, Lm = L;
    bool limited = false;
    int flags = 0;
    if (run == 1) {
        o.integrated_lufs = L; o.true_peak_dbtp = dbtp; o.true_peak = P;
        if (pl.measure) {
            o.target_gain_db = 0.0; o.lift_db = 0.0; o.planned_gain_db = 0.0; o.gain_db = 0.0; o.factor = 1.0; o.output_lufs = L;
            o.flags = 0;
            out[clip] = o;
            return;
        }
        if (pl.gate_fallback && L == -HUGE_VAL && P > 0.0) {       // gateFallbackGainDB (actions_database.go:1353-1360)
            lift = fmin(pl.ceiling - dbtp, pl.target + 70.0);
            o.target_gain_db = 0.0; o.lift_db = lift; o.planned_gain_db = lift; o.gain_db = 0.0; o.factor = 1.0;
            o.output_lufs = -HUGE_VAL; o.flags = BNHIP_LOUDNESS_GATE_LIFTED;
            out[clip] = o;
            pre[clip] = loud_factor(lift); act[clip] = 1;
            return;
        }
        act[clip] = 0;
        planned = loud_plan_gain(L, dbtp, pl.target, pl.ceiling, &o.target_gain_db, &limited);
    } else {                                                       // refineLiftedGainDB (:1378-1384)
        o = out[clip];
        lift = o.lift_db;
        flags = BNHIP_LOUDNESS_GATE_LIFTED;
        planned = lift + loud_plan_gain(L, dbtp, pl.target, pl.ceiling, &o.target_gain_db, &limited);
        if (L == -HUGE_VAL) planned = lift;
    }
    if (limited) flags |= BNHIP_LOUDNESS_PEAK_LIMITED;
    double gain = planned;                                         // ClampGainDB (audionorm.go:217-229)
    if (gain > pl.max_gain) { gain = pl.max_gain; flags |= BNHIP_LOUDNESS_CLAMPED; }
    else if (gain < -pl.max_gain) { gain = -pl.max_gain; flags |= BNHIP_LOUDNESS_CLAMPED; }
    o.lift_db = lift; o.planned_gain_db = planned; o.gain_db = gain; o.factor = loud_factor(gain);
    o.output_lufs = Lm == -HUGE_VAL ? -HUGE_VAL : Lm + (gain - lift);
    o.flags = flags;
    out[clip] = o;
}

// ApplyInt16 (pcmgain.go:52-63) with the clip's reported factor; factor 1 copies
__global__ __launch_bounds__(256) void k_loud_gain(const int16_t* __restrict__ pcm, ClipGeom geo, const bnhip_loudness* __restrict__ res,
                                                   int16_t* __restrict__ out) {
    const int clip = blockIdx.y;
    const double f = res[clip].factor;
    const long long i0 = clip_start(geo, clip);
    const int n = clip_len(geo, clip);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        out[i0 + i] = (int16_t)pcm_gained(pcm[i0 + i], f);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

int loudness_sub_block(int rate) { return (int)std::floor(0.1 * (double)rate + 0.5); }

int loudness_split(const Clips& clips, int S) {
    const long long sub_blocks = (long long)clips.sum([&](int n) { return n / S; });
    for (int q = 8; q > 1; q >>= 1)
        if (S % q == 0 && sub_blocks * q <= LOUD_MAX_LANES) return q;
    return 1;
}

std::vector<double> loudness_table(int rate, int seg_len) {
    std::vector<double> t((size_t)LOUD_TABLE);
    const double fs = (double)rate, pi = 3.14159265358979323846;
    {   // kHighShelf (kweight.go:39-52): the BS.1770-4 analog prototype through the bilinear transform
        const double f0 = 1681.974450955533, Q = 0.7071752369554196, GdB = 3.999843853973347, VbEx = 0.4996667741545416;
        const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, GdB / 20.0), Vb = std::pow(Vh, VbEx), K2 = K * K;
        const double a0 = 1.0 + K / Q + K2;
        t[0] = (Vh + Vb * K / Q + K2) / a0;
        t[1] = 2.0 * (K2 - Vh) / a0;
        t[2] = (Vh - Vb * K / Q + K2) / a0;
        t[3] = 2.0 * (K2 - 1.0) / a0;
        t[4] = (1.0 - K / Q + K2) / a0;
    }
    {   // kHighPass (:57-68)
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs), K2 = K * K, a0 = 1.0 + K / Q + K2;
        t[5] = 1.0; t[6] = -2.0; t[7] = 1.0;
        t[8] = 2.0 * (K2 - 1.0) / a0;
        t[9] = (1.0 - K / Q + K2) / a0;
    }
    for (int i = 0; i < 10; i++) t[i] = (double)(float)t[i];               // newBiquadState (meter.go:45-50)
    // M: the cascade with no input, from each unit state, over one segment
    const int S = seg_len;
    for (int j = 0; j < 4; j++) {
        KwState s{0.0, 0.0, j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0, j == 3 ? 1.0 : 0.0};
        for (int i = 0; i < S; i++) kw_step(t.data(), s, 0.0);
        t[LOUD_TAB_M + 0 * 4 + j] = s.u1; t[LOUD_TAB_M + 1 * 4 + j] = s.u2;
        t[LOUD_TAB_M + 2 * 4 + j] = s.y1; t[LOUD_TAB_M + 3 * 4 + j] = s.y2;
    }
    // buildTruePeakKernel (truepeak.go:55-110): Kaiser(beta 9) windowed sinc, 128 taps, each phase divided by its sum
    auto i0 = [](double x) {
        double sum = 1.0, term = 1.0;
        const double half = x / 2.0;
        for (int k = 1; k < 40; k++) {
            term *= (half / (double)k) * (half / (double)k);
            sum += term;
            if (term < 1e-15 * sum) break;
        }
        return sum;
    };
    constexpr int PL = LOUD_TP_PHASES * LOUD_TP_TAPS;
    double proto[PL];
    const double center = (double)(PL - 1) / 2.0;
    for (int i = 0; i < PL; i++) {
        const double x = ((double)i - center) / (double)LOUD_TP_PHASES, px = pi * x;
        const double r = 2.0 * (double)i / (double)(PL - 1) - 1.0;
        proto[i] = (x == 0.0 ? 1.0 : std::sin(px) / px) * (i0(9.0 * std::sqrt(1.0 - r * r)) / i0(9.0));
    }
    for (int p = 0; p < LOUD_TP_PHASES; p++) {
        double sum = 0.0;
        for (int k = 0; k < LOUD_TP_TAPS; k++) sum += proto[p + LOUD_TP_PHASES * k];
        for (int k = 0; k < LOUD_TP_TAPS; k++) {
            double c = proto[p + LOUD_TP_PHASES * k];
            if (sum != 0.0) c /= sum;
            t[LOUD_TAB_TP + k * LOUD_TP_PHASES + p] = (double)(float)c;     // tpKernelRev (truepeak.go:35-43)
        }
    }
    return t;
}

namespace {

long long tp_tiles(int n) { return ((long long)n + LOUD_TP_DRAIN + LOUD_TP_TILE - 1) / LOUD_TP_TILE; }

// the arrays of Gs sub-blocks cut q ways and T tiles of n_clips clips, after `tables` bytes of prefix tables
size_t work_bytes(size_t tables, size_t n_clips, size_t Gs, int q, size_t T) {
    const size_t G = Gs * (size_t)q;
    return tables + 2 * align256(G * 32) + align256(G * 8) + 2 * align256(Gs * 8) + align256(T * 8) + align256(n_clips * 8) + align256(n_clips * 4);
}
void carve(LoudWork& w, char* p, size_t Gs, size_t T) {
    w.zs = (double*)p; p += align256((size_t)w.G * 32);
    w.st = (double*)p; p += align256((size_t)w.G * 32);
    w.Ep = (double*)p; p += align256((size_t)w.G * 8);
    w.E1 = (double*)p; p += align256(Gs * 8);
    w.E2 = (double*)p; p += align256(Gs * 8);
    w.tp = (double*)p; p += align256(T * 8);
    w.pre = (double*)p; p += align256((size_t)w.n_clips * 8);
    w.act = (int*)p;
}
size_t tables_bytes(const Clips& clips) { return clips.lens ? align256(3 * ((size_t)clips.n_clips + 1) * 8) : 0; }

}  // namespace

size_t loudness_workspace_bytes(const Clips& clips, int S) {
    return work_bytes(tables_bytes(clips), (size_t)clips.n_clips, clips.sum([&](int n) { return n / S; }), loudness_split(clips, S),
                      clips.sum(tp_tiles));
}

LoudWork loudness_work(const Clips& clips, int S, void* d_block) {
    const int n_clips = clips.n_clips;
    LoudWork w;
    w.n_clips = n_clips; w.n = clips.n; w.S = S;
    w.q = loudness_split(clips, S); w.Sq = S / w.q;
    long long sub_blocks;
    if (!clips.lens) {
        w.max_n = clips.n; w.Ns = clips.n / S;
        w.tp_blocks = (int)tp_tiles(clips.n);
        w.tiles = (long long)n_clips * w.tp_blocks;
        sub_blocks = (long long)n_clips * w.Ns;
    } else {
        // start[n_clips + 1], then sub0[n_clips + 1], then tile0[n_clips + 1]
        w.tables.resize(3 * ((size_t)n_clips + 1));
        long long* start = w.tables.data(), *sub0 = start + n_clips + 1, *tile0 = sub0 + n_clips + 1;
        start[0] = sub0[0] = tile0[0] = 0;
        for (int c = 0; c < n_clips; c++) {
            const int len = clips.lens[c];
            start[c + 1] = start[c] + len; sub0[c + 1] = sub0[c] + len / S; tile0[c + 1] = tile0[c] + tp_tiles(len);
            w.max_n = std::max(w.max_n, len);
        }
        w.tiles = tile0[n_clips];
        sub_blocks = sub0[n_clips];
        w.start = (const long long*)d_block;
        w.sub0 = w.start + n_clips + 1; w.tile0 = w.sub0 + n_clips + 1;
    }
    w.G = sub_blocks * w.q;
    carve(w, (char*)d_block + tables_bytes(clips), (size_t)sub_blocks, (size_t)w.tiles);
    return w;
}

void launch_loudness(const int16_t* pcm, const LoudWork& w, const double* d_table, const LoudPlan& plan, bnhip_loudness* out,
                     int16_t* out_pcm, hipStream_t s) {
    // (a pageable source is staged before hipMemcpyAsync returns, so the host tables need not outlive the call)
    if (!w.tables.empty()) (void)hipMemcpyAsync((void*)w.start, w.tables.data(), w.tables.size() * 8, hipMemcpyHostToDevice, s);
    LoudGeom g;
    g.c.n_clips = w.n_clips; g.c.n = w.n; g.c.start = w.start;
    g.Ns = w.Ns; g.tp_blocks = w.tp_blocks; g.sub0 = w.sub0; g.tile0 = w.tile0;
    hipLaunchKernelGGL(k_loud_init, dim3((w.n_clips + 255) / 256), dim3(256), 0, s, w.n_clips, w.pre, w.act);
    const unsigned kw_blocks = (unsigned)((w.G + KW_LANES - 1) / KW_LANES);
    const dim3 tp_grid = w.tile0 ? dim3((unsigned)w.tiles) : dim3((unsigned)w.tp_blocks, (unsigned)w.n_clips);
    const int runs = !plan.measure && plan.gate_fallback ? 2 : 1;
    for (int run = 1; run <= runs; run++) {
        double* E = run == 1 ? w.E1 : w.E2;
        if (w.G > 0) {
            hipLaunchKernelGGL(k_loud_kweight<0>, dim3(kw_blocks), dim3(KW_LANES), 0, s, pcm, g, w.Sq, w.q, w.G, d_table, w.pre, w.act,
                               (const double*)nullptr, w.zs);
            hipLaunchKernelGGL(k_loud_scan, dim3((w.n_clips + 63) / 64), dim3(64), 0, s, g, w.q, d_table, w.act, w.zs, w.st);
            hipLaunchKernelGGL(k_loud_kweight<1>, dim3(kw_blocks), dim3(KW_LANES), 0, s, pcm, g, w.Sq, w.q, w.G, d_table, w.pre, w.act,
                               (const double*)w.st, w.Ep);
        }
        hipLaunchKernelGGL(k_loud_truepeak, tp_grid, dim3(TP_THREADS), 0, s, pcm, g, d_table, w.pre, w.act, w.tp);
        hipLaunchKernelGGL(k_loud_tail, dim3(w.n_clips), dim3(64), 0, s, run, w.S, g, w.q, w.Ep, E, w.tp, plan, w.pre, w.act, out);
    }
    if (out_pcm) {
        const unsigned gx = (unsigned)std::min<long long>(((long long)w.max_n + 255) / 256, 1024);
        hipLaunchKernelGGL(k_loud_gain, dim3(gx, w.n_clips), dim3(256), 0, s, pcm, g.c, out, out_pcm);
    }
}

}  // namespace bnhip
