// EBU R 128 clip loudness (loudness.hip, api_loudness.cpp bnhip_loudness_*): K-weighted gated integrated loudness, 4x oversampled
// true peak, the gain plan and the saturating int16 gain of a batch of equally long mono clips, or of a ragged burst of clips of any
// lengths (ragged.h), the spec of DESIGN.md §9 in fp64.
//
// The order in which a sub-block's squares are added depends on the split q (q partial sums, each left to right, added in
// order), and on nothing else of the call.  So two calls give a clip the same bits exactly when they use the same q: a ragged
// call and the uniform calls of its clips one by one agree bit for bit when both splits are equal (always, while both calls stay
// under LOUD_MAX_LANES / 8 sub-blocks and 8 divides S), and to rounding otherwise.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/bnhip.h"
#include "ragged.h"

namespace bnhip {

constexpr int LOUD_MIN_RATE = 8000;                      // minSampleRate (audionorm/meter.go:21)
constexpr int LOUD_TP_PHASES = 4, LOUD_TP_TAPS = 32;     // oversample, tapsPerPhase (truepeak.go:13-14)
constexpr int LOUD_TP_DRAIN = LOUD_TP_TAPS / 2;          // positions past the clip's end (truepeak.go:151-167)
constexpr int LOUD_TP_TILE = 1024;                       // true-peak positions per block
// The table of one rate, what the kernels read: [0..4] stage 1 (b0 b1 b2 a1 a2), [5..9] stage 2, [10..25] the 4 x 4 homogeneous
// map M of the cascade over one segment (row major, state order u1 u2 y1 y2), [26..153] the true-peak taps c[t][p].
constexpr int LOUD_TAB_M = 10, LOUD_TAB_TP = 26, LOUD_TABLE = LOUD_TAB_TP + LOUD_TP_PHASES * LOUD_TP_TAPS;

// S = floor(0.1 rate + 0.5): Go's math.Round of subBlockSamples (meter.go:91-93)
int loudness_sub_block(int rate);
// Segments per sub-block: a sub-block is cut into q equal segments, one lane each, so that a small batch still fills the device
// (the recurrence is latency bound: a lane's time is its segment's length).  The largest of 8, 4, 2, 1 that divides S and keeps
// the call under LOUD_MAX_LANES lanes.
constexpr long long LOUD_MAX_LANES = 1 << 18;
// The rule works on a call's total, the sum of its clips' len / S sub-blocks: q * sub_blocks <= LOUD_MAX_LANES.  So a ragged burst of
// equal lengths has the uniform batch's split.
int loudness_split(const Clips& clips, int S);
// the table above for segments of seg_len samples, computed on the host (libm tan / pow / sin; float32-rounded coefficients
// widened to double)
std::vector<double> loudness_table(int rate, int seg_len);

// What the tail decides with: measure != 0 leaves the plan fields neutral.
struct LoudPlan {
    double target, ceiling, max_gain;       // T, C, |max_gain_db|
    double gate_abs, gate_rel;              // A, R
    int gate_fallback, measure;
};

// The geometry of one call and its scratch; every array lives in one caller-supplied device block.
struct LoudWork {
    int n_clips = 0, n = 0, S = 0, Ns = 0, tp_blocks = 0;       // (n, Ns, tp_blocks: per clip, uniform only)
    int max_n = 0;                          // the longest clip
    int q = 1, Sq = 0;                      // segments per sub-block, samples per segment
    long long G = 0, tiles = 0;             // segments (q per sub-block) and true-peak tiles of all clips
    // ragged only: the host's prefix tables start | sub0 | tile0, [n_clips + 1] each, which launch_loudness copies to the head of
    // the block, where the three pointers point; NULL for a uniform batch
    std::vector<long long> tables;
    const long long *start = nullptr, *sub0 = nullptr, *tile0 = nullptr;
    double *zs = nullptr, *st = nullptr;    // [G][4] zero-state end states, true start states
    double* Ep = nullptr;                   // [G] per-segment sums of y^2 of the running measurement
    double *E1 = nullptr, *E2 = nullptr;    // [G / q] sub-block energies of the clips, of the lifted clips; clip after clip
    double* tp = nullptr;                   // [tiles] per-tile max |.|, clip after clip
    double* pre = nullptr;                  // [n_clips] pre-gain factor of the running measurement
    int* act = nullptr;                     // [n_clips] clip takes part in the running measurement
};
// A ragged burst's block begins with its prefix tables; a clip shorter than S has no sub-block.
size_t loudness_workspace_bytes(const Clips& clips, int S);
LoudWork loudness_work(const Clips& clips, int S, void* d_block);

// pcm int16 [n_clips][n], or the packed clips of a ragged work; d_table: loudness_table on the device; out: bnhip_loudness [n_clips] on the device; out_pcm nullable.
// Enqueues: a ragged work's table copy, init, the measurement (pass A, scan, pass B, true peak), the tail, with plan.gate_fallback the measurement of the
// lifted clips and their tail, and with out_pcm the gain.  Nothing is synchronised.
void launch_loudness(const int16_t* pcm, const LoudWork& w, const double* d_table, const LoudPlan& plan, bnhip_loudness* out,
                     int16_t* out_pcm, hipStream_t s);


// What an entry of another unit needs of api_loudness.cpp (the fused loudness + FLAC entries of api_flac.cpp, the chain of
// api_denoise.cpp):
// the argument checks of the normalise entries, clips_check (api_oneshot.h) included, answered before any device is touched; -> 0
// or a negative BNHIP_E_*
int loudness_args_check(const Clips& clips, int rate, double target, double ceiling, double max_gain);
// the device (already made current) has its table looked up or uploaded, and the normalise kernels are enqueued on s
int loudness_enqueue(const char* what, int device, const int16_t* d_pcm, const Clips& clips, int rate, double target, double ceiling,
                     double max_gain, int gate_fallback, bnhip_loudness* d_out, int16_t* d_out_pcm, void* d_workspace, hipStream_t s);

}  // namespace bnhip
