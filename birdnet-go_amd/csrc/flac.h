// FLAC encoding of a batch of equally long mono int16 clips, or of a ragged burst of clips of any lengths, on the device (flac.hip,
// api_flac.cpp bnhip_flac_*): the project's own deterministic encoder of DESIGN.md §9 "FLAC", a valid RFC 9639 stream per clip.
// Every byte is pinned: integer arithmetic, and for the LPC candidates (lpc_order > 0) an fp64 recursion of stated operation order,
// each operation rounded once (-ffp-contract=off).  A clip's stream depends on its own samples, gain, rate, seek_interval and
// lpc_order alone: the ragged form (ragged.h) gives the bytes of the uniform form called per clip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/bnhip.h"
#include "ragged.h"

namespace bnhip {

constexpr int FLAC_BLOCK = 4096;                         // samples per frame; the last frame holds n mod 4096 if that is non-zero
constexpr int FLAC_MAX_ORDER = 4;                        // FIXED predictor orders 0..4
constexpr int FLAC_MAX_LPC_ORDER = 8;                    // LPC predictor orders 1..8 (lpc_order 0: none are tried)
constexpr int FLAC_LPC_PRECISION = 12;                   // bits of a quantised coefficient
constexpr int FLAC_LPC_MAX_SHIFT = 15;                   // the 5-bit shift field is signed: 0..15 here
constexpr int FLAC_MAX_PORDER = 5;                       // partition orders 0..5
constexpr int FLAC_MAX_K = 14;                           // Rice parameters 0..14 (4-bit field; 15 is the escape, never written)
constexpr int FLAC_MAX_RATE = 1048575;                   // STREAMINFO's 20 bits
constexpr int FLAC_STREAM_HEAD = 4 + 4 + 34;             // "fLaC", the block header, STREAMINFO
constexpr int FLAC_SEEK_POINT = 18;

enum { FLAC_CONSTANT = 0, FLAC_VERBATIM = 1, FLAC_FIXED = 2, FLAC_LPC = 3 };      // a candidate's family

// One frame's analysis: the winner of the candidate list.  bits: the subframe's; bytes: the whole frame's, CRC-16 included.
struct FlacRecord {
    uint8_t kind, order, porder, reserved;
    uint32_t bits, bytes;
    uint8_t k[1 << FLAC_MAX_PORDER];
    uint32_t reserved2;
};
static_assert(sizeof(FlacRecord) == 48, "FlacRecord layout");
// Beside the record of a frame analysed with lpc_order > 0: the winning LPC order's quantised coefficients (q[0] multiplies x[i - 1])
// and shift; zeros where another family won.
struct FlacLpc {
    int16_t q[FLAC_MAX_LPC_ORDER];
    int32_t shift;
};
static_assert(sizeof(FlacLpc) == 20, "FlacLpc layout");

// The geometry of one call and its scratch; every array lives in one caller-supplied device block.
struct FlacWork {
    int n_clips = 0, n = 0, rate = 0, seek_interval = 0;
    int lpc_order = 0;                       // 0: CONSTANT / FIXED / VERBATIM only; M in 1..8: LPC orders 1..M are candidates too
    int frames = 0;                          // per clip (uniform)
    long long total_frames = 0;              // of all clips
    // ragged only: the host's prefix tables start[n_clips + 1] | frame0[n_clips + 1], which launch_flac copies to the head of the
    // block, where `start` and `frame0` point; NULL for a uniform batch
    std::vector<long long> tables;
    const long long *start = nullptr, *frame0 = nullptr;
    FlacRecord* rec = nullptr;               // [total_frames], clip after clip
    unsigned long long* rel = nullptr;       // [total_frames] byte offset of the frame's header from its clip's first frame's header
    unsigned long long* clip_bytes = nullptr;  // [n_clips]
    uint32_t *fmin = nullptr, *fmax = nullptr;  // [n_clips] smallest / largest frame
    FlacLpc* lpc = nullptr;                  // [total_frames], only with lpc_order > 0
};
int flac_frames(int n);
int flac_seek_points(int n, int seek_interval);
// the VERBATIM bound: no stream of n samples is longer (n_clips such streams); of a call's clips, the sum of its clips' bounds
size_t flac_max_bytes(int n_clips, int n, int seek_interval);
size_t flac_max_bytes(const Clips& clips, int seek_interval);
// A ragged burst's block begins with its prefix tables; a uniform batch's has none, and with lpc_order 0 no side array either.
size_t flac_workspace_bytes(const Clips& clips, int lpc_order);
FlacWork flac_work(const Clips& clips, int rate, int seek_interval, void* d_block, int lpc_order);

// pcm int16 [n_clips][n], or the packed clips of a ragged work; factor [n_clips] nullable (the gain of pcmgain.h, applied as the samples are staged); out: the streams
// back to back, offsets uint64 [n_clips + 1].  Enqueues a ragged work's table copy, analyse, the two layout scans, the stream headers and emit; w.lpc_order picks
// the kernels' LPC forms (0: the forms without).  Nothing is synchronised; no kernel writes at or past out + out_cap.
void launch_flac(const int16_t* pcm, const double* factor, const FlacWork& w, uint8_t* out, size_t out_cap,
                 unsigned long long* offsets, hipStream_t s);

}  // namespace bnhip
