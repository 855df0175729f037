// The capture bank (include/bnhip.h, "Capture bank"; capture_bank.hip, api_capture_bank.cpp): every source's recent audio as a ring of
// mono int16 on the device, written once per tick and cut into detection clips where it lies.  The bank's rings are one block of
// max_sources * capacity samples, ring s at sample s * capacity; capacity is a multiple of 1024 samples, so every ring starts at a
// 16-byte line and a line never straddles a ring's end.  The sample at position P of a source's clock lies at cell P mod capacity.
//
// Both kernels are copies with nothing to reuse: what they are built for is the width of the accesses and that no two lanes of a
// launch store to the same cell.  Plain loads and stores, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "clips.h"

namespace bnhip {

constexpr long long CAPTURE_ALIGN = 1024;        // samples a ring's capacity is rounded up to (capture.go:97: 2048 bytes)

// One run of a call's frames that is stored, and that lies in its ring without a wrap: samples src .. src + n of the call's packed
// frames go to cells dst .. dst + n of the bank's block (dst = source * capacity + position mod capacity).
struct CapPiece {
    long long src, dst, n;
};

// k_capture_write.  pcm: the call's stored samples packed back to back at `bits` (16, 24 or 32), pcm_samples of them; pieces:
// [n_pieces], n >= 1 each, no two of them sharing a cell; tile0: [n_pieces + 1] prefix of cut_tiles(dst, n), tile0[n_pieces] <=
// INT_MAX.  rings: the bank's block of ring_samples samples, 16-byte aligned.  A sample is stored as sample_pcm16(frame_sample<bits>)
// (pcm_sample.h): a 16-bit sample as itself.
void launch_capture_write(const void* pcm, long long pcm_samples, int bits, const CapPiece* pieces, const long long* tile0, int n_pieces,
                          long long n_tiles, int16_t* rings, long long ring_samples, hipStream_t s);

// k_ring_cut: the cut of clips.h out of the rings.  spans: [n_clips], `recording` the source (inside the bank), `start` the first
// cell's position in its ring (0 .. capacity - 1), length 1 .. capacity; ostart / tile0 / out as launch_cut_clips takes them.
// aligned: each lane builds its line from two 16-byte loads and four v_alignbyte_b32; else from eight element loads.
void launch_ring_cut(const int16_t* rings, long long capacity, int n_sources, const bnhip_clip_span* spans, const long long* ostart,
                     const long long* tile0, int n_clips, long long n_tiles, int16_t* out, bool aligned, hipStream_t s);

// The ring as a Cutter of clips.h.  The plan's spans carry positions on their sources' clocks (checked by the caller to lie in what
// the rings hold); the table that goes up carries ring cells instead.
struct RingCutter : Cutter {
    const int16_t* d_rings;
    long long capacity;
    int n_sources;
    mutable std::vector<bnhip_clip_span> cells;      // (alive until the call has synchronised)
    RingCutter(const int16_t* rings, long long cap, int n) : d_rings(rings), capacity(cap), n_sources(n) {}
    size_t table_bytes(const CutPlan& p) const override { return p.table_bytes(); }
    hipError_t enqueue(const CutPlan& p, void* d_tables, int16_t* d_out) const override;
};

// which form of k_ring_cut the library launches ("Capture bank": the measurement that chose it); the
// environment variable BNHIP_RING_CUT=aligned|element overrides it for that measurement
bool ring_cut_aligned();

}  // namespace bnhip

// The bank itself (api_capture_bank.cpp; api_level.cpp's fused write reaches it too).  The clocks are the host's.
struct bnhip_capture_bank {
    struct Source {
        int64_t written = 0;            // samples given since creation or reset
        int64_t floor = 0;              // no position below this one is readable
    };
    std::mutex mu;                      // calls on one bank are serialised
    int device = 0, max_sources = 0, rate = 0;
    int64_t capacity = 0;               // samples of one ring, a multiple of CAPTURE_ALIGN
    std::vector<Source> src;
    hipStream_t stream = nullptr;       // the writes' own
    int16_t* d_rings = nullptr;         // [max_sources][capacity]
    uint8_t* h_stage = nullptr; void* d_stage = nullptr; size_t stage_cap = 0;   // pieces | tile prefix | packed frames
    int64_t oldest(int s) const { return std::max<int64_t>({0, src[(size_t)s].written - capacity, src[(size_t)s].floor}); }
    ~bnhip_capture_bank() {             // (bank_free has drained the stream)
        if (stream) hipStreamDestroy(stream);
        for (void* p : {(void*)d_rings, d_stage}) if (p) hipFree(p);
        if (h_stage) hipHostFree(h_stage);
    }
};

namespace bnhip {

// What a write stores, worked out before any device call (under the bank's lock): the checks of bnhip_capture_bank_write, each
// source's total, and per frame what is stored of it (a source's samples of this call but the last `capacity` are not), cut where
// the ring wraps.  Sample q of a source's call lies at position written + q, in cell (written + q) mod capacity: the stored ones are
// at most `capacity` consecutive positions, so no two of them share a cell.
struct CapturePlan {
    struct Part { int frame; int64_t from, n; };          // samples from .. from + n of the frame are stored
    std::vector<int64_t> total;                           // [max_sources]: the call's samples of each source
    std::vector<int32_t> listed;                          // the call's sources, in the order they first appear
    std::vector<Part> parts;
    std::vector<CapPiece> pieces;
    std::vector<long long> tile0;                         // [pieces + 1]
    int64_t packed = 0;                                   // stored samples, all parts
};
// frame_at NULL: the parts are staged packed back to back in parts order (a piece's src counts from there); else frame f's sample 0
// is staged at sample frame_at[f] of the PCM and the frames are staged whole.  -> BNHIP_OK or BNHIP_E_INVALID
int capture_plan(const bnhip_capture_bank* b, int n_frames, const int32_t* sources, const int64_t* n_samples, const void* const* frames,
                 const int64_t* frame_at, CapturePlan* p);
// "a failed write" of bnhip.h: nothing the launch could have touched is readable again
void capture_write_failed(bnhip_capture_bank* b, const CapturePlan& p);
void capture_write_commit(bnhip_capture_bank* b, const CapturePlan& p);

}  // namespace bnhip
