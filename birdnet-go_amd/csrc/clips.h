// Detection clips cut out of analysed recordings (clips.hip, api_clips.cpp): the spans of a call's events are copied out of the slot
// block of analyze.h - the recordings as the windows are framed from them - into mono int16 clips packed back to back, which is the
// layout the ragged clip entries take (ragged.h).  The clips are then normalised, encoded and rendered where they lie.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/bnhip.h"
#include "api_oneshot.h"

namespace bnhip {

// output samples of one block of k_cut_clips: 256 lanes of one 16-byte store each
constexpr int CUT_TILE = 2048;
// Clip c lands at sample ostart[c] of the output, which need not be a multiple of 8, while a block's lanes store at 16-byte lines
// of the output: the clip's tiles are counted from the line its first sample lies in.
inline long long cut_tiles(long long ostart, long long len) { return ((ostart & 7) + len + CUT_TILE - 1) / CUT_TILE; }

// k_cut_clips.  block: the slot block, its samples at `bits` (0: float32, the slots k_resample_slots writes); slot: [n_rec][2] as in
// WinView; spans: [n_clips], each of length >= 1 and inside its recording; ostart: [n_clips + 1] prefix of the lengths; tile0:
// [n_clips + 1] prefix of cut_tiles(ostart[c], length[c]), tile0[n_clips] <= INT_MAX.  out: 16-byte aligned, ostart[n_clips] samples.
// A sample is converted by sample_pcm16 (pcm_sample.h) from what k_frame_windows reads.
void launch_cut_clips(const void* block, int bits, const long long* slot, const bnhip_clip_span* spans, const long long* ostart,
                      const long long* tile0, int n_clips, long long n_tiles, int16_t* out, hipStream_t s);

// What the cut needs on the device besides the slot block, from the host's spans: those of non-zero length, in order.
struct CutPlan {
    std::vector<bnhip_clip_span> spans;       // [n_clips]
    std::vector<int> lens;                    // [n_clips]
    std::vector<long long> tables;            // ostart[n_clips + 1] | tile0[n_clips + 1]
    int n_clips() const { return (int)spans.size(); }
    long long total() const { return tables.empty() ? 0 : tables[spans.size()]; }
    long long n_tiles() const { return tables.empty() ? 0 : tables.back(); }
    size_t table_bytes() const { return tables.size() * 8 + spans.size() * sizeof(bnhip_clip_span); }
};
// the first `limit` spans of non-zero length among spans[0 .. n_spans)
CutPlan cut_plan(const bnhip_clip_span* spans, size_t n_spans, int limit);
// the plan's tables go to d_tables (table_bytes(), 8-byte aligned) and the cut is enqueued behind them on s
hipError_t cut_enqueue(const CutPlan& p, const void* d_block, int bits, const long long* d_slot, void* d_tables, int16_t* d_out, hipStream_t s);

// Where an export's clips are cut from: the slot block of a file-analysis call, or the rings of a capture bank (capture_bank.h).
// enqueue() puts the plan's tables at d_tables (table_bytes(), 8-byte aligned) and the cut into d_out behind them, on the null stream.
struct Cutter {
    virtual size_t table_bytes(const CutPlan& p) const = 0;
    virtual hipError_t enqueue(const CutPlan& p, void* d_tables, int16_t* d_out) const = 0;
    virtual ~Cutter() {}
};
struct SlotCutter : Cutter {
    const void* d_block;
    int bits;
    const long long* d_slot;
    SlotCutter(const void* block, int b, const long long* slot) : d_block(block), bits(b), d_slot(slot) {}
    size_t table_bytes(const CutPlan& p) const override { return p.table_bytes(); }
    hipError_t enqueue(const CutPlan& p, void* d_tables, int16_t* d_out) const override { return cut_enqueue(p, d_block, bits, d_slot, d_tables, d_out, nullptr); }
};

// what the span rule refuses of its settings (pre_samples, post_samples, max_samples); -> 0 or BNHIP_E_INVALID
int span_rule_check(const bnhip_clip_export* x);
// What bnhip_analyze_channels_pcm_clips checks of its export settings before any device is touched; -> 0 or a negative BNHIP_E_*
int clip_export_check(const bnhip_clip_export* x, const bnhip_clips_out* o, int model_rate);
// The export behind the spans, whatever they are cut from: o->spans[0 .. n_spans) are known and checked; the capacity rule, and - for
// n_clips > 0 - one DevCarve, the cut, the normalise, the FLAC encode, the render and the PNG encode on the null stream, and the
// copies that bring the records and the streams down.
int clip_export_spans(const char* what, int device, const Cutter& cut, size_t n_spans, int rate, const bnhip_clip_export* x, bnhip_clips_out* o);
// The second phase of that call, behind the events: the spans of the events written, then clip_export_spans over the slot block.
// d_block / d_slot: the call's slot block and slot table, still on the device; n_out: the recordings' lengths at the model's rate.
int clip_export_run(int device, const void* d_block, int bits, const long long* d_slot, const int64_t* n_out, int n_recordings, int hop,
                    int model_rate, const bnhip_clip_export* x, bnhip_clips_out* o);

}  // namespace bnhip
