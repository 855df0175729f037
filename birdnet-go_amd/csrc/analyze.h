// File analysis (api_analyze.cpp, analyze_recordings.cpp, analyze.hip): the overlapping windows of a burst of recordings are framed on the device.
//
// The recordings sit in ONE device block, recording r in a slot of its own: the slot starts 16-byte aligned and holds the
// recording's samples followed by zeros up to a whole quad (4 samples).  Window j of recording r starts at sample j * hop of the
// slot and has min(n_samples, len[r] - j * hop) valid samples; the model sees the rest of its clip as zeros (wav.frame_clips pads
// the last window of a recording the same way).  Windows are numbered through the burst: `first` is the prefix table of the
// recordings' window counts (ragged.h), so window w belongs to the r with first[r] <= w < first[r + 1] and is its window w - first[r].
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace bnhip {

// What a launch needs to find its windows.  first: [n_rec + 1] window prefix; slot: [n_rec][2] = {byte offset of the slot in the
// block, samples in the recording}; w0: the burst window that the launch's block 0 takes.  first == nullptr: no table (the input
// is a batch of whole clips).
struct WinView {
    const long long* first = nullptr;
    const long long* slot = nullptr;
    int n_rec = 0, hop = 0, w0 = 0;
};
inline WinView win_at(WinView v, int dw) { v.w0 += dw; return v; }

// host: the framing rule of wav.frame_clips in integers.  first[0] = 0, first[r + 1] = first[r] + windows of a recording of
// lengths[r] samples: a window is kept when it is the recording's first, or remain >= n_samples, or remain >= min_tail; framing
// stops when remain <= n_samples.  -> first[n_rec]
long long analyze_windows(const long long* lengths, int n_rec, int n_samples, int hop, long long min_tail, long long* first);
// bytes of a sample on the device (bits 0: float32)
inline size_t analyze_sample_bytes(int bits) { return bits ? (size_t)bits / 8 : 4; }
// bytes of a recording's slot: whole quads, then up to the next 16-byte line
inline size_t analyze_slot_bytes(long long len, int bits) { return ((size_t)((len + 3) / 4 * 4) * analyze_sample_bytes(bits) + 15) / 16 * 16; }

// k_frame_windows: windows [v.w0, v.w0 + n) as float32 clips [n][n_samples], converted as launch_pcm_to_f32 converts (bits 0: copied),
// element loads at any alignment, zeros behind the valid samples.
void launch_frame_windows(const void* block, int bits, const WinView& v, int n, int n_samples, float* out, hipStream_t s);

// One detection: the row of a window's top-k that reaches the threshold.  (bnhip_detection of the C ABI, field for field)
struct DetRow { int32_t recording, window, cls; float confidence; };
// bytes of scratch that launch_detections needs for W windows (per-window offsets, per-block bases)
size_t detections_scratch_bytes(int W);
// k_detections: conf / idx are the dense top-k [W][k] (descending per window).  Rows with confidence >= threshold (a NaN is not),
// ordered by window, then rank, land in rows[0 .. min(cap, total)); *d_total = total.  Three launches: per-window counts with
// a block scan, a scan of the block totals, the scatter - the order needs no atomics.
void launch_detections(const float* conf, const int32_t* idx, int W, int k, float threshold, const WinView& v, void* scratch, DetRow* rows,
                       unsigned long long cap, unsigned long long* d_total, hipStream_t s);

}  // namespace bnhip
