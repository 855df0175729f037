// The cut of clips.h: spans of the slot block -> packed mono int16 clips.
#include "clips.h"

#include "pcm_sample.h"
#include "ragged.h"

namespace bnhip {

// ------------------------------------------------------------------------------------------ k_cut_clips
// A flat grid over the tile prefix; a block finds its clip with the search of ragged.h.  A lane owns one 16-byte line of the
// OUTPUT (8 samples from a multiple of 8 on): a clip starts at any sample of the packed output and a span at any sample of a
// recording of 2-, 3- or 4-byte elements, so the loads are element loads (as k_frame_windows') and the store is wide wherever the
// whole line belongs to the clip - everywhere but in a clip's first and last line, where the lane stores its own samples one by one
// (the neighbouring clip's block writes the rest of that line).  Two spans may overlap in the source; no two lanes share an
// output sample.
template <int BITS>
__global__ __launch_bounds__(256) void k_cut_clips(const char* __restrict__ block, const long long* __restrict__ slot,
                                                   const bnhip_clip_span* __restrict__ spans, const long long* __restrict__ ostart,
                                                   const long long* __restrict__ tile0, int n_clips, int16_t* __restrict__ out) {
    const long long b = blockIdx.x;
    const int c = ragged_clip(tile0, n_clips, b);
    const bnhip_clip_span sp = spans[c];
    const long long o0 = ostart[c];
    // (the host has checked that the span lies inside its recording; a lane never reads past the recording whatever the table says)
    const long long len = min(ostart[c + 1] - o0, slot[2 * sp.recording + 1] - sp.start);
    const char* rec = block + slot[2 * sp.recording];
    const long long g = (o0 & ~7ll) + (b - tile0[c]) * CUT_TILE + (long long)threadIdx.x * 8;      // the line's first output sample
    const long long i0 = g - o0;                                                                   // ... as a sample of the clip
    const int lo = (int)max(-i0, 0ll), hi = (int)min(len - i0, 8ll);                               // the lane's samples j of the line
    if (lo >= hi) return;
    union { int16_t q[8]; int4 v; } u;
#pragma unroll
    for (int j = 0; j < 8; j++) u.q[j] = j >= lo && j < hi ? sample_pcm16(frame_sample<BITS>(rec, sp.start + i0 + j)) : (int16_t)0;
    if (hi - lo == 8) {
        *reinterpret_cast<int4*>(out + g) = u.v;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) if (j >= lo && j < hi) out[g + j] = u.q[j];
    }
}

void launch_cut_clips(const void* block, int bits, const long long* slot, const bnhip_clip_span* spans, const long long* ostart,
                      const long long* tile0, int n_clips, long long n_tiles, int16_t* out, hipStream_t s) {
    if (n_clips <= 0 || n_tiles <= 0) return;
    const dim3 grid((unsigned)n_tiles);
    const char* b = static_cast<const char*>(block);
    if (bits == 0) hipLaunchKernelGGL(k_cut_clips<0>, grid, dim3(256), 0, s, b, slot, spans, ostart, tile0, n_clips, out);
    else if (bits == 16) hipLaunchKernelGGL(k_cut_clips<16>, grid, dim3(256), 0, s, b, slot, spans, ostart, tile0, n_clips, out);
    else if (bits == 24) hipLaunchKernelGGL(k_cut_clips<24>, grid, dim3(256), 0, s, b, slot, spans, ostart, tile0, n_clips, out);
    else hipLaunchKernelGGL(k_cut_clips<32>, grid, dim3(256), 0, s, b, slot, spans, ostart, tile0, n_clips, out);
}

CutPlan cut_plan(const bnhip_clip_span* spans, size_t n_spans, int limit) {
    CutPlan p;
    for (size_t i = 0; i < n_spans && (int)p.spans.size() < limit; i++) {
        if (spans[i].length < 1) continue;
        p.spans.push_back(spans[i]);
        p.lens.push_back(spans[i].length);
    }
    const size_t n = p.spans.size();
    if (!n) return p;
    p.tables.assign(2 * (n + 1), 0);
    long long* ostart = p.tables.data();
    long long* tile0 = ostart + n + 1;
    for (size_t c = 0; c < n; c++) {
        ostart[c + 1] = ostart[c] + p.lens[c];
        tile0[c + 1] = tile0[c] + cut_tiles(ostart[c], p.lens[c]);
    }
    return p;
}

hipError_t cut_enqueue(const CutPlan& p, const void* d_block, int bits, const long long* d_slot, void* d_tables, int16_t* d_out, hipStream_t s) {
    const int n = p.n_clips();
    if (!n) return hipSuccess;
    char* t = static_cast<char*>(d_tables);
    const size_t tab_bytes = p.tables.size() * 8;
    hipError_t he = hipMemcpyAsync(t, p.tables.data(), tab_bytes, hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(t + tab_bytes, p.spans.data(), p.spans.size() * sizeof(bnhip_clip_span), hipMemcpyHostToDevice, s);
    if (he != hipSuccess) return he;
    const long long* ostart = reinterpret_cast<const long long*>(t);
    launch_cut_clips(d_block, bits, d_slot, reinterpret_cast<const bnhip_clip_span*>(t + tab_bytes), ostart, ostart + n + 1, n, p.n_tiles(), d_out, s);
    return hipGetLastError();
}

}  // namespace bnhip
