// The kernels of capture_bank.h: frames -> rings (k_capture_write), rings -> packed clips (k_ring_cut).
#include "capture_bank.h"

#include <cstdlib>
#include <cstring>

#include "pcm_sample.h"
#include "ragged.h"

namespace bnhip {

// ------------------------------------------------------------------------------------------ k_capture_write
// k_cut_clips mirrored: a flat grid over the tile prefix of the call's pieces, a block finds its piece with the search of ragged.h,
// and a lane owns one 16-byte line of the RING (8 cells from a multiple of 8 on; a ring's capacity is a multiple of 8, so a line
// lies in one ring).  A piece begins at any cell and at any sample of the packed frames of 2-, 3- or 4-byte elements, so the loads
// are element loads and the store is wide wherever the whole line belongs to the piece - everywhere but in a piece's first and
// last line, where the lane stores its own cells one by one.  Adjacent pieces of one source share a line but never a cell, and
// the host lets no two pieces of a call share a cell (a source's frames beyond the ring's length are trimmed there).
template <int BITS>
__global__ __launch_bounds__(256) void k_capture_write(const char* __restrict__ pcm, long long pcm_samples, const CapPiece* __restrict__ pieces,
                                                       const long long* __restrict__ tile0, int n_pieces, int16_t* __restrict__ rings,
                                                       long long ring_samples) {
    const long long b = blockIdx.x;
    const int c = ragged_clip(tile0, n_pieces, b);
    const CapPiece pc = pieces[c];
    const long long g = (pc.dst & ~7ll) + (b - tile0[c]) * CUT_TILE + (long long)threadIdx.x * 8;   // the line's first cell
    const long long i0 = g - pc.dst;                                                               // ... as a sample of the piece
    // (the host has checked the pieces; a lane never reads past the frames nor stores outside the block whatever the table says)
    const long long n = min(pc.n, pcm_samples - pc.src);
    const int lo = (int)max(-i0, 0ll), hi = (int)min(n - i0, 8ll);                                   // the lane's cells j of the line
    if (lo >= hi || pc.src < 0 || g < 0 || g + 8 > ring_samples) return;
    union { int16_t q[8]; int4 v; } u;
#pragma unroll
    for (int j = 0; j < 8; j++) u.q[j] = j >= lo && j < hi ? sample_pcm16(frame_sample<BITS>(pcm, pc.src + i0 + j)) : (int16_t)0;
    if (hi - lo == 8) {
        *reinterpret_cast<int4*>(rings + g) = u.v;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) if (j >= lo && j < hi) rings[g + j] = u.q[j];
    }
}

void launch_capture_write(const void* pcm, long long pcm_samples, int bits, const CapPiece* pieces, const long long* tile0, int n_pieces,
                          long long n_tiles, int16_t* rings, long long ring_samples, hipStream_t s) {
    if (n_pieces <= 0 || n_tiles <= 0) return;
    const dim3 grid((unsigned)n_tiles);
    const char* p = static_cast<const char*>(pcm);
    if (bits == 16) hipLaunchKernelGGL(k_capture_write<16>, grid, dim3(256), 0, s, p, pcm_samples, pieces, tile0, n_pieces, rings, ring_samples);
    else if (bits == 24) hipLaunchKernelGGL(k_capture_write<24>, grid, dim3(256), 0, s, p, pcm_samples, pieces, tile0, n_pieces, rings, ring_samples);
    else hipLaunchKernelGGL(k_capture_write<32>, grid, dim3(256), 0, s, p, pcm_samples, pieces, tile0, n_pieces, rings, ring_samples);
}

// ------------------------------------------------------------------------------------------ k_ring_cut
// The geometry of k_cut_clips: a lane owns one 16-byte line of the packed output, a clip's tiles are counted from the line its
// first sample lies in, and the partial first and last lines are stored per sample.  The source is int16 in a ring that starts at a
// 16-byte line and whose length is a multiple of 8, so the 8 cells behind any cell p lie in ring lines p / 8 and p / 8 + 1 (mod the
// ring's lines).  ALIGNED: those two lines are loaded whole and the lane's line is four dwords out of their eight, shifted by
// (p & 7) samples: a dword pick by (p & 7) >> 1 and v_alignbyte_b32 by ((p & 7) & 1) * 2 bytes.  Neither load can leave the ring.
// Otherwise eight element loads, as k_cut_clips<16>; the two forms give the same bytes.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_ring_cut(const int16_t* __restrict__ rings, long long capacity, int n_sources,
                                                  const bnhip_clip_span* __restrict__ spans, const long long* __restrict__ ostart,
                                                  const long long* __restrict__ tile0, int n_clips, int16_t* __restrict__ out) {
    const long long b = blockIdx.x;
    const int c = ragged_clip(tile0, n_clips, b);
    const bnhip_clip_span sp = spans[c];
    const long long o0 = ostart[c];
    // (the host has checked the spans; a lane never leaves the bank's block whatever the table says)
    if (sp.recording < 0 || sp.recording >= n_sources || sp.start < 0 || sp.start >= capacity) return;
    const long long len = min(ostart[c + 1] - o0, capacity);
    const int16_t* ring = rings + (long long)sp.recording * capacity;
    const long long g = (o0 & ~7ll) + (b - tile0[c]) * CUT_TILE + (long long)threadIdx.x * 8;      // the line's first output sample
    const long long i0 = g - o0;                                                                   // ... as a sample of the clip
    const int lo = (int)max(-i0, 0ll), hi = (int)min(len - i0, 8ll);                               // the lane's samples j of the line
    if (lo >= hi) return;
    long long p = sp.start + i0;                   // the ring cell of the line's sample 0: -7 <= start + i0 < 2 * capacity
    if (p < 0) p += capacity;
    if (p >= capacity) p -= capacity;
    union { int16_t q[8]; int4 v; uint32_t d[4]; } u;
    if (ALIGNED) {
        const long long lines = capacity >> 3, l0 = p >> 3, l1 = l0 + 1 == lines ? 0 : l0 + 1;
        const int4 a = reinterpret_cast<const int4*>(ring)[l0], e = reinterpret_cast<const int4*>(ring)[l1];
        const uint32_t w[8] = {(uint32_t)a.x, (uint32_t)a.y, (uint32_t)a.z, (uint32_t)a.w, (uint32_t)e.x, (uint32_t)e.y, (uint32_t)e.z, (uint32_t)e.w};
        const int r = (int)(p & 7), k = r >> 1;
        const uint32_t sh = (uint32_t)(r & 1) * 2;
        uint32_t t[5];
#pragma unroll
        for (int j = 0; j < 5; j++) t[j] = k == 0 ? w[j] : k == 1 ? w[j + 1] : k == 2 ? w[j + 2] : w[j + 3];
#pragma unroll
        for (int j = 0; j < 4; j++) u.d[j] = __builtin_amdgcn_alignbyte(t[j + 1], t[j], sh);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            long long q = p + j;
            if (q >= capacity) q -= capacity;
            u.q[j] = j >= lo && j < hi ? ring[q] : (int16_t)0;
        }
    }
    if (hi - lo == 8) {
        *reinterpret_cast<int4*>(out + g) = u.v;
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) if (j >= lo && j < hi) out[g + j] = u.q[j];
    }
}

void launch_ring_cut(const int16_t* rings, long long capacity, int n_sources, const bnhip_clip_span* spans, const long long* ostart,
                     const long long* tile0, int n_clips, long long n_tiles, int16_t* out, bool aligned, hipStream_t s) {
    if (n_clips <= 0 || n_tiles <= 0) return;
    const dim3 grid((unsigned)n_tiles);
    if (aligned) hipLaunchKernelGGL(k_ring_cut<true>, grid, dim3(256), 0, s, rings, capacity, n_sources, spans, ostart, tile0, n_clips, out);
    else hipLaunchKernelGGL(k_ring_cut<false>, grid, dim3(256), 0, s, rings, capacity, n_sources, spans, ostart, tile0, n_clips, out);
}

bool ring_cut_aligned() {
    static const bool aligned = [] {
        const char* e = getenv("BNHIP_RING_CUT");
        return !(e && strcmp(e, "element") == 0);
    }();
    return aligned;
}

hipError_t RingCutter::enqueue(const CutPlan& p, void* d_tables, int16_t* d_out) const {
    const int n = p.n_clips();
    if (!n) return hipSuccess;
    cells = p.spans;
    for (bnhip_clip_span& q : cells) q.start %= capacity;
    char* t = static_cast<char*>(d_tables);
    const size_t tab_bytes = p.tables.size() * 8;
    hipError_t he = hipMemcpyAsync(t, p.tables.data(), tab_bytes, hipMemcpyHostToDevice, nullptr);
    if (he == hipSuccess) he = hipMemcpyAsync(t + tab_bytes, cells.data(), cells.size() * sizeof(bnhip_clip_span), hipMemcpyHostToDevice, nullptr);
    if (he != hipSuccess) return he;
    const long long* ostart = reinterpret_cast<const long long*>(t);
    launch_ring_cut(d_rings, capacity, n_sources, reinterpret_cast<const bnhip_clip_span*>(t + tab_bytes), ostart, ostart + n + 1, n, p.n_tiles(),
                    d_out, ring_cut_aligned(), nullptr);
    return hipGetLastError();
}

}  // namespace bnhip
