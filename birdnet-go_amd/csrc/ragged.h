// The geometry of a burst of clips as the loudness and FLAC kernels see it (loudness.hip, flac.hip).  A uniform batch is n_clips
// clips of n samples and needs no table: clip c starts at c * n.  A ragged burst packs clips of lengths len[c] >= 1 back to back,
// clip c at start[c] = the sum of the lengths before it (64-bit, no padding), and every per-clip count the kernels index by
// (FLAC frames, loudness sub-blocks, true-peak tiles) gets a prefix table of n_clips + 1 entries beside it.  The kernels are stated
// once: a NULL table means the uniform arithmetic.
//
// A flat unit (a frame, a segment, a tile) finds its clip by a binary search over its prefix table: at most 17 steps over a table
// that stays in L2, against a unit's work of at least a hundred recurrence steps or a 4096-sample frame.  The search needs no LDS
// (k_flac_analyse<true> has none to spare), no per-unit array to size, upload and keep in step with the lengths, and it skips
// clips that own no unit (a clip shorter than a sub-block) by construction.
//
// The host states the same burst as a Clips, and every host function of the clip entries (sizes, workspaces, launches, checks) takes
// one: the uniform / ragged decision is made once per kernel family, where the launch's geometry is worked out.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace bnhip {

// The clips of one call on the host: lens NULL for a uniform batch of n_clips clips of n samples, else the host lengths of a ragged
// burst (n is 0 then).
struct Clips {
    int n_clips = 0, n = 0;
    const int* lens = nullptr;
    static Clips uniform(int n_clips, int n) { return {n_clips, n, nullptr}; }
    static Clips ragged(int n_clips, const int* lens) { return {n_clips, 0, lens}; }
    // the sum over the clips of per_clip(length); a uniform batch's is the product, with no walk over the clips
    template <class F>
    size_t sum(F per_clip) const {
        if (!lens) return (size_t)n_clips * (size_t)per_clip(n);
        size_t s = 0;
        for (int c = 0; c < n_clips; c++) s += (size_t)per_clip(lens[c]);
        return s;
    }
    size_t total() const { return sum([](int len) { return len; }); }
};

// The samples of a burst: start NULL for a uniform batch of n-sample clips, else the prefix table [n_clips + 1].
struct ClipGeom {
    int n_clips = 0, n = 0;
    const long long* start = nullptr;
};
__device__ __forceinline__ long long clip_start(const ClipGeom& g, int clip) { return g.start ? g.start[clip] : (long long)clip * g.n; }
__device__ __forceinline__ int clip_len(const ClipGeom& g, int clip) { return g.start ? (int)(g.start[clip + 1] - g.start[clip]) : g.n; }

// The clip that owns flat unit u < t[n_clips]: the c with t[c] <= u < t[c + 1] (t is non-decreasing, t[0] = 0).
__device__ __forceinline__ int ragged_clip(const long long* __restrict__ t, int n_clips, long long u) {
    int lo = 0, hi = n_clips;                               // t[lo] <= u < t[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace bnhip
