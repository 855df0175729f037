// The detection-event rule in streaming form (include/bnhip.h, "Detection events: the real-time bank"; api_event_bank.cpp): every
// source's pending detections stay on the device across calls, and a call feeds them the top-k rows of the windows it brings.
//
// A source's state is one slab: its slots as a struct of arrays (class or -1 for a free slot, first / last / best window, count,
// confidence; in a bank created extended also the deadline, events.h) and behind them the source's latest veto-hit window and, in
// its padding, the latest dog-hit window (-1: none; include/bnhip.h, "Detection events: dog-bark and daylight filters").  A
// launch reads the slab of the source's parity and writes the other; the host flips the parity only once the whole call has
// succeeded (stream_bank.h).  Three launches make a call: the update (one wave per source of the call), a one-block scan of the
// sources' answered counts, and the emit that ranks each source's staged events by (class, first window).  Compares and integer
// counts only; no rank comes from the return value of an atomic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "events.h"

namespace bnhip {

constexpr int EVENT_PENDING = -1;
constexpr int EVB_DAYLIGHT_SPANS = 8;            // daylight spans of a source (BNHIP_EVENT_DAYLIGHT_SPANS)
constexpr int EVB_MAX_SLOTS = 4096;              // k * hold_windows (extended: k * W) at the most: a source's slots fit one wave's LDS
enum EvbMode { EVB_PROCESS = 0, EVB_FLUSH = 1, EVB_PENDING = 2 };

// arrays of a slab and of the update's LDS: six, and in a bank created extended the slots' deadlines as the seventh (96 / 112 KiB at
// EVB_MAX_SLOTS, inside the CU's 160 KiB)
__host__ __device__ inline int evb_arrays(bool extended) { return extended ? 7 : 6; }
// ints of one slab: the arrays of `slots`, then the veto window and the dog window (padded to 16 bytes)
__host__ __device__ inline size_t evb_slab_ints(int slots, bool extended = false) { return (size_t)slots * evb_arrays(extended) + 4; }

// One source of a call, sources ascending.  Its rows are rowmap[row_off .. row_off + n_windows) (row numbers of the call, in
// call order); row j is window clock + j.  Its staged events go to stage[stage_off ..).
struct EvbGroup {
    int32_t source;
    int32_t clock;                               // the source's windows before this call
    int32_t n_windows;
    uint32_t row_off;
    uint32_t stage_off, stage_cap;
    int32_t rd_parity;                           // slab to read; -1: the source has no state yet (every slot free, no veto window)
    int32_t wr_parity;                           // slab to write; in the flush mode -1: none, else the source keeps a dog window and its
                                                 // freed slab goes there
};

struct EvbCall {
    const EvbGroup* groups;                      // [n_groups]
    int n_groups;
    const int32_t* rowmap;
    const float* conf;                           // [rows][k]
    const int32_t* idx;
    int k, slots, mode;
    bool extended;                               // the bank was created extended: a slot carries its deadline
    const int32_t* day;                          // [n_groups][EVB_DAYLIGHT_SPANS][2] the sources' daylight spans [from, to), an unused one
                                                 // 0, 0; NULL: none (always without f.g.daylight)
    int32_t* state;                              // [max_sources][2][evb_slab_ints(slots, extended)]
    Event* stage;                                // the call's staging area
    uint32_t* counts;                            // [n_groups] answered events of each source, then [n_groups] their exclusive bases
    unsigned long long* head;                    // [0] the call's answered events, [1] non-zero: a source ran out of slots or staging
    Event* out;                                  // the answer, at most out_cap events
    unsigned long long out_cap;
};

// Dynamic thresholds (include/bnhip.h, "Detection events: dynamic thresholds").  The learning state is per class and shared by all
// sources of the bank: a pair of slabs with a parity of its own, read and written like a source's (the host flips the parity in the
// same commit).  Three per-class passes and a marking pass run around the launches above:
//   k_evd_prepare  before the update: expiry, the post-expiry state to the other slab, the call's effective thresholds, flags cleared.
//   k_evd_mark     after the emit: the call's rows mark the classes they touch, the sources' staged events the classes they approve
//                  (a store of one value, and a maximum taken on the bits of positive floats: both free of order).
//   k_evd_apply    touch and learn on the other slab, and the number of change records into the upper half of head[1].
//   k_evd_changes  one block, leaves at once when that number is 0: the records in (class, reason) order by a scan.
constexpr int EVD_EXPIRY = 0, EVD_HIGH_CONFIDENCE = 1;
constexpr int EVD_FIRST_CHANGES = 16;            // change records that come down with the count (the first events give them room)

// One change record (bnhip_threshold_change of the C ABI, field for field)
struct ThresholdChange {
    int32_t cls, previous_level, new_level, reason;
    float previous_value, new_value, confidence;
    int32_t pad;
};

// The effective threshold of a class at a level, stated once for the kernels and the host (getAdjustedConfidenceThreshold,
// dynamic_threshold.go): level 0 answers base bit for bit; a NaN base stays NaN at every level.
__host__ __device__ inline float ev_threshold(float base, int level, float min_threshold) {
    if (level <= 0) return base;
    const double v = (double)base * (level == 1 ? 0.75 : level == 2 ? 0.5 : 0.25), lo = (double)min_threshold;
    return (float)(v < lo ? lo : v);
}

// One slab of the class state: expires [n] and learned_at [n] (int64), then level [n] and count [n] (int32)
__host__ __device__ inline size_t evd_slab_bytes(int n_classes) { return (size_t)n_classes * 24; }
struct EvdSlab {
    long long* expires; long long* learned_at; int32_t* level; int32_t* count;
};
__host__ __device__ inline EvdSlab evd_slab(char* state, int n_classes, int parity) {
    char* p = state + (size_t)parity * evd_slab_bytes(n_classes);
    const size_t n = (size_t)n_classes;
    return {reinterpret_cast<long long*>(p), reinterpret_cast<long long*>(p + n * 8), reinterpret_cast<int32_t*>(p + n * 16),
            reinterpret_cast<int32_t*>(p + n * 20)};
}
// bytes of a dynamic bank's device area: state [2] | thr_eff, touch, best bits, change flags [n_classes] | records [2 * n_classes]
__host__ __device__ inline size_t evd_area_bytes(int n_classes) { return 2 * evd_slab_bytes(n_classes) + (size_t)n_classes * (16 + 64); }

struct EvdCall {
    char* area;                                  // evd_area_bytes(n_classes)
    int rd_parity;                               // the slab to read; the other is written
    const float* base;                           // the filter's class_threshold [n_classes]; f.thr is thr_eff inside the area
    const uint8_t* dynamic;                      // [n_classes], non-zero: the class learns
    uint32_t n_rows;                             // entries of the call's row map
    long long now, valid, cooldown;
    float trigger, min_threshold;
    ThresholdChange* first;                      // the first EVD_FIRST_CHANGES records again, beside the call's head
    __host__ __device__ float* thr_eff() const { return reinterpret_cast<float*>(area + 2 * evd_slab_bytes(n_classes)); }
    __host__ __device__ uint32_t* touch() const { return reinterpret_cast<uint32_t*>(thr_eff() + n_classes); }
    __host__ __device__ uint32_t* best() const { return touch() + n_classes; }
    __host__ __device__ uint32_t* flags() const { return best() + n_classes; }
    __host__ __device__ ThresholdChange* records() const { return reinterpret_cast<ThresholdChange*>(flags() + n_classes); }
    int n_classes;
};

// The call's launches on s; f.thr and f.veto (never NULL here) are device tables of f.n_classes entries.  d (NULL: none, and then
// exactly the launches of a bank without dynamic thresholds): f.thr is d->thr_eff(), written here before the update reads it; such
// a call runs its per-class passes also with no source in it.
void launch_event_bank(const EvbCall& c, const EventFilterDev& f, hipStream_t s, const EvdCall* d = nullptr);

}  // namespace bnhip
