// The detection-event rule in streaming form (include/bnhip.h, "Detection events: the real-time bank"; api_event_bank.cpp): every
// source's pending detections stay on the device across calls, and a call feeds them the top-k rows of the windows it brings.
//
// A source's state is one slab: its slots as a struct of arrays (class or -1 for a free slot, first / last / best window, count,
// confidence; in a bank created extended also the deadline, events.h) and behind them the source's latest veto-hit window.  A
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
constexpr int EVB_MAX_SLOTS = 4096;              // k * hold_windows (extended: k * W) at the most: a source's slots fit one wave's LDS
enum EvbMode { EVB_PROCESS = 0, EVB_FLUSH = 1, EVB_PENDING = 2 };

// arrays of a slab and of the update's LDS: six, and in a bank created extended the slots' deadlines as the seventh (96 / 112 KiB at
// EVB_MAX_SLOTS, inside the CU's 160 KiB)
__host__ __device__ inline int evb_arrays(bool extended) { return extended ? 7 : 6; }
// ints of one slab: the arrays of `slots`, then the veto window (padded to 16 bytes)
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
    int32_t wr_parity;                           // slab to write (process mode only)
};

struct EvbCall {
    const EvbGroup* groups;                      // [n_groups]
    int n_groups;
    const int32_t* rowmap;
    const float* conf;                           // [rows][k]
    const int32_t* idx;
    int k, slots, mode;
    bool extended;                               // the bank was created extended: a slot carries its deadline
    int32_t* state;                              // [max_sources][2][evb_slab_ints(slots, extended)]
    Event* stage;                                // the call's staging area
    uint32_t* counts;                            // [n_groups] answered events of each source, then [n_groups] their exclusive bases
    unsigned long long* head;                    // [0] the call's answered events, [1] non-zero: a source ran out of slots or staging
    Event* out;                                  // the answer, at most out_cap events
    unsigned long long out_cap;
};

// The call's launches on s; f.thr and f.veto (never NULL here) are device tables of f.n_classes entries.
void launch_event_bank(const EvbCall& c, const EventFilterDev& f, hipStream_t s);

}  // namespace bnhip
