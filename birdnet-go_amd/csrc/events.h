// Detection events (api_events.cpp, api_analyze.cpp, events.hip): the detection rows of a file-analysis call merged on the device into what the
// reference's processor reports - a per-class threshold, repeated hits of one class in one recording merged into an event held
// for a fixed number of windows, the minimum hit count and the privacy veto (include/bnhip.h, "Detection events").
//
// The rule needs compares and a maximum only; every step is a scan, a stable sort or a segmented walk, so the answer is a function
// of the rows alone, whatever the grid.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "analyze.h"

namespace bnhip {

// One event (bnhip_event of the C ABI, field for field)
struct Event {
    int32_t recording, cls, first_window, last_window, best_window, count;
    float confidence;
    int32_t status;
};
constexpr int EVENTS_KEEP_DROPPED = 1;
constexpr int EVENT_KEPT = 0, EVENT_FEW = 1, EVENT_VETOED = 2;

// The filter as the kernels read it: thr [n_classes] and veto [n_classes] (or NULL) are device pointers.
struct EventFilterDev {
    const float* thr;
    const uint8_t* veto;
    float veto_thr;
    int hold, min_count, flags, n_classes;
};

// radix passes (8-bit digits) that keys up to max_key need: 1..4
int events_passes(unsigned long long max_key);
// bytes of scratch for up to N rows; the scratch starts 256-byte aligned
size_t events_scratch_bytes(size_t N);
// where launch_events leaves the number of events (all that the filter answers, whatever the cap): 8 bytes inside the scratch
unsigned long long* events_total(void* scratch);
// rows [min(*d_n, N)], nondecreasing in (recording, window): the events in (recording, class, first_window) order land in
// out[0 .. min(cap, total)).  N is the host's bound on the row count and sizes every grid; blocks behind *d_n leave at once.
void launch_events(const DetRow* rows, const unsigned long long* d_n, size_t N, const EventFilterDev& f, int passes, void* scratch,
                   Event* out, unsigned long long cap, hipStream_t s);

}  // namespace bnhip
