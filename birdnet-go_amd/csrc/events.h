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
constexpr int EVENT_KEPT = 0, EVENT_FEW = 1, EVENT_VETOED = 2, EVENT_DOG = 3, EVENT_DAYLIGHT = 4;

// Extended capture's numbers (bnhip_event_extend without its table), in windows.  max_windows == 0: no extend, every deadline is
// b + hold.
struct EventExtend {
    int max_windows = 0, short_wait = 0, medium_from = 0, medium_wait = 0, long_from = 0, long_wait = 0;
};
// The sliding deadline (include/bnhip.h, "Detection events: extended capture"; calculateExtendedFlushDeadline,
// extended_capture.go:311-329), stated once for both kernels and the host: an event of a sliding class opened at window b, hit at
// window w >= b, is due at min(w + wait(w - b), b + max_windows).  b < the deadline the hit joined under <= b + max_windows, so the
// answer is at least w + 1.
__host__ __device__ inline long long ev_deadline(long long b, long long w, int hold, const EventExtend& x) {
    const long long t = w - b;
    const long long wait = t < x.medium_from ? (hold > x.short_wait ? hold : x.short_wait) : t < x.long_from ? x.medium_wait : x.long_wait;
    const long long d = w + wait, most = b + x.max_windows;
    return d < most ? d : most;
}
// W: no live event's deadline lies further behind its last hit
inline int ev_longest_wait(int hold, const EventExtend& x) {
    int W = hold > x.short_wait ? hold : x.short_wait;
    W = x.medium_wait > W ? x.medium_wait : W;
    return x.long_wait > W ? x.long_wait : W;
}

// The dog-bark and daylight guards as the kernels read them (include/bnhip.h, "Detection events: dog-bark and daylight filters"):
// three class tables on the device, each NULL for none.  The file tail reads the daylight spans as rows (recording, from, to),
// ascending and disjoint; the bank brings its sources' spans with the call (events_bank.h) and leaves spans NULL.
struct EventGuardsDev {
    const uint8_t* dog = nullptr;
    const uint8_t* dog_filtered = nullptr;
    const uint8_t* daylight = nullptr;
    float dog_thr = 0.0f;
    int dog_remember = 0;
    const int32_t* spans = nullptr;
    int n_spans = 0;
    // a result that marks its window as a dog hit: float32, strict, false for a NaN on either side
    __host__ __device__ bool dog_hit(int cls, float x) const { return dog && dog[cls] != 0 && x > dog_thr; }
    // an event due at d, the largest dog-hit window before d being v (-1: none): dropped as a recent dog bark
    __host__ __device__ bool dog_drops(int cls, long long d, long long v) const {
        return dog_filtered && dog_filtered[cls] != 0 && v >= 0 && v < d && d - v <= dog_remember;
    }
};

// The filter as the kernels read it: thr [n_classes] and veto [n_classes] (or NULL) are device pointers; with x.max_windows > 0 the
// classes with slide[c] != 0 (slide NULL: all of them) take the sliding deadline.
struct EventFilterDev {
    const float* thr;
    const uint8_t* veto;
    float veto_thr;
    int hold, min_count, flags, n_classes;
    const uint8_t* slide = nullptr;
    EventExtend x{};
    EventGuardsDev g{};
    __host__ __device__ bool slides(int cls) const { return x.max_windows > 0 && (!slide || slide[cls] != 0); }
};

// radix passes (8-bit digits) that keys up to max_key need: 1..4
int events_passes(unsigned long long max_key);
// bytes of scratch for up to N rows; the scratch starts 256-byte aligned.  guarded: with room for the dog hits of a filter whose
// g.dog is set
size_t events_scratch_bytes(size_t N, bool guarded = false);
// where launch_events leaves the number of events (all that the filter answers, whatever the cap): 8 bytes inside the scratch
unsigned long long* events_total(void* scratch);
// rows [min(*d_n, N)], nondecreasing in (recording, window); with f.g.dog the scratch is a guarded one: the events in (recording, class, first_window) order land in
// out[0 .. min(cap, total)).  N is the host's bound on the row count and sizes every grid; blocks behind *d_n leave at once.
void launch_events(const DetRow* rows, const unsigned long long* d_n, size_t N, const EventFilterDev& f, int passes, void* scratch,
                   Event* out, unsigned long long cap, hipStream_t s);

}  // namespace bnhip
