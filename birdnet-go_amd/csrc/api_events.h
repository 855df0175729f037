// What the event tail's two callers share (api_events.cpp: the tail alone; api_analyze.cpp: the tail of an analysis call): the
// filter's refusals, its tables on the device, and the copy that brings a counted list of records down.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "api_oneshot.h"
#include "events.h"

namespace bnhip {

constexpr unsigned long long EVENT_MAX_ROWS = 1ull << 31;

// every refusal of the filter itself; -> 0 or a negative BNHIP_E_*
int event_filter_check(const bnhip_event_filter* f);
// every refusal of an extend beside a filter that event_filter_check has passed (x NULL: refused); k > 0: also k * W
int event_extend_check(int hold_windows, const bnhip_event_extend* x, int k = 0);
// the extend's numbers as the kernels read them
EventExtend event_extend_numbers(const bnhip_event_extend* x);
// bytes of the filter's tables on the device: class_threshold [n_classes], then class_veto [n_classes] where there is one, then
// an extend's class_extended [n_classes] where there is one
inline size_t event_tables_bytes(int n_classes, bool extended = false) { return (size_t)n_classes * 4 + (size_t)n_classes * (extended ? 2 : 1); }
// the tables go up to d_tables (event_tables_bytes) on s, a failure into b; -> the filter as the kernels read it.  x: the extend
// that event_extend_check has passed, or NULL for none
EventFilterDev event_filter_upload(const bnhip_event_filter* f, int n_classes, char* d_tables, hipStream_t s, DevBlocks& b,
                                   const bnhip_event_extend* x = nullptr);

// Guards (include/bnhip.h, "Detection events: dog-bark and daylight filters").  Every refusal of the struct itself but its spans
// (g NULL: refused): the bank's set_guards needs no more
int event_guards_check(const bnhip_event_guards* g);
// ... and of its spans; max_recording: the largest recording of the call
int event_guards_spans_check(const bnhip_event_guards* g, int max_recording);
// bytes of the guards' part on the device: class_dog, class_dog_filtered, class_daylight [n_classes] each, then the spans
inline size_t event_guards_bytes(int n_classes, const bnhip_event_guards* g) {
    return ((size_t)n_classes * 3 + 3) / 4 * 4 + (size_t)(g ? g->n_spans : 0) * 12;
}
// the guards' tables and spans go up to d_guards (event_guards_bytes, 4-byte aligned) on s and into fd.g, a failure into b
void event_guards_upload(const bnhip_event_guards* g, int n_classes, char* d_guards, hipStream_t s, DevBlocks& b, EventFilterDev& fd);

// A list the device has counted (detection rows, events): the count comes down and s is synchronised, then min(*total, cap)
// records are copied to out - that copy is left in flight on s.  A failure goes into b.
void fetch_counted(const void* d_total, const void* d_records, size_t record_bytes, size_t cap, void* out, unsigned long long* total, hipStream_t s,
                   DevBlocks& b);

// the real-time bank (api_event_bank.cpp), as the tick entry (api_predict.cpp) needs it
int event_bank_device(const bnhip_event_bank* b);
int event_bank_k(const bnhip_event_bank* b);
// one tick at a time feeds a bank: held from before the first chunk until the bank's call has returned
std::mutex& event_bank_tick_mutex(bnhip_event_bank* b);
// room on the bank's device for the rows of a tick, kept and grown by the bank: conf [n_rows][k], idx [n_rows][k]
int event_bank_rows(bnhip_event_bank* b, size_t n_rows, float** d_conf, int32_t** d_idx);

}  // namespace bnhip
