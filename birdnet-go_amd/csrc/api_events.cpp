// C ABI of detection events (events.h): the event tail alone over rows the host holds, the reference's minimum hit count, and what
// the tail of an analysis call shares with them (api_events.h).
#include "api_events.h"

#include <algorithm>
#include <cmath>
#include <string>

using namespace bnhip;

static_assert(sizeof(bnhip_detection) == 16 && sizeof(DetRow) == 16, "a detection row is 16 bytes");
static_assert(sizeof(bnhip_event) == 32 && sizeof(Event) == 32, "an event is 32 bytes");
static_assert(BNHIP_EVENTS_KEEP_DROPPED == EVENTS_KEEP_DROPPED, "the flag of events.h");

namespace bnhip {

int event_filter_check(const bnhip_event_filter* f) {
    if (!f || !f->class_threshold) return set_err(BNHIP_E_INVALID, "NULL event filter / class_threshold");
    if (f->hold_windows < 1) return set_err(BNHIP_E_INVALID, "hold_windows must be at least 1");
    if (f->min_count < 1) return set_err(BNHIP_E_INVALID, "min_count must be at least 1");
    if (f->flags & ~BNHIP_EVENTS_KEEP_DROPPED) return set_err(BNHIP_E_INVALID, "unknown event filter flags");
    return BNHIP_OK;
}

int event_extend_check(int hold_windows, const bnhip_event_extend* x, int k) {
    if (!x) return set_err(BNHIP_E_INVALID, "NULL event extend");
    if (x->max_windows < hold_windows) return set_err(BNHIP_E_INVALID, "max_windows must be at least hold_windows");
    if (x->short_wait < 1) return set_err(BNHIP_E_INVALID, "short_wait must be at least 1");
    if (x->medium_wait < 1) return set_err(BNHIP_E_INVALID, "medium_wait must be at least 1");
    if (x->long_wait < 1) return set_err(BNHIP_E_INVALID, "long_wait must be at least 1");
    if (x->medium_from < 1) return set_err(BNHIP_E_INVALID, "medium_from must be at least 1");
    if (x->long_from < x->medium_from) return set_err(BNHIP_E_INVALID, "long_from must be at least medium_from");
    if (k > 0 && (long long)k * ev_longest_wait(hold_windows, event_extend_numbers(x)) > 4096)
        return set_err(BNHIP_E_INVALID, "k * W must be at most 4096 (W: the longest of hold_windows, short_wait, medium_wait, long_wait)");
    return BNHIP_OK;
}

EventExtend event_extend_numbers(const bnhip_event_extend* x) {
    EventExtend n;
    n.max_windows = x->max_windows; n.short_wait = x->short_wait; n.medium_from = x->medium_from; n.medium_wait = x->medium_wait;
    n.long_from = x->long_from; n.long_wait = x->long_wait;
    return n;
}

EventFilterDev event_filter_upload(const bnhip_event_filter* f, int n_classes, char* d_tables, hipStream_t s, DevBlocks& b,
                                   const bnhip_event_extend* x) {
    char* d_veto = f->class_veto ? d_tables + (size_t)n_classes * 4 : nullptr;
    char* d_slide = x && x->class_extended ? d_tables + (size_t)n_classes * 5 : nullptr;
    if (b.he == hipSuccess) b.he = hipMemcpyAsync(d_tables, f->class_threshold, (size_t)n_classes * 4, hipMemcpyHostToDevice, s);
    if (b.he == hipSuccess && d_veto) b.he = hipMemcpyAsync(d_veto, f->class_veto, (size_t)n_classes, hipMemcpyHostToDevice, s);
    if (b.he == hipSuccess && d_slide) b.he = hipMemcpyAsync(d_slide, x->class_extended, (size_t)n_classes, hipMemcpyHostToDevice, s);
    EventFilterDev fd{reinterpret_cast<const float*>(d_tables), reinterpret_cast<const uint8_t*>(d_veto), f->veto_threshold, f->hold_windows,
                      f->min_count, f->flags, n_classes};
    if (x) { fd.slide = reinterpret_cast<const uint8_t*>(d_slide); fd.x = event_extend_numbers(x); }
    return fd;
}

int event_guards_check(const bnhip_event_guards* g) {
    if (!g) return set_err(BNHIP_E_INVALID, "NULL event guards");
    if (g->dog_remember_windows < 0) return set_err(BNHIP_E_INVALID, "dog_remember_windows must not be negative");
    return BNHIP_OK;
}

int event_guards_spans_check(const bnhip_event_guards* g, int max_recording) {
    if (g->n_spans < 0 || g->n_spans > (1 << 20)) return set_err(BNHIP_E_INVALID, "n_spans must be in [0, 2^20]");
    if (g->n_spans > 0 && !g->daylight_spans) return set_err(BNHIP_E_INVALID, "NULL daylight_spans");
    for (int i = 0; i < g->n_spans; i++) {
        const int32_t* sp = g->daylight_spans + (size_t)i * 3;
        const std::string who = "daylight span " + std::to_string(i) + ": ";
        if (sp[0] < 0 || sp[0] > max_recording) return set_err(BNHIP_E_INVALID, who + "recording outside the call");
        if (sp[1] < 0 || sp[2] <= sp[1]) return set_err(BNHIP_E_INVALID, who + "needs 0 <= from < to");
        if (i && (sp[0] < sp[-3] || (sp[0] == sp[-3] && sp[1] < sp[-1])))
            return set_err(BNHIP_E_INVALID, who + "spans must ascend by (recording, from) and not overlap");
    }
    return BNHIP_OK;
}

void event_guards_upload(const bnhip_event_guards* g, int n_classes, char* d_guards, hipStream_t s, DevBlocks& b, EventFilterDev& fd) {
    const size_t n = (size_t)n_classes;
    const uint8_t* tables[3] = {g->class_dog, g->class_dog_filtered, g->class_daylight};
    const uint8_t* dev[3] = {nullptr, nullptr, nullptr};
    for (int t = 0; t < 3; t++) {
        if (!tables[t]) continue;
        dev[t] = reinterpret_cast<const uint8_t*>(d_guards) + n * t;
        if (b.he == hipSuccess) b.he = hipMemcpyAsync(d_guards + n * t, tables[t], n, hipMemcpyHostToDevice, s);
    }
    char* d_spans = d_guards + (n * 3 + 3) / 4 * 4;
    if (g->n_spans > 0 && b.he == hipSuccess)
        b.he = hipMemcpyAsync(d_spans, g->daylight_spans, (size_t)g->n_spans * 12, hipMemcpyHostToDevice, s);
    fd.g.dog = dev[0]; fd.g.dog_filtered = dev[1]; fd.g.daylight = dev[2];
    fd.g.dog_thr = g->dog_threshold; fd.g.dog_remember = g->dog_remember_windows;
    fd.g.spans = g->n_spans > 0 ? reinterpret_cast<const int32_t*>(d_spans) : nullptr;
    fd.g.n_spans = g->n_spans;
}

void fetch_counted(const void* d_total, const void* d_records, size_t record_bytes, size_t cap, void* out, unsigned long long* total, hipStream_t s,
                   DevBlocks& b) {
    if (b.he == hipSuccess) b.he = hipMemcpyAsync(total, d_total, 8, hipMemcpyDeviceToHost, s);
    if (b.he == hipSuccess) b.he = hipStreamSynchronize(s);
    const size_t n = (size_t)std::min<unsigned long long>(*total, cap);
    if (b.he == hipSuccess && n) b.he = hipMemcpyAsync(out, d_records, n * record_bytes, hipMemcpyDeviceToHost, s);
}

}  // namespace bnhip

// what the LDS top-k holds (api_predict.cpp): with recording < 65 535 a (recording, class) key is below 2^32
static constexpr int EVENT_MAX_CLASSES = 150 * 1024 / 4;

namespace {

// the tail alone over rows the host holds: one pass over the rows for every refusal, one DevCarve (rows, their count, the filter's
// tables, the scratch, the events), the rows and tables up, the tail's launches, the count and the events down.  extended: under
// `extend`, which is then required; guarded: under `guards`, which are then required
int detection_events(int device, const bnhip_detection* rows, size_t n_rows, int n_classes, const bnhip_event_filter* filter, bool extended,
                     const bnhip_event_extend* extend, bnhip_event* out, size_t cap, size_t* n_out, bool guarded = false,
                     const bnhip_event_guards* guards = nullptr) {
    const char* what = "detection_events";
    if (!n_out || (cap && !out) || (n_rows && !rows)) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (int rc = event_filter_check(filter)) return rc;
    if (extended) if (int rc = event_extend_check(filter->hold_windows, extend)) return rc;
    if (guarded) if (int rc = event_guards_check(guards)) return rc;
    if (guarded) if (int rc = event_guards_spans_check(guards, 65534)) return rc;
    if (n_classes < 1 || n_classes > EVENT_MAX_CLASSES) return set_err(BNHIP_E_INVALID, "n_classes must be in [1, 38400]");
    if (n_rows >= EVENT_MAX_ROWS) return set_err(BNHIP_E_INVALID, "2^31 detection rows or more");
    int max_rec = 0;
    for (size_t i = 0; i < n_rows; i++) {
        const bnhip_detection& q = rows[i];
        const std::string who = "row " + std::to_string(i) + ": ";
        if (q.recording < 0 || q.recording > 65534) return set_err(BNHIP_E_INVALID, who + "recording must be in [0, 65534]");
        if (q.window < 0) return set_err(BNHIP_E_INVALID, who + "negative window");
        if (q.class_index < 0 || q.class_index >= n_classes) return set_err(BNHIP_E_INVALID, who + "class_index outside the table");
        if (i && (q.recording < rows[i - 1].recording || (q.recording == rows[i - 1].recording && q.window < rows[i - 1].window)))
            return set_err(BNHIP_E_INVALID, who + "rows must be nondecreasing in (recording, window)");
        max_rec = std::max(max_rec, (int)q.recording);
    }
    if (n_rows == 0) { *n_out = 0; return BNHIP_OK; }
    if (int rc = use_device(device)) return rc;
    const size_t ev_cap = std::min(cap, n_rows);
    DevCarve cv;
    const size_t o_rows = cv.add(n_rows * sizeof(DetRow)), o_count = cv.add(8), o_tab = cv.add(event_tables_bytes(n_classes, extended));
    const size_t o_scr = cv.add(events_scratch_bytes(n_rows, guarded && guards->class_dog)), o_out = cv.add(ev_cap * sizeof(Event));
    const size_t o_guards = guarded ? cv.add(event_guards_bytes(n_classes, guards)) : 0;
    DevBlocks b;
    cv.alloc(b);
    const unsigned long long n64 = n_rows;
    if (b.he == hipSuccess) b.he = hipMemcpy(cv.at<void>(o_rows), rows, n_rows * sizeof(DetRow), hipMemcpyHostToDevice);
    if (b.he == hipSuccess) b.he = hipMemcpy(cv.at<void>(o_count), &n64, 8, hipMemcpyHostToDevice);
    EventFilterDev fd = event_filter_upload(filter, n_classes, cv.at<char>(o_tab), nullptr, b, extended ? extend : nullptr);
    if (guarded) event_guards_upload(guards, n_classes, cv.at<char>(o_guards), nullptr, b, fd);
    if (b.he != hipSuccess) return hip_fail(what, b);
    launch_events(cv.at<DetRow>(o_rows), cv.at<unsigned long long>(o_count), n_rows, fd, events_passes((unsigned long long)(max_rec + 1) * n_classes - 1),
                  cv.at<void>(o_scr), cv.at<Event>(o_out), ev_cap, nullptr);
    if (int rc = launch_status(what)) { hipDeviceSynchronize(); return rc; }
    unsigned long long total = 0;
    fetch_counted(events_total(cv.at<void>(o_scr)), cv.at<void>(o_out), sizeof(Event), ev_cap, out, &total, nullptr, b);
    if (b.he == hipSuccess) b.he = hipStreamSynchronize(nullptr);
    if (b.he != hipSuccess) return hip_fail(what, b);
    *n_out = (size_t)total;
    return BNHIP_OK;
}

}  // namespace

extern "C" {

int bnhip_detection_events(int device, const bnhip_detection* rows, size_t n_rows, int n_classes, const bnhip_event_filter* filter,
                           bnhip_event* out, size_t cap, size_t* n_out) {
    BN_GUARD_BEGIN
    return detection_events(device, rows, n_rows, n_classes, filter, false, nullptr, out, cap, n_out);
    BN_GUARD_END((void)0)
}

int bnhip_detection_events_extended(int device, const bnhip_detection* rows, size_t n_rows, int n_classes, const bnhip_event_filter* filter,
                                    const bnhip_event_extend* extend, bnhip_event* out, size_t cap, size_t* n_out) {
    BN_GUARD_BEGIN
    return detection_events(device, rows, n_rows, n_classes, filter, true, extend, out, cap, n_out);
    BN_GUARD_END((void)0)
}

int bnhip_detection_events_guarded(int device, const bnhip_detection* rows, size_t n_rows, int n_classes, const bnhip_event_filter* filter,
                                   const bnhip_event_extend* extend, const bnhip_event_guards* guards, bnhip_event* out, size_t cap,
                                   size_t* n_out) {
    BN_GUARD_BEGIN
    return detection_events(device, rows, n_rows, n_classes, filter, extend != nullptr, extend, out, cap, n_out, true, guards);
    BN_GUARD_END((void)0)
}

// ev_deadline for the host (events.h), host only
int64_t bnhip_event_deadline(int32_t hold_windows, const bnhip_event_extend* extend, int64_t first_window, int64_t window) {
    if (hold_windows < 1) return set_err(BNHIP_E_INVALID, "hold_windows must be at least 1");
    if (int rc = event_extend_check(hold_windows, extend)) return rc;
    if (first_window < 0 || window < first_window) return set_err(BNHIP_E_INVALID, "window must be at least first_window, and neither negative");
    return ev_deadline(first_window, window, hold_windows, event_extend_numbers(extend));
}

// calculateMinDetectionsFromSettings (processor.go:1669-1729), host only
int bnhip_event_min_count(int level, double overlap_seconds) {
    if (level == 0) return 1;
    static const double share[6] = {0.0, 0.20, 0.30, 0.50, 0.60, 0.70};
    const double segment = std::max(0.1, 3.0 - overlap_seconds);
    const double required = 6.0 / segment * (level >= 1 && level <= 5 ? share[level] : 0.30) - 1e-9;
    return (int)std::max(1.0, std::ceil(required));
}

}  // extern "C"
