// C ABI of file analysis: whole recordings in, the top-k of every overlapping window (or the detection rows above a threshold, or
// the detection events merged from them) out, in one call - the windows are framed on the device (analyze.h).  How the recordings
// are stated, checked and brought there - at their own rates and depths, interleaved with a channel picked or mixed - is
// analyze_recordings.h; the event tail is events.h / api_events.h, the clip export that can follow it clips.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <variant>
#include <vector>

#include "analyze_recordings.h"
#include "api_events.h"
#include "api_model.h"
#include "clips.h"

using namespace bnhip;

namespace bnhip {

// wav.frame_clips: p = 0; loop { remain = L - p; keep if first | remain >= clip | remain >= min_tail; stop if remain <= clip; p += hop }.
// Every window in front of the last one visited has remain > clip and is kept; the last one visited is window
// J = ceil((L - clip) / hop) (0 for L <= clip), which starts inside the recording because hop <= clip.
long long analyze_windows(const long long* lengths, int n_rec, int n_samples, int hop, long long min_tail, long long* first) {
    long long total = 0;
    first[0] = 0;
    for (int r = 0; r < n_rec; r++) {
        const long long L = lengths[r];
        const long long J = L > n_samples ? (L - n_samples + hop - 1) / hop : 0;
        const long long remain = L - J * hop;
        const bool keep = J == 0 || remain >= n_samples || remain >= min_tail;
        total += J + (keep ? 1 : 0);
        first[r + 1] = total;
    }
    return total;
}

}  // namespace bnhip

namespace {

constexpr size_t TOPK_LDS_MAX = 150 * 1024;             // the top-k kernel keeps one clip's confidences in LDS (api_predict.cpp)

// the table arguments of every entry; n_samples is the window (the model's clip)
int check_table(const int64_t* lengths, int n_recordings, int n_samples, int hop, int64_t min_tail) {
    if (!lengths) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_recordings < 1 || n_recordings > 65535) return set_err(BNHIP_E_INVALID, "n_recordings must be in [1, 65535]");
    if (n_samples < 1) return set_err(BNHIP_E_INVALID, "n_samples must be positive");
    if (hop < 1 || hop > n_samples) return set_err(BNHIP_E_INVALID, "hop must be in [1, n_samples]");
    if (min_tail < 0) return set_err(BNHIP_E_INVALID, "min_tail must not be negative");
    long long total = 0;
    for (int r = 0; r < n_recordings; r++) {
        if (lengths[r] < 1) return set_err(BNHIP_E_INVALID, "every recording needs at least one sample");
        if (lengths[r] > ANALYZE_MAX_SAMPLES - total) return set_err(BNHIP_E_INVALID, "burst of 2^36 samples or more");
        total += lengths[r];
    }
    return BNHIP_OK;
}

// checked lengths -> the window table: fills first [n + 1] (the ABI's int64_t or the device table's long long), -> the windows
template <class T>
long long window_table(const int64_t* lengths, int n_recordings, int n_samples, int hop, int64_t min_tail, T* first) {
    std::vector<long long> len64(lengths, lengths + n_recordings), first64((size_t)n_recordings + 1);
    const long long W = analyze_windows(len64.data(), n_recordings, n_samples, hop, min_tail, first64.data());
    std::copy(first64.begin(), first64.end(), first);
    return W;
}

// the window-table entries of the two forms that resample
template <class Rec>
long long windows_entry(const Rec* recs, int n_recordings, int model_rate, int n_samples, int hop, int64_t min_tail, int64_t* first_window,
                        int64_t* resampled_length) {
    if (!first_window) return set_err(BNHIP_E_INVALID, "NULL argument");
    Recordings rec;
    if (int rc = describe(recs, n_recordings, model_rate, &rec)) return rc;
    if (int rc = check_table(rec.lengths(), n_recordings, n_samples, hop, min_tail)) return rc;
    const long long W = window_table(rec.lengths(), n_recordings, n_samples, hop, min_tail, first_window);
    if (resampled_length) std::copy(rec.n_out.begin(), rec.n_out.end(), resampled_length);
    return W;
}

// ---- a call: what is asked (Request), of which recordings (Recordings, analyze_recordings.h), answered how (Answer)
struct Request { bnhip_model* m; const void* pcm; int hop; int64_t min_tail; int activation; double sensitivity; int k; };
// the three answers; complete(): no pointer the answer needs is NULL.  Events: every non-NaN row stays on the device (the caller's
// cap counts events) and the reference's result post-filters run there as the call's tail (events.h)
struct TopK { float* conf; int32_t* idx; bool complete() const { return conf && idx; } };
struct Rows { float threshold; bnhip_detection* out; size_t cap; size_t* n_out; bool complete() const { return n_out && (!cap || out); } };
struct Events {
    const bnhip_event_filter* filter; bnhip_event* out; size_t cap; size_t* n_out;
    bool extended = false; const bnhip_event_extend* extend = nullptr;      // the _extended entries: under this extend, then required
    bool guarded = false; const bnhip_event_guards* guards = nullptr;       // the _guarded entries: under these guards, then required
    bool complete() const { return n_out && (!cap || out); }
};
// what bnhip_analyze_channels_pcm_clips adds to its events call: the export settings and where everything goes (clips.h)
struct ClipsTail { const bnhip_clip_export* x; bnhip_clips_out* o; int model_rate; };
struct Answer {
    std::variant<TopK, Rows, Events> what;
    int32_t* chosen = nullptr;                    // the channels entries: [n] what was read of each recording, or NULL
    bnhip_flac_decode_result* flac_result = nullptr;      // the FLAC entries: [n] what the decoder found of each stream
    const ClipsTail* clips = nullptr;             // with the events down and the recordings still in their slots, the clip export runs
};

// Every bnhip_analyze_* device entry.  The windows of rec's slots are framed and classified in chunks of max_batch, and the answer
// comes down: the top-k, the detection rows behind it, or the events behind those.
int analyze(const Request& q, Recordings& rec, const Answer& a) {
    const char* what = "file analysis";
    const TopK* tk = std::get_if<TopK>(&a.what);
    const Rows* rw = std::get_if<Rows>(&a.what);
    const Events* ev = std::get_if<Events>(&a.what);
    const int64_t* lengths = rec.lengths();
    if (!q.m || !q.pcm || !lengths || (rec.flac() && !a.flac_result)) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (!std::visit([](const auto& w) { return w.complete(); }, a.what)) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (ev) if (int rc = event_filter_check(ev->filter)) return rc;
    if (ev && ev->extended) if (int rc = event_extend_check(ev->filter->hold_windows, ev->extend)) return rc;
    if (ev && ev->guarded) if (int rc = event_guards_check(ev->guards)) return rc;
    if (ev && ev->guarded) if (int rc = event_guards_spans_check(ev->guards, rec.n - 1)) return rc;
    if (rec.bits != 0 && rec.bits != 16 && rec.bits != 24 && rec.bits != 32)
        return set_err(BNHIP_E_INVALID, "unsupported bit depth: " + std::to_string(rec.bits) + " (supported: 0 = float32, 16, 24, 32)");
    if (q.k <= 0) return set_err(BNHIP_E_INVALID, "k must be positive");
    if (q.activation < 0 || q.activation > 2) return set_err(BNHIP_E_INVALID, "unknown activation");
    Engine& e = q.m->eng();
    if (int rc = check_table(lengths, rec.n, e.n_samples, q.hop, q.min_tail)) return rc;
    std::vector<long long> table((size_t)rec.n * 3 + 1);              // first[n + 1], then slot[n][2]
    long long* first = table.data();
    long long* slot = first + rec.n + 1;
    const long long W64 = window_table(lengths, rec.n, e.n_samples, q.hop, q.min_tail, first);
    const int kk = std::min(q.k, e.n_classes);
    // (an argument error like the others: answered before the handle is looked at)
    if (ev && (unsigned long long)(W64 * kk) >= EVENT_MAX_ROWS) return set_err(BNHIP_E_INVALID, "2^31 detection rows or more");
    if (q.m->engs.size() > 1) return set_err(BNHIP_E_INVALID, "file analysis runs on one device; use a single-device handle");
    if (e.device < 0) return set_err(BNHIP_E_INVALID, "plan-only model cannot run");
    if ((size_t)e.n_classes * 4 > TOPK_LDS_MAX) return set_err(BNHIP_E_UNSUPPORTED, "too many classes for the LDS top-k");
    if (int rc = rate_plans(&rec)) return rc;
    if (W64 > INT_MAX) return set_err(BNHIP_E_INVALID, "more than INT_MAX windows");
    const int W = (int)W64;
    const SlotPlan sp = slot_plan(rec, slot);
    if (hipSetDevice(e.device) != hipSuccess) return set_err(BNHIP_E_RUNTIME, "hipSetDevice failed");
    // whatever an earlier asynchronous call still has queued on the engine's streams finishes first (as host_run does)
    e.sync_contexts();
    if (e.stream) hipStreamSynchronize(e.stream);
    // one allocation: the recordings' parts | tables | top-k confidences | top-k indices, behind them for rows the detection
    // scratch | row count | rows, and for events the filter's tables | the event scratch (events.h) | the events
    const size_t n_rows_max = (size_t)W * kk, tk_bytes = n_rows_max * 4;
    const size_t out_cap = rw ? std::min(rw->cap, n_rows_max) : ev ? std::min(ev->cap, n_rows_max) : 0;      // records that come down
    const size_t rows_cap = ev ? n_rows_max : out_cap;
    DevCarve cv;
    cv.own_below = 0;
    const SlotDev dv = slot_reserve(sp, cv);
    const size_t o_table = cv.add(table.size() * 8), o_conf = cv.add(tk_bytes), o_idx = cv.add(tk_bytes);
    size_t o_scr = 0, o_total = 0, o_rows = 0, o_evtab = 0, o_evscr = 0, o_evout = 0, o_evguards = 0;
    if (!tk) { o_scr = cv.add(detections_scratch_bytes(W)); o_total = cv.add(8); o_rows = cv.add(rows_cap * sizeof(DetRow)); }
    if (ev) {
        o_evtab = cv.add(event_tables_bytes(e.n_classes, ev->extended)); o_evscr = cv.add(events_scratch_bytes(n_rows_max, ev->guarded && ev->guards->class_dog));
        o_evout = cv.add(out_cap * sizeof(Event));
        if (ev->guarded) o_evguards = cv.add(event_guards_bytes(e.n_classes, ev->guards));
    }
    DevBlocks b;
    cv.alloc(b);
    if (b.he != hipSuccess) return hip_fail(what, b);
    slot_upload(sp, q.pcm, rec, slot, e.device, dv, e.stream, b);
    AN_HIP(b, hipMemcpyAsync(cv.at<void>(o_table), table.data(), table.size() * 8, hipMemcpyHostToDevice, e.stream));
    EventFilterDev fd{};
    if (ev) fd = event_filter_upload(ev->filter, e.n_classes, cv.at<char>(o_evtab), e.stream, b, ev->extended ? ev->extend : nullptr);
    if (ev && ev->guarded) event_guards_upload(ev->guards, e.n_classes, cv.at<char>(o_evguards), e.stream, b, fd);
    WinView view;
    view.first = cv.at<long long>(o_table);
    view.slot = view.first + rec.n + 1;
    view.n_rec = rec.n; view.hop = q.hop; view.w0 = 0;
    float* d_conf = cv.at<float>(o_conf);
    int32_t* d_idx = cv.at<int32_t>(o_idx);
    // the windows in chunks of max_batch, every chunk enqueued behind the previous one (as bnhip_range_heatmap runs its rows)
    bool ran = true;                              // e.run answers a failure with its own text
    std::string err;
    for (int w0 = 0; b.he == hipSuccess && w0 < W; w0 += e.max_batch) {
        const int n = std::min(e.max_batch, W - w0);
        PcmSource ps;
        ps.samples = dv.at(dv.block); ps.bits = rec.bits; ps.win = win_at(view, w0);
        ran = e.run(e.d_stage_in, n, e.d_stage_logits, nullptr, &err, ps);
        if (!ran) break;
        launch_activation(e.d_stage_logits, e.d_post_conf, n, e.n_classes, q.activation, q.sensitivity, e.stream);
        launch_topk(e.d_post_conf, n, e.n_classes, kk, d_conf + (size_t)w0 * kk, d_idx + (size_t)w0 * kk, e.stream);
    }
    auto ok = [&] { return ran && b.he == hipSuccess; };
    unsigned long long total = 0;
    if (ok() && !tk) {
        launch_detections(d_conf, d_idx, W, kk, rw ? rw->threshold : -INFINITY, view, cv.at<void>(o_scr), cv.at<DetRow>(o_rows), rows_cap,
                          cv.at<unsigned long long>(o_total), e.stream);
        // the event tail reads the rows where they lie, and their count where launch_detections left it
        if (ev) launch_events(cv.at<DetRow>(o_rows), cv.at<unsigned long long>(o_total), n_rows_max, fd,
                              events_passes((unsigned long long)rec.n * e.n_classes - 1), cv.at<void>(o_evscr), cv.at<Event>(o_evout), out_cap, e.stream);
    }
    if (ok()) AN_HIP(b, hipGetLastError());
    if (ok() && ev) {
        fetch_counted(events_total(cv.at<void>(o_evscr)), cv.at<void>(o_evout), sizeof(Event), out_cap, ev->out, &total, e.stream, b);
    } else if (ok() && rw) {
        fetch_counted(cv.at<void>(o_total), cv.at<void>(o_rows), sizeof(DetRow), out_cap, rw->out, &total, e.stream, b);
    } else if (ok()) {
        AN_HIP(b, hipMemcpyAsync(tk->conf, d_conf, tk_bytes, hipMemcpyDeviceToHost, e.stream));
        AN_HIP(b, hipMemcpyAsync(tk->idx, d_idx, tk_bytes, hipMemcpyDeviceToHost, e.stream));
    }
    if (ok() && rec.multi) {
        rec.chosen.resize(rec.n);
        AN_HIP(b, hipMemcpyAsync(rec.chosen.data(), dv.at<int>(dv.chsel) + rec.n, (size_t)rec.n * 4, hipMemcpyDeviceToHost, e.stream));
    }
    if (ok() && rec.flac())
        AN_HIP(b, hipMemcpyAsync(a.flac_result, dv.at<void>(dv.flac_res), (size_t)rec.n * sizeof(bnhip_flac_decode_result), hipMemcpyDeviceToHost,
                                 e.stream));
    {
        const hipError_t he = hipStreamSynchronize(e.stream);
        if (b.he == hipSuccess) b.he = he;
    }
    // the continuation: nothing of the call is in flight any more, and the recordings are where the windows were framed from
    int rc = BNHIP_OK;
    if (ok() && a.clips) {
        a.clips->o->n_events = (size_t)total;
        rc = clip_export_run(e.device, dv.at(dv.block), rec.bits, view.slot, lengths, rec.n, q.hop, a.clips->model_rate, a.clips->x, a.clips->o);
    }
    if (!ok()) {
        e.mm_dirty = true;
        if (ran) return hip_fail(what, b);
        (void)hipGetLastError();
        return set_err(BNHIP_E_RUNTIME, err);
    }
    if (rw) *rw->n_out = (size_t)total;
    if (ev) *ev->n_out = (size_t)total;
    if (rc == BNHIP_OK && a.chosen) rec.copy_chosen(a.chosen);
    return rc;
}

// an entry: its recordings as it states them (the arguments of a describe()) taken to their description, then the body
template <class... Form>
int analyze_entry(const Request& q, const Answer& a, Form... form) {
    Recordings rec;
    if (int rc = describe(form..., &rec)) return rc;
    return analyze(q, rec, a);
}

}  // namespace

// the arguments every device entry names alike
#define AN_REQUEST {.m = m, .pcm = pcm, .hop = hop, .min_tail = min_tail, .activation = activation, .sensitivity = sensitivity, .k = k}

extern "C" {

long long bnhip_analyze_windows(const int64_t* lengths, int n_recordings, int n_samples, int hop, int64_t min_tail, int64_t* first_window) {
    if (!first_window) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (int rc = check_table(lengths, n_recordings, n_samples, hop, min_tail)) return rc;
    BN_GUARD_BEGIN
    return window_table(lengths, n_recordings, n_samples, hop, min_tail, first_window);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_pcm_topk(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                           int64_t min_tail, int activation, double sensitivity, int k, float* out_conf, int32_t* out_idx) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = TopK{.conf = out_conf, .idx = out_idx}}, bits_per_sample, lengths, n_recordings);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_pcm(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                      int64_t min_tail, int activation, double sensitivity, int k, float threshold, bnhip_detection* out, size_t cap,
                      size_t* n_out) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = Rows{.threshold = threshold, .out = out, .cap = cap, .n_out = n_out}},
                        bits_per_sample, lengths, n_recordings);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_pcm_events(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                             int64_t min_tail, int activation, double sensitivity, int k, const bnhip_event_filter* filter, bnhip_event* out,
                             size_t cap, size_t* n_out) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = Events{.filter = filter, .out = out, .cap = cap, .n_out = n_out}},
                        bits_per_sample, lengths, n_recordings);
    BN_GUARD_END((void)0)
}

// ---- recordings at their own rates and depths
long long bnhip_analyze_mixed_windows(const bnhip_recording* recs, int n_recordings, int model_rate, int n_samples, int hop, int64_t min_tail,
                                      int64_t* first_window, int64_t* resampled_length) {
    BN_GUARD_BEGIN
    return windows_entry(recs, n_recordings, model_rate, n_samples, hop, min_tail, first_window, resampled_length);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_mixed_pcm_topk(bnhip_model* m, const void* pcm, const bnhip_recording* recs, int n_recordings, int model_rate, int hop,
                                 int64_t min_tail, int activation, double sensitivity, int k, float* out_conf, int32_t* out_idx) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = TopK{.conf = out_conf, .idx = out_idx}}, recs, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_mixed_pcm(bnhip_model* m, const void* pcm, const bnhip_recording* recs, int n_recordings, int model_rate, int hop,
                            int64_t min_tail, int activation, double sensitivity, int k, float threshold, bnhip_detection* out, size_t cap,
                            size_t* n_out) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = Rows{.threshold = threshold, .out = out, .cap = cap, .n_out = n_out}}, recs, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_mixed_pcm_events(bnhip_model* m, const void* pcm, const bnhip_recording* recs, int n_recordings, int model_rate, int hop,
                                   int64_t min_tail, int activation, double sensitivity, int k, const bnhip_event_filter* filter,
                                   bnhip_event* out, size_t cap, size_t* n_out) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = Events{.filter = filter, .out = out, .cap = cap, .n_out = n_out}}, recs, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

// ---- recordings as FLAC streams: the channels calls over what each STREAMINFO says, decoded on the device
long long bnhip_analyze_flac_windows(const uint8_t* streams, const uint64_t* offsets, int n_recordings, int model_rate, int n_samples, int hop,
                                     int64_t min_tail, int64_t* first_window, int64_t* resampled_length) {
    BN_GUARD_BEGIN
    if (!first_window) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_recordings < 1 || n_recordings > 65535) return set_err(BNHIP_E_INVALID, "n_recordings must be in [1, 65535]");
    const std::vector<int32_t> select((size_t)n_recordings, BNHIP_CHANNEL_MIX);
    Recordings rec;
    if (int rc = describe(streams, offsets, select.data(), n_recordings, model_rate, &rec)) return rc;
    if (int rc = check_table(rec.lengths(), n_recordings, n_samples, hop, min_tail)) return rc;
    const long long W = window_table(rec.lengths(), n_recordings, n_samples, hop, min_tail, first_window);
    if (resampled_length) std::copy(rec.n_out.begin(), rec.n_out.end(), resampled_length);
    return W;
    BN_GUARD_END((void)0)
}

#define AN_FLAC_REQUEST {.m = m, .pcm = streams, .hop = hop, .min_tail = min_tail, .activation = activation, .sensitivity = sensitivity, .k = k}

int bnhip_analyze_flac_topk(bnhip_model* m, const uint8_t* streams, const uint64_t* offsets, const int32_t* select, int n_recordings,
                            int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k, float* out_conf,
                            int32_t* out_idx, int32_t* chosen, bnhip_flac_decode_result* result) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_FLAC_REQUEST, {.what = TopK{.conf = out_conf, .idx = out_idx}, .chosen = chosen, .flac_result = result},
                        streams, offsets, select, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_flac(bnhip_model* m, const uint8_t* streams, const uint64_t* offsets, const int32_t* select, int n_recordings, int model_rate,
                       int hop, int64_t min_tail, int activation, double sensitivity, int k, float threshold, bnhip_detection* out, size_t cap,
                       size_t* n_out, int32_t* chosen, bnhip_flac_decode_result* result) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_FLAC_REQUEST,
                        {.what = Rows{.threshold = threshold, .out = out, .cap = cap, .n_out = n_out}, .chosen = chosen, .flac_result = result},
                        streams, offsets, select, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_flac_events(bnhip_model* m, const uint8_t* streams, const uint64_t* offsets, const int32_t* select, int n_recordings,
                              int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                              const bnhip_event_filter* filter, bnhip_event* out, size_t cap, size_t* n_out, int32_t* chosen,
                              bnhip_flac_decode_result* result) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_FLAC_REQUEST,
                        {.what = Events{.filter = filter, .out = out, .cap = cap, .n_out = n_out}, .chosen = chosen, .flac_result = result},
                        streams, offsets, select, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

// ---- multichannel recordings
long long bnhip_analyze_channels_windows(const bnhip_channels_recording* recs, int n_recordings, int model_rate, int n_samples, int hop,
                                         int64_t min_tail, int64_t* first_window, int64_t* resampled_length) {
    BN_GUARD_BEGIN
    return windows_entry(recs, n_recordings, model_rate, n_samples, hop, min_tail, first_window, resampled_length);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_channels_pcm_topk(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate,
                                    int hop, int64_t min_tail, int activation, double sensitivity, int k, float* out_conf, int32_t* out_idx,
                                    int32_t* chosen) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = TopK{.conf = out_conf, .idx = out_idx}, .chosen = chosen}, recs, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_channels_pcm(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate, int hop,
                               int64_t min_tail, int activation, double sensitivity, int k, float threshold, bnhip_detection* out, size_t cap,
                               size_t* n_out, int32_t* chosen) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = Rows{.threshold = threshold, .out = out, .cap = cap, .n_out = n_out}, .chosen = chosen},
                        recs, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_channels_pcm_events(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate,
                                      int hop, int64_t min_tail, int activation, double sensitivity, int k, const bnhip_event_filter* filter,
                                      bnhip_event* out, size_t cap, size_t* n_out, int32_t* chosen) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = Events{.filter = filter, .out = out, .cap = cap, .n_out = n_out}, .chosen = chosen},
                        recs, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_channels_pcm_events_extended(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                               int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                               const bnhip_event_filter* filter, const bnhip_event_extend* extend, bnhip_event* out, size_t cap,
                                               size_t* n_out, int32_t* chosen) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = Events{.filter = filter, .out = out, .cap = cap, .n_out = n_out, .extended = true, .extend = extend},
                                      .chosen = chosen},
                        recs, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_channels_pcm_events_guarded(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                              int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                              const bnhip_event_filter* filter, const bnhip_event_extend* extend,
                                              const bnhip_event_guards* guards, bnhip_event* out, size_t cap, size_t* n_out, int32_t* chosen) {
    BN_GUARD_BEGIN
    return analyze_entry(AN_REQUEST, {.what = Events{.filter = filter, .out = out, .cap = cap, .n_out = n_out, .extended = extend != nullptr,
                                                     .extend = extend, .guarded = true, .guards = guards},
                                      .chosen = chosen},
                        recs, n_recordings, model_rate);
    BN_GUARD_END((void)0)
}

}  // extern "C"

// the events call with the clip export as its continuation (clips.h; the span rule and the export itself: api_clips.cpp)
static int analyze_clips(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate, int hop,
                         int64_t min_tail, int activation, double sensitivity, int k, const bnhip_event_filter* filter, bool extended,
                         const bnhip_event_extend* extend, int32_t* chosen, const bnhip_clip_export* x, bnhip_clips_out* out,
                         bool guarded = false, const bnhip_event_guards* guards = nullptr) {
    if (int rc = clip_export_check(x, out, model_rate)) return rc;
    if (int rc = event_filter_check(filter)) return rc;
    if (filter->flags & BNHIP_EVENTS_KEEP_DROPPED) return set_err(BNHIP_E_INVALID, "the clip export takes kept events only: BNHIP_EVENTS_KEEP_DROPPED is refused");
    const ClipsTail tail{x, out, model_rate};
    size_t n_events = 0;
    return analyze_entry(AN_REQUEST, {.what = Events{.filter = filter, .out = out->events, .cap = out->event_cap, .n_out = &n_events,
                                                     .extended = extended, .extend = extend, .guarded = guarded, .guards = guards},
                                      .chosen = chosen, .clips = &tail},
                        recs, n_recordings, model_rate);
}

extern "C" {

int bnhip_analyze_channels_pcm_clips(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate,
                                     int hop, int64_t min_tail, int activation, double sensitivity, int k, const bnhip_event_filter* filter,
                                     int32_t* chosen, const bnhip_clip_export* x, bnhip_clips_out* out) {
    BN_GUARD_BEGIN
    return analyze_clips(m, pcm, recs, n_recordings, model_rate, hop, min_tail, activation, sensitivity, k, filter, false, nullptr, chosen, x, out);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_channels_pcm_clips_extended(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                              int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                              const bnhip_event_filter* filter, const bnhip_event_extend* extend, int32_t* chosen,
                                              const bnhip_clip_export* x, bnhip_clips_out* out) {
    BN_GUARD_BEGIN
    return analyze_clips(m, pcm, recs, n_recordings, model_rate, hop, min_tail, activation, sensitivity, k, filter, true, extend, chosen, x, out);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_channels_pcm_clips_guarded(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings,
                                             int model_rate, int hop, int64_t min_tail, int activation, double sensitivity, int k,
                                             const bnhip_event_filter* filter, const bnhip_event_extend* extend,
                                             const bnhip_event_guards* guards, int32_t* chosen, const bnhip_clip_export* x,
                                             bnhip_clips_out* out) {
    BN_GUARD_BEGIN
    return analyze_clips(m, pcm, recs, n_recordings, model_rate, hop, min_tail, activation, sensitivity, k, filter, extend != nullptr, extend,
                         chosen, x, out, true, guards);
    BN_GUARD_END((void)0)
}

}  // extern "C"
