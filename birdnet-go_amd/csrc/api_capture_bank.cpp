// C ABI of the capture bank (capture_bank.h; include/bnhip.h, "Capture bank"), and the span rule on a running clock
// (bnhip_capture_spans, host only).
//
// The clocks are the host's, as the event bank's: written[s] counts the samples ever given for source s, floor[s] is the first
// position a read may still trust.  A write is one transaction on the bank's stream - one staging copy (the pieces and their tile
// prefix, then the packed frames), one launch, one synchronise - and a commit that runs only once everything succeeded.  The
// rings are too large to keep in pairs of slabs, so a write that fails on the device cannot leave them as they were: it leaves the
// clocks as they were and raises the floor of every source of the call behind every cell the launch may have touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "capture_bank.h"
#include "flac.h"
#include "stream_bank.h"

using namespace bnhip;

namespace {

constexpr const char* WHAT = "capture bank";

int cap_fail(const char* what, hipError_t he) {
    (void)hipGetLastError();
    return set_err(he == hipErrorOutOfMemory ? BNHIP_E_NOMEM : BNHIP_E_RUNTIME, std::string(what) + ": " + hipGetErrorString(he));
}

// what read and export check of their spans before any device call; -> 0 or BNHIP_E_INVALID
int spans_check(const bnhip_capture_bank* b, const bnhip_clip_span* spans, int n_spans, long long* total) {
    if (n_spans < 1 || n_spans > 65535) return set_err(BNHIP_E_INVALID, "n_spans must be in [1, 65535]");
    *total = 0;
    for (int i = 0; i < n_spans; i++) {
        const bnhip_clip_span& q = spans[i];
        const std::string who = "span " + std::to_string(i) + ": ";
        if (q.recording < 0 || q.recording >= b->max_sources) return set_err(BNHIP_E_INVALID, who + "no such capture bank source: " + std::to_string(q.recording));
        if (q.length < 0) return set_err(BNHIP_E_INVALID, who + "negative length");
        if (q.length == 0) continue;
        if (q.start < b->oldest(q.recording)) return set_err(BNHIP_E_INVALID, who + "begins before the oldest sample its ring holds");
        if (q.start > b->src[(size_t)q.recording].written - q.length) return set_err(BNHIP_E_INVALID, who + "ends behind the last sample written");
        *total += q.length;
    }
    if (*total > RAGGED_MAX_SAMPLES) return set_err(BNHIP_E_INVALID, "the clips' total length must be below 2^36 samples");
    return BNHIP_OK;
}

// the span rule of bnhip.h "Capture bank" for one event of a source
void capture_span(const bnhip_event& e, int64_t written, int64_t oldest, int64_t origin, int hop, const bnhip_clip_export* x, bnhip_clip_span* span,
                  int32_t* status) {
    const int64_t P0 = origin + (int64_t)e.first_window * hop - x->pre_samples;
    const int64_t P1 = origin + (int64_t)(x->extended ? e.last_window : e.first_window) * hop + x->post_samples;
    const int64_t begin = std::max(P0, oldest);
    *span = bnhip_clip_span{begin, 0, e.recording};
    if (e.status != 0) { *status = BNHIP_CAPTURE_DROPPED; return; }
    if (P1 > written) { *status = BNHIP_CAPTURE_NOT_YET; return; }
    if (begin >= P1) { *status = BNHIP_CAPTURE_GONE; return; }
    span->length = (int32_t)(std::min(P1, begin + x->max_samples) - begin);
    *status = begin > P0 ? BNHIP_CAPTURE_CLAMPED : BNHIP_CAPTURE_OK;
}

}  // namespace

namespace bnhip {

int capture_plan(const bnhip_capture_bank* b, int n_frames, const int32_t* sources, const int64_t* n_samples, const void* const* frames,
                 const int64_t* frame_at, CapturePlan* p) {
    const int64_t cap = b->capacity;
    // ---- check, and each source's total
    p->total.assign((size_t)b->max_sources, 0);
    int64_t given = 0;
    for (int f = 0; f < n_frames; f++) {
        const std::string who = "frame " + std::to_string(f) + ": ";
        if (sources[f] < 0 || sources[f] >= b->max_sources) return set_err(BNHIP_E_INVALID, who + "no such capture bank source: " + std::to_string(sources[f]));
        if (n_samples[f] < 0) return set_err(BNHIP_E_INVALID, who + "negative frame length");
        if (n_samples[f] > 0 && !frames[f]) return set_err(BNHIP_E_INVALID, who + "frame pointer is NULL");
        if (n_samples[f] > RAGGED_MAX_SAMPLES - given) return set_err(BNHIP_E_INVALID, "the frames' total length must be below 2^36 samples");
        given += n_samples[f];
        if (p->total[(size_t)sources[f]] == 0 && n_samples[f] > 0) p->listed.push_back(sources[f]);
        p->total[(size_t)sources[f]] += n_samples[f];
    }
    // ---- per frame what is stored of it, cut where the ring wraps
    p->tile0.assign(1, 0);
    std::vector<int64_t> seen((size_t)b->max_sources, 0);                 // samples of the source in the frames before
    for (int f = 0; f < n_frames; f++) {
        const int s = sources[f];
        const int64_t q0 = seen[(size_t)s], skip = std::max<int64_t>(p->total[(size_t)s] - cap, 0);
        seen[(size_t)s] += n_samples[f];
        const int64_t from = std::max(q0, skip) - q0, n = n_samples[f] - from;
        if (n <= 0) continue;
        p->parts.push_back(CapturePlan::Part{f, from, n});
        int64_t pos = b->src[(size_t)s].written + q0 + from, src = frame_at ? frame_at[f] + from : p->packed, left = n;
        while (left > 0) {
            const int64_t cell = pos % cap, run = std::min(left, cap - cell);
            p->pieces.push_back(CapPiece{src, (long long)s * cap + cell, run});
            p->tile0.push_back(p->tile0.back() + cut_tiles((long long)s * cap + cell, run));
            pos += run; src += run; left -= run;
        }
        p->packed += n;
    }
    if (p->tile0.back() > INT_MAX) return set_err(BNHIP_E_INVALID, "the frames' stored samples must fit 2^31 - 1 tiles of 2048");
    return BNHIP_OK;
}

void capture_write_failed(bnhip_capture_bank* b, const CapturePlan& p) {
    for (int32_t s : p.listed) {
        bnhip_capture_bank::Source& S = b->src[(size_t)s];
        S.floor = std::max(S.floor, S.written + p.total[(size_t)s] - b->capacity);
    }
}

void capture_write_commit(bnhip_capture_bank* b, const CapturePlan& p) {
    for (int32_t s : p.listed) b->src[(size_t)s].written += p.total[(size_t)s];
}

}  // namespace bnhip

extern "C" {

int bnhip_capture_bank_create(int device, int max_sources, int64_t capacity_samples, int rate, bnhip_capture_bank** out) {
    if (!out) return set_err(BNHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (max_sources < 1 || max_sources > 65535) return set_err(BNHIP_E_INVALID, "max_sources must be in [1, 65535]");
    if (capacity_samples < 1 || capacity_samples > (int64_t)INT32_MAX + 1 - CAPTURE_ALIGN)
        return set_err(BNHIP_E_INVALID, "capacity_samples must be in [1, 2^31 - 1024]");
    if (rate < 1 || rate > FLAC_MAX_RATE) return set_err(BNHIP_E_INVALID, "sample rate must be in [1, 1048575]");
    bnhip_capture_bank* b = nullptr;
    BN_GUARD_BEGIN
    if (int rc = use_device(device)) return rc;
    b = new bnhip_capture_bank();
    b->device = device; b->max_sources = max_sources; b->rate = rate;
    b->capacity = (capacity_samples + CAPTURE_ALIGN - 1) / CAPTURE_ALIGN * CAPTURE_ALIGN;
    b->src.resize((size_t)max_sources);
    hipError_t he = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (he != hipSuccess) b->stream = nullptr;
    const size_t ring_bytes = (size_t)max_sources * (size_t)b->capacity * 2;
    if (he == hipSuccess) he = hipMalloc((void**)&b->d_rings, ring_bytes);
    if (he == hipSuccess) he = hipMemset(b->d_rings, 0, ring_bytes);
    if (he != hipSuccess) {
        bank_free(b); b = nullptr;
        return cap_fail("capture bank create", he);
    }
    *out = b;
    return BNHIP_OK;
    BN_GUARD_END(bank_free(b))
}

int bnhip_capture_bank_info(const bnhip_capture_bank* b, int* max_sources, int64_t* capacity_samples, int* rate) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (max_sources) *max_sources = b->max_sources;
    if (capacity_samples) *capacity_samples = b->capacity;
    if (rate) *rate = b->rate;
    return BNHIP_OK;
}

int bnhip_capture_bank_positions(bnhip_capture_bank* b, int64_t* written, int64_t* oldest) {
    if (!b || !written || !oldest) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    for (int s = 0; s < b->max_sources; s++) {
        written[s] = b->src[(size_t)s].written;
        oldest[s] = b->oldest(s);
    }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

// host only: nothing below `written` is readable, and a reset source has written nothing
int bnhip_capture_bank_reset(bnhip_capture_bank* b, int source) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (source < -1 || source >= b->max_sources) return set_err(BNHIP_E_INVALID, "no such capture bank source: " + std::to_string(source));
    for (int s = source < 0 ? 0 : source; s < (source < 0 ? b->max_sources : source + 1); s++) b->src[(size_t)s] = bnhip_capture_bank::Source();
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_capture_bank_write(bnhip_capture_bank* b, int n_frames, const int32_t* sources, const int64_t* n_samples, const void* const* frames,
                             int bits_per_sample) {
    if (!b || (n_frames > 0 && (!sources || !n_samples || !frames))) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_frames < 0) return set_err(BNHIP_E_INVALID, "n_frames is negative");
    if (bits_per_sample != 16 && bits_per_sample != 24 && bits_per_sample != 32) return set_err(BNHIP_E_INVALID, "bits_per_sample must be 16, 24 or 32");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    const int64_t cap = b->capacity;
    const size_t bytes = (size_t)bits_per_sample / 8;
    CapturePlan plan;
    if (int rc = capture_plan(b, n_frames, sources, n_samples, frames, nullptr, &plan)) return rc;
    if (plan.listed.empty()) return BNHIP_OK;
    const std::vector<CapPiece>& pieces = plan.pieces;
    const std::vector<long long>& tile0 = plan.tile0;
    const int64_t packed = plan.packed;
    // ---- stage
    hipSetDevice(b->device);
    const size_t o_tile = pieces.size() * sizeof(CapPiece), o_pcm = (o_tile + tile0.size() * 8 + 15) / 16 * 16;
    const size_t stage_bytes = o_pcm + (size_t)packed * bytes;
    if (!bank_grow((void**)&b->h_stage, &b->d_stage, &b->stage_cap, stage_bytes))
        return set_err(BNHIP_E_NOMEM, std::string("allocation failed (") + WHAT + " staging)");
    memcpy(b->h_stage, pieces.data(), o_tile);
    memcpy(b->h_stage + o_tile, tile0.data(), tile0.size() * 8);
    uint8_t* pk = b->h_stage + o_pcm;
    for (const CapturePlan::Part& p : plan.parts) {
        memcpy(pk, static_cast<const uint8_t*>(frames[p.frame]) + (size_t)p.from * bytes, (size_t)p.n * bytes);
        pk += (size_t)p.n * bytes;
    }
    // ---- run
    const char* ds = static_cast<const char*>(b->d_stage);
    hipError_t he = hipMemcpyAsync(b->d_stage, b->h_stage, stage_bytes, hipMemcpyHostToDevice, b->stream);
    bool launched = false;
    if (he == hipSuccess) {
        launch_capture_write(ds + o_pcm, packed, bits_per_sample, reinterpret_cast<const CapPiece*>(ds), reinterpret_cast<const long long*>(ds + o_tile),
                             (int)pieces.size(), tile0.back(), b->d_rings, (long long)b->max_sources * cap, b->stream);
        launched = true;
        he = hipGetLastError();
    }
    const hipError_t hs = hipStreamSynchronize(b->stream);
    if (he == hipSuccess) he = hs;
    if (he != hipSuccess) {
        // the launch may have stored any part of what it was given: nothing it could have touched is readable again
        if (launched) capture_write_failed(b, plan);
        return cap_fail(WHAT, he);
    }
    // ---- commit: everything above succeeded
    capture_write_commit(b, plan);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

// the cut alone: one DevCarve (the cut's tables, the clips), the cut, one D2H copy
int bnhip_capture_bank_read_pcm16(bnhip_capture_bank* b, const bnhip_clip_span* spans, int n_spans, int16_t* out_pcm) {
    const char* what = "capture_bank_read_pcm16";
    if (!b || !spans || !out_pcm) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    long long total = 0;
    if (int rc = spans_check(b, spans, n_spans, &total)) return rc;
    const CutPlan plan = cut_plan(spans, (size_t)n_spans, n_spans);
    if (plan.n_clips() == 0) return BNHIP_OK;
    if (int rc = use_device(b->device)) return rc;
    const RingCutter cut(b->d_rings, b->capacity, b->max_sources);
    DevCarve cv;
    const size_t o_tab = cv.add(cut.table_bytes(plan)), o_out = cv.add((size_t)total * 2);
    DevBlocks blk;
    cv.alloc(blk);
    if (blk.he == hipSuccess) blk.he = cut.enqueue(plan, cv.at<void>(o_tab), cv.at<int16_t>(o_out));
    // (the null stream orders the copy after the kernel; it is the call's synchronise)
    if (blk.he == hipSuccess) blk.he = hipMemcpy(out_pcm, cv.at<void>(o_out), (size_t)total * 2, hipMemcpyDeviceToHost);
    if (blk.he != hipSuccess) { hipDeviceSynchronize(); return hip_fail(what, blk); }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_capture_bank_clips(bnhip_capture_bank* b, const bnhip_clip_span* spans, int n_spans, const bnhip_clip_export* x, bnhip_clips_out* out) {
    if (!b || !spans) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (int rc = clip_export_check(x, out, b->rate)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    long long total = 0;
    if (int rc = spans_check(b, spans, n_spans, &total)) return rc;
    memcpy(out->spans, spans, (size_t)n_spans * sizeof(bnhip_clip_span));
    return clip_export_spans("capture_bank_clips", b->device, RingCutter(b->d_rings, b->capacity, b->max_sources), (size_t)n_spans, b->rate, x, out);
    BN_GUARD_END((void)0)
}

void bnhip_capture_bank_destroy(bnhip_capture_bank* b) {
    try { bank_free(b); } catch (...) {}
}

int bnhip_capture_spans(const bnhip_event* events, size_t n_events, int n_sources, const int64_t* written, const int64_t* oldest,
                        const int64_t* origins, int hop, const bnhip_clip_export* x, bnhip_clip_span* spans, int32_t* status) {
    BN_GUARD_BEGIN
    if (!written || !oldest || !x || (n_events && (!events || !spans || !status))) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_sources < 1) return set_err(BNHIP_E_INVALID, "n_sources must be at least 1");
    if (hop < 1) return set_err(BNHIP_E_INVALID, "hop must be at least 1");
    if (int rc = span_rule_check(x)) return rc;
    for (size_t i = 0; i < n_events; i++)
        if (events[i].recording < 0 || events[i].recording >= n_sources)
            return set_err(BNHIP_E_INVALID, "event " + std::to_string(i) + ": source outside the table");
    for (size_t i = 0; i < n_events; i++) {
        const int s = events[i].recording;
        capture_span(events[i], written[s], oldest[s], origins ? origins[s] : 0, hop, x, &spans[i], &status[i]);
    }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

}  // extern "C"
