// Detection clips from analysed recordings (clips.h): the span rule (bnhip_event_clip_spans), the cut alone
// (bnhip_recording_clips_pcm16), and the second phase of bnhip_analyze_channels_pcm_clips - the cut, the normalise, the FLAC encode,
// the render and the PNG encode over the clips where they lie.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "analyze_recordings.h"
#include "clip_source.h"
#include "clips.h"
#include "flac.h"
#include "loudness.h"
#include "png.h"

using namespace bnhip;

static_assert(sizeof(bnhip_clip_span) == 16, "a clip span is 16 bytes");

namespace bnhip {

int span_rule_check(const bnhip_clip_export* x) {
    if (x->pre_samples < 0) return set_err(BNHIP_E_INVALID, "pre_samples must not be negative");
    if (x->post_samples < 1) return set_err(BNHIP_E_INVALID, "post_samples must be at least 1");
    if (x->max_samples < 1) return set_err(BNHIP_E_INVALID, "max_samples must be at least 1");
    return 0;
}

}  // namespace bnhip

namespace {

// the rule of bnhip.h "Detection clips" for one event of a recording of N samples at the model's rate
bnhip_clip_span event_span(const bnhip_event& e, long long N, int hop, const bnhip_clip_export* x) {
    auto clamp = [N](long long v) { return std::min(std::max(v, 0ll), N); };
    const long long begin = clamp((long long)e.first_window * hop - x->pre_samples);
    long long end = clamp((long long)(x->extended ? e.last_window : e.first_window) * hop + x->post_samples);
    end = std::min(end, begin + x->max_samples);
    return bnhip_clip_span{begin, e.status != 0 ? 0 : (int32_t)(end - begin), e.recording};
}

int event_spans(const bnhip_event* events, size_t n_events, const int64_t* n_out, int n_recordings, int hop, const bnhip_clip_export* x,
                bnhip_clip_span* spans) {
    for (size_t i = 0; i < n_events; i++)
        if (events[i].recording < 0 || events[i].recording >= n_recordings)
            return set_err(BNHIP_E_INVALID, "event " + std::to_string(i) + ": recording outside the table");
    for (size_t i = 0; i < n_events; i++) spans[i] = event_span(events[i], n_out[events[i].recording], hop, x);
    return BNHIP_OK;
}

// The clips of an export as a ClipSource (clip_source.h): cut by the call's Cutter, normalised into d_pcm (or cut straight into it),
// and encoded from there; the records and the FLAC streams come down in finish().
struct ExportSource : ClipSource {
    const char* what;
    int device, rate;
    const Cutter& cut;
    const CutPlan& plan;
    Clips clips;
    const bnhip_clip_export* x;
    bnhip_clips_out* o;
    size_t cap, res_bytes;
    size_t o_tab = 0, o_cut = 0, o_res = 0, o_lws = 0, o_bytes = 0, o_off = 0, o_fws = 0;
    int rc = 0;                              // the normalise's own refusal, with its text: what the entry answers instead of a HIP error
    std::string err;
    ExportSource(const char* w, int dev, const Cutter& ct, const CutPlan& p, int r, const bnhip_clip_export* xx, bnhip_clips_out* oo)
        : what(w), device(dev), rate(r), cut(ct), plan(p), clips(Clips::ragged(p.n_clips(), p.lens.data())), x(xx),
          o(oo), cap(flac_max_bytes(clips, xx->seek_interval)), res_bytes((size_t)p.n_clips() * sizeof(bnhip_loudness)) {}
    void reserve(DevCarve& cv) override {
        o_tab = cv.add(cut.table_bytes(plan));
        if (x->normalize) {
            o_cut = cv.add((size_t)plan.total() * 2);
            o_res = cv.add(res_bytes);
            o_lws = cv.add(loudness_workspace_bytes(clips, loudness_sub_block(rate)));
        }
        o_bytes = cv.add(cap);
        o_off = cv.add(((size_t)clips.n_clips + 1) * 8);
        o_fws = cv.add(flac_workspace_bytes(clips, x->lpc_order));
    }
    hipError_t fill(const DevCarve& cv, int16_t* d_pcm, size_t) override {
        int16_t* d_cut = x->normalize ? cv.at<int16_t>(o_cut) : d_pcm;
        const hipError_t he = cut.enqueue(plan, cv.at<void>(o_tab), d_cut);
        if (he != hipSuccess) return he;
        if (x->normalize) {
            rc = loudness_enqueue(what, device, d_cut, clips, rate, x->target_lufs, x->true_peak_dbtp, x->max_gain_db, x->gate_fallback,
                                  cv.at<bnhip_loudness>(o_res), d_pcm, cv.at<void>(o_lws), nullptr);
            if (rc) { err = bnhip_last_error(); hipDeviceSynchronize(); return hipErrorUnknown; }
        }
        launch_flac(d_pcm, nullptr, flac_work(clips, rate, x->seek_interval, cv.at<void>(o_fws), x->lpc_order), cv.at<uint8_t>(o_bytes), cap,
                    cv.at<unsigned long long>(o_off), nullptr);
        return hipGetLastError();
    }
    hipError_t finish(const DevCarve& cv) override {
        hipError_t he = hipSuccess;
        if (x->normalize) he = hipMemcpy(o->loudness, cv.at<void>(o_res), res_bytes, hipMemcpyDeviceToHost);
        if (he == hipSuccess) he = fetch_streams(cv.at<unsigned long long>(o_off), cv.at<uint8_t>(o_bytes), clips.n_clips, o->flac_offsets, o->flac);
        return he;
    }
};

// an export without images: the source's parts and the clips in one DevCarve, its fill, its finish (whose first copy is the
// call's synchronise)
int audio_run(const char* what, int device, ExportSource& src) {
    const int rc = use_device(device);
    if (rc) return rc;
    const size_t pcm_bytes = (size_t)src.plan.total() * 2;
    DevCarve cv;
    const size_t o_pcm = cv.add(pcm_bytes);
    src.reserve(cv);
    DevBlocks b;
    cv.alloc(b);
    if (b.he == hipSuccess) b.he = src.fill(cv, cv.at<int16_t>(o_pcm), pcm_bytes);
    if (b.he == hipSuccess) b.he = src.finish(cv);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(what, b);
}

}  // namespace

namespace bnhip {

int clip_export_check(const bnhip_clip_export* x, const bnhip_clips_out* o, int model_rate) {
    if (!x || !o || !o->spans || !o->flac_offsets || (o->event_cap && !o->events) || (o->flac_cap && !o->flac) || (x->normalize && !o->loudness))
        return set_err(BNHIP_E_INVALID, "NULL argument");
    if (int rc = span_rule_check(x)) return rc;
    if (x->lpc_order < 0 || x->lpc_order > FLAC_MAX_LPC_ORDER) return set_err(BNHIP_E_INVALID, "lpc_order must be in [0, 8]");
    if (model_rate < 1 || model_rate > FLAC_MAX_RATE) return set_err(BNHIP_E_INVALID, "sample rate must be in [1, 1048575]");
    if (x->seek_interval < 0) return set_err(BNHIP_E_INVALID, "seek_interval must not be negative");
    if (x->normalize)
        if (int rc = loudness_args_check(Clips::uniform(1, 1), model_rate, x->target_lufs, x->true_peak_dbtp, x->max_gain_db)) return rc;
    if (x->width < 0) return set_err(BNHIP_E_INVALID, "width must be in [0, 4096]");
    if (x->width > 0) {
        if (!o->png_offsets || !x->palette || (o->png_cap && !o->png)) return set_err(BNHIP_E_INVALID, "NULL argument");
        if (x->rate_out < 0) return set_err(BNHIP_E_INVALID, "sample rates must be positive");
        if (int rc = png_args_check(1, x->width, x->height)) return rc;
        const int N = spectrogram_image_check(x->width, x->height, x->window, x->top_db, x->range_db);
        if (N < 0) return N;
    }
    return BNHIP_OK;
}

int clip_export_spans(const char* what, int device, const Cutter& cut, size_t n_spans, int rate, const bnhip_clip_export* x, bnhip_clips_out* o) {
    o->n_clips = 0;
    // the capacity rule: clips in span order for as long as their streams' bounds fit what the caller has room for
    int n = 0;
    size_t flac_need = 0;
    for (size_t i = 0; i < n_spans && n < 65535; i++) {
        if (o->spans[i].length < 1) continue;
        flac_need += flac_max_bytes(1, o->spans[i].length, x->seek_interval);
        if (flac_need > o->flac_cap) break;
        if (x->width > 0 && png_max_bytes(n + 1, x->width, x->height) > o->png_cap) break;
        n++;
    }
    if (n == 0) return BNHIP_OK;
    const CutPlan plan = cut_plan(o->spans, n_spans, n);
    ExportSource src(what, device, cut, plan, rate, x, o);
    if (int rc = clips_check(src.clips)) return rc;
    const int rc = x->width > 0 ? spectrogram_png_run(what, device, src, src.clips, rate, x->rate_out, x->width, x->height, x->window, x->top_db,
                                                      x->range_db, x->palette, o->png, o->png_cap, o->png_offsets)
                                : audio_run(what, device, src);
    if (src.rc) return set_err(src.rc, src.err);
    if (rc == BNHIP_OK) o->n_clips = (size_t)n;
    return rc;
}

int clip_export_run(int device, const void* d_block, int bits, const long long* d_slot, const int64_t* n_out, int n_recordings, int hop,
                    int model_rate, const bnhip_clip_export* x, bnhip_clips_out* o) {
    const size_t n_written = std::min(o->event_cap, o->n_events);
    o->n_clips = 0;
    if (int rc = event_spans(o->events, n_written, n_out, n_recordings, hop, x, o->spans)) return rc;
    return clip_export_spans("analyze_channels_pcm_clips", device, SlotCutter(d_block, bits, d_slot), n_written, model_rate, x, o);
}

}  // namespace bnhip

extern "C" {

int bnhip_event_clip_spans(const bnhip_event* events, size_t n_events, const int64_t* resampled_length, int n_recordings, int hop,
                           const bnhip_clip_export* x, bnhip_clip_span* spans) {
    BN_GUARD_BEGIN
    if (!resampled_length || !x || (n_events && (!events || !spans))) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_recordings < 1) return set_err(BNHIP_E_INVALID, "n_recordings must be at least 1");
    if (hop < 1) return set_err(BNHIP_E_INVALID, "hop must be at least 1");
    if (int rc = span_rule_check(x)) return rc;
    return event_spans(events, n_events, resampled_length, n_recordings, hop, x, spans);
    BN_GUARD_END((void)0)
}

// the cut alone: one DevCarve (the recordings' parts, the slot table, the cut's tables, the clips), the upload, the cut, one D2H copy
int bnhip_recording_clips_pcm16(int device, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate,
                                const bnhip_clip_span* spans, int n_spans, int16_t* out_pcm) {
    BN_GUARD_BEGIN
    const char* what = "recording_clips_pcm16";
    if (!pcm || !spans || !out_pcm) return set_err(BNHIP_E_INVALID, "NULL argument");
    Recordings rec;
    if (int rc = describe(recs, n_recordings, model_rate, &rec)) return rc;
    if (n_spans < 1 || n_spans > 65535) return set_err(BNHIP_E_INVALID, "n_spans must be in [1, 65535]");
    long long total = 0;
    for (int i = 0; i < n_spans; i++) {
        const bnhip_clip_span& q = spans[i];
        const std::string who = "span " + std::to_string(i) + ": ";
        if (q.recording < 0 || q.recording >= n_recordings) return set_err(BNHIP_E_INVALID, who + "recording outside the table");
        if (q.length < 0) return set_err(BNHIP_E_INVALID, who + "negative length");
        if (q.start < 0 || q.start > rec.n_out[q.recording] - q.length) return set_err(BNHIP_E_INVALID, who + "outside its recording");
        total += q.length;
    }
    if (total > RAGGED_MAX_SAMPLES) return set_err(BNHIP_E_INVALID, "the clips' total length must be below 2^36 samples");
    if (int rc = rate_plans(&rec)) return rc;
    const CutPlan plan = cut_plan(spans, (size_t)n_spans, n_spans);
    if (plan.n_clips() == 0) return BNHIP_OK;
    std::vector<long long> slot((size_t)n_recordings * 2);
    const SlotPlan sp = slot_plan(rec, slot.data());
    if (int rc = use_device(device)) return rc;
    DevCarve cv;
    const SlotDev dv = slot_reserve(sp, cv);
    const size_t o_slot = cv.add(slot.size() * 8), o_tab = cv.add(plan.table_bytes()), o_out = cv.add((size_t)total * 2);
    DevBlocks b;
    cv.alloc(b);
    if (b.he != hipSuccess) return hip_fail(what, b);
    slot_upload(sp, pcm, rec, slot.data(), device, dv, nullptr, b);
    AN_HIP(b, hipMemcpyAsync(cv.at<void>(o_slot), slot.data(), slot.size() * 8, hipMemcpyHostToDevice, nullptr));
    AN_HIP(b, cut_enqueue(plan, dv.at(dv.block), rec.bits, cv.at<long long>(o_slot), cv.at<void>(o_tab), cv.at<int16_t>(o_out), nullptr));
    // (the null stream orders the copy after the kernels; it is the call's synchronise)
    AN_HIP(b, hipMemcpy(out_pcm, cv.at<void>(o_out), (size_t)total * 2, hipMemcpyDeviceToHost));
    if (b.he != hipSuccess) { hipDeviceSynchronize(); return hip_fail(what, b); }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

}  // extern "C"
