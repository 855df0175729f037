// C ABI of the audio level bank (levels.h; include/bnhip.h, "Audio level bank"), the level rule itself (bnhip_audio_level, host
// only) and the capture write that also measures (bnhip_capture_bank_write_levels).
//
// A call is one transaction, as every bank call of stream_bank.h: check everything, stage the tables, the zeroed records and the
// frames (each at a 16-byte line), one H2D copy, one launch, one D2H copy of the integer records, one synchronise, then the commit.
// The commit is host work: the level of every frame by the rule, then `latest` and the accumulators per stream in call order, as
// AudioLevelStats.Record does (internal/analysis/audio_level_stats.go:42-73).  The bank keeps nothing on the device but its
// staging, so a failed call changes nothing.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "capture_bank.h"
#include "levels.h"
#include "stream_bank.h"

using namespace bnhip;

struct LevelStream {
    bool measured = false;
    bnhip_audio_level_data latest = {};
    int64_t sum = 0, count = 0, zero_count = 0, clip_count = 0;     // audioLevelAccum
    int32_t min = 0, max = 0;
};

struct bnhip_level_bank : StreamBank<LevelStream, LevelRecord> {
    static constexpr const char* what = "level bank";
};

namespace bnhip {

int audio_level(uint64_t sum_squares, int64_t n_samples, bool clipping) {
    if (n_samples <= 0) return 0;                                       // buffer_consumer.go:275-277, 290-292
    const double rms = std::sqrt((double)sum_squares / (double)n_samples);
    const double db = 20 * std::log10(rms / 32768.0);
    double scaled = (db - (-60.0)) * (100.0 / 50.0);
    if (clipping) scaled = std::fmax(scaled, 95.0);
    if (scaled < 0) scaled = 0;                                         // (silence: -Inf)
    else if (scaled > 100) scaled = 100;
    return (int)scaled;
}

}  // namespace bnhip

namespace {

int level_fail(const char* what, hipError_t he) {
    (void)hipGetLastError();
    return set_err(he == hipErrorOutOfMemory ? BNHIP_E_NOMEM : BNHIP_E_RUNTIME, std::string(what) + ": " + hipGetErrorString(he));
}

// The measured frames of a call, checked and laid out: frame f of the call (streams[f] >= 0) is record k = rec_of[f].
struct LevelPlan {
    std::vector<int> rec_of;                      // [n_frames], -1: not measured
    std::vector<int64_t> at;                      // [n_frames]: the byte of the staged PCM the frame begins at
    std::vector<LevelFrame> frames;               // [measured]
    std::vector<long long> tile0;                 // [measured + 1]
    size_t pcm_bytes = 0;
    size_t table_bytes() const { return frames.size() * (sizeof(LevelFrame) + sizeof(LevelRecord)) + tile0.size() * 8; }
};

// what process and the fused write check of the level bank's side before any device call (under its lock); skip: streams[f] == -1
// is a frame that is staged but not measured.  Every frame is staged whole at a level_frame_align(bits) boundary.
int level_plan(const bnhip_level_bank* b, int n_frames, const int32_t* streams, const int64_t* n_samples, const void* const* frames, int bits,
               bool skip, LevelPlan* p) {
    const size_t bytes = (size_t)bits / 8, align = level_frame_align(bits);
    p->rec_of.assign((size_t)n_frames, -1);
    p->at.assign((size_t)n_frames, 0);
    p->tile0.assign(1, 0);
    int64_t given = 0;
    for (int f = 0; f < n_frames; f++) {
        const std::string who = "frame " + std::to_string(f) + ": ";
        const bool measured = !(skip && streams[f] == -1);
        if (measured)
            if (int rc = bank_stream_check(b, streams[f])) return rc;
        if (n_samples[f] < 0) return set_err(BNHIP_E_INVALID, who + "negative frame length");
        if (n_samples[f] > 0 && !frames[f]) return set_err(BNHIP_E_INVALID, who + "frame pointer is NULL");
        if (measured && n_samples[f] > LEVEL_MAX_FRAME) return set_err(BNHIP_E_INVALID, who + "a measured frame holds at most 2^23 samples");
        if (n_samples[f] > RAGGED_MAX_SAMPLES - given) return set_err(BNHIP_E_INVALID, "the frames' total length must be below 2^36 samples");
        given += n_samples[f];
        p->at[(size_t)f] = (int64_t)p->pcm_bytes;
        p->pcm_bytes = (p->pcm_bytes + (size_t)n_samples[f] * bytes + align - 1) / align * align;
        if (!measured) continue;
        p->rec_of[(size_t)f] = (int)p->frames.size();
        p->frames.push_back(LevelFrame{(long long)p->at[(size_t)f], (long long)n_samples[f]});
        p->tile0.push_back(p->tile0.back() + level_tiles(n_samples[f], bits));
    }
    if (p->tile0.back() > INT_MAX) return set_err(BNHIP_E_INVALID, "the measured frames must fit 2^31 - 1 tiles");
    return BNHIP_OK;
}

// the plan's tables at `stage` (8-byte aligned): frames | tile prefix | zeroed records; -> the records' offset from `stage`
size_t level_stage_tables(const LevelPlan& p, uint8_t* stage) {
    const size_t o_tile = p.frames.size() * sizeof(LevelFrame), o_rec = o_tile + p.tile0.size() * 8;
    memcpy(stage, p.frames.data(), o_tile);
    memcpy(stage + o_tile, p.tile0.data(), p.tile0.size() * 8);
    memset(stage + o_rec, 0, p.frames.size() * sizeof(LevelRecord));
    return o_rec;
}

void level_stage_frames(const LevelPlan& p, int n_frames, const int64_t* n_samples, const void* const* frames, size_t bytes, uint8_t* pcm) {
    for (int f = 0; f < n_frames; f++)
        if (n_samples[f] > 0) memcpy(pcm + p.at[(size_t)f], frames[f], (size_t)n_samples[f] * bytes);
}

// the level launch over tables staged by level_stage_tables at d_tables, the PCM at d_pcm
void level_launch(const LevelPlan& p, const char* d_tables, const char* d_pcm, int bits, hipStream_t s) {
    const size_t o_tile = p.frames.size() * sizeof(LevelFrame), o_rec = o_tile + p.tile0.size() * 8;
    launch_frame_levels(d_pcm, (long long)p.pcm_bytes, bits, reinterpret_cast<const LevelFrame*>(d_tables),
                        reinterpret_cast<const long long*>(d_tables + o_tile), (int)p.frames.size(), p.tile0.back(),
                        reinterpret_cast<LevelRecord*>(const_cast<char*>(d_tables + o_rec)), s);
}

// The commit: everything before succeeded.  rec: the device's records, [measured].  levels[f] for every frame of the call; a
// frame that was not measured answers stream -1 and changes nothing.
void level_commit(bnhip_level_bank* b, const LevelPlan& p, int n_frames, const int32_t* streams, const int64_t* n_samples, const LevelRecord* rec,
                  bnhip_audio_level_data* levels) {
    for (int f = 0; f < n_frames; f++) {
        bnhip_audio_level_data& L = levels[f];
        memset(&L, 0, sizeof L);
        L.stream = -1; L.frame = f;
        const int k = p.rec_of[(size_t)f];
        if (k < 0) continue;
        L.stream = streams[f];
        L.n_samples = n_samples[f];
        L.sum_squares = rec[k].sum_squares;
        L.clipped_samples = (int64_t)rec[k].clipped_samples;
        L.clipping = rec[k].clipped_samples != 0;
        L.level = audio_level(L.sum_squares, L.n_samples, L.clipping != 0);
        LevelStream& S = b->st[(size_t)L.stream];
        S.latest = L;
        S.measured = true;
        if (S.count == 0) { S.min = S.max = L.level; }                  // (audio_level_stats.go:52-63)
        else { S.min = std::min(S.min, L.level); S.max = std::max(S.max, L.level); }
        S.sum += L.level;
        S.count++;
        if (L.level == 0) S.zero_count++;
        if (L.clipping) S.clip_count++;
    }
}

void level_stats_clear(LevelStream& S) { S.sum = S.count = S.zero_count = S.clip_count = 0; S.min = S.max = 0; }

int bits_check(int bits) {
    if (bits != 16 && bits != 24 && bits != 32) return set_err(BNHIP_E_INVALID, "bits_per_sample must be 16, 24 or 32");
    return BNHIP_OK;
}

}  // namespace

extern "C" {

int bnhip_audio_level(uint64_t sum_squares, int64_t n_samples, int clipping, int* level) {
    if (!level) return set_err(BNHIP_E_INVALID, "level is NULL");
    if (n_samples < 0 || n_samples > LEVEL_MAX_FRAME) return set_err(BNHIP_E_INVALID, "n_samples must be in [0, 2^23]");
    *level = audio_level(sum_squares, n_samples, clipping != 0);
    return BNHIP_OK;
}

int bnhip_level_bank_create(int device, int max_streams, bnhip_level_bank** out) {
    if (!out) return set_err(BNHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (max_streams < 1 || max_streams > 65535) return set_err(BNHIP_E_INVALID, "max_streams must be in [1, 65535]");
    BN_GUARD_BEGIN
    if (int rc = use_device(device)) return rc;
    return bank_create(device, max_streams, out, [](bnhip_level_bank&) { return hipSuccess; });
    BN_GUARD_END((void)0)
}

int bnhip_level_bank_add_stream(bnhip_level_bank* b, int* out_stream) { return bank_add_stream(b, out_stream); }

int bnhip_level_bank_remove_stream(bnhip_level_bank* b, int stream) { return bank_remove_stream(b, stream); }

int bnhip_level_bank_process_pcm(bnhip_level_bank* b, int n_frames, const int32_t* streams, const int64_t* n_samples, const void* const* frames,
                                 int bits_per_sample, bnhip_audio_level_data* levels) {
    if (!b || (n_frames > 0 && (!streams || !n_samples || !frames || !levels))) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_frames < 0) return set_err(BNHIP_E_INVALID, "n_frames is negative");
    if (int rc = bits_check(bits_per_sample)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    LevelPlan plan;
    if (int rc = level_plan(b, n_frames, streams, n_samples, frames, bits_per_sample, false, &plan)) return rc;
    if (n_frames == 0) return BNHIP_OK;
    const LevelRecord* rec = nullptr;
    if (plan.tile0.back() > 0) {
        // ---- stage: tables | pad to a 16-byte line | frames
        hipSetDevice(b->device);
        const size_t o_pcm = (plan.table_bytes() + 15) / 16 * 16, stage_bytes = o_pcm + plan.pcm_bytes;
        if (!bank_grow((void**)&b->h_stage, &b->d_stage, &b->stage_cap, stage_bytes))
            return set_err(BNHIP_E_NOMEM, std::string("allocation failed (") + b->what + " staging)");
        const size_t o_rec = level_stage_tables(plan, b->h_stage), rec_bytes = plan.frames.size() * sizeof(LevelRecord);
        level_stage_frames(plan, n_frames, n_samples, frames, (size_t)bits_per_sample / 8, b->h_stage + o_pcm);
        // ---- run
        const char* ds = static_cast<const char*>(b->d_stage);
        hipError_t he = hipMemcpyAsync(b->d_stage, b->h_stage, stage_bytes, hipMemcpyHostToDevice, b->stream);
        if (he == hipSuccess) {
            level_launch(plan, ds, ds + o_pcm, bits_per_sample, b->stream);
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipMemcpyAsync(b->h_stage + o_rec, ds + o_rec, rec_bytes, hipMemcpyDeviceToHost, b->stream);
        const hipError_t hs = hipStreamSynchronize(b->stream);
        if (he == hipSuccess) he = hs;
        if (he != hipSuccess) return level_fail(b->what, he);
        rec = reinterpret_cast<const LevelRecord*>(b->h_stage + o_rec);
    }
    // ---- commit (a call of empty frames alone ran nothing: its records are zero)
    const std::vector<LevelRecord> zero(rec ? 0 : plan.frames.size(), LevelRecord{0, 0});
    level_commit(b, plan, n_frames, streams, n_samples, rec ? rec : zero.data(), levels);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_level_bank_latest(bnhip_level_bank* b, bnhip_audio_level_data* out) {
    if (!b || !out) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    for (size_t s = 0; s < b->st.size(); s++) {
        const auto& S = b->st[s];
        if (S.live && S.measured) { out[s] = S.latest; continue; }
        memset(&out[s], 0, sizeof out[s]);
        out[s].stream = -1;
    }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_level_bank_stats(bnhip_level_bank* b, int stream, int reset, bnhip_audio_level_stats* out) {
    if (!b || !out) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (int rc = bank_stream_check(b, stream)) return rc;
    LevelStream& S = b->st[(size_t)stream];
    memset(out, 0, sizeof *out);
    out->sum = S.sum; out->count = S.count; out->zero_count = S.zero_count; out->clip_count = S.clip_count;
    out->min = S.min; out->max = S.max;
    if (S.count > 0) {                                                  // audio_level_stats.go:114-120
        out->avg_level = (int32_t)(S.sum / S.count);
        out->zero_pct = (int32_t)(S.zero_count * 100 / S.count);
        out->clipping_pct = (int32_t)(S.clip_count * 100 / S.count);
    }
    if (reset) level_stats_clear(S);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_level_bank_reset(bnhip_level_bank* b, int stream) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (stream != -1)
        if (int rc = bank_stream_check(b, stream)) return rc;
    for (size_t s = 0; s < b->st.size(); s++) {
        auto& S = b->st[s];
        if (!S.live || (stream != -1 && (size_t)stream != s)) continue;
        S.measured = false;
        S.latest = bnhip_audio_level_data{};
        level_stats_clear(S);
    }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

void bnhip_level_bank_destroy(bnhip_level_bank* b) {
    try { bank_free(b); } catch (...) {}
}

// bnhip_capture_bank_write with the frames also measured where the upload has put them: the capture bank's stream and staging,
// both banks' checks first, both commits last.  The locks are taken capture bank first, then level bank, here and nowhere else.
int bnhip_capture_bank_write_levels(bnhip_capture_bank* cb, bnhip_level_bank* lb, int n_frames, const int32_t* sources, const int32_t* level_streams,
                                    const int64_t* n_samples, const void* const* frames, int bits_per_sample, bnhip_audio_level_data* levels) {
    const char* what = "capture bank (write with levels)";
    if (!cb || !lb || (n_frames > 0 && (!sources || !level_streams || !n_samples || !frames || !levels))) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_frames < 0) return set_err(BNHIP_E_INVALID, "n_frames is negative");
    if (int rc = bits_check(bits_per_sample)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lc(cb->mu);
    std::lock_guard<std::mutex> ll(lb->mu);
    if (cb->device != lb->device) return set_err(BNHIP_E_INVALID, "the capture bank and the level bank are on different devices");
    const size_t bytes = (size_t)bits_per_sample / 8;
    // ---- both banks' checks and plans; the pieces' src follow the whole-frame layout
    LevelPlan lp;
    if (int rc = level_plan(lb, n_frames, level_streams, n_samples, frames, bits_per_sample, true, &lp)) return rc;
    std::vector<int64_t> frame_at((size_t)n_frames);
    for (int f = 0; f < n_frames; f++) frame_at[(size_t)f] = lp.at[(size_t)f] / (int64_t)bytes;
    CapturePlan cp;
    if (int rc = capture_plan(cb, n_frames, sources, n_samples, frames, frame_at.data(), &cp)) return rc;
    if (n_frames == 0) return BNHIP_OK;
    const LevelRecord* rec = nullptr;
    const std::vector<LevelRecord> zero(lp.frames.size(), LevelRecord{0, 0});
    if (!cp.pieces.empty() || lp.tile0.back() > 0) {
        // ---- stage: pieces | their tile prefix | the level tables | pad to a 16-byte line | whole frames
        hipSetDevice(cb->device);
        const size_t o_tile = cp.pieces.size() * sizeof(CapPiece), o_lvl = o_tile + cp.tile0.size() * 8;
        const size_t o_pcm = (o_lvl + lp.table_bytes() + 15) / 16 * 16, stage_bytes = o_pcm + lp.pcm_bytes;
        if (!bank_grow((void**)&cb->h_stage, &cb->d_stage, &cb->stage_cap, stage_bytes))
            return set_err(BNHIP_E_NOMEM, std::string("allocation failed (") + what + " staging)");
        memcpy(cb->h_stage, cp.pieces.data(), o_tile);
        memcpy(cb->h_stage + o_tile, cp.tile0.data(), cp.tile0.size() * 8);
        const size_t o_rec = o_lvl + level_stage_tables(lp, cb->h_stage + o_lvl), rec_bytes = lp.frames.size() * sizeof(LevelRecord);
        level_stage_frames(lp, n_frames, n_samples, frames, bytes, cb->h_stage + o_pcm);
        // ---- run
        const char* ds = static_cast<const char*>(cb->d_stage);
        hipError_t he = hipMemcpyAsync(cb->d_stage, cb->h_stage, stage_bytes, hipMemcpyHostToDevice, cb->stream);
        bool launched = false;
        if (he == hipSuccess) {
            launch_capture_write(ds + o_pcm, (long long)(lp.pcm_bytes / bytes), bits_per_sample, reinterpret_cast<const CapPiece*>(ds),
                                 reinterpret_cast<const long long*>(ds + o_tile), (int)cp.pieces.size(), cp.tile0.back(), cb->d_rings,
                                 (long long)cb->max_sources * cb->capacity, cb->stream);
            launched = !cp.pieces.empty();
            level_launch(lp, ds + o_lvl, ds + o_pcm, bits_per_sample, cb->stream);
            he = hipGetLastError();
        }
        if (he == hipSuccess && rec_bytes) he = hipMemcpyAsync(cb->h_stage + o_rec, ds + o_rec, rec_bytes, hipMemcpyDeviceToHost, cb->stream);
        const hipError_t hs = hipStreamSynchronize(cb->stream);
        if (he == hipSuccess) he = hs;
        if (he != hipSuccess) {
            if (launched) capture_write_failed(cb, cp);                 // the capture bank's rule; the level bank is unchanged
            return level_fail(what, he);
        }
        rec = reinterpret_cast<const LevelRecord*>(cb->h_stage + o_rec);
    }
    // ---- both commits
    capture_write_commit(cb, cp);
    level_commit(lb, lp, n_frames, level_streams, n_samples, rec ? rec : zero.data(), levels);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

}  // extern "C"
