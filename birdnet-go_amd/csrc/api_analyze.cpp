// C ABI of file analysis: whole recordings in, the top-k of every overlapping window (or the detection rows above a threshold) out,
// in one call - the windows are framed on the device (analyze.h).  Recordings at their own rates and depths are resampled and
// converted there too (resample.h, the slot launch), and multichannel recordings go up interleaved: a channel is picked or the
// channels are mixed in that launch, where asked after a measurement of the channels' energies on the device (channels.h).
// Any of the calls can end in detection events instead of rows: the rows stay on the device and the reference's result post-filters run
// there as the call's tail (events.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "analyze.h"
#include "api_model.h"
#include "api_oneshot.h"
#include "channels.h"
#include "clips.h"
#include "events.h"
#include "resample.h"

using namespace bnhip;

static_assert(sizeof(bnhip_detection) == 16 && sizeof(DetRow) == 16, "a detection row is 16 bytes");
static_assert(sizeof(bnhip_event) == 32 && sizeof(Event) == 32, "an event is 32 bytes");
static_assert(BNHIP_EVENTS_KEEP_DROPPED == EVENTS_KEEP_DROPPED, "the flag of events.h");
static_assert(sizeof(bnhip_recording) == 16, "a recording's description is 16 bytes");
static_assert(sizeof(bnhip_channels_recording) == 24, "a multichannel recording's description is 24 bytes");
static_assert(sizeof(bnhip_channel_energy) == 24, "a channel's energy record is 24 bytes");
static_assert(BNHIP_CHANNEL_MIX == CHANNEL_MIX && BNHIP_CHANNEL_AUTO == CHANNEL_AUTO, "the selection constants of channels.h");

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
constexpr long long ANALYZE_MAX_SAMPLES = (1ll << 36) - 1;

// the table arguments of all three entries; n_samples is the window (the model's clip)
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

// ---- recordings at their own rates and depths (the bnhip_analyze_mixed_* entries)
// What the mixed entries add to a call: the recordings as they are in their files (the raw block), resampled and converted on the
// device into the float32 slots that the chunk loop frames - `lengths` of analyze() are then the n_out, at the model's rate.
struct RatePlan { int rate; int rec; ResamplePlan p; size_t tab_off; };     // rec: the first recording at that rate (for error texts)
struct Mixed {
    const bnhip_recording* recs = nullptr;
    int model_rate = 0;
    std::vector<int64_t> n_out;                   // [n_rec] samples at the model's rate
    std::vector<RatePlan> plans;                  // the distinct rates that differ from the model's, ascending
    std::vector<int> plan_of;                     // [n_rec] index into plans, -1: at the model's rate
    long long n_tiles = 0;
    bool plain = false;                           // every recording at the model's rate, one depth: the existing body as it is
    // the channels entries, where a recording has two channels or more (else empty: the call is the mixed one): [n_rec] each; a
    // recording's `length` then counts frames.  select: a channel, CHANNEL_MIX or CHANNEL_AUTO (channels.h)
    std::vector<int> channels, select;
    std::vector<int32_t> chosen;                  // [n_rec], filled by analyze(): what was read
    int ch(int r) const { return channels.empty() ? 1 : channels[r]; }
};

// The phase tables of one set of rates, concatenated in one device buffer and kept (api_oneshot.h): a second call with the same
// rates designs and uploads nothing.
struct RateSetTable {
    int device, model_rate;
    std::vector<int> rates;                       // ascending; their [L][T] tables follow one another in d
    float* d;
};
TableCache<RateSetTable> g_rate_tables;

constexpr long long MIXED_MAX_LEN = (1ll << 31) - 1;

// the recordings of a mixed call: every refusal that needs neither the handle nor a device; fills mx
int mixed_check(const bnhip_recording* recs, int n_recordings, int model_rate, Mixed* mx) {
    if (!recs) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_recordings < 1 || n_recordings > 65535) return set_err(BNHIP_E_INVALID, "n_recordings must be in [1, 65535]");
    if (model_rate <= 0) return set_err(BNHIP_E_INVALID, "model_rate must be positive");
    mx->recs = recs; mx->model_rate = model_rate;
    mx->n_out.resize(n_recordings); mx->plan_of.assign(n_recordings, -1);
    long long total_in = 0, total_out = 0;
    bool plain = true;
    for (int r = 0; r < n_recordings; r++) {
        const bnhip_recording& q = recs[r];
        const std::string who = "recording " + std::to_string(r) + ": ";
        if (q.bits_per_sample != 0 && q.bits_per_sample != 16 && q.bits_per_sample != 24 && q.bits_per_sample != 32)
            return set_err(BNHIP_E_INVALID, who + "unsupported bit depth: " + std::to_string(q.bits_per_sample) + " (supported: 0 = float32, 16, 24, 32)");
        if (q.rate <= 0) return set_err(BNHIP_E_INVALID, who + "the sample rate must be positive");
        if (q.length < 1) return set_err(BNHIP_E_INVALID, "every recording needs at least one sample");
        if (q.length > MIXED_MAX_LEN) return set_err(BNHIP_E_INVALID, who + "2^31 samples or more");
        // ceil(length * L / M) in 64 bits (bnhip_resample_length): length < 2^31 and L < 2^31
        const long long no = q.rate == model_rate ? (long long)q.length : resample_plan(q.rate, model_rate, nullptr).end(q.length);
        if (no > MIXED_MAX_LEN) return set_err(BNHIP_E_INVALID, who + "2^31 samples or more at the model's rate");
        if (q.length > ANALYZE_MAX_SAMPLES - total_in || no > ANALYZE_MAX_SAMPLES - total_out)
            return set_err(BNHIP_E_INVALID, "burst of 2^36 samples or more");
        total_in += q.length; total_out += no;
        mx->n_out[r] = no;
        mx->n_tiles += resample_slot_tiles(no);
        plain = plain && q.rate == model_rate && q.bits_per_sample == recs[0].bits_per_sample;
    }
    if (mx->n_tiles > INT_MAX) return set_err(BNHIP_E_INVALID, "more resample tiles than a 31-bit grid");
    mx->plain = plain;
    if (plain) return BNHIP_OK;
    std::vector<int> rates;
    for (int r = 0; r < n_recordings; r++) if (recs[r].rate != model_rate) rates.push_back(recs[r].rate);
    std::sort(rates.begin(), rates.end());
    rates.erase(std::unique(rates.begin(), rates.end()), rates.end());
    for (int rate : rates) mx->plans.push_back(RatePlan{rate, -1, ResamplePlan{}, 0});
    for (int r = 0; r < n_recordings; r++) {
        if (recs[r].rate == model_rate) continue;
        const int pi = (int)(std::lower_bound(rates.begin(), rates.end(), recs[r].rate) - rates.begin());
        mx->plan_of[r] = pi;
        if (mx->plans[pi].rec < 0) mx->plans[pi].rec = r;
    }
    return BNHIP_OK;
}

// the geometry of every rate of the call; a phase table that does not fit LDS is refused here, before any allocation
int mixed_plans(Mixed* mx) {
    size_t off = 0;
    for (RatePlan& rp : mx->plans) {
        rp.p = resample_plan(rp.rate, mx->model_rate, nullptr);
        if (!rp.p.fits_lds())
            return set_err(BNHIP_E_UNSUPPORTED, "recording " + std::to_string(rp.rec) + ": resampling " + std::to_string(rp.rate) + " Hz to " +
                                                    std::to_string(mx->model_rate) + " Hz needs a phase table larger than LDS");
        rp.tab_off = off;
        off += (size_t)rp.p.L * rp.p.T;
    }
    // (a descriptor states a table's offset in an int: tens of thousands of distinct rates with tables near the LDS limit)
    if (off > (size_t)INT_MAX) return set_err(BNHIP_E_UNSUPPORTED, "the call's phase tables exceed 2^31 floats");
    return BNHIP_OK;
}

// the call's concatenated phase tables on the current device, from the cache or designed now; -> NULL: the upload failed
const float* mixed_tables(const Mixed& mx, int device, const TableLock& lock) {
    std::vector<int> rates;
    for (const RatePlan& rp : mx.plans) rates.push_back(rp.rate);
    const RateSetTable* t = g_rate_tables.find(
        lock, [&](const RateSetTable& e) { return e.device == device && e.model_rate == mx.model_rate && e.rates == rates; },
        [&](RateSetTable& e) {
            std::vector<float> all, one;
            for (const RatePlan& rp : mx.plans) {
                (void)resample_plan(rp.rate, mx.model_rate, &one);
                all.insert(all.end(), one.begin(), one.end());
            }
            e.device = device; e.model_rate = mx.model_rate; e.rates = rates;
            e.d = upload_table(all);
            return e.d != nullptr;
        });
    return t ? t->d : nullptr;
}

// ---- multichannel recordings (the bnhip_analyze_channels_* entries, bnhip_channel_energy_pcm)
// The recordings of a channels call as the mixed call sees them (base: length in frames, rate, depth), and what the channels add.
struct Channels {
    std::vector<bnhip_recording> base;
    std::vector<int> channels, select;
    bool multi = false;                           // a recording has two channels or more
};

// every refusal of the channel fields, and of the burst's size in samples; fills ch.  (What the mixed call refuses of base - the
// depths, rates and lengths - is mixed_check's to answer; measure: the measurement entry, where a float32 recording is refused
// whatever its select)
int channels_check(const bnhip_channels_recording* recs, int n_recordings, bool measure, Channels* ch) {
    if (!recs) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_recordings < 1 || n_recordings > 65535) return set_err(BNHIP_E_INVALID, "n_recordings must be in [1, 65535]");
    ch->base.resize(n_recordings); ch->channels.resize(n_recordings); ch->select.resize(n_recordings);
    long long total = 0;
    for (int r = 0; r < n_recordings; r++) {
        const bnhip_channels_recording& q = recs[r];
        const std::string who = "recording " + std::to_string(r) + ": ";
        if (q.channels < 1 || q.channels > CHANNELS_MAX) return set_err(BNHIP_E_INVALID, who + "channels must be in [1, 16]");
        if (q.select < CHANNEL_AUTO || q.select >= q.channels)
            return set_err(BNHIP_E_INVALID, who + "select must be a channel index, BNHIP_CHANNEL_MIX or BNHIP_CHANNEL_AUTO");
        if ((measure || q.select == CHANNEL_AUTO) && q.bits_per_sample == 0)
            return set_err(BNHIP_E_INVALID, who + "the channel energies are measured on integer depths; a float32 recording takes a channel or the mix");
        if (q.length >= 1 && q.length <= MIXED_MAX_LEN) {      // (else mixed_check refuses the length)
            if (q.length * q.channels > ANALYZE_MAX_SAMPLES - total) return set_err(BNHIP_E_INVALID, "burst of 2^36 samples or more");
            total += q.length * q.channels;
        }
        ch->base[r] = bnhip_recording{q.length, q.rate, q.bits_per_sample};
        ch->channels[r] = q.channels; ch->select[r] = q.select;
        ch->multi = ch->multi || q.channels > 1;
    }
    return BNHIP_OK;
}

// computeRmsDbfs (ffmpeg/analyze.go) from a channel's exact sum of squares, in 16-bit units: rms16 = sqrt(E / length) / 2^(bits - 16);
// below 1 the reference answers -96
double channel_rms_dbfs(unsigned long long lo, unsigned long long hi, int bits, long long length) {
    const double e = (double)hi * 18446744073709551616.0 + (double)lo;
    const double rms16 = std::sqrt(e / (double)length) / (double)(1ll << (bits - 16));
    return rms16 < 1.0 ? -96.0 : 20.0 * std::log10(rms16 / 32768.0);
}

// ---- detection events (the bnhip_*_events entries, bnhip_detection_events)
constexpr int EVENT_MAX_CLASSES = (int)(TOPK_LDS_MAX / 4);     // 38 400: with recording < 65 535 a (recording, class) key is below 2^32
constexpr unsigned long long EVENT_MAX_ROWS = 1ull << 31;

// what an events entry adds to its sibling's arguments: the filter and where the events go
struct EventsOut { const bnhip_event_filter* f; bnhip_event* out; };

// every refusal of the filter itself
int event_filter_check(const bnhip_event_filter* f) {
    if (!f || !f->class_threshold) return set_err(BNHIP_E_INVALID, "NULL event filter / class_threshold");
    if (f->hold_windows < 1) return set_err(BNHIP_E_INVALID, "hold_windows must be at least 1");
    if (f->min_count < 1) return set_err(BNHIP_E_INVALID, "min_count must be at least 1");
    if (f->flags & ~BNHIP_EVENTS_KEEP_DROPPED) return set_err(BNHIP_E_INVALID, "unknown event filter flags");
    return BNHIP_OK;
}

// bytes of the filter's tables on the device: class_threshold [n_classes], then class_veto [n_classes] where there is one
size_t event_tables_bytes(int n_classes) { return (size_t)n_classes * 4 + (size_t)n_classes; }

#define AN_HIP(call, what)                                                                         \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (ok && e_ != hipSuccess) { ok = false; err = std::string(what) + ": " + hipGetErrorString(e_); } \
    } while (0)

// ---- the recordings on the device (every device entry of this file)
// What a call's recordings need there, worked out on the host.  The slot block: recording r at slot[2 r] (analyze.h).
// mixed: the raw block (every recording as it is in its file, from a 16-byte line on), a descriptor per recording and the tile prefix
// channels: the raw block holds interleaved frames; beside the descriptors lie the channel counts and the selection table
// [n_rec] each, and the recordings that ask for a measurement have a descriptor and a tile prefix of their own (channels.h)
struct SlotPlan {
    size_t block_bytes = 0, raw_bytes = 0, rs_lds = 0;
    std::vector<ResampleSlotDesc> desc;
    std::vector<long long> tile0, etile0;
    std::vector<EnergyDesc> edesc;
    std::vector<int> chsel;
    bool mc = false;
    long long n_etiles = 0;
};
// bits / lengths state the slots (mixed: float32, the n_out); fills slot [n_rec][2]
SlotPlan slot_plan(const int64_t* lengths, int n_recordings, int bits, const Mixed* mx, long long* slot) {
    SlotPlan sp;
    for (int r = 0; r < n_recordings; r++) {
        slot[2 * r] = (long long)sp.block_bytes; slot[2 * r + 1] = lengths[r];
        sp.block_bytes += analyze_slot_bytes(lengths[r], bits);
    }
    sp.mc = mx && !mx->channels.empty();
    if (mx) {
        sp.desc.resize(n_recordings); sp.tile0.assign((size_t)n_recordings + 1, 0);
        for (int r = 0; r < n_recordings; r++) {
            const bnhip_recording& q = mx->recs[r];
            ResampleSlotDesc& ds = sp.desc[r];
            ds.in_off = (long long)sp.raw_bytes; ds.out_off = slot[2 * r];
            ds.n_in = (int)q.length; ds.n_out = (int)lengths[r]; ds.bits = q.bits_per_sample;
            ds.L = ds.M = ds.T = ds.half = ds.tab_off = 0;
            if (mx->plan_of[r] >= 0) {
                const RatePlan& rp = mx->plans[mx->plan_of[r]];
                ds.L = rp.p.L; ds.M = rp.p.M; ds.T = rp.p.T; ds.half = rp.p.half; ds.tab_off = (int)rp.tab_off;
                sp.rs_lds = std::max(sp.rs_lds, resample_lds(rp.p.L, rp.p.M, rp.p.T));
            }
            sp.raw_bytes += ((size_t)q.length * mx->ch(r) * analyze_sample_bytes(q.bits_per_sample) + 15) / 16 * 16;
            sp.tile0[r + 1] = sp.tile0[r] + resample_slot_tiles(lengths[r]);
        }
    }
    if (sp.mc) {
        sp.chsel.assign(mx->channels.begin(), mx->channels.end());
        sp.chsel.insert(sp.chsel.end(), mx->select.begin(), mx->select.end());
        sp.etile0.push_back(0);
        for (int r = 0; r < n_recordings; r++) {
            if (mx->select[r] != CHANNEL_AUTO) continue;
            sp.edesc.push_back(EnergyDesc{sp.desc[r].in_off, sp.desc[r].n_in, sp.desc[r].bits, mx->channels[r], r});
            sp.etile0.push_back(sp.etile0.back() + energy_tiles(sp.desc[r].n_in));
        }
    }
    sp.n_etiles = sp.edesc.empty() ? 0 : sp.etile0.back();
    return sp;
}

// where a call has carved the plan's parts: the slot block and its bytes up to the next part (zero-filled on the fast path), then
// (mixed) the raw block, the descriptors, the tile prefix, (channels) the counts and selections, the measurement's descriptors, tile
// prefix, partials and sums
struct SlotDev {
    char* block;
    size_t block_room;
    char *raw, *desc, *tile0, *chsel, *edesc, *etile0, *part, *energy;
};

// The recordings go up and the slot block is filled, on s: the slots' zero fill and one copy per recording into its slot, or
// (mixed) one copy per recording into the raw block, the tables, the measurement where a recording asks for one, and the slot
// launch (k_resample_slots writes every slot whole, its zeros included).  The first failure is left in ok / err.
void slot_upload(const SlotPlan& sp, const void* pcm, int bits, const int64_t* lengths, int n_recordings, const long long* slot, const Mixed* mx,
                 int device, const SlotDev& dv, hipStream_t s, bool& ok, std::string& err) {
    if (!mx) AN_HIP(hipMemsetAsync(dv.block, 0, dv.block_room, s), "memset");
    const char* src = static_cast<const char*>(pcm);
    for (int r = 0; ok && r < n_recordings; r++) {
        const size_t bytes = mx ? (size_t)mx->recs[r].length * mx->ch(r) * analyze_sample_bytes(mx->recs[r].bits_per_sample)
                                : (size_t)lengths[r] * analyze_sample_bytes(bits);
        AN_HIP(hipMemcpyAsync(mx ? dv.raw + sp.desc[r].in_off : dv.block + slot[2 * r], src, bytes, hipMemcpyHostToDevice, s), "H2D copy");
        src += bytes;
    }
    if (!mx) return;
    // (the lock is held from the tables' lookup until the launch that reads them is enqueued, api_oneshot.h)
    TableLock lock(g_rate_tables.mu);
    const float* d_tables = mx->plans.empty() ? nullptr : mixed_tables(*mx, device, lock);
    if (ok && !mx->plans.empty() && !d_tables) { ok = false; err = "phase table upload failed"; }
    AN_HIP(hipMemcpyAsync(dv.desc, sp.desc.data(), sp.desc.size() * sizeof(ResampleSlotDesc), hipMemcpyHostToDevice, s), "H2D copy");
    AN_HIP(hipMemcpyAsync(dv.tile0, sp.tile0.data(), sp.tile0.size() * 8, hipMemcpyHostToDevice, s), "H2D copy");
    const ResampleSlotDesc* d_desc = reinterpret_cast<const ResampleSlotDesc*>(dv.desc);
    const long long* d_tile0 = reinterpret_cast<const long long*>(dv.tile0);
    if (sp.mc) {
        // the selections go up as asked for; the measurement, if any recording asks for one, overwrites its entries on the
        // device, and the slot launch behind it reads them there
        int* d_ch = reinterpret_cast<int*>(dv.chsel);
        AN_HIP(hipMemcpyAsync(d_ch, sp.chsel.data(), sp.chsel.size() * 4, hipMemcpyHostToDevice, s), "H2D copy");
        if (!sp.edesc.empty()) {
            AN_HIP(hipMemcpyAsync(dv.edesc, sp.edesc.data(), sp.edesc.size() * sizeof(EnergyDesc), hipMemcpyHostToDevice, s), "H2D copy");
            AN_HIP(hipMemcpyAsync(dv.etile0, sp.etile0.data(), sp.etile0.size() * 8, hipMemcpyHostToDevice, s), "H2D copy");
            if (ok) launch_channel_energy(dv.raw, reinterpret_cast<const EnergyDesc*>(dv.edesc), reinterpret_cast<const long long*>(dv.etile0),
                                          (int)sp.edesc.size(), sp.n_etiles, reinterpret_cast<unsigned long long*>(dv.part),
                                          reinterpret_cast<unsigned long long*>(dv.energy), d_ch + n_recordings, s);
        }
        if (ok) launch_resample_slots_mc(dv.raw, dv.block, d_tables, d_desc, d_tile0, n_recordings, sp.tile0[n_recordings], sp.rs_lds, d_ch,
                                         d_ch + n_recordings, s);
    } else if (ok) {
        launch_resample_slots(dv.raw, dv.block, d_tables, d_desc, d_tile0, n_recordings, sp.tile0[n_recordings], sp.rs_lds, s);
    }
}

// what bnhip_analyze_channels_pcm_clips adds to its events call: the export settings and where everything goes (clips.h)
struct ClipsTail { const bnhip_clip_export* x; bnhip_clips_out* o; int model_rate; };

// bnhip_analyze_pcm_topk, and with `det` the detection rows behind it.  mx (the mixed entries): pcm holds the recordings as mx
// describes them, and bits / lengths state the float32 slots they are resampled into - what the chunk loop frames.  ct: with the
// events down and the recordings still in their slots, the clip export runs as the call's continuation.
int analyze(bnhip_model* m, const void* pcm, int bits, const int64_t* lengths, int n_recordings, int hop, int64_t min_tail, int activation,
            double sensitivity, int k, float* out_conf, int32_t* out_idx, bool det, float threshold, bnhip_detection* out_rows, size_t cap,
            size_t* n_out, Mixed* mx = nullptr, const EventsOut* ev = nullptr, const ClipsTail* ct = nullptr) {
    if (!m || !pcm || !lengths) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (det ? (!n_out || (cap && !(ev ? (const void*)ev->out : (const void*)out_rows))) : (!out_conf || !out_idx))
        return set_err(BNHIP_E_INVALID, "NULL argument");
    if (ev) if (int rc = event_filter_check(ev->f)) return rc;
    if (bits != 0 && bits != 16 && bits != 24 && bits != 32)
        return set_err(BNHIP_E_INVALID, "unsupported bit depth: " + std::to_string(bits) + " (supported: 0 = float32, 16, 24, 32)");
    if (k <= 0) return set_err(BNHIP_E_INVALID, "k must be positive");
    if (activation < 0 || activation > 2) return set_err(BNHIP_E_INVALID, "unknown activation");
    Engine& e = m->eng();
    if (int rc = check_table(lengths, n_recordings, e.n_samples, hop, min_tail)) return rc;
    if (ev) {                                     // (an argument error like the others: answered before the handle is looked at)
        std::vector<long long> len64(lengths, lengths + n_recordings), first((size_t)n_recordings + 1);
        const long long rows_max = analyze_windows(len64.data(), n_recordings, e.n_samples, hop, min_tail, first.data()) * std::min(k, e.n_classes);
        if ((unsigned long long)rows_max >= EVENT_MAX_ROWS) return set_err(BNHIP_E_INVALID, "2^31 detection rows or more");
    }
    if (m->engs.size() > 1) return set_err(BNHIP_E_INVALID, "file analysis runs on one device; use a single-device handle");
    if (e.device < 0) return set_err(BNHIP_E_INVALID, "plan-only model cannot run");
    if ((size_t)e.n_classes * 4 > TOPK_LDS_MAX) return set_err(BNHIP_E_UNSUPPORTED, "too many classes for the LDS top-k");
    if (mx) if (int rc = mixed_plans(mx)) return rc;
    std::vector<long long> table((size_t)n_recordings * 3 + 1);       // first[n + 1], then slot[n][2]
    long long* first = table.data();
    long long* slot = first + n_recordings + 1;
    std::vector<long long> len64(lengths, lengths + n_recordings);
    const long long W64 = analyze_windows(len64.data(), n_recordings, e.n_samples, hop, min_tail, first);
    if (W64 > INT_MAX) return set_err(BNHIP_E_INVALID, "more than INT_MAX windows");
    const int W = (int)W64, kk = std::min(k, e.n_classes);
    const SlotPlan sp = slot_plan(lengths, n_recordings, bits, mx, slot);
    const size_t block_bytes = sp.block_bytes, raw_bytes = sp.raw_bytes;
    const std::vector<ResampleSlotDesc>& desc = sp.desc;
    const std::vector<long long>&tile0 = sp.tile0, &etile0 = sp.etile0;
    const std::vector<EnergyDesc>& edesc = sp.edesc;
    const std::vector<int>& chsel = sp.chsel;
    const bool mc = sp.mc;
    const long long n_etiles = sp.n_etiles;
    if (hipSetDevice(e.device) != hipSuccess) return set_err(BNHIP_E_RUNTIME, "hipSetDevice failed");
    // whatever an earlier asynchronous call still has queued on the engine's streams finishes first (as host_run does)
    e.sync_contexts();
    if (e.stream) hipStreamSynchronize(e.stream);
    // one allocation: recordings | tables | top-k confidences | top-k indices | detection scratch | row count | rows
    // (mixed: | raw block | descriptors, tile prefix)
    // events: every row stays on the device (the caller's cap counts events), and behind everything else lie the filter's tables,
    // the event scratch (events.h) and the events
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t table_bytes = table.size() * 8, tk_bytes = (size_t)W * kk * 4;
    const size_t n_rows_max = (size_t)W * kk, ev_cap = ev ? std::min(cap, n_rows_max) : 0;
    const size_t rows_cap = ev ? n_rows_max : det ? std::min(cap, n_rows_max) : 0;
    const size_t o_table = up(block_bytes), o_conf = o_table + up(table_bytes), o_idx = o_conf + up(tk_bytes), o_scr = o_idx + up(tk_bytes);
    const size_t o_total = o_scr + (det ? up(detections_scratch_bytes(W)) : 0), o_rows = o_total + (det ? 256 : 0);
    const size_t o_raw = o_rows + up(rows_cap * sizeof(DetRow)), o_desc = o_raw + up(raw_bytes);
    const size_t desc_bytes = desc.size() * sizeof(ResampleSlotDesc), o_chsel = o_desc + (mx ? up(desc_bytes) + up(tile0.size() * 8) : 0);
    // (channels: | channel counts, selections | measurement descriptors | their tile prefix | tile partials | sums)
    const size_t o_edesc = o_chsel + up(chsel.size() * 4), o_etile0 = o_edesc + up(edesc.size() * sizeof(EnergyDesc));
    const size_t o_part = o_etile0 + (edesc.empty() ? 0 : up(etile0.size() * 8)), o_energy = o_part + up((size_t)n_etiles * ENERGY_ROW_BYTES);
    const size_t o_evtab = o_energy + up(edesc.size() * ENERGY_ROW_BYTES), o_evscr = o_evtab + (ev ? up(event_tables_bytes(e.n_classes)) : 0);
    const size_t o_evout = o_evscr + (ev ? up(events_scratch_bytes(n_rows_max)) : 0);
    const size_t all_bytes = o_evout + up(ev_cap * sizeof(Event));
    char* d = nullptr;
    if (hipMalloc((void**)&d, all_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(BNHIP_E_NOMEM, "device allocation failed (file analysis)");
    }
    bool ok = true;
    std::string err;
    const SlotDev dv{d, o_table, d + o_raw, d + o_desc, d + o_desc + up(desc_bytes), d + o_chsel, d + o_edesc, d + o_etile0, d + o_part, d + o_energy};
    slot_upload(sp, pcm, bits, lengths, n_recordings, slot, mx, e.device, dv, e.stream, ok, err);
    AN_HIP(hipMemcpyAsync(d + o_table, table.data(), table_bytes, hipMemcpyHostToDevice, e.stream), "H2D copy");
    if (ev) {
        AN_HIP(hipMemcpyAsync(d + o_evtab, ev->f->class_threshold, (size_t)e.n_classes * 4, hipMemcpyHostToDevice, e.stream), "H2D copy");
        if (ev->f->class_veto)
            AN_HIP(hipMemcpyAsync(d + o_evtab + (size_t)e.n_classes * 4, ev->f->class_veto, (size_t)e.n_classes, hipMemcpyHostToDevice, e.stream),
                   "H2D copy");
    }
    WinView view;
    view.first = reinterpret_cast<const long long*>(d + o_table);
    view.slot = view.first + n_recordings + 1;
    view.n_rec = n_recordings; view.hop = hop; view.w0 = 0;
    float* d_conf = reinterpret_cast<float*>(d + o_conf);
    int32_t* d_idx = reinterpret_cast<int32_t*>(d + o_idx);
    // the windows in chunks of max_batch, every chunk enqueued behind the previous one (as bnhip_range_heatmap runs its rows)
    for (int w0 = 0; ok && w0 < W; w0 += e.max_batch) {
        const int n = std::min(e.max_batch, W - w0);
        PcmSource ps;
        ps.samples = d; ps.bits = bits; ps.win = win_at(view, w0);
        ok = e.run(e.d_stage_in, n, e.d_stage_logits, nullptr, &err, ps);
        if (!ok) break;
        launch_activation(e.d_stage_logits, e.d_post_conf, n, e.n_classes, activation, sensitivity, e.stream);
        launch_topk(e.d_post_conf, n, e.n_classes, kk, d_conf + (size_t)w0 * kk, d_idx + (size_t)w0 * kk, e.stream);
    }
    unsigned long long total = 0;
    if (ok && det) {
        launch_detections(d_conf, d_idx, W, kk, threshold, view, d + o_scr, reinterpret_cast<DetRow*>(d + o_rows), rows_cap,
                          reinterpret_cast<unsigned long long*>(d + o_total), e.stream);
        // the event tail reads the rows where they lie, and their count where launch_detections left it
        if (ev) {
            const uint8_t* d_veto = ev->f->class_veto ? reinterpret_cast<const uint8_t*>(d + o_evtab + (size_t)e.n_classes * 4) : nullptr;
            const EventFilterDev fd{reinterpret_cast<const float*>(d + o_evtab), d_veto, ev->f->veto_threshold, ev->f->hold_windows, ev->f->min_count,
                                    ev->f->flags, e.n_classes};
            launch_events(reinterpret_cast<const DetRow*>(d + o_rows), reinterpret_cast<const unsigned long long*>(d + o_total), n_rows_max, fd,
                          events_passes((unsigned long long)n_recordings * e.n_classes - 1), d + o_evscr, reinterpret_cast<Event*>(d + o_evout), ev_cap,
                          e.stream);
        }
    }
    if (ok) AN_HIP(hipGetLastError(), "kernel launch");
    if (ok && ev) {
        AN_HIP(hipMemcpyAsync(&total, events_total(d + o_evscr), 8, hipMemcpyDeviceToHost, e.stream), "D2H copy");
        AN_HIP(hipStreamSynchronize(e.stream), "file analysis");
        const size_t n_ev = (size_t)std::min<unsigned long long>(total, ev_cap);
        if (ok && n_ev) AN_HIP(hipMemcpyAsync(ev->out, d + o_evout, n_ev * sizeof(Event), hipMemcpyDeviceToHost, e.stream), "D2H copy");
    } else if (ok && det) {
        AN_HIP(hipMemcpyAsync(&total, d + o_total, 8, hipMemcpyDeviceToHost, e.stream), "D2H copy");
        AN_HIP(hipStreamSynchronize(e.stream), "file analysis");
        const size_t n_rows = (size_t)std::min<unsigned long long>(total, rows_cap);
        if (ok && n_rows) AN_HIP(hipMemcpyAsync(out_rows, d + o_rows, n_rows * sizeof(DetRow), hipMemcpyDeviceToHost, e.stream), "D2H copy");
    } else if (ok) {
        AN_HIP(hipMemcpyAsync(out_conf, d_conf, tk_bytes, hipMemcpyDeviceToHost, e.stream), "D2H copy");
        AN_HIP(hipMemcpyAsync(out_idx, d_idx, tk_bytes, hipMemcpyDeviceToHost, e.stream), "D2H copy");
    }
    if (ok && mc) {
        mx->chosen.resize(n_recordings);
        AN_HIP(hipMemcpyAsync(mx->chosen.data(), d + o_chsel + (size_t)n_recordings * 4, (size_t)n_recordings * 4, hipMemcpyDeviceToHost, e.stream),
               "D2H copy");
    }
    {
        const hipError_t he = hipStreamSynchronize(e.stream);
        if (ok && he != hipSuccess) { ok = false; err = std::string("file analysis: ") + hipGetErrorString(he); }
    }
    // the continuation: nothing of the call is in flight any more, and the recordings are where the windows were framed from
    int rc_tail = BNHIP_OK;
    if (ok && ct) {
        ct->o->n_events = (size_t)total;
        rc_tail = clip_export_run(e.device, d, bits, view.slot, lengths, n_recordings, hop, ct->model_rate, ct->x, ct->o);
    }
    hipFree(d);
    if (!ok) { (void)hipGetLastError(); e.mm_dirty = true; return set_err(BNHIP_E_RUNTIME, err); }
    if (det) *n_out = (size_t)total;
    return rc_tail;
}

}  // namespace

extern "C" {

long long bnhip_analyze_windows(const int64_t* lengths, int n_recordings, int n_samples, int hop, int64_t min_tail, int64_t* first_window) {
    if (!first_window) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (int rc = check_table(lengths, n_recordings, n_samples, hop, min_tail)) return rc;
    BN_GUARD_BEGIN
    std::vector<long long> len64(lengths, lengths + n_recordings), first((size_t)n_recordings + 1);
    const long long W = analyze_windows(len64.data(), n_recordings, n_samples, hop, min_tail, first.data());
    std::copy(first.begin(), first.end(), first_window);
    return W;
    BN_GUARD_END((void)0)
}

int bnhip_analyze_pcm_topk(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                           int64_t min_tail, int activation, double sensitivity, int k, float* out_conf, int32_t* out_idx) {
    BN_GUARD_BEGIN
    return analyze(m, pcm, bits_per_sample, lengths, n_recordings, hop, min_tail, activation, sensitivity, k, out_conf, out_idx, false, 0.f,
                   nullptr, 0, nullptr);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_pcm(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                      int64_t min_tail, int activation, double sensitivity, int k, float threshold, bnhip_detection* out, size_t cap,
                      size_t* n_out) {
    BN_GUARD_BEGIN
    return analyze(m, pcm, bits_per_sample, lengths, n_recordings, hop, min_tail, activation, sensitivity, k, nullptr, nullptr, true, threshold,
                   out, cap, n_out);
    BN_GUARD_END((void)0)
}

// the events entries: the rows entry with every non-NaN row kept on the device (threshold -inf) and the event tail behind it
int bnhip_analyze_pcm_events(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                             int64_t min_tail, int activation, double sensitivity, int k, const bnhip_event_filter* filter, bnhip_event* out,
                             size_t cap, size_t* n_out) {
    BN_GUARD_BEGIN
    const EventsOut ev{filter, out};
    return analyze(m, pcm, bits_per_sample, lengths, n_recordings, hop, min_tail, activation, sensitivity, k, nullptr, nullptr, true, -INFINITY,
                   nullptr, cap, n_out, nullptr, &ev);
    BN_GUARD_END((void)0)
}

// ---- recordings at their own rates and depths
long long bnhip_analyze_mixed_windows(const bnhip_recording* recs, int n_recordings, int model_rate, int n_samples, int hop, int64_t min_tail,
                                      int64_t* first_window, int64_t* resampled_length) {
    BN_GUARD_BEGIN
    if (!first_window) return set_err(BNHIP_E_INVALID, "NULL argument");
    Mixed mx;
    if (int rc = mixed_check(recs, n_recordings, model_rate, &mx)) return rc;
    if (int rc = check_table(mx.n_out.data(), n_recordings, n_samples, hop, min_tail)) return rc;
    std::vector<long long> len64(mx.n_out.begin(), mx.n_out.end()), first((size_t)n_recordings + 1);
    const long long W = analyze_windows(len64.data(), n_recordings, n_samples, hop, min_tail, first.data());
    std::copy(first.begin(), first.end(), first_window);
    if (resampled_length) std::copy(mx.n_out.begin(), mx.n_out.end(), resampled_length);
    return W;
    BN_GUARD_END((void)0)
}

// the two device entries: a burst that the existing entries take as it is goes to them
static int analyze_mixed(bnhip_model* m, const void* pcm, const bnhip_recording* recs, int n_recordings, int model_rate, int hop, int64_t min_tail,
                         int activation, double sensitivity, int k, float* out_conf, int32_t* out_idx, bool det, float threshold,
                         bnhip_detection* out_rows, size_t cap, size_t* n_out, const EventsOut* ev = nullptr) {
    Mixed mx;
    if (int rc = mixed_check(recs, n_recordings, model_rate, &mx)) return rc;
    return analyze(m, pcm, mx.plain ? recs[0].bits_per_sample : 0, mx.n_out.data(), n_recordings, hop, min_tail, activation, sensitivity, k, out_conf,
                   out_idx, det, threshold, out_rows, cap, n_out, mx.plain ? nullptr : &mx, ev);
}

int bnhip_analyze_mixed_pcm_topk(bnhip_model* m, const void* pcm, const bnhip_recording* recs, int n_recordings, int model_rate, int hop,
                                 int64_t min_tail, int activation, double sensitivity, int k, float* out_conf, int32_t* out_idx) {
    BN_GUARD_BEGIN
    return analyze_mixed(m, pcm, recs, n_recordings, model_rate, hop, min_tail, activation, sensitivity, k, out_conf, out_idx, false, 0.f, nullptr, 0,
                         nullptr);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_mixed_pcm(bnhip_model* m, const void* pcm, const bnhip_recording* recs, int n_recordings, int model_rate, int hop,
                            int64_t min_tail, int activation, double sensitivity, int k, float threshold, bnhip_detection* out, size_t cap,
                            size_t* n_out) {
    BN_GUARD_BEGIN
    return analyze_mixed(m, pcm, recs, n_recordings, model_rate, hop, min_tail, activation, sensitivity, k, nullptr, nullptr, true, threshold, out, cap,
                         n_out);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_mixed_pcm_events(bnhip_model* m, const void* pcm, const bnhip_recording* recs, int n_recordings, int model_rate, int hop,
                                   int64_t min_tail, int activation, double sensitivity, int k, const bnhip_event_filter* filter,
                                   bnhip_event* out, size_t cap, size_t* n_out) {
    BN_GUARD_BEGIN
    const EventsOut ev{filter, out};
    return analyze_mixed(m, pcm, recs, n_recordings, model_rate, hop, min_tail, activation, sensitivity, k, nullptr, nullptr, true, -INFINITY, nullptr,
                         cap, n_out, &ev);
    BN_GUARD_END((void)0)
}

// ---- multichannel recordings
long long bnhip_analyze_channels_windows(const bnhip_channels_recording* recs, int n_recordings, int model_rate, int n_samples, int hop,
                                         int64_t min_tail, int64_t* first_window, int64_t* resampled_length) {
    BN_GUARD_BEGIN
    if (!first_window) return set_err(BNHIP_E_INVALID, "NULL argument");
    Channels ch;
    if (int rc = channels_check(recs, n_recordings, false, &ch)) return rc;
    return bnhip_analyze_mixed_windows(ch.base.data(), n_recordings, model_rate, n_samples, hop, min_tail, first_window, resampled_length);
    BN_GUARD_END((void)0)
}

// the two device entries: a burst of mono recordings is the mixed call, with that call's own fast path
static int analyze_channels(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate, int hop,
                            int64_t min_tail, int activation, double sensitivity, int k, float* out_conf, int32_t* out_idx, bool det, float threshold,
                            bnhip_detection* out_rows, size_t cap, size_t* n_out, int32_t* chosen, const EventsOut* ev = nullptr,
                            const ClipsTail* ct = nullptr) {
    Channels ch;
    if (int rc = channels_check(recs, n_recordings, false, &ch)) return rc;
    Mixed mx;
    if (int rc = mixed_check(ch.base.data(), n_recordings, model_rate, &mx)) return rc;
    if (ch.multi) {
        mx.plain = false;
        mx.channels = ch.channels; mx.select = ch.select;
    }
    const int rc = analyze(m, pcm, mx.plain ? ch.base[0].bits_per_sample : 0, mx.n_out.data(), n_recordings, hop, min_tail, activation, sensitivity, k,
                           out_conf, out_idx, det, threshold, out_rows, cap, n_out, mx.plain ? nullptr : &mx, ev, ct);
    if (rc == BNHIP_OK && chosen) {
        // (one channel: channel 0 is what auto picks, and a mix of one channel is asked for and answered as a mix)
        for (int r = 0; r < n_recordings; r++) chosen[r] = ch.multi ? mx.chosen[r] : ch.select[r] == CHANNEL_AUTO ? 0 : ch.select[r];
    }
    return rc;
}

int bnhip_analyze_channels_pcm_topk(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate,
                                    int hop, int64_t min_tail, int activation, double sensitivity, int k, float* out_conf, int32_t* out_idx,
                                    int32_t* chosen) {
    BN_GUARD_BEGIN
    return analyze_channels(m, pcm, recs, n_recordings, model_rate, hop, min_tail, activation, sensitivity, k, out_conf, out_idx, false, 0.f, nullptr,
                            0, nullptr, chosen);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_channels_pcm(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate, int hop,
                               int64_t min_tail, int activation, double sensitivity, int k, float threshold, bnhip_detection* out, size_t cap,
                               size_t* n_out, int32_t* chosen) {
    BN_GUARD_BEGIN
    return analyze_channels(m, pcm, recs, n_recordings, model_rate, hop, min_tail, activation, sensitivity, k, nullptr, nullptr, true, threshold, out,
                            cap, n_out, chosen);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_channels_pcm_events(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate,
                                      int hop, int64_t min_tail, int activation, double sensitivity, int k, const bnhip_event_filter* filter,
                                      bnhip_event* out, size_t cap, size_t* n_out, int32_t* chosen) {
    BN_GUARD_BEGIN
    const EventsOut ev{filter, out};
    return analyze_channels(m, pcm, recs, n_recordings, model_rate, hop, min_tail, activation, sensitivity, k, nullptr, nullptr, true, -INFINITY,
                            nullptr, cap, n_out, chosen, &ev);
    BN_GUARD_END((void)0)
}

// ---- detection clips (clips.h; the span rule and the export's second phase: api_clips.cpp)
// the events call with the clip export as its continuation
int bnhip_analyze_channels_pcm_clips(bnhip_model* m, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate,
                                     int hop, int64_t min_tail, int activation, double sensitivity, int k, const bnhip_event_filter* filter,
                                     int32_t* chosen, const bnhip_clip_export* x, bnhip_clips_out* out) {
    BN_GUARD_BEGIN
    if (int rc = clip_export_check(x, out, model_rate)) return rc;
    if (int rc = event_filter_check(filter)) return rc;
    if (filter->flags & BNHIP_EVENTS_KEEP_DROPPED) return set_err(BNHIP_E_INVALID, "the clip export takes kept events only: BNHIP_EVENTS_KEEP_DROPPED is refused");
    const EventsOut ev{filter, out->events};
    const ClipsTail ct{x, out, model_rate};
    size_t n_events = 0;
    return analyze_channels(m, pcm, recs, n_recordings, model_rate, hop, min_tail, activation, sensitivity, k, nullptr, nullptr, true, -INFINITY,
                            nullptr, out->event_cap, &n_events, chosen, &ev, &ct);
    BN_GUARD_END((void)0)
}

// the cut alone: one DevCarve (the slot block, the slot table, with a burst off the fast path the parts of slot_upload, the cut's
// tables, the clips), the upload, the cut, one D2H copy
int bnhip_recording_clips_pcm16(int device, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, int model_rate,
                                const bnhip_clip_span* spans, int n_spans, int16_t* out_pcm) {
    BN_GUARD_BEGIN
    const char* what = "recording_clips_pcm16";
    if (!pcm || !spans || !out_pcm) return set_err(BNHIP_E_INVALID, "NULL argument");
    Channels ch;
    if (int rc = channels_check(recs, n_recordings, false, &ch)) return rc;
    Mixed mx;
    if (int rc = mixed_check(ch.base.data(), n_recordings, model_rate, &mx)) return rc;
    if (ch.multi) {
        mx.plain = false;
        mx.channels = ch.channels; mx.select = ch.select;
    }
    if (n_spans < 1 || n_spans > 65535) return set_err(BNHIP_E_INVALID, "n_spans must be in [1, 65535]");
    long long total = 0;
    for (int i = 0; i < n_spans; i++) {
        const bnhip_clip_span& q = spans[i];
        const std::string who = "span " + std::to_string(i) + ": ";
        if (q.recording < 0 || q.recording >= n_recordings) return set_err(BNHIP_E_INVALID, who + "recording outside the table");
        if (q.length < 0) return set_err(BNHIP_E_INVALID, who + "negative length");
        if (q.start < 0 || q.start > mx.n_out[q.recording] - q.length) return set_err(BNHIP_E_INVALID, who + "outside its recording");
        total += q.length;
    }
    if (total > RAGGED_MAX_SAMPLES) return set_err(BNHIP_E_INVALID, "the clips' total length must be below 2^36 samples");
    Mixed* pm = mx.plain ? nullptr : &mx;
    if (pm) if (int rc = mixed_plans(pm)) return rc;
    const CutPlan plan = cut_plan(spans, (size_t)n_spans, n_spans);
    if (plan.n_clips() == 0) return BNHIP_OK;
    const int bits = pm ? 0 : ch.base[0].bits_per_sample;
    std::vector<long long> slot((size_t)n_recordings * 2);
    const SlotPlan sp = slot_plan(mx.n_out.data(), n_recordings, bits, pm, slot.data());
    if (int rc = use_device(device)) return rc;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    DevCarve cv;
    const size_t o_block = cv.add(up(sp.block_bytes)), o_slot = cv.add(slot.size() * 8), o_tab = cv.add(plan.table_bytes());
    const size_t o_out = cv.add((size_t)total * 2);
    const size_t o_raw = cv.add(sp.raw_bytes), o_desc = cv.add(sp.desc.size() * sizeof(ResampleSlotDesc)), o_tile0 = cv.add(sp.tile0.size() * 8);
    const size_t o_chsel = cv.add(sp.chsel.size() * 4), o_edesc = cv.add(sp.edesc.size() * sizeof(EnergyDesc)), o_etile0 = cv.add(sp.etile0.size() * 8);
    const size_t o_part = cv.add((size_t)sp.n_etiles * ENERGY_ROW_BYTES), o_energy = cv.add(sp.edesc.size() * ENERGY_ROW_BYTES);
    DevBlocks b;
    cv.alloc(b);
    if (b.he != hipSuccess) return hip_fail(what, b);
    bool ok = true;
    std::string err;
    const SlotDev dv{cv.at<char>(o_block), up(sp.block_bytes), cv.at<char>(o_raw), cv.at<char>(o_desc), cv.at<char>(o_tile0), cv.at<char>(o_chsel),
                     cv.at<char>(o_edesc), cv.at<char>(o_etile0), cv.at<char>(o_part), cv.at<char>(o_energy)};
    slot_upload(sp, pcm, bits, mx.n_out.data(), n_recordings, slot.data(), pm, device, dv, nullptr, ok, err);
    AN_HIP(hipMemcpyAsync(cv.at<void>(o_slot), slot.data(), slot.size() * 8, hipMemcpyHostToDevice, nullptr), "H2D copy");
    if (ok) AN_HIP(cut_enqueue(plan, dv.block, bits, cv.at<long long>(o_slot), cv.at<void>(o_tab), cv.at<int16_t>(o_out), nullptr), "clip cut");
    // (the null stream orders the copy after the kernels; it is the call's synchronise)
    if (ok) AN_HIP(hipMemcpy(out_pcm, cv.at<void>(o_out), (size_t)total * 2, hipMemcpyDeviceToHost), "D2H copy");
    if (!ok) { hipDeviceSynchronize(); (void)hipGetLastError(); return set_err(BNHIP_E_RUNTIME, std::string(what) + ": " + err); }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

// ---- detection events
// the tail alone over rows the host holds: one pass over the rows for every refusal, one block (rows | tables | scratch | events),
// the rows and tables up, the tail's launches, the count and the events down
int bnhip_detection_events(int device, const bnhip_detection* rows, size_t n_rows, int n_classes, const bnhip_event_filter* filter,
                           bnhip_event* out, size_t cap, size_t* n_out) {
    BN_GUARD_BEGIN
    const char* what = "detection_events";
    if (!n_out || (cap && !out) || (n_rows && !rows)) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (int rc = event_filter_check(filter)) return rc;
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
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t ev_cap = std::min(cap, n_rows);
    const size_t o_count = up(n_rows * sizeof(DetRow)), o_tab = o_count + 256, o_scr = o_tab + up(event_tables_bytes(n_classes));
    const size_t o_out = o_scr + up(events_scratch_bytes(n_rows)), all_bytes = o_out + up(ev_cap * sizeof(Event));
    DevBlocks b;
    char* d = static_cast<char*>(b.get(all_bytes));
    const unsigned long long n64 = n_rows;
    if (b.he == hipSuccess) b.he = hipMemcpy(d, rows, n_rows * sizeof(DetRow), hipMemcpyHostToDevice);
    if (b.he == hipSuccess) b.he = hipMemcpy(d + o_count, &n64, 8, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) b.he = hipMemcpy(d + o_tab, filter->class_threshold, (size_t)n_classes * 4, hipMemcpyHostToDevice);
    if (b.he == hipSuccess && filter->class_veto)
        b.he = hipMemcpy(d + o_tab + (size_t)n_classes * 4, filter->class_veto, (size_t)n_classes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail(what, b);
    const uint8_t* d_veto = filter->class_veto ? reinterpret_cast<const uint8_t*>(d + o_tab + (size_t)n_classes * 4) : nullptr;
    const EventFilterDev fd{reinterpret_cast<const float*>(d + o_tab), d_veto, filter->veto_threshold, filter->hold_windows, filter->min_count,
                            filter->flags, n_classes};
    launch_events(reinterpret_cast<const DetRow*>(d), reinterpret_cast<const unsigned long long*>(d + o_count), n_rows, fd,
                  events_passes((unsigned long long)(max_rec + 1) * n_classes - 1), d + o_scr, reinterpret_cast<Event*>(d + o_out), ev_cap, nullptr);
    if (int rc = launch_status(what)) { hipDeviceSynchronize(); return rc; }
    // (the null stream orders the copies after the kernels; the first one is the call's synchronise)
    unsigned long long total = 0;
    b.he = hipMemcpy(&total, events_total(d + o_scr), 8, hipMemcpyDeviceToHost);
    const size_t n_ev = (size_t)std::min<unsigned long long>(total, ev_cap);
    if (b.he == hipSuccess && n_ev) b.he = hipMemcpy(out, d + o_out, n_ev * sizeof(Event), hipMemcpyDeviceToHost);
    if (b.he != hipSuccess) return hip_fail(what, b);
    *n_out = (size_t)total;
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

// calculateMinDetectionsFromSettings (processor.go:1669-1729), host only
int bnhip_event_min_count(int level, double overlap_seconds) {
    if (level == 0) return 1;
    static const double share[6] = {0.0, 0.20, 0.30, 0.50, 0.60, 0.70};
    const double segment = std::max(0.1, 3.0 - overlap_seconds);
    const double required = 6.0 / segment * (level >= 1 && level <= 5 ? share[level] : 0.30) - 1e-9;
    return (int)std::max(1.0, std::ceil(required));
}

// the measurement alone: one DevCarve (the raw block, the descriptors and tile prefix, the partials, the sums, the decisions), one
// H2D copy per recording, the two launches, the sums and decisions down
int bnhip_channel_energy_pcm(int device, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, bnhip_channel_energy* out,
                             int32_t* chosen) {
    BN_GUARD_BEGIN
    const char* what = "channel_energy_pcm";
    if (!pcm || !out) return set_err(BNHIP_E_INVALID, "NULL argument");
    Channels ch;
    if (int rc = channels_check(recs, n_recordings, true, &ch)) return rc;
    std::vector<EnergyDesc> edesc(n_recordings);
    std::vector<long long> etile0((size_t)n_recordings + 1, 0);
    size_t raw_bytes = 0, n_rows = 0;
    for (int r = 0; r < n_recordings; r++) {
        const bnhip_recording& q = ch.base[r];
        const std::string who = "recording " + std::to_string(r) + ": ";
        if (q.bits_per_sample != 16 && q.bits_per_sample != 24 && q.bits_per_sample != 32)
            return set_err(BNHIP_E_INVALID, who + "unsupported bit depth: " + std::to_string(q.bits_per_sample) + " (supported: 16, 24, 32)");
        if (q.rate <= 0) return set_err(BNHIP_E_INVALID, who + "the sample rate must be positive");
        if (q.length < 1) return set_err(BNHIP_E_INVALID, "every recording needs at least one sample");
        if (q.length > MIXED_MAX_LEN) return set_err(BNHIP_E_INVALID, who + "2^31 samples or more");
        edesc[r] = EnergyDesc{(long long)raw_bytes, (int)q.length, q.bits_per_sample, ch.channels[r], r};
        etile0[r + 1] = etile0[r] + energy_tiles(q.length);
        raw_bytes += ((size_t)q.length * ch.channels[r] * analyze_sample_bytes(q.bits_per_sample) + 15) / 16 * 16;
        n_rows += ch.channels[r];
    }
    if (int rc = use_device(device)) return rc;
    const long long n_tiles = etile0[n_recordings];
    DevCarve cv;
    const size_t o_raw = cv.add(raw_bytes), o_desc = cv.add(edesc.size() * sizeof(EnergyDesc)), o_tile0 = cv.add(etile0.size() * 8);
    const size_t o_part = cv.add((size_t)n_tiles * ENERGY_ROW_BYTES), o_sums = cv.add((size_t)n_recordings * ENERGY_ROW_BYTES);
    const size_t o_sel = cv.add((size_t)n_recordings * 4);
    DevBlocks b;
    cv.alloc(b);
    const char* src = static_cast<const char*>(pcm);
    for (int r = 0; b.he == hipSuccess && r < n_recordings; r++) {
        const size_t bytes = (size_t)ch.base[r].length * ch.channels[r] * analyze_sample_bytes(ch.base[r].bits_per_sample);
        b.he = hipMemcpy(cv.at<char>(o_raw) + edesc[r].in_off, src, bytes, hipMemcpyHostToDevice);
        src += bytes;
    }
    if (b.he == hipSuccess) b.he = hipMemcpy(cv.at<void>(o_desc), edesc.data(), edesc.size() * sizeof(EnergyDesc), hipMemcpyHostToDevice);
    if (b.he == hipSuccess) b.he = hipMemcpy(cv.at<void>(o_tile0), etile0.data(), etile0.size() * 8, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail(what, b);
    launch_channel_energy(cv.at<void>(o_raw), cv.at<EnergyDesc>(o_desc), cv.at<long long>(o_tile0), n_recordings, n_tiles,
                          cv.at<unsigned long long>(o_part), cv.at<unsigned long long>(o_sums), cv.at<int>(o_sel), nullptr);
    if (int rc = launch_status(what)) { hipDeviceSynchronize(); return rc; }
    // (the null stream orders the copies after the kernels; the first one is the call's synchronise)
    std::vector<unsigned long long> sums((size_t)n_recordings * 2 * CHANNELS_MAX);
    std::vector<int32_t> sel(n_recordings);
    b.he = hipMemcpy(sums.data(), cv.at<void>(o_sums), sums.size() * 8, hipMemcpyDeviceToHost);
    if (b.he == hipSuccess) b.he = hipMemcpy(sel.data(), cv.at<void>(o_sel), sel.size() * 4, hipMemcpyDeviceToHost);
    if (b.he != hipSuccess) return hip_fail(what, b);
    bnhip_channel_energy* o = out;
    for (int r = 0; r < n_recordings; r++) {
        for (int c = 0; c < ch.channels[r]; c++, o++) {
            o->sum_lo = sums[((size_t)r * CHANNELS_MAX + c) * 2];
            o->sum_hi = sums[((size_t)r * CHANNELS_MAX + c) * 2 + 1];
            o->rms_dbfs = channel_rms_dbfs(o->sum_lo, o->sum_hi, ch.base[r].bits_per_sample, ch.base[r].length);
        }
        if (chosen) chosen[r] = sel[r];
    }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

}  // extern "C"
