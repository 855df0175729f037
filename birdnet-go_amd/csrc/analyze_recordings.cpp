// The recordings of a file-analysis call (analyze_recordings.h): the C ABI's three forms to one description, the refusals, the
// rate plans and their cached phase tables, and the upload that fills the slot block.
#include "analyze_recordings.h"

#include <algorithm>
#include <climits>
#include <string>

#include "flac_parse.h"

using namespace bnhip;

static_assert(sizeof(bnhip_recording) == 16, "a recording's description is 16 bytes");
static_assert(sizeof(bnhip_channels_recording) == 24, "a multichannel recording's description is 24 bytes");
static_assert(BNHIP_CHANNEL_MIX == CHANNEL_MIX && BNHIP_CHANNEL_AUTO == CHANNEL_AUTO, "the selection constants of channels.h");

namespace {

constexpr long long MIXED_MAX_LEN = (1ll << 31) - 1;

// The phase tables of one set of rates, concatenated in one device buffer and kept (api_oneshot.h): a second call with the same
// rates designs and uploads nothing.
struct RateSetTable {
    int device, model_rate;
    std::vector<int> rates;                       // ascending; their [L][T] tables follow one another in d
    float* d;
};
TableCache<RateSetTable> g_rate_tables;

// the call's concatenated phase tables on the current device, from the cache or designed now; -> NULL: the upload failed
const float* rate_tables(const Recordings& rec, int device, const TableLock& lock) {
    std::vector<int> rates;
    for (const RatePlan& rp : rec.plans) rates.push_back(rp.rate);
    const RateSetTable* t = g_rate_tables.find(
        lock, [&](const RateSetTable& e) { return e.device == device && e.model_rate == rec.model_rate && e.rates == rates; },
        [&](RateSetTable& e) {
            std::vector<float> all, one;
            for (const RatePlan& rp : rec.plans) {
                (void)resample_plan(rp.rate, rec.model_rate, &one);
                all.insert(all.end(), one.begin(), one.end());
            }
            e.device = device; e.model_rate = rec.model_rate; e.rates = rates;
            e.d = upload_table(all);
            return e.d != nullptr;
        });
    return t ? t->d : nullptr;
}

int count_check(const void* recs, int n_recordings) {
    if (!recs) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_recordings < 1 || n_recordings > 65535) return set_err(BNHIP_E_INVALID, "n_recordings must be in [1, 65535]");
    return BNHIP_OK;
}

// rec->recs at model_rate: what the mixed call refuses of them, their lengths at the model's rate and which rates need a plan
int mixed_describe(int model_rate, Recordings* rec) {
    if (model_rate <= 0) return set_err(BNHIP_E_INVALID, "model_rate must be positive");
    const std::vector<bnhip_recording>& recs = rec->recs;
    rec->model_rate = model_rate;
    rec->n_out.resize(rec->n); rec->plan_of.assign(rec->n, -1);
    long long total_in = 0, total_out = 0;
    bool same = true;
    for (int r = 0; r < rec->n; r++) {
        const bnhip_recording& q = recs[r];
        const std::string who = "recording " + std::to_string(r) + ": ";
        if (int rc = recording_check(q, r, true)) return rc;
        // ceil(length * L / M) in 64 bits (bnhip_resample_length): length < 2^31 and L < 2^31
        const long long no = q.rate == model_rate ? (long long)q.length : resample_plan(q.rate, model_rate, nullptr).end(q.length);
        if (no > MIXED_MAX_LEN) return set_err(BNHIP_E_INVALID, who + "2^31 samples or more at the model's rate");
        if (q.length > ANALYZE_MAX_SAMPLES - total_in || no > ANALYZE_MAX_SAMPLES - total_out)
            return set_err(BNHIP_E_INVALID, "burst of 2^36 samples or more");
        total_in += q.length; total_out += no;
        rec->n_out[r] = no;
        rec->n_tiles += resample_slot_tiles(no);
        same = same && q.rate == model_rate && q.bits_per_sample == recs[0].bits_per_sample;
    }
    if (rec->n_tiles > INT_MAX) return set_err(BNHIP_E_INVALID, "more resample tiles than a 31-bit grid");
    rec->plain = same && !rec->multi;
    rec->bits = rec->plain ? recs[0].bits_per_sample : 0;
    if (same) return BNHIP_OK;
    std::vector<int> rates;
    for (const bnhip_recording& q : recs) if (q.rate != model_rate) rates.push_back(q.rate);
    std::sort(rates.begin(), rates.end());
    rates.erase(std::unique(rates.begin(), rates.end()), rates.end());
    for (int rate : rates) rec->plans.push_back(RatePlan{rate, -1, ResamplePlan{}, 0});
    for (int r = 0; r < rec->n; r++) {
        if (recs[r].rate == model_rate) continue;
        const int pi = (int)(std::lower_bound(rates.begin(), rates.end(), recs[r].rate) - rates.begin());
        rec->plan_of[r] = pi;
        if (rec->plans[pi].rec < 0) rec->plans[pi].rec = r;
    }
    return BNHIP_OK;
}

}  // namespace

namespace bnhip {

int recording_check(const bnhip_recording& q, int r, bool float32) {
    const std::string who = "recording " + std::to_string(r) + ": ";
    if (!(q.bits_per_sample == 0 && float32) && q.bits_per_sample != 16 && q.bits_per_sample != 24 && q.bits_per_sample != 32)
        return set_err(BNHIP_E_INVALID, who + "unsupported bit depth: " + std::to_string(q.bits_per_sample) + " (supported: " +
                                            (float32 ? "0 = float32, " : "") + "16, 24, 32)");
    if (q.rate <= 0) return set_err(BNHIP_E_INVALID, who + "the sample rate must be positive");
    if (q.length < 1) return set_err(BNHIP_E_INVALID, "every recording needs at least one sample");
    if (q.length > MIXED_MAX_LEN) return set_err(BNHIP_E_INVALID, who + "2^31 samples or more");
    return BNHIP_OK;
}

int describe(int bits, const int64_t* lengths, int n_recordings, Recordings* rec) {
    rec->n = n_recordings; rec->bits = bits; rec->given = lengths;
    return BNHIP_OK;
}

int describe(const bnhip_recording* recs, int n_recordings, int model_rate, Recordings* rec) {
    if (int rc = count_check(recs, n_recordings)) return rc;
    rec->n = n_recordings;
    rec->recs.assign(recs, recs + n_recordings);
    return mixed_describe(model_rate, rec);
}

int describe(const bnhip_channels_recording* recs, int n_recordings, int model_rate, Recordings* rec) {
    if (int rc = channels_check(recs, n_recordings, false, rec)) return rc;
    return mixed_describe(model_rate, rec);
}

int describe(const uint8_t* streams, const uint64_t* offsets, const int32_t* select, int n_recordings, int model_rate, Recordings* rec) {
    if (int rc = count_check(streams, n_recordings)) return rc;
    if (!offsets || !select) return set_err(BNHIP_E_INVALID, "NULL argument");
    std::vector<bnhip_channels_recording> recs((size_t)n_recordings);
    rec->flac_infos.resize((size_t)n_recordings);
    rec->flac_offsets = offsets;
    for (int r = 0; r < n_recordings; r++) {
        const std::string who = "recording " + std::to_string(r) + ": ";
        if (offsets[r + 1] < offsets[r]) return set_err(BNHIP_E_INVALID, "offsets must ascend");
        bnhip_flac_info& in = rec->flac_infos[(size_t)r];
        flac_stream_info(streams + offsets[r], (size_t)(offsets[r + 1] - offsets[r]), &in, true);
        if (in.status == BNHIP_FLAC_BAD_METADATA) return set_err(BNHIP_E_INVALID, who + "not a FLAC stream, or its metadata blocks are damaged");
        if (in.status != BNHIP_FLAC_OK)
            return set_err(BNHIP_E_INVALID, who + "a FLAC stream of " + std::to_string(in.channels) + " channels, " + std::to_string(in.bits) +
                                                " bits, block size " + std::to_string(in.max_block) +
                                                " is not decoded (1 or 2 channels, 16 or 24 bits, a fixed block size up to 8192, or 16384 for mono 16-bit)");
        recs[(size_t)r] = bnhip_channels_recording{(int64_t)in.total_samples, (int32_t)in.rate, (int32_t)in.bits, (int32_t)in.channels, select[r]};
    }
    if (int rc = flacdec_burst_check(n_recordings, rec->flac_infos.data(), offsets, nullptr, true)) return rc;
    return describe(recs.data(), n_recordings, model_rate, rec);
}

// (what the mixed call refuses of the recordings - the depths, rates and lengths - is recording_check's to answer)
int channels_check(const bnhip_channels_recording* recs, int n_recordings, bool measure, Recordings* rec) {
    if (int rc = count_check(recs, n_recordings)) return rc;
    rec->n = n_recordings;
    rec->recs.resize(n_recordings); rec->channels.resize(n_recordings); rec->select.resize(n_recordings);
    long long total = 0;
    for (int r = 0; r < n_recordings; r++) {
        const bnhip_channels_recording& q = recs[r];
        const std::string who = "recording " + std::to_string(r) + ": ";
        if (q.channels < 1 || q.channels > CHANNELS_MAX) return set_err(BNHIP_E_INVALID, who + "channels must be in [1, 16]");
        if (q.select < CHANNEL_AUTO || q.select >= q.channels)
            return set_err(BNHIP_E_INVALID, who + "select must be a channel index, BNHIP_CHANNEL_MIX or BNHIP_CHANNEL_AUTO");
        if ((measure || q.select == CHANNEL_AUTO) && q.bits_per_sample == 0)
            return set_err(BNHIP_E_INVALID, who + "the channel energies are measured on integer depths; a float32 recording takes a channel or the mix");
        if (q.length >= 1 && q.length <= MIXED_MAX_LEN) {      // (else recording_check refuses the length)
            if (q.length * q.channels > ANALYZE_MAX_SAMPLES - total) return set_err(BNHIP_E_INVALID, "burst of 2^36 samples or more");
            total += q.length * q.channels;
        }
        rec->recs[r] = bnhip_recording{q.length, q.rate, q.bits_per_sample};
        rec->channels[r] = q.channels; rec->select[r] = q.select;
        rec->multi = rec->multi || q.channels > 1;
    }
    return BNHIP_OK;
}

int rate_plans(Recordings* rec) {
    size_t off = 0;
    for (RatePlan& rp : rec->plans) {
        rp.p = resample_plan(rp.rate, rec->model_rate, nullptr);
        if (!rp.p.fits_lds())
            return set_err(BNHIP_E_UNSUPPORTED, "recording " + std::to_string(rp.rec) + ": resampling " + std::to_string(rp.rate) + " Hz to " +
                                                    std::to_string(rec->model_rate) + " Hz needs a phase table larger than LDS");
        rp.tab_off = off;
        off += (size_t)rp.p.L * rp.p.T;
    }
    // (a descriptor states a table's offset in an int: tens of thousands of distinct rates with tables near the LDS limit)
    if (off > (size_t)INT_MAX) return set_err(BNHIP_E_UNSUPPORTED, "the call's phase tables exceed 2^31 floats");
    return BNHIP_OK;
}

EnergyPlan energy_plan(const Recordings& rec, bool all) {
    EnergyPlan en;
    en.tile0.push_back(0);
    size_t in_off = 0;
    for (int r = 0; r < rec.n; in_off += rec.raw_footprint(r), r++) {
        if (!all && rec.select[r] != CHANNEL_AUTO) continue;
        const bnhip_recording& q = rec.recs[r];
        en.desc.push_back(EnergyDesc{(long long)in_off, (int)q.length, q.bits_per_sample, rec.channels[r], r});
        en.tile0.push_back(en.tile0.back() + energy_tiles(q.length));
    }
    return en;
}

SlotPlan slot_plan(const Recordings& rec, long long* slot) {
    SlotPlan sp;
    const int64_t* lengths = rec.lengths();
    for (int r = 0; r < rec.n; r++) {
        slot[2 * r] = (long long)sp.block_bytes; slot[2 * r + 1] = lengths[r];
        sp.block_bytes += analyze_slot_bytes(lengths[r], rec.bits);
    }
    if (rec.flac()) {
        sp.flac_bytes = (size_t)rec.flac_offsets[rec.n];
        sp.flac_ws = flacdec_workspace_bytes(rec.n, rec.flac_infos.data(), rec.flac_offsets, true);
        sp.flac_res = (size_t)rec.n * sizeof(bnhip_flac_decode_result);
    }
    if (rec.plain) return sp;
    sp.desc.resize(rec.n); sp.tile0.assign((size_t)rec.n + 1, 0);
    for (int r = 0; r < rec.n; r++) {
        const bnhip_recording& q = rec.recs[r];
        ResampleSlotDesc& ds = sp.desc[r];
        ds.in_off = (long long)sp.raw_bytes; ds.out_off = slot[2 * r];
        ds.n_in = (int)q.length; ds.n_out = (int)lengths[r]; ds.bits = q.bits_per_sample;
        ds.L = ds.M = ds.T = ds.half = ds.tab_off = 0;
        if (rec.plan_of[r] >= 0) {
            const RatePlan& rp = rec.plans[rec.plan_of[r]];
            ds.L = rp.p.L; ds.M = rp.p.M; ds.T = rp.p.T; ds.half = rp.p.half; ds.tab_off = (int)rp.tab_off;
            sp.rs_lds = std::max(sp.rs_lds, resample_lds(rp.p.L, rp.p.M, rp.p.T));
        }
        sp.raw_bytes += rec.raw_footprint(r);
        sp.tile0[r + 1] = sp.tile0[r] + resample_slot_tiles(lengths[r]);
    }
    if (rec.multi) {
        sp.chsel.assign(rec.channels.begin(), rec.channels.end());
        sp.chsel.insert(sp.chsel.end(), rec.select.begin(), rec.select.end());
        sp.en = energy_plan(rec, false);
    }
    return sp;
}

SlotDev slot_reserve(const SlotPlan& sp, DevCarve& cv) {
    SlotDev dv;
    dv.cv = &cv;
    dv.block_room = (sp.block_bytes + 255) / 256 * 256;
    dv.block = cv.add(dv.block_room);
    dv.raw = cv.add(sp.raw_bytes);
    dv.desc = cv.add(sp.desc.size() * sizeof(ResampleSlotDesc));
    dv.tile0 = cv.add(sp.tile0.size() * 8);
    dv.chsel = cv.add(sp.chsel.size() * 4);
    dv.edesc = cv.add(sp.en.desc.size() * sizeof(EnergyDesc));
    dv.etile0 = cv.add(sp.en.tile0.size() * 8);
    dv.part = cv.add((size_t)sp.en.n_tiles() * ENERGY_ROW_BYTES);
    dv.energy = cv.add(sp.en.desc.size() * ENERGY_ROW_BYTES);
    dv.flac_in = cv.add(sp.flac_bytes);
    dv.flac_ws = cv.add(sp.flac_ws);
    dv.flac_res = cv.add(sp.flac_res);
    return dv;
}

void slot_upload(const SlotPlan& sp, const void* pcm, const Recordings& rec, const long long* slot, int device, const SlotDev& dv, hipStream_t s,
                 DevBlocks& b) {
    char *block = dv.at(dv.block), *raw = dv.at(dv.raw);
    if (rec.plain) AN_HIP(b, hipMemsetAsync(block, 0, dv.block_room, s));
    const char* src = static_cast<const char*>(pcm);
    if (rec.flac()) {
        // the compressed bytes go up once, and the decoder writes what the copies would have brought: recording r's interleaved
        // PCM at its own depth, on its 16-byte line of the raw block or in its slot; a frame it does not restore stays zero
        const size_t first = (size_t)rec.flac_offsets[0];
        if (sp.flac_bytes > first) AN_HIP(b, hipMemcpyAsync(dv.at(dv.flac_in) + first, src + first, sp.flac_bytes - first, hipMemcpyHostToDevice, s));
        if (!rec.plain) AN_HIP(b, hipMemsetAsync(raw, 0, sp.raw_bytes, s));
        if (b.he == hipSuccess) {
            FlacDecWork w = flacdec_work(rec.n, rec.flac_infos.data(), rec.flac_offsets, dv.at<void>(dv.flac_ws), true);
            for (int r = 0; r < rec.n; r++) flacdec_place(w, r, (unsigned long long)(rec.plain ? slot[2 * r] : sp.desc[r].in_off));
            launch_flacdec(dv.at<uint8_t>(dv.flac_in), w, rec.plain ? block : raw, rec.plain ? sp.block_bytes : sp.raw_bytes,
                           dv.at<bnhip_flac_decode_result>(dv.flac_res), s);
        }
    } else {
        for (int r = 0; r < rec.n; src += rec.raw_bytes(r), r++)
            AN_HIP(b, hipMemcpyAsync(rec.plain ? block + slot[2 * r] : raw + sp.desc[r].in_off, src, rec.raw_bytes(r), hipMemcpyHostToDevice, s));
    }
    if (rec.plain) return;
    // (the lock is held from the tables' lookup until the launch that reads them is enqueued, api_oneshot.h)
    TableLock lock(g_rate_tables.mu);
    const float* d_tables = rec.plans.empty() ? nullptr : rate_tables(rec, device, lock);
    if (!rec.plans.empty() && !d_tables) AN_HIP(b, hipErrorOutOfMemory);          // (the phase tables' upload failed)
    AN_HIP(b, hipMemcpyAsync(dv.at(dv.desc), sp.desc.data(), sp.desc.size() * sizeof(ResampleSlotDesc), hipMemcpyHostToDevice, s));
    AN_HIP(b, hipMemcpyAsync(dv.at(dv.tile0), sp.tile0.data(), sp.tile0.size() * 8, hipMemcpyHostToDevice, s));
    const ResampleSlotDesc* d_desc = dv.at<ResampleSlotDesc>(dv.desc);
    const long long* d_tile0 = dv.at<long long>(dv.tile0);
    if (rec.multi) {
        // the selections go up as asked for; the measurement, if any recording asks for one, overwrites its entries on the
        // device, and the slot launch behind it reads them there
        int* d_ch = dv.at<int>(dv.chsel);
        AN_HIP(b, hipMemcpyAsync(d_ch, sp.chsel.data(), sp.chsel.size() * 4, hipMemcpyHostToDevice, s));
        if (!sp.en.desc.empty()) {
            AN_HIP(b, hipMemcpyAsync(dv.at(dv.edesc), sp.en.desc.data(), sp.en.desc.size() * sizeof(EnergyDesc), hipMemcpyHostToDevice, s));
            AN_HIP(b, hipMemcpyAsync(dv.at(dv.etile0), sp.en.tile0.data(), sp.en.tile0.size() * 8, hipMemcpyHostToDevice, s));
            if (b.he == hipSuccess)
                launch_channel_energy(raw, dv.at<EnergyDesc>(dv.edesc), dv.at<long long>(dv.etile0), (int)sp.en.desc.size(), sp.en.n_tiles(),
                                      dv.at<unsigned long long>(dv.part), dv.at<unsigned long long>(dv.energy), d_ch + rec.n, s);
        }
        if (b.he == hipSuccess)
            launch_resample_slots_mc(raw, block, d_tables, d_desc, d_tile0, rec.n, sp.tile0[rec.n], sp.rs_lds, d_ch, d_ch + rec.n, s);
    } else if (b.he == hipSuccess) {
        launch_resample_slots(raw, block, d_tables, d_desc, d_tile0, rec.n, sp.tile0[rec.n], sp.rs_lds, s);
    }
}

}  // namespace bnhip
