// C ABI of the sound level bank.
#include <hip/hip_runtime.h>

#include <cmath>
#include <deque>

#include "soundlevel_bank.h"
#include "stream_bank.h"

using namespace bnhip;

// ------------------------------------------------------------------------------------------------ sound level bank
// The 1/3-octave sound level monitor (soundlevel.Processor, internal/audiocore/soundlevel/processor.go; one per source behind a
// SoundLevelConsumer route, internal/analysis/sound_level_consumer.go:103-150) for every source of one sample rate at once,
// one k_soundlevel_bank launch per call.  The device runs the band filters and hands back the sum of squares of every
// 1-second block a call completes; the host replays ProcessSamples's schedule (at most one measurement per non-empty frame,
// :258-327) and builds the interval statistics (generateSoundLevelData :349-412).  Each stream's filter state is a fixed pair
// of device slabs of SL_MAX_BANDS x {x1, x2, y1, y2, sum}.
struct SoundLevelStream {
    bool fresh = true;                  // the next call starts from zero state (new stream, reset)
    int interval = 1;                   // seconds per report (NewProcessor clamps below 1 to 1)
    long long unmeasured = 0;           // samples in ProcessSamples's buffer: finished blocks not yet measured + the open block
    std::deque<double> fifo;            // the finished blocks not yet measured: n_bands sums each, oldest first
    int count = 0;                      // measurements of the open interval (measurementCount)
    std::vector<double> slots;          // their dB, n_bands per measurement, in slot order
};

struct bnhip_soundlevel_bank : StreamBank<SoundLevelStream, double> {
    static constexpr const char* what = "sound level bank";
    int fs = 0, n_bands = 0;
    double bands[SL_MAX_BANDS][6] = {};   // {c, b0, b1, b2, a1, a2}
    std::vector<double> coef;              // n_bands x {b0, b1, b2, a1, a2}: the band table every call stages
    double* d_state = nullptr;          // [max_streams][2][SL_SLAB]
    ~bnhip_soundlevel_bank() { if (d_state) hipFree(d_state); }
};

namespace {

// ISO 266 1/3-octave centres (processor.go:20-23)
constexpr double SL_CENTRES[] = {25, 31.5, 40, 50, 63, 80, 100, 125, 160, 200, 250, 315, 400, 500, 630, 800,
                                 1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300, 8000, 10000, 12500, 16000, 20000};
constexpr double SL_INV_LN10 = 0x1.bcb7b1526e50ep-2;    // Go's 1/Ln10, as math.Log10 multiplies by it (1.0 / 2.302585092994046 is an ulp lower)

bool sl_unstable(const double* c6) {            // processor.go:212-214: the poles must lie inside the unit circle
    return std::fabs(c6[5]) >= 1.0 || std::fabs(c6[4]) >= 1.0 + c6[5];
}

// NewProcessor's band selection (:120-141) and newOctaveBandFilter (:161-225) -> {c, b0, b1, b2, a1, a2} per band
int sl_design(int rate, double (*o)[6], int* n) {
    const double fs = rate, nyquist = fs / 2.0, threshold = nyquist * 0.95;
    int k = 0;
    for (double c : SL_CENTRES) {
        if (c * std::pow(2.0, 1.0 / 6.0) >= threshold) continue;
        const double low = c / std::pow(2.0, 1.0 / 6.0), high = c * std::pow(2.0, 1.0 / 6.0);
        if (low <= 0 || high >= nyquist) return set_err(BNHIP_E_INVALID, "sound level band out of range at " + std::to_string(c) + " Hz");
        const double omega = 2.0 * M_PI * c / fs, so = std::sin(omega), co = std::cos(omega);
        double q = c / (high - low);
        if (q < 0.5) q = 0.5;
        const double alpha = so / (2.0 * q), a0 = 1.0 + alpha;
        const double r[6] = {c, alpha / a0, 0.0 / a0, -alpha / a0, -2.0 * co / a0, (1.0 - alpha) / a0};
        if (sl_unstable(r)) return set_err(BNHIP_E_INVALID, "unstable sound level band at " + std::to_string(c) + " Hz");
        memcpy(o[k++], r, sizeof r);
    }
    *n = k;
    return BNHIP_OK;
}

// one measurement of a band: calculateRMS's sqrt, the clamp to [1e-10, 10] and 20 * Log10 (processor.go:272-290)
double sl_db(double sum, int fs) {
    double rms = std::sqrt(sum / (double)fs);
    if (rms < 1e-10) rms = 1e-10;
    else if (rms > 10.0) rms = 10.0;
    const double db = 20.0 * (std::log(rms) * SL_INV_LN10);
    return std::isfinite(db) ? db : -100.0;
}

// generateSoundLevelData (:349-412) over the interval's measurements, slot order
void sl_report(const bnhip_soundlevel_bank* b, const SoundLevelStream& S, int stream, int frame, bnhip_sound_level* r) {
    memset(r, 0, sizeof *r);
    r->stream = stream; r->frame = frame; r->duration_s = S.interval; r->n_bands = b->n_bands;
    const int n = S.count;
    for (int j = 0; j < b->n_bands; j++) {
        double lo = S.slots[j], hi = S.slots[j], sum = 0.0;
        for (int k = 0; k < n; k++) {
            const double v = S.slots[(size_t)k * b->n_bands + j];
            if (!std::isfinite(v)) continue;
            if (v < lo) lo = v;
            if (v > hi) hi = v;
            sum += v;
        }
        const double mean = sum / (double)n;
        r->center_hz[j] = b->bands[j][0];
        r->min_db[j] = std::isfinite(lo) ? lo : -100.0;
        r->max_db[j] = std::isfinite(hi) ? hi : -100.0;
        r->mean_db[j] = std::isfinite(mean) ? mean : -100.0;
        r->sample_count[j] = n;
    }
}

// frames f = 0..n_frames-1 of streams[f]; reports go to reports[0..max_reports) in frame order.  plan replays ProcessSamples's
// schedule from the counts alone, so a report buffer that is too small is refused before anything runs.
int sl_run(bnhip_soundlevel_bank* b, int n_frames, const int* streams, const int16_t* const* frames, const int* n_in,
           bnhip_sound_level* reports, int max_reports, int* n_reports) {
    const int fs = b->fs, nb = b->n_bands;
    std::vector<SoundLevelDesc> desc;
    auto plan = [&](std::vector<BankGroup>& groups, const std::vector<int>& frame_group, std::vector<long long>& cnt) -> int {
        std::vector<long long> unmeasured(groups.size());
        std::vector<int> count(groups.size());
        for (size_t gi = 0; gi < groups.size(); gi++) {
            const auto& S = b->st[groups[gi].stream];
            unmeasured[gi] = S.unmeasured;
            count[gi] = S.count;
            groups[gi].run = groups[gi].n_in > 0;
        }
        long long n_rep = 0;
        for (int f = 0; f < n_frames; f++) {
            const int gi = frame_group[f];
            const long long n = n_in[f];
            const long long fill = unmeasured[gi] % fs;
            cnt[f] = (fill + n) / fs * nb;                         // blocks the frame completes, n_bands sums each
            if (n == 0) continue;                                  // not a call: the consumer returns first (sound_level_consumer.go:117)
            unmeasured[gi] += n;
            if (unmeasured[gi] < fs) continue;
            unmeasured[gi] -= fs;                                  // one measurement per call, the overflow carries
            if (++count[gi] >= b->st[groups[gi].stream].interval) {
                count[gi] = 0;
                n_rep++;
            }
        }
        if (n_rep > max_reports)
            return set_err(BNHIP_E_INVALID, "max_reports too small: the call gives " + std::to_string(n_rep) + " reports");
        return BNHIP_OK;
    };
    auto describe = [&](const std::vector<BankGroup>& groups, long long in_total, long long out_total, BankBlob* hdr) -> int {
        if (in_total > INT32_MAX / 2 || out_total > INT32_MAX / 2) return set_err(BNHIP_E_INVALID, "sound level bank call too large");
        for (const BankGroup& g : groups) {
            if (!g.run) continue;
            const auto& S = b->st[g.stream];
            SoundLevelDesc d{};
            d.in_off = g.in_off; d.n = (int)g.n_in; d.fill = (int)(S.unmeasured % fs); d.out_off = g.out_off;
            d.st_rd = S.fresh ? -1 : (g.stream * 2 + S.parity) * SL_SLAB;
            d.st_wr = (g.stream * 2 + (S.parity ^ 1)) * SL_SLAB;
            desc.push_back(d);
        }
        // a wave runs 2 streams, both as many steps as the longer
        for (size_t k0 = 0; k0 < desc.size(); k0 += 2) {
            const int steps = std::max(desc[k0].n, k0 + 1 < desc.size() ? desc[k0 + 1].n : 0);
            desc[k0].blk_steps = (steps + 31) / 32 * 32;
        }
        hdr[0] = {desc.data(), desc.size() * sizeof(SoundLevelDesc)};
        hdr[1] = {b->coef.data(), b->coef.size() * sizeof(double)};
        return BNHIP_OK;
    };
    auto launch = [&](const uint8_t* d_hdr, const int16_t* d_pcm, double* d_out) -> int {
        return launch_soundlevel_bank(reinterpret_cast<const SoundLevelDesc*>(d_hdr), (int)desc.size(),
                                      reinterpret_cast<const double*>(d_hdr + desc.size() * sizeof(SoundLevelDesc)), nb, fs, d_pcm,
                                      b->d_state, d_out, b->stream);
    };
    auto commit = [&](const BankGroup& g, size_t) {
        auto& S = b->st[g.stream];
        S.parity ^= 1;
        S.fresh = false;
    };
    int n_rep = 0;
    auto deliver = [&](int f, const double* sums, int count) {
        auto& S = b->st[streams[f]];
        S.fifo.insert(S.fifo.end(), sums, sums + count);
        if (n_in[f] == 0) return;
        S.unmeasured += n_in[f];
        if (S.unmeasured < fs) return;
        S.unmeasured -= fs;
        for (int j = 0; j < nb; j++) {                             // the oldest finished block (the buffer's first fs samples)
            S.slots.push_back(sl_db(S.fifo.front(), fs));
            S.fifo.pop_front();
        }
        if (++S.count >= S.interval) {
            sl_report(b, S, streams[f], f, &reports[n_rep++]);
            S.count = 0;                                           // resetIntervalBuffer: filters and the second buffers are kept
            S.slots.clear();
        }
    };
    const int rc = bank_call(b, n_frames, streams, frames, n_in, false, INT64_MAX, plan, describe, launch, commit, deliver);
    if (rc == BNHIP_OK) *n_reports = n_rep;
    return rc;
}

}  // namespace

extern "C" {

int bnhip_soundlevel_bands(int sample_rate, double* bands6, int cap, int* n_bands) {
    if (!n_bands) return set_err(BNHIP_E_INVALID, "n_bands is NULL");
    *n_bands = 0;
    if (sample_rate <= 0) return set_err(BNHIP_E_INVALID, "invalid sample rate: " + std::to_string(sample_rate));
    if (cap < 0) return set_err(BNHIP_E_INVALID, "cap is negative");
    BN_GUARD_BEGIN
    double tbl[SL_MAX_BANDS][6];
    int n = 0;
    if (int rc = sl_design(sample_rate, tbl, &n)) return rc;
    *n_bands = n;
    if (!bands6) return BNHIP_OK;
    if (cap < n) return set_err(BNHIP_E_INVALID, "cap below the band count " + std::to_string(n));
    memcpy(bands6, tbl, sizeof(double) * 6 * n);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_soundlevel_bank_create(int device, int sample_rate, int max_streams, const double* bands6, int n_bands,
                                 bnhip_soundlevel_bank** out) {
    if (!out) return set_err(BNHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (sample_rate <= 0) return set_err(BNHIP_E_INVALID, "invalid sample rate: " + std::to_string(sample_rate));   // processor.go:85-91
    if (max_streams < 1 || max_streams > (1 << 20)) return set_err(BNHIP_E_INVALID, "max_streams must be in [1, 1048576]");
    BN_GUARD_BEGIN
    double tbl[SL_MAX_BANDS][6];
    int n = 0;
    if (!bands6) {
        if (int rc = sl_design(sample_rate, tbl, &n)) return rc;
    } else {
        if (n_bands < 1 || n_bands > SL_MAX_BANDS) return set_err(BNHIP_E_INVALID, "n_bands must be in [1, 32]");
        for (int j = 0; j < n_bands; j++) {
            const double* c = bands6 + 6 * j;
            for (int i = 0; i < 6; i++)
                if (!std::isfinite(c[i])) return set_err(BNHIP_E_INVALID, "band " + std::to_string(j) + " has a non-finite value");
            if (!(c[0] > 0)) return set_err(BNHIP_E_INVALID, "band " + std::to_string(j) + " has a centre frequency <= 0");
            if (sl_unstable(c)) return set_err(BNHIP_E_INVALID, "band " + std::to_string(j) + " is unstable");
            memcpy(tbl[j], c, sizeof tbl[j]);
        }
        n = n_bands;
    }
    if (n < 1) return set_err(BNHIP_E_INVALID, "no sound level band fits below 0.95 x Nyquist");
    int rc = use_device(device);
    if (rc) return rc;
    return bank_create(device, max_streams, out, [&](bnhip_soundlevel_bank& b) {
        b.fs = sample_rate;
        b.n_bands = n;
        memcpy(b.bands, tbl, sizeof(double) * 6 * n);
        for (int j = 0; j < n; j++) b.coef.insert(b.coef.end(), tbl[j] + 1, tbl[j] + 6);
        return hipMalloc((void**)&b.d_state, (size_t)max_streams * 2 * SL_SLAB * sizeof(double));
    });
    BN_GUARD_END((void)0)
}

int bnhip_soundlevel_bank_add_stream(bnhip_soundlevel_bank* b, int interval_s, int* out_stream) {
    if (int rc = bank_add_stream(b, out_stream)) return rc;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    b->st[*out_stream].interval = std::max(interval_s, 1);     // processor.go:93-95
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_soundlevel_bank_remove_stream(bnhip_soundlevel_bank* b, int stream) { return bank_remove_stream(b, stream); }

int bnhip_soundlevel_bank_reset(bnhip_soundlevel_bank* b, int stream) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (int rc = bank_stream_check(b, stream)) return rc;
    auto& S = b->st[stream];                                   // Processor.Reset (:331-346): the interval is kept
    S.fresh = true;
    S.unmeasured = 0;
    S.fifo.clear();
    S.count = 0;
    S.slots.clear();
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_soundlevel_bank_process_pcm16(bnhip_soundlevel_bank* b, int n_frames, const int* streams, const int16_t* const* frames,
                                        const int* n_in, bnhip_sound_level* reports, int max_reports, int* n_reports) {
    if (!b || !n_reports || max_reports < 0 || (max_reports > 0 && !reports)) return set_err(BNHIP_E_INVALID, "NULL argument");
    *n_reports = 0;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    return sl_run(b, n_frames, streams, frames, n_in, reports, max_reports, n_reports);
    BN_GUARD_END((void)0)
}

void bnhip_soundlevel_bank_destroy(bnhip_soundlevel_bank* b) {
    try { bank_free(b); } catch (...) {}
}

}  // extern "C"
