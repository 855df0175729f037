// C ABI of the equalizer bank and the filter designer.
#include <hip/hip_runtime.h>

#include <cmath>

#include "eq_bank.h"
#include "stream_bank.h"

using namespace bnhip;

// ------------------------------------------------------------------------------------------------ equalizer bank
// The analysis route's EQ + gain (AudioRouter.applyProcessing, internal/audiocore/router.go:1006-1080, the route the analysis
// BufferConsumer gets from AddRoute with the source's chain and gain, internal/analysis/audio_pipeline_service.go:1005-1006)
// for every source of a bank at once, one k_eq_bank launch per call.  The chains live on the host and travel with each call
// (descriptors | coefficients | PCM16), so set_chain and reset touch no device memory; each stream's filter state is a fixed
// pair of device slabs of EQ_MAX_STAGES x {in1, in2, out1, out2} doubles.
struct EqStream {
    bool fresh = true;                  // the next call starts from zero state (new stream, new chain, reset)
    int n_stages = 0;
    double gain = 1.0;
    double coef[EQ_MAX_STAGES][5] = {};   // {b0, b1, b2, a1, a2} / a0 per stage: filter f, pass p, in chain order
    bool passthrough() const { return n_stages == 0 && gain == 1.0; }
};

constexpr int EQ_SLAB = EQ_MAX_STAGES * 4;     // doubles of one state slab

struct bnhip_eq_bank : StreamBank<EqStream> {
    static constexpr const char* what = "equalizer bank";
    double* d_state = nullptr;          // [max_streams][2][EQ_MAX_STAGES][4]
    ~bnhip_eq_bank() { if (d_state) hipFree(d_state); }

    // Every frame's output has as many samples as its input.  A pass-through stream (no stages, gain 1) is not converted: its frames
    // are delivered as they are, as the reference skips the route's processing (router.go:848).  (flush is always false here.)
    template <class Deliver>
    int run(int n_frames, const int* streams, const int16_t* const* frames, const int* n_in, bool flush,
            long long out_cap, Deliver deliver) {
        std::vector<EqBankDesc> desc;
        std::vector<double> coef;
        auto plan = [&](std::vector<BankGroup>& groups, const std::vector<int>&, std::vector<long long>&) -> int {
            for (BankGroup& g : groups) {
                g.pass = st[g.stream].passthrough();
                g.run = g.n_in > 0 && !g.pass;
            }
            return BNHIP_OK;
        };
        auto describe = [&](const std::vector<BankGroup>& groups, long long in_total, long long, BankBlob* hdr) -> int {
            if (in_total > INT32_MAX / 4) return set_err(BNHIP_E_INVALID, "equalizer bank call too large");
            for (const BankGroup& g : groups) {
                if (!g.run) continue;
                const auto& S = st[g.stream];
                EqBankDesc d{};
                d.gain = S.gain; d.in_off = g.in_off; d.n = (int)g.n_in; d.n_stages = S.n_stages;
                d.coef_off = (int)coef.size();
                for (int s = 0; s < S.n_stages; s++) coef.insert(coef.end(), S.coef[s], S.coef[s] + 5);
                d.st_rd = S.fresh ? -1 : (g.stream * 2 + S.parity) * EQ_SLAB;
                d.st_wr = (g.stream * 2 + (S.parity ^ 1)) * EQ_SLAB;
                desc.push_back(d);
            }
            // a wave runs 4 streams, every row of it as many steps as its longest
            for (size_t k0 = 0; k0 < desc.size(); k0 += 4) {
                long long steps = 0;
                for (size_t k = k0; k < std::min(desc.size(), k0 + 4); k++)
                    steps = std::max<long long>(steps, desc[k].n + std::max(desc[k].n_stages, 1) - 1);
                desc[k0].blk_steps = (int)((steps + 15) / 16 * 16);
            }
            hdr[0] = {desc.data(), desc.size() * sizeof(EqBankDesc)};
            hdr[1] = {coef.data(), coef.size() * sizeof(double)};
            return BNHIP_OK;
        };
        auto launch = [&](const uint8_t* d_hdr, const int16_t* d_pcm, int16_t* d_out) -> int {
            return launch_eq_bank(reinterpret_cast<const EqBankDesc*>(d_hdr), (int)desc.size(),
                                  reinterpret_cast<const double*>(d_hdr + desc.size() * sizeof(EqBankDesc)), d_pcm, d_state, d_out, stream);
        };
        auto commit = [&](const BankGroup& g, size_t) {
            auto& S = st[g.stream];
            S.parity ^= 1;
            S.fresh = false;
        };
        return bank_call(this, n_frames, streams, frames, n_in, flush, out_cap, plan, describe, launch, commit, deliver);
    }
};

namespace {

// RBJ audio-EQ-cookbook biquads (R. Bristow-Johnson, "Cookbook formulae for audio EQ biquad filter coefficients"), raw
// {b0, b1, b2, a0, a1, a2}.  w0 = 2 pi f / Fs; alpha = sin(w0) / (2 Q), or for a bandwidth in octaves
// alpha = sin(w0) sinh(ln(2) / 2 * BW * w0 / sin(w0)); A = 10^(dBgain / 40).
double eq_hz_to_octaves(double f, double width) {         // equalizer.go hzToOctaves: the band's lower edge stays above 1 Hz
    double half = width / 2.0;
    if (half >= f - 1.0) half = f - 1.0;
    if (half <= 0) half = 0.01;
    double lower = f - half;
    if (lower <= 0) lower = 0.01;
    return std::log2((f + half) / lower);
}

int eq_design(int type, double fs, double f, double q, double width, double gain_db, int passes, double* o) {
    if (passes < 1) return set_err(BNHIP_E_INVALID, "passes must be 1 or greater");
    const bool by_width = type == BNHIP_EQ_BANDPASS || type == BNHIP_EQ_BANDREJECT || type == BNHIP_EQ_PEAKING;
    if (by_width && f <= 0) return set_err(BNHIP_E_INVALID, "frequency must be greater than 0");
    if (by_width && width <= 0) return set_err(BNHIP_E_INVALID, "width must be greater than 0");
    const double w0 = 2.0 * M_PI * f / fs, cw = std::cos(w0), sw = std::sin(w0);
    const double alpha = by_width ? sw * std::sinh(std::log(2.0) / 2.0 * eq_hz_to_octaves(f, width) * w0 / sw) : sw / (2.0 * q);
    const double A = std::pow(10.0, gain_db / 40.0);
    double b0, b1, b2, a0, a1, a2;
    switch (type) {
    case BNHIP_EQ_LOWPASS:
        b0 = (1.0 - cw) / 2.0; b1 = 1.0 - cw; b2 = b0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
    case BNHIP_EQ_HIGHPASS:
        b0 = (1.0 + cw) / 2.0; b1 = -(1.0 + cw); b2 = b0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
    case BNHIP_EQ_ALLPASS:
        b0 = 1.0 - alpha; b1 = -2.0 * cw; b2 = 1.0 + alpha; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
    case BNHIP_EQ_BANDPASS:        // constant 0 dB peak gain
        b0 = alpha; b1 = 0.0; b2 = -alpha; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
    case BNHIP_EQ_BANDREJECT:
        b0 = 1.0; b1 = -2.0 * cw; b2 = 1.0; a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha; break;
    case BNHIP_EQ_LOWSHELF: {
        const double bs = std::sqrt(A) / q * sw;     // 2 sqrt(A) alpha with the shelf's Q
        b0 = A * ((A + 1.0) - (A - 1.0) * cw + bs); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cw); b2 = A * ((A + 1.0) - (A - 1.0) * cw - bs);
        a0 = (A + 1.0) + (A - 1.0) * cw + bs; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cw); a2 = (A + 1.0) + (A - 1.0) * cw - bs;
        break;
    }
    case BNHIP_EQ_HIGHSHELF: {
        const double bs = std::sqrt(A) / q * sw;
        b0 = A * ((A + 1.0) + (A - 1.0) * cw + bs); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cw); b2 = A * ((A + 1.0) + (A - 1.0) * cw - bs);
        a0 = (A + 1.0) - (A - 1.0) * cw + bs; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cw); a2 = (A + 1.0) - (A - 1.0) * cw - bs;
        break;
    }
    case BNHIP_EQ_PEAKING:
        b0 = 1.0 + alpha * A; b1 = -2.0 * cw; b2 = 1.0 - alpha * A; a0 = 1.0 + alpha / A; a1 = -2.0 * cw; a2 = 1.0 - alpha / A; break;
    default:
        return set_err(BNHIP_E_INVALID, "unknown filter type " + std::to_string(type));
    }
    const double r[6] = {b0, b1, b2, a0, a1, a2};
    for (double v : r)
        if (!std::isfinite(v)) return set_err(BNHIP_E_INVALID, "filter parameters give non-finite coefficients");
    if (a0 == 0.0) return set_err(BNHIP_E_INVALID, "filter parameters give a0 == 0");
    memcpy(o, r, sizeof r);
    return BNHIP_OK;
}

}  // namespace

extern "C" {

int bnhip_eq_bank_create(int device, int max_streams, bnhip_eq_bank** out) {
    if (!out) return set_err(BNHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (max_streams < 1 || max_streams > (1 << 20)) return set_err(BNHIP_E_INVALID, "max_streams must be in [1, 1048576]");
    BN_GUARD_BEGIN
    int rc = use_device(device);
    if (rc) return rc;
    return bank_create(device, max_streams, out, [&](bnhip_eq_bank& b) {
        return hipMalloc((void**)&b.d_state, (size_t)max_streams * 2 * EQ_SLAB * sizeof(double));
    });
    BN_GUARD_END((void)0)
}

int bnhip_eq_bank_add_stream(bnhip_eq_bank* b, int* out_stream) { return bank_add_stream(b, out_stream); }
int bnhip_eq_bank_remove_stream(bnhip_eq_bank* b, int stream) { return bank_remove_stream(b, stream); }

int bnhip_eq_bank_set_chain(bnhip_eq_bank* b, int stream, const double* sections, int n_sections, const int* passes, double gain_linear) {
    if (!b || n_sections < 0 || (n_sections > 0 && (!sections || !passes))) return set_err(BNHIP_E_INVALID, "bad equalizer chain arguments");
    if (!std::isfinite(gain_linear)) return set_err(BNHIP_E_INVALID, "gain is not finite");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (int rc = bank_stream_check(b, stream)) return rc;
    bnhip_eq_bank::Stream ns;
    long long stages = 0;
    for (int k = 0; k < n_sections; k++) {
        const double* c = sections + 6 * k;           // {b0, b1, b2, a0, a1, a2}
        for (int j = 0; j < 6; j++)
            if (!std::isfinite(c[j])) return set_err(BNHIP_E_INVALID, "section " + std::to_string(k) + " has a non-finite coefficient");
        if (c[3] == 0.0) return set_err(BNHIP_E_INVALID, "section " + std::to_string(k) + " has a0 == 0");
        if (passes[k] < 1) return set_err(BNHIP_E_INVALID, "passes must be 1 or greater");
        stages += passes[k];
        if (stages > EQ_MAX_STAGES)
            return set_err(BNHIP_E_UNSUPPORTED, "equalizer chain has more than " + std::to_string(EQ_MAX_STAGES) + " stages (filters x passes)");
        // NewFilter's precomputed coefficients (equalizer.go:112-136): each divided by a0
        const double n5[5] = {c[0] / c[3], c[1] / c[3], c[2] / c[3], c[4] / c[3], c[5] / c[3]};
        for (int p = 0; p < passes[k]; p++) memcpy(ns.coef[ns.n_stages++], n5, sizeof n5);
    }
    ns.gain = gain_linear;
    ns.live = true;
    b->st[stream] = ns;                                   // a fresh chain: zero state (UpdateFilterChain installs new filters)
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_eq_bank_reset(bnhip_eq_bank* b, int stream) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (int rc = bank_stream_check(b, stream)) return rc;
    b->st[stream].fresh = true;
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_eq_bank_process_pcm16(bnhip_eq_bank* b, int n_frames, const int* streams, const int16_t* const* frames, const int* n_in,
                                int16_t* out, size_t out_cap, int* out_count) {
    return bank_to_buffer(b, n_frames, streams, frames, n_in, false, out, out_cap, out_count);
}

int bnhip_windows_write_equalized(bnhip_windows* w, bnhip_eq_bank* b, int n_frames, const int* streams, const int* sources,
                                  const int16_t* const* frames, const int* n_in) {
    return bank_to_rings(w, b, n_frames, streams, sources, frames, n_in);
}

int bnhip_eq_design(int type, double sample_rate, double frequency, double q, double width_hz, double gain_db, int passes,
                    double* section6) {
    if (!section6) return set_err(BNHIP_E_INVALID, "section6 is NULL");
    if (!std::isfinite(sample_rate) || !std::isfinite(frequency) || !std::isfinite(q) || !std::isfinite(width_hz) ||
        !std::isfinite(gain_db) || sample_rate <= 0)
        return set_err(BNHIP_E_INVALID, "filter parameters must be finite and the sample rate positive");
    BN_GUARD_BEGIN
    return eq_design(type, sample_rate, frequency, q, width_hz, gain_db, passes, section6);
    BN_GUARD_END((void)0)
}

void bnhip_eq_bank_destroy(bnhip_eq_bank* b) {
    try { bank_free(b); } catch (...) {}
}

}  // extern "C"
