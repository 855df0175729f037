// C ABI of the channel measurement alone (channels.h): the per-channel energies of multichannel recordings and what "auto" picks.
#include <cmath>

#include "analyze_recordings.h"

using namespace bnhip;

static_assert(sizeof(bnhip_channel_energy) == 24, "a channel's energy record is 24 bytes");

namespace {

// computeRmsDbfs (ffmpeg/analyze.go) from a channel's exact sum of squares, in 16-bit units: rms16 = sqrt(E / length) / 2^(bits - 16);
// below 1 the reference answers -96
double channel_rms_dbfs(unsigned long long lo, unsigned long long hi, int bits, long long length) {
    const double e = (double)hi * 18446744073709551616.0 + (double)lo;
    const double rms16 = std::sqrt(e / (double)length) / (double)(1ll << (bits - 16));
    return rms16 < 1.0 ? -96.0 : 20.0 * std::log10(rms16 / 32768.0);
}

}  // namespace

extern "C" {

// one DevCarve (the raw block, the descriptors and tile prefix, the partials, the sums, the decisions), one H2D copy per recording,
// the two launches, the sums and decisions down
int bnhip_channel_energy_pcm(int device, const void* pcm, const bnhip_channels_recording* recs, int n_recordings, bnhip_channel_energy* out,
                             int32_t* chosen) {
    BN_GUARD_BEGIN
    const char* what = "channel_energy_pcm";
    if (!pcm || !out) return set_err(BNHIP_E_INVALID, "NULL argument");
    Recordings rec;
    if (int rc = channels_check(recs, n_recordings, true, &rec)) return rc;
    size_t raw_bytes = 0;
    for (int r = 0; r < n_recordings; r++) {
        if (int rc = recording_check(rec.recs[r], r, false)) return rc;
        raw_bytes += rec.raw_footprint(r);
    }
    const EnergyPlan en = energy_plan(rec, true);
    if (int rc = use_device(device)) return rc;
    DevCarve cv;
    const size_t o_raw = cv.add(raw_bytes), o_desc = cv.add(en.desc.size() * sizeof(EnergyDesc)), o_tile0 = cv.add(en.tile0.size() * 8);
    const size_t o_part = cv.add((size_t)en.n_tiles() * ENERGY_ROW_BYTES), o_sums = cv.add((size_t)n_recordings * ENERGY_ROW_BYTES);
    const size_t o_sel = cv.add((size_t)n_recordings * 4);
    DevBlocks b;
    cv.alloc(b);
    const char* src = static_cast<const char*>(pcm);
    for (int r = 0; r < n_recordings; src += rec.raw_bytes(r), r++)
        AN_HIP(b, hipMemcpy(cv.at<char>(o_raw) + en.desc[r].in_off, src, rec.raw_bytes(r), hipMemcpyHostToDevice));
    AN_HIP(b, hipMemcpy(cv.at<void>(o_desc), en.desc.data(), en.desc.size() * sizeof(EnergyDesc), hipMemcpyHostToDevice));
    AN_HIP(b, hipMemcpy(cv.at<void>(o_tile0), en.tile0.data(), en.tile0.size() * 8, hipMemcpyHostToDevice));
    if (b.he != hipSuccess) return hip_fail(what, b);
    launch_channel_energy(cv.at<void>(o_raw), cv.at<EnergyDesc>(o_desc), cv.at<long long>(o_tile0), n_recordings, en.n_tiles(),
                          cv.at<unsigned long long>(o_part), cv.at<unsigned long long>(o_sums), cv.at<int>(o_sel), nullptr);
    if (int rc = launch_status(what)) { hipDeviceSynchronize(); return rc; }
    // (the null stream orders the copies after the kernels; the first one is the call's synchronise)
    std::vector<unsigned long long> sums((size_t)n_recordings * 2 * CHANNELS_MAX);
    std::vector<int32_t> sel(n_recordings);
    AN_HIP(b, hipMemcpy(sums.data(), cv.at<void>(o_sums), sums.size() * 8, hipMemcpyDeviceToHost));
    AN_HIP(b, hipMemcpy(sel.data(), cv.at<void>(o_sel), sel.size() * 4, hipMemcpyDeviceToHost));
    if (b.he != hipSuccess) return hip_fail(what, b);
    bnhip_channel_energy* o = out;
    for (int r = 0; r < n_recordings; r++) {
        for (int c = 0; c < rec.channels[r]; c++, o++) {
            o->sum_lo = sums[((size_t)r * CHANNELS_MAX + c) * 2];
            o->sum_hi = sums[((size_t)r * CHANNELS_MAX + c) * 2 + 1];
            o->rms_dbfs = channel_rms_dbfs(o->sum_lo, o->sum_hi, rec.recs[r].bits_per_sample, rec.recs[r].length);
        }
        if (chosen) chosen[r] = sel[r];
    }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

}  // extern "C"
