// C ABI of the clip loudness entries (bnhip_loudness_measure_pcm16, bnhip_loudness_normalize_pcm16, bnhip_loudness_workspace_size,
// bnhip_loudness_normalize_device) and of their forms for a ragged burst (bnhip_loudness_ragged_workspace_size,
// bnhip_loudness_ragged_normalize_pcm16, bnhip_loudness_ragged_normalize_device).  Each operation has one body over a Clips
// (ragged.h), which the entries of both forms call with their own names; every host-pointer entry takes its device memory as one DevCarve
// (api_oneshot.h).
#include <hip/hip_runtime.h>

#include <cmath>

#include "api_oneshot.h"
#include "loudness.h"

using namespace bnhip;

namespace {

// the coefficient table of one (device, rate, segment length); -> NULL on an allocation / copy failure
struct LoudTable { int device, rate, seg_len; double* d; };
TableCache<LoudTable> g_tables;
const LoudTable* loud_table(const TableLock& lk, int device, int rate, int seg_len) {
    return g_tables.find(lk, [&](const LoudTable& e) { return e.device == device && e.rate == rate && e.seg_len == seg_len; },
                         [&](LoudTable& e) { e = {device, rate, seg_len, upload_table(loudness_table(rate, seg_len))}; return e.d != nullptr; });
}

// validateDims' rate rule (audionorm.go:266-276); -> 0 or a negative BNHIP_E_*
int rate_check(int rate) {
    if (rate < LOUD_MIN_RATE) return set_err(BNHIP_E_INVALID, "sample rate too low; minimum is 8000 Hz (K-weighting is undefined below it)");
    return 0;
}
// what every entry checks before any device is touched
int dims_check(const Clips& c, int rate) {
    const int rc = clips_check(c);
    return rc ? rc : rate_check(rate);
}

// Options.validate (audionorm.go:278-293) and the clamp's magnitude
int plan_check(double target, double ceiling, double max_gain) {
    if (!std::isfinite(target)) return set_err(BNHIP_E_INVALID, "target loudness must be finite");
    if (target >= 0.0 || target <= -70.0) return set_err(BNHIP_E_INVALID, "target loudness out of range (-70, 0)");
    if (!std::isfinite(ceiling)) return set_err(BNHIP_E_INVALID, "true-peak ceiling must be finite");
    if (ceiling > 0.0) return set_err(BNHIP_E_INVALID, "true-peak ceiling must be <= 0");
    if (std::isnan(max_gain)) return set_err(BNHIP_E_INVALID, "max_gain_db must not be NaN");
    return 0;
}

LoudPlan make_plan(double target, double ceiling, double max_gain, int gate_fallback, int measure) {
    LoudPlan p;
    p.target = target; p.ceiling = ceiling; p.max_gain = std::fabs(max_gain);
    p.gate_abs = (double)(float)std::pow(10.0, (-70.0 - -0.691) / 10.0);          // absGateEnergy (meter.go:27-34)
    p.gate_rel = (double)(float)std::pow(10.0, -10.0 / 10.0);                       // relGateEnergyFactor
    p.gate_fallback = gate_fallback != 0; p.measure = measure;
    return p;
}

// the device (already made current) has its table looked up or uploaded, and the kernels of `plan` are enqueued on s
int enqueue(const char* what, int device, const int16_t* d_pcm, const Clips& c, int rate, const LoudPlan& plan, bnhip_loudness* d_out,
            int16_t* d_out_pcm, void* d_workspace, hipStream_t s) {
    const int S = loudness_sub_block(rate);
    TableLock lk(g_tables.mu);
    const LoudTable* tab = loud_table(lk, device, rate, S / loudness_split(c, S));
    if (!tab) return set_err(BNHIP_E_NOMEM, "device allocation failed (loudness table)");
    launch_loudness(d_pcm, loudness_work(c, S, d_workspace), tab->d, plan, d_out, d_out_pcm, s);
    return launch_status(what);
}

// the host-pointer form of every entry, after its checks: one DevCarve (the clips, the gained clips, the records, the workspace),
// one H2D copy, the kernels, the D2H copies
int run_pcm16(const char* what, int device, const int16_t* pcm, const Clips& c, int rate, const LoudPlan& plan, int16_t* out_pcm,
              bnhip_loudness* out, double* sub_energy) {
    int rc = use_device(device);
    if (rc) return rc;
    const int S = loudness_sub_block(rate);
    const size_t pcm_bytes = c.total() * 2, res_bytes = (size_t)c.n_clips * sizeof(bnhip_loudness);
    DevCarve cv;
    const size_t o_pcm = cv.add(pcm_bytes), o_out = out_pcm ? cv.add(pcm_bytes) : 0, o_res = cv.add(res_bytes);
    const size_t o_ws = cv.add(loudness_workspace_bytes(c, S));
    DevBlocks b;
    cv.alloc(b);
    int16_t* d_pcm = cv.at<int16_t>(o_pcm);
    int16_t* d_out_pcm = out_pcm ? cv.at<int16_t>(o_out) : nullptr;
    bnhip_loudness* d_res = cv.at<bnhip_loudness>(o_res);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail(what, b);
    rc = enqueue(what, device, d_pcm, c, rate, plan, d_res, d_out_pcm, cv.at<void>(o_ws), nullptr);
    if (rc) { hipDeviceSynchronize(); return rc; }
    // (the null stream orders the copies after the kernels; the first one is the call's synchronise)
    b.he = hipMemcpy(out, d_res, res_bytes, hipMemcpyDeviceToHost);
    if (b.he == hipSuccess && out_pcm) b.he = hipMemcpy(out_pcm, d_out_pcm, pcm_bytes, hipMemcpyDeviceToHost);
    if (b.he == hipSuccess && sub_energy) {
        const LoudWork w = loudness_work(c, S, cv.at<void>(o_ws));             // (E1: the sub-block energies, clip after clip)
        if (w.G > 0) b.he = hipMemcpy(sub_energy, w.E1, (size_t)(w.G / w.q) * 8, hipMemcpyDeviceToHost);
    }
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(what, b);
}

int workspace_size(const Clips& c, int rate, size_t* bytes) {
    const int rc = dims_check(c, rate);
    if (rc) return rc;
    *bytes = loudness_workspace_bytes(c, loudness_sub_block(rate));
    return BNHIP_OK;
}

// the device entries: `size_entry` is the bnhip_*_workspace_size a short workspace is told of
int normalize_device(const char* what, const char* size_entry, int device, const int16_t* d_pcm, const Clips& c, int rate, double target,
                     double ceiling, double max_gain, int gate_fallback, int16_t* d_out_pcm, bnhip_loudness* d_out, void* d_workspace,
                     size_t workspace_bytes, void* hip_stream) {
    int rc = loudness_args_check(c, rate, target, ceiling, max_gain);
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, loudness_workspace_bytes(c, loudness_sub_block(rate)), size_entry);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    return loudness_enqueue(what, device, d_pcm, c, rate, target, ceiling, max_gain, gate_fallback, d_out, d_out_pcm, d_workspace,
                            reinterpret_cast<hipStream_t>(hip_stream));
}

}  // namespace

namespace bnhip {

int loudness_args_check(const Clips& c, int rate, double target, double ceiling, double max_gain) {
    const int rc = dims_check(c, rate);
    return rc ? rc : plan_check(target, ceiling, max_gain);
}

int loudness_enqueue(const char* what, int device, const int16_t* d_pcm, const Clips& c, int rate, double target, double ceiling,
                     double max_gain, int gate_fallback, bnhip_loudness* d_out, int16_t* d_out_pcm, void* d_workspace, hipStream_t s) {
    return enqueue(what, device, d_pcm, c, rate, make_plan(target, ceiling, max_gain, gate_fallback, 0), d_out, d_out_pcm, d_workspace, s);
}

}  // namespace bnhip

extern "C" {

int bnhip_loudness_measure_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, bnhip_loudness* out, double* sub_energy) {
    if (!pcm || !out) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const Clips c = Clips::uniform(n_clips, n);
    const int rc = dims_check(c, rate);
    if (rc) return rc;
    return run_pcm16("loudness_measure_pcm16", device, pcm, c, rate, make_plan(-23.0, -1.0, 0.0, 0, 1), nullptr, out, sub_energy);
    BN_GUARD_END((void)0)
}

int bnhip_loudness_normalize_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, double target_lufs,
                                   double true_peak_dbtp, double max_gain_db, int gate_fallback, int16_t* out_pcm, bnhip_loudness* out) {
    if (!pcm || !out) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const Clips c = Clips::uniform(n_clips, n);
    const int rc = loudness_args_check(c, rate, target_lufs, true_peak_dbtp, max_gain_db);
    if (rc) return rc;
    return run_pcm16("loudness_normalize_pcm16", device, pcm, c, rate, make_plan(target_lufs, true_peak_dbtp, max_gain_db, gate_fallback, 0),
                     out_pcm, out, nullptr);
    BN_GUARD_END((void)0)
}

int bnhip_loudness_workspace_size(int n_clips, int n, int rate, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    return workspace_size(Clips::uniform(n_clips, n), rate, bytes);
}

int bnhip_loudness_normalize_device(int device, const int16_t* d_pcm, int n_clips, int n, int rate, double target_lufs,
                                    double true_peak_dbtp, double max_gain_db, int gate_fallback, int16_t* d_out_pcm,
                                    bnhip_loudness* d_out, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_pcm || !d_out || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    return normalize_device("loudness_normalize_device", "bnhip_loudness_workspace_size", device, d_pcm, Clips::uniform(n_clips, n), rate,
                            target_lufs, true_peak_dbtp, max_gain_db, gate_fallback, d_out_pcm, d_out, d_workspace, workspace_bytes, hip_stream);
    BN_GUARD_END((void)0)
}

int bnhip_loudness_ragged_workspace_size(int n_clips, const int* lens, int rate, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = lens_check(n_clips, lens);
    return rc ? rc : workspace_size(Clips::ragged(n_clips, lens), rate, bytes);
}

int bnhip_loudness_ragged_normalize_device(int device, const int16_t* d_pcm, int n_clips, const int* lens, int rate, double target_lufs,
                                           double true_peak_dbtp, double max_gain_db, int gate_fallback, int16_t* d_out_pcm,
                                           bnhip_loudness* d_out, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_pcm || !d_out || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int rc = lens_check(n_clips, lens);
    if (rc) return rc;
    return normalize_device("loudness_ragged_normalize_device", "bnhip_loudness_ragged_workspace_size", device, d_pcm,
                            Clips::ragged(n_clips, lens), rate, target_lufs, true_peak_dbtp, max_gain_db, gate_fallback, d_out_pcm, d_out,
                            d_workspace, workspace_bytes, hip_stream);
    BN_GUARD_END((void)0)
}

int bnhip_loudness_ragged_normalize_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, double target_lufs,
                                          double true_peak_dbtp, double max_gain_db, int gate_fallback, int16_t* out_pcm, bnhip_loudness* out) {
    if (!pcm || !out) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const Clips c = Clips::ragged(n_clips, lens);
    int rc = lens_check(n_clips, lens);
    if (!rc) rc = loudness_args_check(c, rate, target_lufs, true_peak_dbtp, max_gain_db);
    if (rc) return rc;
    return run_pcm16("loudness_ragged_normalize_pcm16", device, pcm, c, rate,
                     make_plan(target_lufs, true_peak_dbtp, max_gain_db, gate_fallback, 0), out_pcm, out, nullptr);
    BN_GUARD_END((void)0)
}

}  // extern "C"
