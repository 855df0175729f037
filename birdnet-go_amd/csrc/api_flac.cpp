// C ABI of the FLAC entries (bnhip_flac_max_bytes, bnhip_flac_workspace_size, bnhip_flac_encode_device, bnhip_flac_encode_pcm16,
// bnhip_loudness_flac_pcm16) and their forms with LPC predictors (bnhip_flac_lpc_workspace_size, bnhip_flac_lpc_encode_device,
// bnhip_flac_lpc_encode_pcm16, bnhip_loudness_flac_lpc_pcm16): the entries without are those called with lpc_order 0.  And the
// forms for a ragged burst (bnhip_flac_ragged_max_bytes, bnhip_flac_ragged_workspace_size, bnhip_flac_ragged_encode_device,
// bnhip_flac_ragged_encode_pcm16, bnhip_loudness_flac_ragged_pcm16).  Each operation has one body over a Clips (ragged.h), which
// the entries of both forms call with their own names; every host-pointer entry takes its device memory as one DevCarve
// (api_oneshot.h).
#include <hip/hip_runtime.h>

#include <cmath>

#include "api_oneshot.h"
#include "flac.h"
#include "loudness.h"

using namespace bnhip;

namespace {

// what every entry checks of its own arguments before any device is touched; -> 0 or a negative BNHIP_E_*
int params_check(int rate, int seek_interval, int lpc_order) {
    if (lpc_order < 0 || lpc_order > FLAC_MAX_LPC_ORDER) return set_err(BNHIP_E_INVALID, "lpc_order must be in [0, 8]");
    if (rate < 1 || rate > FLAC_MAX_RATE) return set_err(BNHIP_E_INVALID, "sample rate must be in [1, 1048575]");
    if (seek_interval < 0) return set_err(BNHIP_E_INVALID, "seek_interval must not be negative");
    return 0;
}
int dims_check(const Clips& c, int rate, int seek_interval, int lpc_order) {
    const int rc = clips_check(c);
    return rc ? rc : params_check(rate, seek_interval, lpc_order);
}

int factor_check(const double* factor, int n_clips) {
    if (factor)
        for (int i = 0; i < n_clips; i++)
            if (!std::isfinite(factor[i]) || factor[i] < 0.0) return set_err(BNHIP_E_INVALID, "factor must be finite and not negative");
    return 0;
}

// The two forms of an entry differ in the names their errors carry: the entry itself (`what`, for a runtime error) and the size
// entries a short buffer is told of.
struct Names { const char *what, *max_entry, *ws_entry; };

// `cap`: what the form's bnhip_flac_*max_bytes answers for these clips
int cap_check(size_t out_cap, size_t cap, const Names& nm) {
    if (out_cap < cap) return set_err(BNHIP_E_INVALID, std::string("out_cap smaller than ") + nm.max_entry);
    return 0;
}

int max_bytes(const Clips& c, int seek_interval, size_t* bytes) {
    const int rc = dims_check(c, 1, seek_interval, 0);
    if (rc) return rc;
    *bytes = flac_max_bytes(c, seek_interval);
    return BNHIP_OK;
}

int workspace_size(const Clips& c, int lpc_order, size_t* bytes) {
    const int rc = dims_check(c, 1, 0, lpc_order);
    if (rc) return rc;
    *bytes = flac_workspace_bytes(c, lpc_order);
    return BNHIP_OK;
}

int encode_device(const Names& nm, int device, const int16_t* d_pcm, const Clips& c, int rate, const double* d_factor, int seek_interval,
                  uint8_t* d_out, size_t out_cap, uint64_t* d_offsets, void* d_workspace, size_t workspace_bytes, void* hip_stream,
                  int lpc_order) {
    int rc = dims_check(c, rate, seek_interval, lpc_order);
    if (!rc) rc = cap_check(out_cap, flac_max_bytes(c, seek_interval), nm);
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, flac_workspace_bytes(c, lpc_order), nm.ws_entry);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    launch_flac(d_pcm, d_factor, flac_work(c, rate, seek_interval, d_workspace, lpc_order), d_out, out_cap, (unsigned long long*)d_offsets,
                reinterpret_cast<hipStream_t>(hip_stream));
    return launch_status(nm.what);
}

// the host-pointer encode: one DevCarve (the clips, the factors, the streams, the offsets, the workspace)
int encode_pcm16(const Names& nm, int device, const int16_t* pcm, const Clips& c, int rate, const double* factor, int seek_interval,
                 uint8_t* out, size_t out_cap, uint64_t* offsets, int lpc_order) {
    int rc = dims_check(c, rate, seek_interval, lpc_order);
    if (!rc) rc = factor_check(factor, c.n_clips);
    if (rc) return rc;
    const size_t cap = flac_max_bytes(c, seek_interval);
    rc = cap_check(out_cap, cap, nm);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    const size_t pcm_bytes = c.total() * 2;
    DevCarve cv;
    const size_t o_pcm = cv.add(pcm_bytes), o_fac = cv.add((size_t)c.n_clips * 8), o_bytes = cv.add(cap);
    const size_t o_off = cv.add(((size_t)c.n_clips + 1) * 8), o_ws = cv.add(flac_workspace_bytes(c, lpc_order));
    DevBlocks b;
    cv.alloc(b);
    int16_t* d_pcm = cv.at<int16_t>(o_pcm);
    double* d_factor = factor ? cv.at<double>(o_fac) : nullptr;
    uint8_t* d_bytes = cv.at<uint8_t>(o_bytes);
    unsigned long long* d_offsets = cv.at<unsigned long long>(o_off);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he == hipSuccess && factor) b.he = hipMemcpy(d_factor, factor, (size_t)c.n_clips * 8, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        launch_flac(d_pcm, d_factor, flac_work(c, rate, seek_interval, cv.at<void>(o_ws), lpc_order), d_bytes, cap, d_offsets, nullptr);
        b.he = hipGetLastError();
    }
    if (b.he == hipSuccess) b.he = fetch_streams(d_offsets, d_bytes, c.n_clips, offsets, out);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(nm.what, b);
}

// normalise, then encode: one DevCarve (the clips, the normalised clips, which never leave the device, the records, the streams,
// the offsets and both workspaces)
int loudness_flac_pcm16(const Names& nm, int device, const int16_t* pcm, const Clips& c, int rate, double target_lufs, double true_peak_dbtp,
                        double max_gain_db, int gate_fallback, int seek_interval, bnhip_loudness* out, uint8_t* out_bytes, size_t out_cap,
                        uint64_t* offsets, int lpc_order) {
    int rc = loudness_args_check(c, rate, target_lufs, true_peak_dbtp, max_gain_db);
    if (!rc) rc = params_check(rate, seek_interval, lpc_order);
    if (rc) return rc;
    const size_t cap = flac_max_bytes(c, seek_interval);
    rc = cap_check(out_cap, cap, nm);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    const size_t pcm_bytes = c.total() * 2, res_bytes = (size_t)c.n_clips * sizeof(bnhip_loudness);
    DevCarve cv;
    const size_t o_pcm = cv.add(pcm_bytes), o_gained = cv.add(pcm_bytes), o_res = cv.add(res_bytes), o_bytes = cv.add(cap);
    const size_t o_off = cv.add(((size_t)c.n_clips + 1) * 8);
    const size_t o_lws = cv.add(loudness_workspace_bytes(c, loudness_sub_block(rate))), o_fws = cv.add(flac_workspace_bytes(c, lpc_order));
    DevBlocks b;
    cv.alloc(b);
    int16_t* d_pcm = cv.at<int16_t>(o_pcm);
    int16_t* d_gained = cv.at<int16_t>(o_gained);
    bnhip_loudness* d_res = cv.at<bnhip_loudness>(o_res);
    uint8_t* d_bytes = cv.at<uint8_t>(o_bytes);
    unsigned long long* d_offsets = cv.at<unsigned long long>(o_off);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail(nm.what, b);
    rc = loudness_enqueue(nm.what, device, d_pcm, c, rate, target_lufs, true_peak_dbtp, max_gain_db, gate_fallback, d_res, d_gained,
                          cv.at<void>(o_lws), nullptr);
    if (rc) { hipDeviceSynchronize(); return rc; }
    launch_flac(d_gained, nullptr, flac_work(c, rate, seek_interval, cv.at<void>(o_fws), lpc_order), d_bytes, cap, d_offsets, nullptr);
    b.he = hipGetLastError();
    if (b.he == hipSuccess) b.he = hipMemcpy(out, d_res, res_bytes, hipMemcpyDeviceToHost);
    if (b.he == hipSuccess) b.he = fetch_streams(d_offsets, d_bytes, c.n_clips, offsets, out_bytes);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(nm.what, b);
}

}  // namespace

extern "C" {

int bnhip_flac_max_bytes(int n_clips, int n, int seek_interval, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    return max_bytes(Clips::uniform(n_clips, n), seek_interval, bytes);
}

int bnhip_flac_lpc_workspace_size(int n_clips, int n, int lpc_order, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    return workspace_size(Clips::uniform(n_clips, n), lpc_order, bytes);
}

int bnhip_flac_workspace_size(int n_clips, int n, size_t* bytes) { return bnhip_flac_lpc_workspace_size(n_clips, n, 0, bytes); }

int bnhip_flac_lpc_encode_device(int device, const int16_t* d_pcm, int n_clips, int n, int rate, const double* d_factor, int seek_interval,
                                 uint8_t* d_out, size_t out_cap, uint64_t* d_offsets, void* d_workspace, size_t workspace_bytes, void* hip_stream,
                                 int lpc_order) {
    if (!d_pcm || !d_out || !d_offsets || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const Names nm{"flac_encode_device", "bnhip_flac_max_bytes", lpc_order ? "bnhip_flac_lpc_workspace_size" : "bnhip_flac_workspace_size"};
    return encode_device(nm, device, d_pcm, Clips::uniform(n_clips, n), rate, d_factor, seek_interval, d_out, out_cap, d_offsets, d_workspace,
                         workspace_bytes, hip_stream, lpc_order);
    BN_GUARD_END((void)0)
}

int bnhip_flac_encode_device(int device, const int16_t* d_pcm, int n_clips, int n, int rate, const double* d_factor, int seek_interval,
                             uint8_t* d_out, size_t out_cap, uint64_t* d_offsets, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    return bnhip_flac_lpc_encode_device(device, d_pcm, n_clips, n, rate, d_factor, seek_interval, d_out, out_cap, d_offsets, d_workspace,
                                        workspace_bytes, hip_stream, 0);
}

int bnhip_flac_lpc_encode_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, const double* factor, int seek_interval,
                                uint8_t* out, size_t out_cap, uint64_t* offsets, int lpc_order) {
    if (!pcm || !out || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const Names nm{"flac_encode_pcm16", "bnhip_flac_max_bytes", nullptr};
    return encode_pcm16(nm, device, pcm, Clips::uniform(n_clips, n), rate, factor, seek_interval, out, out_cap, offsets, lpc_order);
    BN_GUARD_END((void)0)
}

int bnhip_flac_encode_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, const double* factor, int seek_interval,
                            uint8_t* out, size_t out_cap, uint64_t* offsets) {
    return bnhip_flac_lpc_encode_pcm16(device, pcm, n_clips, n, rate, factor, seek_interval, out, out_cap, offsets, 0);
}

int bnhip_loudness_flac_lpc_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, double target_lufs, double true_peak_dbtp,
                                  double max_gain_db, int gate_fallback, int seek_interval, bnhip_loudness* out, uint8_t* out_bytes,
                                  size_t out_cap, uint64_t* offsets, int lpc_order) {
    if (!pcm || !out || !out_bytes || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const Names nm{"loudness_flac_pcm16", "bnhip_flac_max_bytes", nullptr};
    return loudness_flac_pcm16(nm, device, pcm, Clips::uniform(n_clips, n), rate, target_lufs, true_peak_dbtp, max_gain_db, gate_fallback,
                               seek_interval, out, out_bytes, out_cap, offsets, lpc_order);
    BN_GUARD_END((void)0)
}

int bnhip_loudness_flac_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, double target_lufs, double true_peak_dbtp,
                              double max_gain_db, int gate_fallback, int seek_interval, bnhip_loudness* out, uint8_t* out_bytes, size_t out_cap,
                              uint64_t* offsets) {
    return bnhip_loudness_flac_lpc_pcm16(device, pcm, n_clips, n, rate, target_lufs, true_peak_dbtp, max_gain_db, gate_fallback, seek_interval, out,
                                         out_bytes, out_cap, offsets, 0);
}

int bnhip_flac_ragged_max_bytes(int n_clips, const int* lens, int seek_interval, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = lens_check(n_clips, lens);
    return rc ? rc : max_bytes(Clips::ragged(n_clips, lens), seek_interval, bytes);
}

int bnhip_flac_ragged_workspace_size(int n_clips, const int* lens, int lpc_order, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = lens_check(n_clips, lens);
    return rc ? rc : workspace_size(Clips::ragged(n_clips, lens), lpc_order, bytes);
}

int bnhip_flac_ragged_encode_device(int device, const int16_t* d_pcm, int n_clips, const int* lens, int rate, const double* d_factor,
                                    int seek_interval, uint8_t* d_out, size_t out_cap, uint64_t* d_offsets, void* d_workspace,
                                    size_t workspace_bytes, void* hip_stream, int lpc_order) {
    if (!d_pcm || !d_out || !d_offsets || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const Names nm{"flac_ragged_encode_device", "bnhip_flac_ragged_max_bytes", "bnhip_flac_ragged_workspace_size"};
    const int rc = lens_check(n_clips, lens);
    if (rc) return rc;
    return encode_device(nm, device, d_pcm, Clips::ragged(n_clips, lens), rate, d_factor, seek_interval, d_out, out_cap, d_offsets, d_workspace,
                         workspace_bytes, hip_stream, lpc_order);
    BN_GUARD_END((void)0)
}

int bnhip_flac_ragged_encode_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, const double* factor,
                                   int seek_interval, uint8_t* out, size_t out_cap, uint64_t* offsets, int lpc_order) {
    if (!pcm || !out || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const Names nm{"flac_ragged_encode_pcm16", "bnhip_flac_ragged_max_bytes", nullptr};
    const int rc = lens_check(n_clips, lens);
    if (rc) return rc;
    return encode_pcm16(nm, device, pcm, Clips::ragged(n_clips, lens), rate, factor, seek_interval, out, out_cap, offsets, lpc_order);
    BN_GUARD_END((void)0)
}

int bnhip_loudness_flac_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, double target_lufs,
                                     double true_peak_dbtp, double max_gain_db, int gate_fallback, int seek_interval, bnhip_loudness* out,
                                     uint8_t* out_bytes, size_t out_cap, uint64_t* offsets, int lpc_order) {
    if (!pcm || !out || !out_bytes || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const Names nm{"loudness_flac_ragged_pcm16", "bnhip_flac_ragged_max_bytes", nullptr};
    const int rc = lens_check(n_clips, lens);
    if (rc) return rc;
    return loudness_flac_pcm16(nm, device, pcm, Clips::ragged(n_clips, lens), rate, target_lufs, true_peak_dbtp, max_gain_db, gate_fallback,
                               seek_interval, out, out_bytes, out_cap, offsets, lpc_order);
    BN_GUARD_END((void)0)
}

}  // extern "C"
