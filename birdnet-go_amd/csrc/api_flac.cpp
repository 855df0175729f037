// C ABI of the FLAC entries (bnhip_flac_max_bytes, bnhip_flac_workspace_size, bnhip_flac_encode_device, bnhip_flac_encode_pcm16,
// bnhip_loudness_flac_pcm16) and their forms with LPC predictors (bnhip_flac_lpc_workspace_size, bnhip_flac_lpc_encode_device,
// bnhip_flac_lpc_encode_pcm16, bnhip_loudness_flac_lpc_pcm16): the entries without are those called with lpc_order 0.  And the
// forms for a ragged burst (bnhip_flac_ragged_max_bytes, bnhip_flac_ragged_workspace_size, bnhip_flac_ragged_encode_device,
// bnhip_flac_ragged_encode_pcm16, bnhip_loudness_flac_ragged_pcm16), whose host-pointer entries take one device block per call.
#include <hip/hip_runtime.h>

#include <cmath>

#include "api_oneshot.h"
#include "flac.h"
#include "loudness.h"

using namespace bnhip;

namespace {

// what every entry checks before any device is touched; -> 0 or a negative BNHIP_E_*
int dims_check(int n_clips, int n, int rate, int seek_interval, int lpc_order = 0) {
    if (const int rc = clip_dims_check(n_clips, n)) return rc;
    if (lpc_order < 0 || lpc_order > FLAC_MAX_LPC_ORDER) return set_err(BNHIP_E_INVALID, "lpc_order must be in [0, 8]");
    if (rate < 1 || rate > FLAC_MAX_RATE) return set_err(BNHIP_E_INVALID, "sample rate must be in [1, 1048575]");
    if (seek_interval < 0) return set_err(BNHIP_E_INVALID, "seek_interval must not be negative");
    return 0;
}

int ragged_dims_check(int n_clips, const int* lens, int rate, int seek_interval, int lpc_order = 0) {
    if (const int rc = ragged_lens_check(n_clips, lens)) return rc;
    return dims_check(1, 1, rate, seek_interval, lpc_order);
}

int factor_check(const double* factor, int n_clips) {
    if (factor)
        for (int i = 0; i < n_clips; i++)
            if (!std::isfinite(factor[i]) || factor[i] < 0.0) return set_err(BNHIP_E_INVALID, "factor must be finite and not negative");
    return 0;
}

int cap_check(int n_clips, int n, int seek_interval, size_t out_cap) {
    if (out_cap < flac_max_bytes(n_clips, n, seek_interval)) return set_err(BNHIP_E_INVALID, "out_cap smaller than bnhip_flac_max_bytes");
    return 0;
}

// offsets first (that copy is the call's synchronise), then exactly offsets[n_clips] bytes
hipError_t fetch(const unsigned long long* d_offsets, const uint8_t* d_bytes, int n_clips, uint64_t* offsets, uint8_t* out) {
    hipError_t he = hipMemcpy(offsets, d_offsets, ((size_t)n_clips + 1) * 8, hipMemcpyDeviceToHost);
    if (he == hipSuccess && offsets[n_clips] > 0) he = hipMemcpy(out, d_bytes, (size_t)offsets[n_clips], hipMemcpyDeviceToHost);
    return he;
}

}  // namespace

extern "C" {

int bnhip_flac_max_bytes(int n_clips, int n, int seek_interval, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = dims_check(n_clips, n, 1, seek_interval);
    if (rc) return rc;
    *bytes = flac_max_bytes(n_clips, n, seek_interval);
    return BNHIP_OK;
}

int bnhip_flac_lpc_workspace_size(int n_clips, int n, int lpc_order, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = dims_check(n_clips, n, 1, 0, lpc_order);
    if (rc) return rc;
    *bytes = flac_workspace_bytes(n_clips, n, lpc_order);
    return BNHIP_OK;
}

int bnhip_flac_workspace_size(int n_clips, int n, size_t* bytes) { return bnhip_flac_lpc_workspace_size(n_clips, n, 0, bytes); }

int bnhip_flac_lpc_encode_device(int device, const int16_t* d_pcm, int n_clips, int n, int rate, const double* d_factor, int seek_interval,
                                 uint8_t* d_out, size_t out_cap, uint64_t* d_offsets, void* d_workspace, size_t workspace_bytes, void* hip_stream,
                                 int lpc_order) {
    if (!d_pcm || !d_out || !d_offsets || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = dims_check(n_clips, n, rate, seek_interval, lpc_order);
    if (!rc) rc = cap_check(n_clips, n, seek_interval, out_cap);
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, flac_workspace_bytes(n_clips, n, lpc_order),
                                  lpc_order ? "bnhip_flac_lpc_workspace_size" : "bnhip_flac_workspace_size");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    launch_flac(d_pcm, d_factor, flac_work(n_clips, n, rate, seek_interval, d_workspace, lpc_order), d_out, out_cap,
                (unsigned long long*)d_offsets, reinterpret_cast<hipStream_t>(hip_stream));
    return launch_status("flac_encode_device");
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
    int rc = dims_check(n_clips, n, rate, seek_interval, lpc_order);
    if (rc) return rc;
    rc = factor_check(factor, n_clips);
    if (!rc) rc = cap_check(n_clips, n, seek_interval, out_cap);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    const size_t pcm_bytes = (size_t)n_clips * n * 2, cap = flac_max_bytes(n_clips, n, seek_interval);
    DevBlocks b;
    int16_t* d_pcm = (int16_t*)b.get(pcm_bytes);
    double* d_factor = factor ? (double*)b.get((size_t)n_clips * 8) : nullptr;
    uint8_t* d_bytes = (uint8_t*)b.get(cap);
    unsigned long long* d_offsets = (unsigned long long*)b.get(((size_t)n_clips + 1) * 8);
    void* d_ws = b.get(flac_workspace_bytes(n_clips, n, lpc_order));
    if (b.he == hipSuccess) b.he = hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he == hipSuccess && factor) b.he = hipMemcpy(d_factor, factor, (size_t)n_clips * 8, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        launch_flac(d_pcm, d_factor, flac_work(n_clips, n, rate, seek_interval, d_ws, lpc_order), d_bytes, cap, d_offsets, nullptr);
        b.he = hipGetLastError();
    }
    if (b.he == hipSuccess) b.he = fetch(d_offsets, d_bytes, n_clips, offsets, out);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("flac_encode_pcm16", b);
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
    int rc = loudness_args_check(n_clips, n, rate, target_lufs, true_peak_dbtp, max_gain_db);
    if (!rc) rc = dims_check(n_clips, n, rate, seek_interval, lpc_order);
    if (!rc) rc = cap_check(n_clips, n, seek_interval, out_cap);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    const size_t pcm_bytes = (size_t)n_clips * n * 2, cap = flac_max_bytes(n_clips, n, seek_interval);
    DevBlocks b;
    int16_t* d_pcm = (int16_t*)b.get(pcm_bytes);
    int16_t* d_gained = (int16_t*)b.get(pcm_bytes);                 // the normalised clips never leave the device
    bnhip_loudness* d_res = (bnhip_loudness*)b.get((size_t)n_clips * sizeof(bnhip_loudness));
    void* d_lws = b.get(loudness_workspace_bytes(n_clips, n, loudness_sub_block(rate)));
    uint8_t* d_bytes = (uint8_t*)b.get(cap);
    unsigned long long* d_offsets = (unsigned long long*)b.get(((size_t)n_clips + 1) * 8);
    void* d_fws = b.get(flac_workspace_bytes(n_clips, n, lpc_order));
    if (b.he == hipSuccess) b.he = hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail("loudness_flac_pcm16", b);
    rc = loudness_enqueue("loudness_flac_pcm16", device, d_pcm, n_clips, n, rate, target_lufs, true_peak_dbtp, max_gain_db, gate_fallback, d_res,
                          d_gained, d_lws, nullptr);
    if (rc) { hipDeviceSynchronize(); return rc; }
    launch_flac(d_gained, nullptr, flac_work(n_clips, n, rate, seek_interval, d_fws, lpc_order), d_bytes, cap, d_offsets, nullptr);
    b.he = hipGetLastError();
    if (b.he == hipSuccess) b.he = hipMemcpy(out, d_res, (size_t)n_clips * sizeof(bnhip_loudness), hipMemcpyDeviceToHost);
    if (b.he == hipSuccess) b.he = fetch(d_offsets, d_bytes, n_clips, offsets, out_bytes);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("loudness_flac_pcm16", b);
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
    const int rc = ragged_dims_check(n_clips, lens, 1, seek_interval);
    if (rc) return rc;
    *bytes = flac_ragged_max_bytes(n_clips, lens, seek_interval);
    return BNHIP_OK;
}

int bnhip_flac_ragged_workspace_size(int n_clips, const int* lens, int lpc_order, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = ragged_dims_check(n_clips, lens, 1, 0, lpc_order);
    if (rc) return rc;
    *bytes = flac_ragged_workspace_bytes(n_clips, lens, lpc_order);
    return BNHIP_OK;
}

int bnhip_flac_ragged_encode_device(int device, const int16_t* d_pcm, int n_clips, const int* lens, int rate, const double* d_factor,
                                    int seek_interval, uint8_t* d_out, size_t out_cap, uint64_t* d_offsets, void* d_workspace,
                                    size_t workspace_bytes, void* hip_stream, int lpc_order) {
    if (!d_pcm || !d_out || !d_offsets || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = ragged_dims_check(n_clips, lens, rate, seek_interval, lpc_order);
    if (!rc && out_cap < flac_ragged_max_bytes(n_clips, lens, seek_interval))
        rc = set_err(BNHIP_E_INVALID, "out_cap smaller than bnhip_flac_ragged_max_bytes");
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, flac_ragged_workspace_bytes(n_clips, lens, lpc_order),
                                  "bnhip_flac_ragged_workspace_size");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    launch_flac(d_pcm, d_factor, flac_ragged_work(n_clips, lens, rate, seek_interval, d_workspace, lpc_order), d_out, out_cap,
                (unsigned long long*)d_offsets, reinterpret_cast<hipStream_t>(hip_stream));
    return launch_status("flac_ragged_encode_device");
    BN_GUARD_END((void)0)
}

int bnhip_flac_ragged_encode_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, const double* factor,
                                   int seek_interval, uint8_t* out, size_t out_cap, uint64_t* offsets, int lpc_order) {
    if (!pcm || !out || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = ragged_dims_check(n_clips, lens, rate, seek_interval, lpc_order);
    if (!rc) rc = factor_check(factor, n_clips);
    if (rc) return rc;
    const size_t cap = flac_ragged_max_bytes(n_clips, lens, seek_interval);
    if (out_cap < cap) return set_err(BNHIP_E_INVALID, "out_cap smaller than bnhip_flac_ragged_max_bytes");
    rc = use_device(device);
    if (rc) return rc;
    // one device block: the clips, the factors, the streams, the offsets, the workspace
    const size_t pcm_bytes = ragged_total(n_clips, lens) * 2;
    DevCarve cv;
    const size_t o_pcm = cv.add(pcm_bytes), o_fac = cv.add((size_t)n_clips * 8), o_bytes = cv.add(cap), o_off = cv.add(((size_t)n_clips + 1) * 8);
    const size_t o_ws = cv.add(flac_ragged_workspace_bytes(n_clips, lens, lpc_order));
    DevBlocks b;
    cv.base = (char*)b.get(cv.bytes());
    int16_t* d_pcm = cv.at<int16_t>(o_pcm);
    double* d_factor = factor ? cv.at<double>(o_fac) : nullptr;
    uint8_t* d_bytes = cv.at<uint8_t>(o_bytes);
    unsigned long long* d_offsets = cv.at<unsigned long long>(o_off);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he == hipSuccess && factor) b.he = hipMemcpy(d_factor, factor, (size_t)n_clips * 8, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        launch_flac(d_pcm, d_factor, flac_ragged_work(n_clips, lens, rate, seek_interval, cv.at<void>(o_ws), lpc_order), d_bytes, cap, d_offsets,
                    nullptr);
        b.he = hipGetLastError();
    }
    if (b.he == hipSuccess) b.he = fetch(d_offsets, d_bytes, n_clips, offsets, out);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("flac_ragged_encode_pcm16", b);
    BN_GUARD_END((void)0)
}

int bnhip_loudness_flac_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, double target_lufs,
                                     double true_peak_dbtp, double max_gain_db, int gate_fallback, int seek_interval, bnhip_loudness* out,
                                     uint8_t* out_bytes, size_t out_cap, uint64_t* offsets, int lpc_order) {
    if (!pcm || !out || !out_bytes || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = loudness_ragged_args_check(n_clips, lens, rate, target_lufs, true_peak_dbtp, max_gain_db);
    if (!rc) rc = ragged_dims_check(n_clips, lens, rate, seek_interval, lpc_order);
    if (rc) return rc;
    const size_t cap = flac_ragged_max_bytes(n_clips, lens, seek_interval);
    if (out_cap < cap) return set_err(BNHIP_E_INVALID, "out_cap smaller than bnhip_flac_ragged_max_bytes");
    rc = use_device(device);
    if (rc) return rc;
    // one device block: the clips, the normalised clips (they never leave the device), the records, the streams, the offsets and
    // both workspaces
    const size_t pcm_bytes = ragged_total(n_clips, lens) * 2, res_bytes = (size_t)n_clips * sizeof(bnhip_loudness);
    DevCarve cv;
    const size_t o_pcm = cv.add(pcm_bytes), o_gained = cv.add(pcm_bytes), o_res = cv.add(res_bytes), o_bytes = cv.add(cap);
    const size_t o_off = cv.add(((size_t)n_clips + 1) * 8);
    const size_t o_lws = cv.add(loudness_ragged_workspace_bytes(n_clips, lens, loudness_sub_block(rate)));
    const size_t o_fws = cv.add(flac_ragged_workspace_bytes(n_clips, lens, lpc_order));
    DevBlocks b;
    cv.base = (char*)b.get(cv.bytes());
    int16_t* d_pcm = cv.at<int16_t>(o_pcm);
    int16_t* d_gained = cv.at<int16_t>(o_gained);
    bnhip_loudness* d_res = cv.at<bnhip_loudness>(o_res);
    uint8_t* d_bytes = cv.at<uint8_t>(o_bytes);
    unsigned long long* d_offsets = cv.at<unsigned long long>(o_off);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail("loudness_flac_ragged_pcm16", b);
    rc = loudness_ragged_enqueue("loudness_flac_ragged_pcm16", device, d_pcm, n_clips, lens, rate, target_lufs, true_peak_dbtp, max_gain_db,
                                 gate_fallback, d_res, d_gained, cv.at<void>(o_lws), nullptr);
    if (rc) { hipDeviceSynchronize(); return rc; }
    launch_flac(d_gained, nullptr, flac_ragged_work(n_clips, lens, rate, seek_interval, cv.at<void>(o_fws), lpc_order), d_bytes, cap, d_offsets,
                nullptr);
    b.he = hipGetLastError();
    if (b.he == hipSuccess) b.he = hipMemcpy(out, d_res, res_bytes, hipMemcpyDeviceToHost);
    if (b.he == hipSuccess) b.he = fetch(d_offsets, d_bytes, n_clips, offsets, out_bytes);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("loudness_flac_ragged_pcm16", b);
    BN_GUARD_END((void)0)
}

}  // extern "C"
