// C ABI of the FLAC decode entries (bnhip_flac_stream_info, bnhip_flac_decode_workspace_size, bnhip_flac_decode_device,
// bnhip_flac_decode_pcm16, and for recordings of 1 or 2 channels at 16 or 24 bits bnhip_flac_recording_info and
// bnhip_flac_decode_recordings*).  The entry that decodes, renders and PNG-encodes in one call, bnhip_flac_spectrogram_png, is in
// api_spectrogram.cpp beside the render's tables.
#include <hip/hip_runtime.h>

#include <vector>

#include "api_oneshot.h"
#include "flac_decode.h"
#include "flac_parse.h"

namespace bnhip {

int flacdec_read_infos(const uint8_t* streams, int n_streams, const uint64_t* offsets, std::vector<bnhip_flac_info>* infos, bool recordings) {
    if (n_streams < 1 || n_streams > 65535) return set_err(BNHIP_E_INVALID, "n_streams must be in [1, 65535]");
    infos->resize((size_t)n_streams);
    for (int c = 0; c < n_streams; c++) {
        if (offsets[c + 1] < offsets[c]) return set_err(BNHIP_E_INVALID, "offsets must ascend");
        flac_stream_info(streams + offsets[c], (size_t)(offsets[c + 1] - offsets[c]), &(*infos)[(size_t)c], recordings);
    }
    return 0;
}

int flacdec_burst_check(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* pcm_samples, bool recordings) {
    const char* why = nullptr;
    if (flacdec_check(n_streams, infos, offsets, pcm_samples, &why, recordings)) return set_err(BNHIP_E_INVALID, why);
    return 0;
}

}  // namespace bnhip

using namespace bnhip;

extern "C" {

int bnhip_flac_stream_info(const uint8_t* stream, size_t n_bytes, bnhip_flac_info* out) {
    if (!stream || !out) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    flac_stream_info(stream, n_bytes, out);
    return BNHIP_OK;
}

int bnhip_flac_decode_workspace_size(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* bytes) {
    if (!infos || !offsets || !bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int rc = flacdec_burst_check(n_streams, infos, offsets, nullptr);
    if (rc) return rc;
    *bytes = flacdec_workspace_bytes(n_streams, infos, offsets);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_flac_decode_device(int device, const uint8_t* d_streams, int n_streams, const uint64_t* offsets, const bnhip_flac_info* infos,
                             int16_t* d_pcm, size_t pcm_cap_samples, bnhip_flac_decode_result* d_result, void* d_workspace,
                             size_t workspace_bytes, void* hip_stream) {
    if (!d_streams || !offsets || !infos || !d_pcm || !d_result || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    size_t need = 0;
    int rc = flacdec_burst_check(n_streams, infos, offsets, &need);
    if (!rc && pcm_cap_samples < need) rc = set_err(BNHIP_E_INVALID, "pcm_cap_samples smaller than the streams' total sample count");
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, flacdec_workspace_bytes(n_streams, infos, offsets), "bnhip_flac_decode_workspace_size");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    launch_flacdec(d_streams, flacdec_work(n_streams, infos, offsets, d_workspace), d_pcm, pcm_cap_samples * 2, d_result,
                   reinterpret_cast<hipStream_t>(hip_stream));
    return launch_status("flac_decode_device");
    BN_GUARD_END((void)0)
}

int bnhip_flac_decode_pcm16(int device, const uint8_t* streams, int n_streams, const uint64_t* offsets, int16_t* pcm, size_t pcm_cap_samples,
                            int* lens, bnhip_flac_decode_result* result) {
    if (!streams || !offsets || !pcm || !lens || !result) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    std::vector<bnhip_flac_info> infos;
    size_t need = 0;
    int rc = flacdec_read_infos(streams, n_streams, offsets, &infos);
    if (!rc) rc = flacdec_burst_check(n_streams, infos.data(), offsets, &need);
    if (!rc && pcm_cap_samples < need) rc = set_err(BNHIP_E_INVALID, "pcm_cap_samples smaller than the streams' total sample count");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    for (int c = 0; c < n_streams; c++) lens[c] = infos[(size_t)c].status == BNHIP_FLAC_OK ? (int)infos[(size_t)c].total_samples : 0;
    // one DevCarve: the streams, the clips, the results, the workspace
    const size_t in_bytes = (size_t)(offsets[n_streams] - offsets[0]), res_bytes = (size_t)n_streams * sizeof(bnhip_flac_decode_result);
    DevCarve cv;
    const size_t o_in = cv.add(offsets[n_streams]), o_pcm = cv.add(need * 2), o_res = cv.add(res_bytes);
    const size_t o_ws = cv.add(flacdec_workspace_bytes(n_streams, infos.data(), offsets));
    DevBlocks b;
    cv.alloc(b);
    uint8_t* d_in = cv.at<uint8_t>(o_in);
    if (b.he == hipSuccess && in_bytes) b.he = hipMemcpy(d_in + offsets[0], streams + offsets[0], in_bytes, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        launch_flacdec(d_in, flacdec_work(n_streams, infos.data(), offsets, cv.at<void>(o_ws)), cv.at<int16_t>(o_pcm), need * 2,
                       cv.at<bnhip_flac_decode_result>(o_res), nullptr);
        b.he = hipGetLastError();
    }
    if (b.he == hipSuccess) b.he = hipMemcpy(result, cv.at<void>(o_res), res_bytes, hipMemcpyDeviceToHost);      // (the call's synchronise)
    if (b.he == hipSuccess && need) b.he = hipMemcpy(pcm, cv.at<void>(o_pcm), need * 2, hipMemcpyDeviceToHost);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("flac_decode_pcm16", b);
    BN_GUARD_END((void)0)
}

// ---- recordings: 1 or 2 channels, 16 or 24 bits, to interleaved PCM at each stream's own depth
int bnhip_flac_recording_info(const uint8_t* stream, size_t n_bytes, bnhip_flac_info* out) {
    if (!stream || !out) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    flac_stream_info(stream, n_bytes, out, true);
    return BNHIP_OK;
}

int bnhip_flac_decode_recordings_workspace_size(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* bytes) {
    if (!infos || !offsets || !bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int rc = flacdec_burst_check(n_streams, infos, offsets, nullptr, true);
    if (rc) return rc;
    *bytes = flacdec_workspace_bytes(n_streams, infos, offsets, true);
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_flac_decode_recordings_device(int device, const uint8_t* d_streams, int n_streams, const uint64_t* offsets, const bnhip_flac_info* infos,
                                        void* d_pcm, size_t pcm_cap_bytes, bnhip_flac_decode_result* d_result, void* d_workspace,
                                        size_t workspace_bytes, void* hip_stream) {
    if (!d_streams || !offsets || !infos || !d_pcm || !d_result || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    size_t need = 0;
    int rc = flacdec_burst_check(n_streams, infos, offsets, &need, true);
    if (!rc && pcm_cap_bytes < need) rc = set_err(BNHIP_E_INVALID, "pcm_cap_bytes smaller than the recordings' total PCM bytes");
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, flacdec_workspace_bytes(n_streams, infos, offsets, true),
                                  "bnhip_flac_decode_recordings_workspace_size");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (need && hipMemsetAsync(d_pcm, 0, need, s) != hipSuccess) return launch_status("flac_decode_recordings_device");
    launch_flacdec(d_streams, flacdec_work(n_streams, infos, offsets, d_workspace, true), d_pcm, pcm_cap_bytes, d_result, s);
    return launch_status("flac_decode_recordings_device");
    BN_GUARD_END((void)0)
}

int bnhip_flac_decode_recordings(int device, const uint8_t* streams, int n_streams, const uint64_t* offsets, void* pcm, size_t pcm_cap_bytes,
                                 uint64_t* pcm_offsets, bnhip_flac_decode_result* result) {
    if (!streams || !offsets || !pcm || !pcm_offsets || !result) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    std::vector<bnhip_flac_info> infos;
    size_t need = 0;
    int rc = flacdec_read_infos(streams, n_streams, offsets, &infos, true);
    if (!rc) rc = flacdec_burst_check(n_streams, infos.data(), offsets, &need, true);
    if (!rc && pcm_cap_bytes < need) rc = set_err(BNHIP_E_INVALID, "pcm_cap_bytes smaller than the recordings' total PCM bytes");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    pcm_offsets[0] = 0;
    for (int c = 0; c < n_streams; c++) pcm_offsets[c + 1] = pcm_offsets[c] + flacdec_pcm_bytes(infos[(size_t)c]);
    // one DevCarve: the streams, the PCM (cleared: a frame that is not restored leaves zeros), the results, the workspace
    const size_t in_bytes = (size_t)(offsets[n_streams] - offsets[0]), res_bytes = (size_t)n_streams * sizeof(bnhip_flac_decode_result);
    DevCarve cv;
    const size_t o_in = cv.add(offsets[n_streams]), o_pcm = cv.add(need), o_res = cv.add(res_bytes);
    const size_t o_ws = cv.add(flacdec_workspace_bytes(n_streams, infos.data(), offsets, true));
    DevBlocks b;
    cv.alloc(b);
    uint8_t* d_in = cv.at<uint8_t>(o_in);
    if (b.he == hipSuccess && in_bytes) b.he = hipMemcpy(d_in + offsets[0], streams + offsets[0], in_bytes, hipMemcpyHostToDevice);
    if (b.he == hipSuccess && need) b.he = hipMemsetAsync(cv.at<void>(o_pcm), 0, need, nullptr);
    if (b.he == hipSuccess) {
        launch_flacdec(d_in, flacdec_work(n_streams, infos.data(), offsets, cv.at<void>(o_ws), true), cv.at<void>(o_pcm), need,
                       cv.at<bnhip_flac_decode_result>(o_res), nullptr);
        b.he = hipGetLastError();
    }
    if (b.he == hipSuccess) b.he = hipMemcpy(result, cv.at<void>(o_res), res_bytes, hipMemcpyDeviceToHost);      // (the call's synchronise)
    if (b.he == hipSuccess && need) b.he = hipMemcpy(pcm, cv.at<void>(o_pcm), need, hipMemcpyDeviceToHost);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("flac_decode_recordings", b);
    BN_GUARD_END((void)0)
}

}  // extern "C"
