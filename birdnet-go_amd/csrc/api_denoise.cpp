// C ABI of the processed-audio entries: the denoiser (bnhip_denoise_workspace_size, bnhip_denoise_device, bnhip_denoise_pcm16) and
// the chain denoise -> normalise -> gain with the clips staying on the device (bnhip_process_pcm16).
//
// Reference paths being replaced: the FFmpeg child process per clip and filter pass of ProcessAudioByID /
// ProcessedSpectrogramByID (internal/api/v2/media/media.go:1200-1447), whose -af chain BuildProcessingFilterChain
// (internal/audiocore/ffmpeg/process.go:212-251) assembles as afftdn, loudnorm, volume in that order from the presets of
// process.go:181-186 and the gain range of process.go:197-203.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "api_oneshot.h"
#include "denoise.h"
#include "loudness.h"

using namespace bnhip;

namespace {

constexpr size_t DN_WORKSPACE = 256;         // the kernel keeps its frames on chip; the device entry's workspace is a token
constexpr double MAX_GAIN_DB = 60.0;         // MaxGainDB (process.go:198)

// the twiddle and window table of one (device, N); -> NULL on an allocation / copy failure
struct DnTable { int device, N; double* d; };
TableCache<DnTable> g_tables;
const DnTable* dn_table(const TableLock& lk, int device, int N) {
    return g_tables.find(lk, [&](const DnTable& e) { return e.device == device && e.N == N; },
                         [&](DnTable& e) { e = {device, N, upload_table(denoise_table(N))}; return e.d != nullptr; });
}

// what every denoise entry checks before any device is touched; -> 0 or a negative BNHIP_E_*
int denoise_check(int n_clips, int n, int frame, double nr_db, double nf_db) {
    if (const int rc = clip_dims_check(n_clips, n)) return rc;
    if (frame < DN_N_MIN || frame > DN_N_MAX || (frame & (frame - 1)) != 0)
        return set_err(BNHIP_E_INVALID, "frame must be a power of two in [64, 4096]");
    if (!std::isfinite(nr_db) || nr_db < DN_NR_MIN || nr_db > DN_NR_MAX) return set_err(BNHIP_E_INVALID, "nr_db must be in [0, 97]");
    if (!std::isfinite(nf_db) || nf_db < DN_NF_MIN || nf_db > DN_NF_MAX) return set_err(BNHIP_E_INVALID, "nf_db must be in [-80, -20]");
    return 0;
}

// the device (already made current) has its table looked up or uploaded, and the kernel is enqueued on s
int denoise_enqueue(const char* what, int device, const int16_t* d_pcm, int n_clips, int n, int frame, double nr_db, double nf_db,
                    int16_t* d_out_pcm, hipStream_t s) {
    TableLock lk(g_tables.mu);
    const DnTable* tab = dn_table(lk, device, frame);
    if (!tab) return set_err(BNHIP_E_NOMEM, "device allocation failed (denoise table)");
    launch_denoise(d_pcm, n_clips, n, frame, nr_db, nf_db, tab->d, d_out_pcm, s);
    return launch_status(what);
}

}  // namespace

extern "C" {

int bnhip_denoise_workspace_size(int n_clips, int n, int frame, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = denoise_check(n_clips, n, frame, DN_NR_MIN, DN_NF_MIN);
    if (rc) return rc;
    *bytes = DN_WORKSPACE;
    return BNHIP_OK;
}

int bnhip_denoise_device(int device, const int16_t* d_pcm, int n_clips, int n, int frame, double nr_db, double nf_db, int16_t* d_out_pcm,
                         void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_pcm || !d_out_pcm || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = denoise_check(n_clips, n, frame, nr_db, nf_db);
    if (!rc) {
        // (a block reads samples that other blocks' outputs would overwrite)
        const uintptr_t a = (uintptr_t)d_pcm, o = (uintptr_t)d_out_pcm, bytes = (uintptr_t)n_clips * (uintptr_t)n * 2;
        if (a < o + bytes && o < a + bytes) rc = set_err(BNHIP_E_INVALID, "d_out_pcm must not overlap d_pcm");
    }
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, DN_WORKSPACE, "bnhip_denoise_workspace_size");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    return denoise_enqueue("denoise_device", device, d_pcm, n_clips, n, frame, nr_db, nf_db, d_out_pcm, reinterpret_cast<hipStream_t>(hip_stream));
    BN_GUARD_END((void)0)
}

int bnhip_denoise_pcm16(int device, const int16_t* pcm, int n_clips, int n, int frame, double nr_db, double nf_db, int16_t* out_pcm) {
    if (!pcm || !out_pcm) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = denoise_check(n_clips, n, frame, nr_db, nf_db);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    const size_t pcm_bytes = (size_t)n_clips * n * 2;
    DevBlocks b;
    int16_t* d_pcm = (int16_t*)b.get(pcm_bytes);
    int16_t* d_out = (int16_t*)b.get(pcm_bytes);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail("denoise_pcm16", b);
    rc = denoise_enqueue("denoise_pcm16", device, d_pcm, n_clips, n, frame, nr_db, nf_db, d_out, nullptr);
    if (rc) { hipDeviceSynchronize(); return rc; }
    // (the null stream orders the copy after the kernel; it is the call's synchronise)
    b.he = hipMemcpy(out_pcm, d_out, pcm_bytes, hipMemcpyDeviceToHost);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("denoise_pcm16", b);
    BN_GUARD_END((void)0)
}

int bnhip_process_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, int frame, double nr_db, double nf_db, int normalize,
                        double target_lufs, double true_peak_dbtp, double gain_db, int16_t* out_pcm, bnhip_loudness* out) {
    if (!pcm || !out_pcm || (normalize && !out)) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const double no_clamp = std::numeric_limits<double>::infinity();
    int rc = clip_dims_check(n_clips, n);
    if (!rc && frame != 0) rc = denoise_check(n_clips, n, frame, nr_db, nf_db);
    if (!rc && normalize) rc = loudness_args_check(n_clips, n, rate, target_lufs, true_peak_dbtp, no_clamp);
    if (!rc && !(std::isfinite(gain_db) && gain_db >= -MAX_GAIN_DB && gain_db <= MAX_GAIN_DB))
        rc = set_err(BNHIP_E_INVALID, "gain_db must be finite and within +-60 dB");
    if (!rc && frame == 0 && !normalize && gain_db == 0.0) rc = set_err(BNHIP_E_INVALID, "no filter active: one of denoise, normalize, gain_db is required");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    // one device block: the clips and two stage outputs (each stage reads one and writes another), the records, the workspace
    const size_t pcm_bytes = (size_t)n_clips * n * 2, res_bytes = (size_t)n_clips * sizeof(bnhip_loudness);
    DevCarve cv;
    const size_t o_in = cv.add(pcm_bytes), o_a = cv.add(pcm_bytes), o_b = normalize ? cv.add(pcm_bytes) : 0;
    const size_t o_res = normalize ? cv.add(res_bytes) : 0;
    const size_t o_ws = normalize ? cv.add(loudness_workspace_bytes(n_clips, n, loudness_sub_block(rate))) : 0;
    DevBlocks b;
    cv.base = (char*)b.get(cv.bytes());
    int16_t* cur = cv.at<int16_t>(o_in);
    if (b.he == hipSuccess) b.he = hipMemcpy(cur, pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail("process_pcm16", b);
    if (frame != 0) {
        int16_t* dst = cv.at<int16_t>(o_a);
        rc = denoise_enqueue("process_pcm16", device, cur, n_clips, n, frame, nr_db, nf_db, dst, nullptr);
        cur = dst;
    }
    if (!rc && normalize) {
        int16_t* dst = cv.at<int16_t>(o_b);
        rc = loudness_enqueue("process_pcm16", device, cur, n_clips, n, rate, target_lufs, true_peak_dbtp, no_clamp, 0,
                              cv.at<bnhip_loudness>(o_res), dst, cv.at<void>(o_ws), nullptr);
        cur = dst;
    }
    if (!rc && gain_db != 0.0) {
        launch_pcm_gain(cur, (size_t)n_clips * n, std::pow(10.0, gain_db / 20.0), cur, nullptr);
        rc = launch_status("process_pcm16");
    }
    if (rc) { hipDeviceSynchronize(); return rc; }
    b.he = hipMemcpy(out_pcm, cur, pcm_bytes, hipMemcpyDeviceToHost);
    if (b.he == hipSuccess && normalize) b.he = hipMemcpy(out, cv.at<bnhip_loudness>(o_res), res_bytes, hipMemcpyDeviceToHost);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("process_pcm16", b);
    BN_GUARD_END((void)0)
}

}  // extern "C"
