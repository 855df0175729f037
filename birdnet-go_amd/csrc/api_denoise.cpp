// C ABI of the processed-audio entries: the denoiser (bnhip_denoise_workspace_size, bnhip_denoise_device, bnhip_denoise_pcm16), the
// chain denoise -> normalise -> gain with the clips staying on the device (bnhip_process_pcm16), and their forms for a ragged burst
// (bnhip_denoise_ragged_workspace_size, bnhip_denoise_ragged_device, bnhip_denoise_ragged_pcm16, bnhip_process_ragged_pcm16).  The
// chain's stage sequence (process_chain.h) is also what bnhip_process_spectrogram_png_ragged_pcm16 (api_spectrogram.cpp) puts in
// front of its render.
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
#include "process_chain.h"

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
int denoise_params_check(int frame, double nr_db, double nf_db) {
    if (frame < DN_N_MIN || frame > DN_N_MAX || (frame & (frame - 1)) != 0)
        return set_err(BNHIP_E_INVALID, "frame must be a power of two in [64, 4096]");
    if (!std::isfinite(nr_db) || nr_db < DN_NR_MIN || nr_db > DN_NR_MAX) return set_err(BNHIP_E_INVALID, "nr_db must be in [0, 97]");
    if (!std::isfinite(nf_db) || nf_db < DN_NF_MIN || nf_db > DN_NF_MAX) return set_err(BNHIP_E_INVALID, "nf_db must be in [-80, -20]");
    return 0;
}
int denoise_check(int n_clips, int n, int frame, double nr_db, double nf_db) {
    if (const int rc = clip_dims_check(n_clips, n)) return rc;
    return denoise_params_check(frame, nr_db, nf_db);
}
int denoise_ragged_check(int n_clips, const int* lens, int frame, double nr_db, double nf_db) {
    if (const int rc = ragged_lens_check(n_clips, lens)) return rc;
    return denoise_params_check(frame, nr_db, nf_db);
}

// the device (already made current) has its table looked up or uploaded, and the kernel is enqueued on s; lens NULL: a uniform
// batch of n-sample clips, else a ragged burst with d_tables (denoise_ragged_table_bytes) for the launch's tables
int denoise_enqueue(const char* what, int device, const int16_t* d_pcm, int n_clips, int n, const int* lens, int frame, double nr_db,
                    double nf_db, int16_t* d_out_pcm, void* d_tables, hipStream_t s) {
    TableLock lk(g_tables.mu);
    const DnTable* tab = dn_table(lk, device, frame);
    if (!tab) return set_err(BNHIP_E_NOMEM, "device allocation failed (denoise table)");
    if (lens) launch_denoise_ragged(d_pcm, n_clips, lens, frame, nr_db, nf_db, tab->d, d_out_pcm, d_tables, s);
    else launch_denoise(d_pcm, n_clips, n, frame, nr_db, nf_db, tab->d, d_out_pcm, s);
    return launch_status(what);
}

// (a block reads samples that other blocks' outputs would overwrite)
int overlap_check(const void* d_pcm, const void* d_out_pcm, size_t samples) {
    const uintptr_t a = (uintptr_t)d_pcm, o = (uintptr_t)d_out_pcm, bytes = (uintptr_t)samples * 2;
    if (a < o + bytes && o < a + bytes) return set_err(BNHIP_E_INVALID, "d_out_pcm must not overlap d_pcm");
    return 0;
}

// the host-pointer denoise of either form: one H2D copy, the kernel, one D2H copy
int denoise_run_pcm16(const char* what, int device, const int16_t* pcm, const ChainClips& c, int frame, double nr_db, double nf_db,
                      int16_t* out_pcm) {
    const size_t pcm_bytes = c.total() * 2;
    DevCarve cv;
    const size_t o_in = cv.add(pcm_bytes), o_out = cv.add(pcm_bytes), o_tab = cv.add(c.lens ? denoise_ragged_table_bytes(c.n_clips) : 0);
    DevBlocks b;
    cv.base = (char*)b.get(cv.bytes());
    if (b.he == hipSuccess) b.he = hipMemcpy(cv.at<void>(o_in), pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail(what, b);
    const int rc = denoise_enqueue(what, device, cv.at<int16_t>(o_in), c.n_clips, c.n, c.lens, frame, nr_db, nf_db, cv.at<int16_t>(o_out),
                                   cv.at<void>(o_tab), nullptr);
    if (rc) { hipDeviceSynchronize(); return rc; }
    // (the null stream orders the copy after the kernel; it is the call's synchronise)
    b.he = hipMemcpy(out_pcm, cv.at<void>(o_out), pcm_bytes, hipMemcpyDeviceToHost);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(what, b);
}

// the host-pointer chain of either form, after chain_check: one device block, one H2D copy, the stages, the D2H copies
int process_run_pcm16(const char* what, int device, const int16_t* pcm, const ChainClips& c, const ChainArgs& a, int16_t* out_pcm,
                      bnhip_loudness* out) {
    DevCarve cv;
    const size_t o_final = cv.add(c.total() * 2);
    const ChainParts p = chain_reserve(cv, c, a);
    DevBlocks b;
    cv.base = (char*)b.get(cv.bytes());
    int16_t* d_final = cv.at<int16_t>(o_final);
    if (b.he == hipSuccess) b.he = hipMemcpy(chain_input(cv, p, a, d_final), pcm, p.pcm_bytes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail(what, b);
    const int rc = chain_enqueue(what, device, cv, p, c, a, d_final);
    if (rc) { hipDeviceSynchronize(); return rc; }
    b.he = hipMemcpy(out_pcm, d_final, p.pcm_bytes, hipMemcpyDeviceToHost);
    if (b.he == hipSuccess && a.normalize) b.he = hipMemcpy(out, cv.at<void>(p.o_res), p.res_bytes, hipMemcpyDeviceToHost);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(what, b);
}

}  // namespace

namespace bnhip {

int chain_check(const ChainClips& c, const ChainArgs& a) {
    const double no_clamp = std::numeric_limits<double>::infinity();
    int rc = c.lens ? ragged_lens_check(c.n_clips, c.lens) : clip_dims_check(c.n_clips, c.n);
    if (!rc && a.frame != 0) rc = denoise_params_check(a.frame, a.nr_db, a.nf_db);
    if (!rc && a.normalize)
        rc = c.lens ? loudness_ragged_args_check(c.n_clips, c.lens, a.rate, a.target_lufs, a.true_peak_dbtp, no_clamp)
                    : loudness_args_check(c.n_clips, c.n, a.rate, a.target_lufs, a.true_peak_dbtp, no_clamp);
    if (!rc && !(std::isfinite(a.gain_db) && a.gain_db >= -MAX_GAIN_DB && a.gain_db <= MAX_GAIN_DB))
        rc = set_err(BNHIP_E_INVALID, "gain_db must be finite and within +-60 dB");
    if (!rc && a.frame == 0 && !a.normalize && a.gain_db == 0.0)
        rc = set_err(BNHIP_E_INVALID, "no filter active: one of denoise, normalize, gain_db is required");
    return rc;
}

ChainParts chain_reserve(DevCarve& cv, const ChainClips& c, const ChainArgs& a) {
    ChainParts p;
    p.pcm_bytes = c.total() * 2;
    p.res_bytes = (size_t)c.n_clips * sizeof(bnhip_loudness);
    if (a.frame != 0 || a.normalize) p.o_other = cv.add(p.pcm_bytes);
    if (a.normalize) {
        const int S = loudness_sub_block(a.rate);
        p.o_res = cv.add(p.res_bytes);
        p.o_lws = cv.add(c.lens ? loudness_ragged_workspace_bytes(c.n_clips, c.lens, S) : loudness_workspace_bytes(c.n_clips, c.n, S));
    }
    if (a.frame != 0 && c.lens) p.o_dws = cv.add(denoise_ragged_table_bytes(c.n_clips));
    return p;
}

int16_t* chain_input(const DevCarve& cv, const ChainParts& p, const ChainArgs& a, int16_t* d_final) {
    // (one of the two stages: other -> final; both: final -> other -> final; neither: the gain, in place)
    return ((a.frame != 0) != (a.normalize != 0)) ? cv.at<int16_t>(p.o_other) : d_final;
}

int chain_enqueue(const char* what, int device, const DevCarve& cv, const ChainParts& p, const ChainClips& c, const ChainArgs& a,
                  int16_t* d_final) {
    const double no_clamp = std::numeric_limits<double>::infinity();
    int16_t* const d_other = cv.at<int16_t>(p.o_other);
    int16_t* cur = chain_input(cv, p, a, d_final);
    int rc = 0;
    if (a.frame != 0) {
        int16_t* dst = cur == d_final ? d_other : d_final;
        rc = denoise_enqueue(what, device, cur, c.n_clips, c.n, c.lens, a.frame, a.nr_db, a.nf_db, dst, cv.at<void>(p.o_dws), nullptr);
        cur = dst;
    }
    if (!rc && a.normalize) {
        int16_t* dst = cur == d_final ? d_other : d_final;
        bnhip_loudness* d_res = cv.at<bnhip_loudness>(p.o_res);
        rc = c.lens ? loudness_ragged_enqueue(what, device, cur, c.n_clips, c.lens, a.rate, a.target_lufs, a.true_peak_dbtp, no_clamp, 0, d_res,
                                              dst, cv.at<void>(p.o_lws), nullptr)
                    : loudness_enqueue(what, device, cur, c.n_clips, c.n, a.rate, a.target_lufs, a.true_peak_dbtp, no_clamp, 0, d_res, dst,
                                       cv.at<void>(p.o_lws), nullptr);
        cur = dst;
    }
    if (!rc && a.gain_db != 0.0) {
        launch_pcm_gain(cur, c.total(), std::pow(10.0, a.gain_db / 20.0), cur, nullptr);
        rc = launch_status(what);
    }
    return rc;
}

}  // namespace bnhip

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
    if (!rc) rc = overlap_check(d_pcm, d_out_pcm, (size_t)n_clips * (size_t)n);
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, DN_WORKSPACE, "bnhip_denoise_workspace_size");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    return denoise_enqueue("denoise_device", device, d_pcm, n_clips, n, nullptr, frame, nr_db, nf_db, d_out_pcm, nullptr,
                           reinterpret_cast<hipStream_t>(hip_stream));
    BN_GUARD_END((void)0)
}

int bnhip_denoise_pcm16(int device, const int16_t* pcm, int n_clips, int n, int frame, double nr_db, double nf_db, int16_t* out_pcm) {
    if (!pcm || !out_pcm) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = denoise_check(n_clips, n, frame, nr_db, nf_db);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    ChainClips c;
    c.n_clips = n_clips; c.n = n;
    return denoise_run_pcm16("denoise_pcm16", device, pcm, c, frame, nr_db, nf_db, out_pcm);
    BN_GUARD_END((void)0)
}

int bnhip_process_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, int frame, double nr_db, double nf_db, int normalize,
                        double target_lufs, double true_peak_dbtp, double gain_db, int16_t* out_pcm, bnhip_loudness* out) {
    if (!pcm || !out_pcm || (normalize && !out)) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    ChainClips c;
    c.n_clips = n_clips; c.n = n;
    const ChainArgs a{rate, frame, nr_db, nf_db, normalize, target_lufs, true_peak_dbtp, gain_db};
    int rc = chain_check(c, a);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    return process_run_pcm16("process_pcm16", device, pcm, c, a, out_pcm, out);
    BN_GUARD_END((void)0)
}

// ---- ragged bursts: n_clips clips of lens[c] samples packed back to back (bnhip.h "Ragged bursts")

int bnhip_denoise_ragged_workspace_size(int n_clips, const int* lens, int frame, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = denoise_ragged_check(n_clips, lens, frame, DN_NR_MIN, DN_NF_MIN);
    if (rc) return rc;
    *bytes = denoise_ragged_table_bytes(n_clips);
    return BNHIP_OK;
}

int bnhip_denoise_ragged_device(int device, const int16_t* d_pcm, int n_clips, const int* lens, int frame, double nr_db, double nf_db,
                                int16_t* d_out_pcm, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_pcm || !d_out_pcm || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = denoise_ragged_check(n_clips, lens, frame, nr_db, nf_db);
    if (!rc) rc = overlap_check(d_pcm, d_out_pcm, ragged_total(n_clips, lens));
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, denoise_ragged_table_bytes(n_clips), "bnhip_denoise_ragged_workspace_size");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    return denoise_enqueue("denoise_ragged_device", device, d_pcm, n_clips, 0, lens, frame, nr_db, nf_db, d_out_pcm, d_workspace,
                           reinterpret_cast<hipStream_t>(hip_stream));
    BN_GUARD_END((void)0)
}

int bnhip_denoise_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int frame, double nr_db, double nf_db,
                               int16_t* out_pcm) {
    if (!pcm || !out_pcm) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = denoise_ragged_check(n_clips, lens, frame, nr_db, nf_db);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    ChainClips c;
    c.n_clips = n_clips; c.lens = lens;
    return denoise_run_pcm16("denoise_ragged_pcm16", device, pcm, c, frame, nr_db, nf_db, out_pcm);
    BN_GUARD_END((void)0)
}

int bnhip_process_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, int frame, double nr_db, double nf_db,
                               int normalize, double target_lufs, double true_peak_dbtp, double gain_db, int16_t* out_pcm,
                               bnhip_loudness* out) {
    if (!pcm || !out_pcm || (normalize && !out)) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    if (!lens) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    ChainClips c;
    c.n_clips = n_clips; c.lens = lens;
    const ChainArgs a{rate, frame, nr_db, nf_db, normalize, target_lufs, true_peak_dbtp, gain_db};
    int rc = chain_check(c, a);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    return process_run_pcm16("process_ragged_pcm16", device, pcm, c, a, out_pcm, out);
    BN_GUARD_END((void)0)
}

}  // extern "C"
