// C ABI of the processed-audio entries: the denoiser (bnhip_denoise_workspace_size, bnhip_denoise_device, bnhip_denoise_pcm16), the
// chain denoise -> normalise -> gain with the clips staying on the device (bnhip_process_pcm16), and their forms for a ragged burst
// (bnhip_denoise_ragged_workspace_size, bnhip_denoise_ragged_device, bnhip_denoise_ragged_pcm16, bnhip_process_ragged_pcm16).  The
// chain's stage sequence (process_chain.h) is also what bnhip_process_spectrogram_png_ragged_pcm16 (api_spectrogram.cpp) puts in
// front of its render.  Each operation has one body over a Clips (ragged.h), which the entries of both forms call with their own
// names.
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
int denoise_check(const Clips& c, int frame, double nr_db, double nf_db) {
    const int rc = clips_check(c);
    return rc ? rc : denoise_params_check(frame, nr_db, nf_db);
}

// the device (already made current) has its table looked up or uploaded, and the kernel is enqueued on s; d_tables:
// denoise_table_bytes for the launch's tables
int denoise_enqueue(const char* what, int device, const int16_t* d_pcm, const Clips& c, int frame, double nr_db, double nf_db,
                    int16_t* d_out_pcm, void* d_tables, hipStream_t s) {
    TableLock lk(g_tables.mu);
    const DnTable* tab = dn_table(lk, device, frame);
    if (!tab) return set_err(BNHIP_E_NOMEM, "device allocation failed (denoise table)");
    launch_denoise(d_pcm, c, frame, nr_db, nf_db, tab->d, d_out_pcm, d_tables, s);
    return launch_status(what);
}

// The device entry's workspace holds a ragged burst's tables; the kernel keeps its frames on chip, so a uniform batch's is a token.
size_t workspace_bytes_of(const Clips& c) { return std::max(DN_WORKSPACE, denoise_table_bytes(c)); }

// (a block reads samples that other blocks' outputs would overwrite)
int overlap_check(const void* d_pcm, const void* d_out_pcm, size_t samples) {
    const uintptr_t a = (uintptr_t)d_pcm, o = (uintptr_t)d_out_pcm, bytes = (uintptr_t)samples * 2;
    if (a < o + bytes && o < a + bytes) return set_err(BNHIP_E_INVALID, "d_out_pcm must not overlap d_pcm");
    return 0;
}

// the host-pointer denoise of either form: one H2D copy, the kernel, one D2H copy
int denoise_run_pcm16(const char* what, int device, const int16_t* pcm, const Clips& c, int frame, double nr_db, double nf_db,
                      int16_t* out_pcm) {
    int rc = denoise_check(c, frame, nr_db, nf_db);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    const size_t pcm_bytes = c.total() * 2;
    DevCarve cv;
    const size_t o_in = cv.add(pcm_bytes), o_out = cv.add(pcm_bytes), o_tab = cv.add(denoise_table_bytes(c));
    DevBlocks b;
    cv.alloc(b);
    if (b.he == hipSuccess) b.he = hipMemcpy(cv.at<void>(o_in), pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail(what, b);
    rc = denoise_enqueue(what, device, cv.at<int16_t>(o_in), c, frame, nr_db, nf_db, cv.at<int16_t>(o_out), cv.at<void>(o_tab), nullptr);
    if (rc) { hipDeviceSynchronize(); return rc; }
    // (the null stream orders the copy after the kernel; it is the call's synchronise)
    b.he = hipMemcpy(out_pcm, cv.at<void>(o_out), pcm_bytes, hipMemcpyDeviceToHost);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(what, b);
}

// the host-pointer chain of either form: one DevCarve, one H2D copy, the stages, the D2H copies
int process_run_pcm16(const char* what, int device, const int16_t* pcm, const Clips& c, const ChainArgs& a, int16_t* out_pcm,
                      bnhip_loudness* out) {
    int rc = chain_check(c, a);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    DevCarve cv;
    const size_t o_final = cv.add(c.total() * 2);
    const ChainParts p = chain_reserve(cv, c, a);
    DevBlocks b;
    cv.alloc(b);
    int16_t* d_final = cv.at<int16_t>(o_final);
    if (b.he == hipSuccess) b.he = hipMemcpy(chain_input(cv, p, a, d_final), pcm, p.pcm_bytes, hipMemcpyHostToDevice);
    if (b.he != hipSuccess) return hip_fail(what, b);
    rc = chain_enqueue(what, device, cv, p, c, a, d_final);
    if (rc) { hipDeviceSynchronize(); return rc; }
    b.he = hipMemcpy(out_pcm, d_final, p.pcm_bytes, hipMemcpyDeviceToHost);
    if (b.he == hipSuccess && a.normalize) b.he = hipMemcpy(out, cv.at<void>(p.o_res), p.res_bytes, hipMemcpyDeviceToHost);
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(what, b);
}

int workspace_size(const Clips& c, int frame, size_t* bytes) {
    const int rc = denoise_check(c, frame, DN_NR_MIN, DN_NF_MIN);
    if (rc) return rc;
    *bytes = workspace_bytes_of(c);
    return BNHIP_OK;
}

int denoise_device(const char* what, const char* size_entry, int device, const int16_t* d_pcm, const Clips& c, int frame, double nr_db,
                   double nf_db, int16_t* d_out_pcm, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    int rc = denoise_check(c, frame, nr_db, nf_db);
    if (!rc) rc = overlap_check(d_pcm, d_out_pcm, c.total());
    if (!rc) rc = workspace_check(d_workspace, workspace_bytes, workspace_bytes_of(c), size_entry);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    return denoise_enqueue(what, device, d_pcm, c, frame, nr_db, nf_db, d_out_pcm, d_workspace, reinterpret_cast<hipStream_t>(hip_stream));
}

}  // namespace

namespace bnhip {

int chain_check(const Clips& c, const ChainArgs& a) {
    const double no_clamp = std::numeric_limits<double>::infinity();
    int rc = clips_check(c);
    if (!rc && a.frame != 0) rc = denoise_params_check(a.frame, a.nr_db, a.nf_db);
    if (!rc && a.normalize) rc = loudness_args_check(c, a.rate, a.target_lufs, a.true_peak_dbtp, no_clamp);
    if (!rc && !(std::isfinite(a.gain_db) && a.gain_db >= -MAX_GAIN_DB && a.gain_db <= MAX_GAIN_DB))
        rc = set_err(BNHIP_E_INVALID, "gain_db must be finite and within +-60 dB");
    if (!rc && a.frame == 0 && !a.normalize && a.gain_db == 0.0)
        rc = set_err(BNHIP_E_INVALID, "no filter active: one of denoise, normalize, gain_db is required");
    return rc;
}

ChainParts chain_reserve(DevCarve& cv, const Clips& c, const ChainArgs& a) {
    ChainParts p;
    p.pcm_bytes = c.total() * 2;
    p.res_bytes = (size_t)c.n_clips * sizeof(bnhip_loudness);
    if (a.frame != 0 || a.normalize) p.o_other = cv.add(p.pcm_bytes);
    if (a.normalize) {
        p.o_res = cv.add(p.res_bytes);
        p.o_lws = cv.add(loudness_workspace_bytes(c, loudness_sub_block(a.rate)));
    }
    if (a.frame != 0) p.o_dws = cv.add(denoise_table_bytes(c));
    return p;
}

int16_t* chain_input(const DevCarve& cv, const ChainParts& p, const ChainArgs& a, int16_t* d_final) {
    // (one of the two stages: other -> final; both: final -> other -> final; neither: the gain, in place)
    return ((a.frame != 0) != (a.normalize != 0)) ? cv.at<int16_t>(p.o_other) : d_final;
}

int chain_enqueue(const char* what, int device, const DevCarve& cv, const ChainParts& p, const Clips& c, const ChainArgs& a,
                  int16_t* d_final) {
    const double no_clamp = std::numeric_limits<double>::infinity();
    int16_t* const d_other = cv.at<int16_t>(p.o_other);
    int16_t* cur = chain_input(cv, p, a, d_final);
    int rc = 0;
    if (a.frame != 0) {
        int16_t* dst = cur == d_final ? d_other : d_final;
        rc = denoise_enqueue(what, device, cur, c, a.frame, a.nr_db, a.nf_db, dst, cv.at<void>(p.o_dws), nullptr);
        cur = dst;
    }
    if (!rc && a.normalize) {
        int16_t* dst = cur == d_final ? d_other : d_final;
        bnhip_loudness* d_res = cv.at<bnhip_loudness>(p.o_res);
        rc = loudness_enqueue(what, device, cur, c, a.rate, a.target_lufs, a.true_peak_dbtp, no_clamp, 0, d_res, dst, cv.at<void>(p.o_lws), nullptr);
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
    return workspace_size(Clips::uniform(n_clips, n), frame, bytes);
}

int bnhip_denoise_device(int device, const int16_t* d_pcm, int n_clips, int n, int frame, double nr_db, double nf_db, int16_t* d_out_pcm,
                         void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_pcm || !d_out_pcm || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    return denoise_device("denoise_device", "bnhip_denoise_workspace_size", device, d_pcm, Clips::uniform(n_clips, n), frame, nr_db, nf_db,
                          d_out_pcm, d_workspace, workspace_bytes, hip_stream);
    BN_GUARD_END((void)0)
}

int bnhip_denoise_pcm16(int device, const int16_t* pcm, int n_clips, int n, int frame, double nr_db, double nf_db, int16_t* out_pcm) {
    if (!pcm || !out_pcm) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    return denoise_run_pcm16("denoise_pcm16", device, pcm, Clips::uniform(n_clips, n), frame, nr_db, nf_db, out_pcm);
    BN_GUARD_END((void)0)
}

int bnhip_process_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate, int frame, double nr_db, double nf_db, int normalize,
                        double target_lufs, double true_peak_dbtp, double gain_db, int16_t* out_pcm, bnhip_loudness* out) {
    if (!pcm || !out_pcm || (normalize && !out)) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const ChainArgs a{rate, frame, nr_db, nf_db, normalize, target_lufs, true_peak_dbtp, gain_db};
    return process_run_pcm16("process_pcm16", device, pcm, Clips::uniform(n_clips, n), a, out_pcm, out);
    BN_GUARD_END((void)0)
}

// ---- ragged bursts: n_clips clips of lens[c] samples packed back to back (bnhip.h "Ragged bursts")

int bnhip_denoise_ragged_workspace_size(int n_clips, const int* lens, int frame, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int rc = lens_check(n_clips, lens);
    return rc ? rc : workspace_size(Clips::ragged(n_clips, lens), frame, bytes);
}

int bnhip_denoise_ragged_device(int device, const int16_t* d_pcm, int n_clips, const int* lens, int frame, double nr_db, double nf_db,
                                int16_t* d_out_pcm, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_pcm || !d_out_pcm || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int rc = lens_check(n_clips, lens);
    if (rc) return rc;
    return denoise_device("denoise_ragged_device", "bnhip_denoise_ragged_workspace_size", device, d_pcm, Clips::ragged(n_clips, lens), frame,
                          nr_db, nf_db, d_out_pcm, d_workspace, workspace_bytes, hip_stream);
    BN_GUARD_END((void)0)
}

int bnhip_denoise_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int frame, double nr_db, double nf_db,
                               int16_t* out_pcm) {
    if (!pcm || !out_pcm) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int rc = lens_check(n_clips, lens);
    if (rc) return rc;
    return denoise_run_pcm16("denoise_ragged_pcm16", device, pcm, Clips::ragged(n_clips, lens), frame, nr_db, nf_db, out_pcm);
    BN_GUARD_END((void)0)
}

int bnhip_process_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, int frame, double nr_db, double nf_db,
                               int normalize, double target_lufs, double true_peak_dbtp, double gain_db, int16_t* out_pcm,
                               bnhip_loudness* out) {
    if (!pcm || !out_pcm || (normalize && !out)) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    if (!lens) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const ChainArgs a{rate, frame, nr_db, nf_db, normalize, target_lufs, true_peak_dbtp, gain_db};
    return process_run_pcm16("process_ragged_pcm16", device, pcm, Clips::ragged(n_clips, lens), a, out_pcm, out);
    BN_GUARD_END((void)0)
}

}  // extern "C"
