// C ABI of the ultrasonic filter's frame-power coefficient of variation (bnhip_us_frame_cv, bnhip_us_frame_cv_device).
#include <hip/hip_runtime.h>

#include "api_oneshot.h"
#include "kernels.h"

using namespace bnhip;

namespace {

// the twiddle table of the ultrasonic FFT of one (device, fft size); -> NULL on an allocation / copy failure
struct TwiddleTable { int device, fft_size; double* d; };
TableCache<TwiddleTable> g_tw;
const TwiddleTable* us_twiddles(const TableLock& lk, int device, int fft_size) {
    return g_tw.find(lk, [&](const TwiddleTable& e) { return e.device == device && e.fft_size == fft_size; },
                     [&](TwiddleTable& e) { e = {device, fft_size, upload_table(us_twiddle_table(fft_size))}; return e.d != nullptr; });
}

// The geometry of a call, before any device is touched.  -> the frame count (>= 2) with *split_bin set; 0 when the filter's
// guards (internal/audiocore/ultrasonic/filter.go:21-37) reject it, which each entry answers in its own way; < 0: a refusal
int us_frames(int n, int sample_rate, int fft_size, int hop, int split_hz, int* split_bin) {
    bool valid = !(n < fft_size || sample_rate <= 0 || fft_size < 2 || hop <= 0) && (fft_size & (fft_size - 1)) == 0 &&
                 !(split_hz < 0 || split_hz >= sample_rate / 2);
    int frames = valid ? 1 + (n - fft_size) / hop : 0;
    if (frames < 2) return 0;
    if ((size_t)fft_size * 16 > 160 * 1024 - 256) return set_err(BNHIP_E_UNSUPPORTED, "FFT size exceeds the LDS-resident limit (8192)");
    double bin_width = (double)sample_rate / (double)fft_size;
    *split_bin = (int)((double)split_hz / bin_width);
    return frames;
}

}  // namespace

extern "C" {

int bnhip_us_frame_cv(int device, const double* samples, int n_clips, int n, int sample_rate, int fft_size, int hop,
                      int split_hz, double* cv, int32_t* ok) {
    if (!samples || !cv || !ok || n_clips <= 0) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int split_bin = 0;
    const int frames = us_frames(n, sample_rate, fft_size, hop, split_hz, &split_bin);
    if (frames < 0) return frames;
    if (frames == 0) {
        for (int i = 0; i < n_clips; i++) { cv[i] = 0.0; ok[i] = 0; }
        return BNHIP_OK;
    }
    int rc = use_device(device);
    if (rc) return rc;
    TableLock lk(g_tw.mu);
    const TwiddleTable* tw = us_twiddles(lk, device, fft_size);
    if (!tw) return set_err(BNHIP_E_NOMEM, "device allocation failed (FFT twiddle table)");
    DevBlocks b;
    double* d_s = (double*)b.get((size_t)n_clips * n * 8);
    double* d_p = (double*)b.get((size_t)n_clips * frames * 8);
    double* d_cv = (double*)b.get((size_t)n_clips * 8);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_s, samples, (size_t)n_clips * n * 8, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        launch_us_frame_power(d_s, 0, n_clips, n, fft_size, hop, frames, split_bin, tw->d, d_p, nullptr);
        launch_us_cv(d_p, n_clips, frames, d_cv, nullptr);
        b.he = hipGetLastError();
        lk.unlock();
        if (b.he == hipSuccess) b.he = hipMemcpy(cv, d_cv, (size_t)n_clips * 8, hipMemcpyDeviceToHost);
    }
    if (b.he != hipSuccess) return hip_fail("us_frame_cv", b);
    for (int i = 0; i < n_clips; i++) ok[i] = 1;
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

// Device-resident form: samples (float64, or raw int16 PCM) and results stay in HBM, work is enqueued on `hip_stream`
// (NULL = the default stream) and not synchronised.  d_scratch holds n_clips * frames float64 frame powers.
int bnhip_us_frame_cv_device(int device, const void* d_samples, int pcm16, int n_clips, int n, int sample_rate, int fft_size, int hop,
                             int split_hz, double* d_scratch, double* d_cv, void* hip_stream) {
    if (!d_samples || !d_cv || !d_scratch || n_clips <= 0) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int split_bin = 0;
    const int frames = us_frames(n, sample_rate, fft_size, hop, split_hz, &split_bin);
    if (frames < 0) return frames;
    if (frames == 0) return set_err(BNHIP_E_INVALID, "geometry rejected by the filter's guards (filter.go:21-37): use the host entry for the (0, false) answer");
    int rc = use_device(device);
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    TableLock lk(g_tw.mu);
    const TwiddleTable* tw = us_twiddles(lk, device, fft_size);
    if (!tw) return set_err(BNHIP_E_NOMEM, "device allocation failed (FFT twiddle table)");
    launch_us_frame_power(d_samples, pcm16 != 0, n_clips, n, fft_size, hop, frames, split_bin, tw->d, d_scratch, st);
    launch_us_cv(d_scratch, n_clips, frames, d_cv, st);
    rc = launch_status("us_frame_cv_device");
    return rc ? rc : frames;
    BN_GUARD_END((void)0)
}

}  // extern "C"
