// C ABI of the ultrasonic filter's frame-power coefficient of variation (bnhip_us_frame_cv, bnhip_us_frame_cv_device).
#include <hip/hip_runtime.h>

#include <mutex>
#include <utility>
#include <vector>

#include "api_common.h"
#include "kernels.h"

using namespace bnhip;

namespace {

// twiddle tables of the ultrasonic FFT, one per (device, fft size), uploaded on first use and kept for the process
std::mutex g_tw_mu;
std::vector<std::pair<std::pair<int, int>, double*>> g_tw;
const double* us_twiddles(int device, int fft_size) {
    std::lock_guard<std::mutex> lk(g_tw_mu);
    for (auto& e : g_tw) if (e.first.first == device && e.first.second == fft_size) return e.second;
    std::vector<double> t = us_twiddle_table(fft_size);
    double* d = nullptr;
    if (hipMalloc((void**)&d, t.size() * 8) != hipSuccess) return nullptr;
    if (hipMemcpy(d, t.data(), t.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { hipFree(d); return nullptr; }
    g_tw.push_back({{device, fft_size}, d});
    return d;
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
    double *d_s = nullptr, *d_p = nullptr, *d_cv = nullptr;
    hipError_t he = hipMalloc((void**)&d_s, (size_t)n_clips * n * 8);
    if (he == hipSuccess) he = hipMalloc((void**)&d_p, (size_t)n_clips * frames * 8);
    if (he == hipSuccess) he = hipMalloc((void**)&d_cv, (size_t)n_clips * 8);
    if (he == hipSuccess) he = hipMemcpy(d_s, samples, (size_t)n_clips * n * 8, hipMemcpyHostToDevice);
    if (he == hipSuccess) {
        const double* d_tw = us_twiddles(device, fft_size);
        if (!d_tw) he = hipErrorOutOfMemory;
        else {
            launch_us_frame_power(d_s, 0, n_clips, n, fft_size, hop, frames, split_bin, d_tw, d_p, nullptr);
            launch_us_cv(d_p, n_clips, frames, d_cv, nullptr);
            he = hipGetLastError();
            if (he == hipSuccess) he = hipMemcpy(cv, d_cv, (size_t)n_clips * 8, hipMemcpyDeviceToHost);
        }
    }
    if (d_s) hipFree(d_s);
    if (d_p) hipFree(d_p);
    if (d_cv) hipFree(d_cv);
    if (he != hipSuccess) return set_err(BNHIP_E_RUNTIME, std::string("us_frame_cv: ") + hipGetErrorString(he));
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
    const double* d_tw = us_twiddles(device, fft_size);
    if (!d_tw) return set_err(BNHIP_E_NOMEM, "device allocation failed (FFT twiddle table)");
    launch_us_frame_power(d_samples, pcm16 != 0, n_clips, n, fft_size, hop, frames, split_bin, d_tw, d_scratch, st);
    launch_us_cv(d_scratch, n_clips, frames, d_cv, st);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) return set_err(BNHIP_E_RUNTIME, std::string("us_frame_cv_device: ") + hipGetErrorString(he));
    return frames;
    BN_GUARD_END((void)0)
}

}  // extern "C"
