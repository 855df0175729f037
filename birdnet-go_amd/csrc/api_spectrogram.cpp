// C ABI of the detection-clip spectrogram images (bnhip_spectrogram_size, bnhip_spectrogram_pcm16, bnhip_spectrogram_device), of
// the render fused with the PNG encoder of api_png.cpp (bnhip_spectrogram_png_pcm16), which needs this file's window and rate tables,
// and of their forms for a ragged burst (bnhip_spectrogram_ragged_workspace_size, bnhip_spectrogram_ragged_pcm16,
// bnhip_spectrogram_png_ragged_pcm16, bnhip_spectrogram_ragged_device), the last also fed by the device FLAC decoder of flac_decode.h
// in place of the host's PCM (bnhip_flac_spectrogram_png), or by the processed-audio chain of process_chain.h behind it
// (bnhip_process_spectrogram_png_ragged_pcm16).  Three bodies over a Clips (ragged.h) serve both forms: image_run (the images come
// back), png_run (the PNG streams come back, from any ClipSource) and device_run; every host-pointer entry takes its device memory as one
// DevCarve (api_oneshot.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <numeric>

#include "api_oneshot.h"
#include "clip_source.h"
#include "flac_decode.h"
#include "kernels.h"
#include "png.h"
#include "process_chain.h"
#include "resample.h"
#include "spectrogram.h"

using namespace bnhip;

namespace {

// fftFriendlyHeight (internal/spectrogram/generator.go:115-123): the smallest 2^k + 1 that is >= width / 2
int fft_friendly_height(int width) {
    const int target = width / 2;
    int n = 1;
    while (n + 1 < target) n *= 2;
    return n + 1;
}

// twiddles + window of one (device, N, window contents); window == NULL: periodic Hann, 0.5 - 0.5 cos(2 pi i / N).
// -> NULL on an allocation / copy failure
struct SpecTable { int device, N; std::vector<double> window; double wsum; double* d; };
TableCache<SpecTable> g_tables;
const SpecTable* spec_table(const TableLock& lk, int device, int N, const double* window) {
    std::vector<double> w((size_t)N);
    for (int i = 0; i < N; i++)
        w[i] = window ? window[i] : 0.5 - 0.5 * std::cos(6.283185307179586476925286766559 * (double)i / (double)N);
    return g_tables.find(lk, [&](const SpecTable& e) { return e.device == device && e.N == N && e.window == w; }, [&](SpecTable& e) {
        double wsum = 0.0;
        for (int i = 0; i < N; i++) wsum += w[i];
        double* d = upload_table(spectrogram_table(N, w.data()));
        e = {device, N, std::move(w), wsum, d};
        return d != nullptr;
    });
}

// the one-shot resampler's phase table of one (device, rate pair), under g_tables.mu like the window tables
struct RateTable { int device, rate_in, rate_out, L, M, T, half; float* d; };
TableCache<RateTable> g_rates;
const RateTable* rate_table(const TableLock& lk, int device, int rate_in, int rate_out) {
    return g_rates.find(lk, [&](const RateTable& e) { return e.device == device && e.rate_in == rate_in && e.rate_out == rate_out; },
                        [&](RateTable& r) {
        const int g = std::gcd(rate_in, rate_out);
        r = {device, rate_in, rate_out, rate_out / g, rate_in / g, 0, 0, nullptr};
        std::vector<float> table;
        resample_design(r.L, r.M, RESAMPLE_BETA, RESAMPLE_HALF_FACTOR, &table, &r.T, &r.half);
        if (resample_lds(r.L, r.M, r.T) > RESAMPLE_LDS_MAX) return true;          // (d stays NULL for a geometry that cannot run)
        return (r.d = upload_table(table)) != nullptr;
    });
}

// what every render entry checks of the image and the level rule before any device is touched; -> the transform length, or a
// negative BNHIP_E_*
int spec_image_check(int width, int height, const double* window, double top_db, double range_db) {
    if (width < 1 || width > 4096) return set_err(BNHIP_E_INVALID, "width must be in [1, 4096]");
    if (height < 2 || ((height - 1) & (height - 2)) != 0) return set_err(BNHIP_E_INVALID, "height must be 2^k + 1");
    if (!std::isfinite(range_db) || range_db <= 0.0) return set_err(BNHIP_E_INVALID, "range_db must be finite and positive");
    if (!std::isfinite(top_db)) return set_err(BNHIP_E_INVALID, "top_db must be finite");
    const long long N = 2LL * (height - 1);
    if (N < SPEC_N_MIN || N > SPEC_N_MAX) return set_err(BNHIP_E_UNSUPPORTED, "FFT size 2 * (height - 1) must be in [64, 4096]");
    if (window) {
        double s = 0.0;
        for (int i = 0; i < (int)N; i++) {
            if (!std::isfinite(window[i])) return set_err(BNHIP_E_INVALID, "window coefficients must be finite");
            s += window[i];
        }
        if (!(s != 0.0)) return set_err(BNHIP_E_INVALID, "window coefficients sum to zero");
    }
    return (int)N;
}
int spec_check(const Clips& c, int width, int height, const double* window, double top_db, double range_db) {
    if (const int rc = clips_check(c)) return rc;
    return spec_image_check(width, height, window, top_db, range_db);
}

// The clips as a call renders them: themselves, or with a rate change every clip at its bnhip_resample_length (lens_out holds a
// ragged burst's), held to what clips_check asks of the input, so that the floats and their tiles stay inside the same limits.
// -> 0 or a BNHIP_E_*
int render_clips(const Clips& c, bool resample, int rate_in, int rate_out, std::vector<int>* lens_out, Clips* r) {
    *r = c;
    if (!resample) return 0;
    if (rate_in <= 0 || rate_out < 0) return set_err(BNHIP_E_INVALID, "sample rates must be positive");
    if (!c.lens) {
        r->n = bnhip_resample_length(c.n, rate_in, rate_out);
    } else {
        lens_out->resize((size_t)c.n_clips);
        for (int i = 0; i < c.n_clips; i++) (*lens_out)[i] = bnhip_resample_length(c.lens[i], rate_in, rate_out);
        r->lens = lens_out->data();
    }
    return clips_check(*r);
}

// What a host-pointer render holds under the table lock: the window table and, with a rate change, the phase table.
struct RenderTables { const SpecTable* tab = nullptr; const RateTable* rt = nullptr; };
int render_tables(const TableLock& lk, int device, int N, const double* window, bool resample, int rate_in, int rate_out, RenderTables* t) {
    if (resample) {
        t->rt = rate_table(lk, device, rate_in, rate_out);
        if (!t->rt) return set_err(BNHIP_E_NOMEM, "device allocation failed (resampler phase table)");
        if (!t->rt->d) return set_err(BNHIP_E_UNSUPPORTED, "resample ratio needs a phase table larger than LDS");
    }
    t->tab = spec_table(lk, device, N, window);
    if (!t->tab) return set_err(BNHIP_E_NOMEM, "device allocation failed (spectrogram table)");
    return 0;
}

// the device parts of a host-pointer render, parts of the call's DevCarve: the clips `c`, the images, with a rate change the
// resampler's floats (the clips `r`), and the tables the two launches take for a ragged burst
struct RenderParts { size_t pcm_bytes, img_bytes, o_pcm, o_img, o_f32, o_rows, o_rtab; };
RenderParts render_parts(DevCarve& cv, const Clips& c, const Clips& r, bool resample, int width, int height) {
    RenderParts p;
    p.pcm_bytes = c.total() * 2;
    p.img_bytes = (size_t)c.n_clips * height * width;
    p.o_pcm = cv.add(p.pcm_bytes); p.o_img = cv.add(p.img_bytes);
    p.o_f32 = cv.add(resample ? r.total() * 4 : 0);
    p.o_rows = cv.add(spectrogram_table_bytes(r));
    p.o_rtab = cv.add(resample ? resample_ragged_table_bytes(c.n_clips) : 0);
    return p;
}
// d_pcm -> d_img on the null stream, through the one-shot resampler where there is a rate change: the general one for a uniform
// batch, the ragged one for a burst.  (The one place that chooses between the two.)
void render_enqueue(const RenderTables& t, const DevCarve& cv, const RenderParts& p, const Clips& c, const Clips& r, int width, int height,
                    double top_db, double range_db) {
    const RateTable* rt = t.rt;
    const int16_t* d_pcm = cv.at<int16_t>(p.o_pcm);
    float* d_f32 = cv.at<float>(p.o_f32);
    if (rt && c.lens) launch_resample_ragged(d_pcm, d_f32, rt->d, c.n_clips, c.lens, r.lens, rt->L, rt->M, rt->T, rt->half, cv.at<void>(p.o_rtab), nullptr);
    else if (rt) launch_resample(d_pcm, d_f32, rt->d, 1, 0, c.n_clips, c.n, r.n, rt->L, rt->M, rt->T, rt->half, 0, 0, nullptr);
    launch_spectrogram(rt ? (const void*)d_f32 : (const void*)d_pcm, rt ? 1 : 0, r, width, height, t.tab->d, t.tab->wsum, top_db, range_db,
                       cv.at<uint8_t>(p.o_img), cv.at<void>(p.o_rows), nullptr);
}

// The sources of this file's entries (ClipSource, clip_source.h): the host's PCM, a decode on the device, the processed-audio chain.
struct PcmSource : ClipSource {
    const int16_t* pcm;
    explicit PcmSource(const int16_t* p) : pcm(p) {}
    hipError_t fill(const DevCarve&, int16_t* d_pcm, size_t pcm_bytes) override { return hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice); }
};
// FLAC streams in host memory: the compressed bytes are what crosses to the device, the clips are decoded where the render reads them
struct FlacSource : ClipSource {
    const uint8_t* streams;
    int n_streams;
    const uint64_t* offsets;
    bnhip_flac_decode_result* result;
    std::vector<bnhip_flac_info> infos;
    size_t o_in = 0, o_res = 0, o_ws = 0;
    FlacSource(const uint8_t* s, int n, const uint64_t* o, bnhip_flac_decode_result* r) : streams(s), n_streams(n), offsets(o), result(r) {}
    void reserve(DevCarve& cv) override {
        o_in = cv.add(offsets[n_streams]);
        o_res = cv.add((size_t)n_streams * sizeof(bnhip_flac_decode_result));
        o_ws = cv.add(flacdec_workspace_bytes(n_streams, infos.data(), offsets));
    }
    hipError_t fill(const DevCarve& cv, int16_t* d_pcm, size_t pcm_bytes) override {
        uint8_t* d_in = cv.at<uint8_t>(o_in);
        const size_t in_bytes = (size_t)(offsets[n_streams] - offsets[0]);
        if (in_bytes) {
            const hipError_t he = hipMemcpy(d_in + offsets[0], streams + offsets[0], in_bytes, hipMemcpyHostToDevice);
            if (he != hipSuccess) return he;
        }
        launch_flacdec(d_in, flacdec_work(n_streams, infos.data(), offsets, cv.at<void>(o_ws)), d_pcm, pcm_bytes,
                       cv.at<bnhip_flac_decode_result>(o_res), nullptr);
        return hipGetLastError();
    }
    hipError_t finish(const DevCarve& cv) override {
        return hipMemcpy(result, cv.at<void>(o_res), (size_t)n_streams * sizeof(bnhip_flac_decode_result), hipMemcpyDeviceToHost);
    }
};

// The host's PCM through the chain denoise -> normalise -> gain: the unprocessed clips are what crosses to the device, the
// processed ones are written where the render reads them and reach the host only if the caller asks for them
struct ProcessSource : ClipSource {
    const int16_t* pcm;
    int device;
    Clips clips;
    ChainArgs args;
    bnhip_loudness* loud;
    int16_t* out_pcm;
    ChainParts parts;
    const int16_t* d_final = nullptr;
    int rc = 0;                              // the chain's own refusal, with its text: what the entry answers instead of a HIP error
    std::string err;
    ProcessSource(const int16_t* p, int dev, const Clips& c, const ChainArgs& a, bnhip_loudness* l, int16_t* o)
        : pcm(p), device(dev), clips(c), args(a), loud(l), out_pcm(o) {}
    void reserve(DevCarve& cv) override { parts = chain_reserve(cv, clips, args); }
    hipError_t fill(const DevCarve& cv, int16_t* d_pcm, size_t pcm_bytes) override {
        const hipError_t he = hipMemcpy(chain_input(cv, parts, args, d_pcm), pcm, pcm_bytes, hipMemcpyHostToDevice);
        if (he != hipSuccess) return he;
        d_final = d_pcm;
        rc = chain_enqueue("process_spectrogram_png_ragged_pcm16", device, cv, parts, clips, args, d_pcm);
        if (rc) { err = bnhip_last_error(); hipDeviceSynchronize(); return hipErrorUnknown; }
        return hipSuccess;
    }
    hipError_t finish(const DevCarve& cv) override {
        hipError_t he = hipSuccess;
        if (args.normalize) he = hipMemcpy(loud, cv.at<void>(parts.o_res), parts.res_bytes, hipMemcpyDeviceToHost);
        if (he == hipSuccess && out_pcm) he = hipMemcpy(out_pcm, d_final, parts.pcm_bytes, hipMemcpyDeviceToHost);
        return he;
    }
};

// The render of either form with the images as its result: one H2D copy, the kernels, one D2H copy.
int image_run(const char* what, int device, const int16_t* pcm, const Clips& c, int rate_in, int rate_out, int width, int height,
              const double* window, double top_db, double range_db, uint8_t* image) {
    const int N = spec_check(c, width, height, window, top_db, range_db);
    if (N < 0) return N;
    const bool resample = rate_out != 0 && rate_out != rate_in;
    std::vector<int> lens_out;
    Clips r;
    int rc = render_clips(c, resample, rate_in, rate_out, &lens_out, &r);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    TableLock lk(g_tables.mu);
    RenderTables t;
    rc = render_tables(lk, device, N, window, resample, rate_in, rate_out, &t);
    if (rc) return rc;
    DevCarve cv;
    const RenderParts p = render_parts(cv, c, r, resample, width, height);
    DevBlocks b;
    cv.alloc(b);
    if (b.he == hipSuccess) b.he = hipMemcpy(cv.at<void>(p.o_pcm), pcm, p.pcm_bytes, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        render_enqueue(t, cv, p, c, r, width, height, top_db, range_db);
        b.he = hipGetLastError();
        lk.unlock();
        if (b.he == hipSuccess) b.he = hipMemcpy(image, cv.at<void>(p.o_img), p.img_bytes, hipMemcpyDeviceToHost);  // (the call's one synchronise)
    }
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(what, b);
}

// The render fused with the PNG encode (png.h: the indices never leave the device), for either form and any source, after the
// entry's own argument checks.  One DevCarve.
int png_run(const char* what, int device, ClipSource& src, const Clips& c, int rate_in, int rate_out, int width, int height,
            const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out, size_t out_cap, uint64_t* offsets) {
    const int n_clips = c.n_clips;
    const int N = spec_check(c, width, height, window, top_db, range_db);
    if (N < 0) return N;
    const bool resample = rate_out != 0 && rate_out != rate_in;
    std::vector<int> lens_out;
    Clips r;
    int rc = png_args_check(n_clips, width, height);
    if (!rc) rc = render_clips(c, resample, rate_in, rate_out, &lens_out, &r);
    if (!rc) rc = png_cap_check(n_clips, width, height, out_cap);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    TableLock lk(g_tables.mu);
    RenderTables t;
    rc = render_tables(lk, device, N, window, resample, rate_in, rate_out, &t);
    if (rc) return rc;
    const size_t cap = png_max_bytes(n_clips, width, height);
    DevCarve cv;
    const RenderParts p = render_parts(cv, c, r, resample, width, height);
    const size_t o_bytes = cv.add(cap), o_off = cv.add(((size_t)n_clips + 1) * 8), o_ws = cv.add(png_workspace_bytes(n_clips, width, height));
    src.reserve(cv);
    DevBlocks b;
    cv.alloc(b);
    uint8_t* d_bytes = cv.at<uint8_t>(o_bytes);
    unsigned long long* d_offsets = cv.at<unsigned long long>(o_off);
    if (b.he == hipSuccess) b.he = src.fill(cv, cv.at<int16_t>(p.o_pcm), p.pcm_bytes);
    if (b.he == hipSuccess) {
        render_enqueue(t, cv, p, c, r, width, height, top_db, range_db);
        launch_png(cv.at<uint8_t>(p.o_img), png_work(n_clips, width, height, palette, cv.at<void>(o_ws)), d_bytes, cap, d_offsets, nullptr);
        b.he = hipGetLastError();
        lk.unlock();
        if (b.he == hipSuccess) b.he = fetch_streams(d_offsets, d_bytes, n_clips, offsets, out);
        if (b.he == hipSuccess) b.he = src.finish(cv);
    }
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(what, b);
}

// The render of device-resident samples on the caller's stream.  `size_entry` names the bnhip_*_workspace_size of a form that takes a
// workspace (a ragged burst's rows); a uniform batch needs none and passes none.
int device_run(const char* what, const char* size_entry, int device, const void* d_samples, int f32, const Clips& c, int width, int height,
               const double* window, double top_db, double range_db, uint8_t* d_image, void* d_workspace, size_t workspace_bytes,
               void* hip_stream) {
    const int N = spec_check(c, width, height, window, top_db, range_db);
    if (N < 0) return N;
    int rc = workspace_check(d_workspace, workspace_bytes, spectrogram_table_bytes(c), size_entry);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    TableLock lk(g_tables.mu);
    const SpecTable* tab = spec_table(lk, device, N, window);
    if (!tab) return set_err(BNHIP_E_NOMEM, "device allocation failed (spectrogram table)");
    launch_spectrogram(d_samples, f32 != 0, c, width, height, tab->d, tab->wsum, top_db, range_db, d_image, d_workspace,
                       reinterpret_cast<hipStream_t>(hip_stream));
    return launch_status(what);
}

}  // namespace

namespace bnhip {

int spectrogram_image_check(int width, int height, const double* window, double top_db, double range_db) {
    return spec_image_check(width, height, window, top_db, range_db);
}
int spectrogram_png_run(const char* what, int device, ClipSource& src, const Clips& c, int rate_in, int rate_out, int width, int height,
                        const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out, size_t out_cap,
                        uint64_t* offsets) {
    return png_run(what, device, src, c, rate_in, rate_out, width, height, window, top_db, range_db, palette, out, out_cap, offsets);
}

}  // namespace bnhip

extern "C" {

int bnhip_spectrogram_size(int width, int* height, int* fft_size) {
    if (!height || !fft_size) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    if (width < 1 || width > 4096) return set_err(BNHIP_E_INVALID, "width must be in [1, 4096]");
    *height = fft_friendly_height(width);
    *fft_size = 2 * (*height - 1);
    if (*fft_size < SPEC_N_MIN || *fft_size > SPEC_N_MAX) return set_err(BNHIP_E_UNSUPPORTED, "FFT size 2 * (height - 1) must be in [64, 4096]");
    return BNHIP_OK;
}

int bnhip_spectrogram_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate_in, int rate_out, int width, int height,
                            const double* window, double top_db, double range_db, uint8_t* image) {
    if (!pcm || !image || n_clips <= 0) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    return image_run("spectrogram_pcm16", device, pcm, Clips::uniform(n_clips, n), rate_in, rate_out, width, height, window, top_db, range_db,
                     image);
    BN_GUARD_END((void)0)
}

// bnhip_spectrogram_pcm16 with the PNG encoder behind the render
int bnhip_spectrogram_png_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate_in, int rate_out, int width, int height,
                                const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out, size_t out_cap,
                                uint64_t* offsets) {
    if (!pcm || !palette || !out || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int rc = png_args_check(n_clips, width, height);                  // (this entry answers as the PNG entries do: n_images first)
    if (rc) return rc;
    PcmSource src(pcm);
    return png_run("spectrogram_png_pcm16", device, src, Clips::uniform(n_clips, n), rate_in, rate_out, width, height, window, top_db, range_db,
                   palette, out, out_cap, offsets);
    BN_GUARD_END((void)0)
}

int bnhip_spectrogram_device(int device, const void* d_samples, int f32, int n_clips, int n, int width, int height,
                             const double* window, double top_db, double range_db, uint8_t* d_image, void* hip_stream) {
    if (!d_samples || !d_image || n_clips <= 0) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    return device_run("spectrogram_device", nullptr, device, d_samples, f32, Clips::uniform(n_clips, n), width, height, window, top_db, range_db,
                      d_image, nullptr, 0, hip_stream);
    BN_GUARD_END((void)0)
}

// ---- ragged bursts: n_clips clips of lens[c] samples packed back to back (bnhip.h "Ragged bursts")

int bnhip_spectrogram_ragged_workspace_size(int n_clips, const int* lens, int width, int height, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const Clips c = Clips::ragged(n_clips, lens);
    int rc = lens_check(n_clips, lens);
    if (!rc) rc = spec_check(c, width, height, nullptr, 0.0, 1.0);
    if (rc < 0) return rc;
    *bytes = spectrogram_table_bytes(c);
    return BNHIP_OK;
}

int bnhip_spectrogram_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate_in, int rate_out, int width,
                                   int height, const double* window, double top_db, double range_db, uint8_t* image) {
    if (!pcm || !image) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int rc = lens_check(n_clips, lens);
    if (rc) return rc;
    return image_run("spectrogram_ragged_pcm16", device, pcm, Clips::ragged(n_clips, lens), rate_in, rate_out, width, height, window, top_db,
                     range_db, image);
    BN_GUARD_END((void)0)
}

int bnhip_spectrogram_png_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate_in, int rate_out, int width,
                                       int height, const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out,
                                       size_t out_cap, uint64_t* offsets) {
    if (!pcm || !palette || !out || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int rc = lens_check(n_clips, lens);
    if (rc) return rc;
    PcmSource src(pcm);
    return png_run("spectrogram_png_ragged_pcm16", device, src, Clips::ragged(n_clips, lens), rate_in, rate_out, width, height, window, top_db,
                   range_db, palette, out, out_cap, offsets);
    BN_GUARD_END((void)0)
}

int bnhip_flac_spectrogram_png(int device, const uint8_t* streams, int n_streams, const uint64_t* offsets, int rate_out, int width, int height,
                               const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out, size_t out_cap,
                               uint64_t* png_offsets, bnhip_flac_decode_result* result) {
    if (!streams || !offsets || !palette || !out || !png_offsets || !result) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    FlacSource src(streams, n_streams, offsets, result);
    int rc = flacdec_read_infos(streams, n_streams, offsets, &src.infos);
    if (!rc) rc = flacdec_burst_check(n_streams, src.infos.data(), offsets, nullptr);
    if (rc) return rc;
    std::vector<int> lens((size_t)n_streams);
    for (int c = 0; c < n_streams; c++) {
        const bnhip_flac_info& in = src.infos[(size_t)c];
        if (in.status != BNHIP_FLAC_OK) return set_err(BNHIP_E_INVALID, "every stream's metadata must be accepted (bnhip_flac_stream_info)");
        if (in.rate != src.infos[0].rate) return set_err(BNHIP_E_INVALID, "every stream must have the same sample rate");
        lens[(size_t)c] = (int)in.total_samples;
    }
    if (src.infos[0].rate > 0x7FFFFFFFu) return set_err(BNHIP_E_INVALID, "sample rates must be positive");
    return png_run("flac_spectrogram_png", device, src, Clips::ragged(n_streams, lens.data()), (int)src.infos[0].rate, rate_out, width, height,
                   window, top_db, range_db, palette, out, out_cap, png_offsets);
    BN_GUARD_END((void)0)
}

// bnhip_process_ragged_pcm16, then bnhip_spectrogram_png_ragged_pcm16 (with its resampler) in one call: the counterpart of
// ProcessedSpectrogramByID (internal/api/v2/media/media.go:1321), whose FFmpeg child (ffmpeg/process.go:212-251) feeds the
// spectrogram generator.  One DevCarve, one synchronising fetch.
int bnhip_process_spectrogram_png_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, int frame, double nr_db,
                                               double nf_db, int normalize, double target_lufs, double true_peak_dbtp, double gain_db,
                                               int rate_out, int width, int height, const double* window, double top_db, double range_db,
                                               const uint8_t* palette, uint8_t* out, size_t out_cap, uint64_t* png_offsets,
                                               bnhip_loudness* loud, int16_t* out_pcm) {
    if (!pcm || !lens || !palette || !out || !png_offsets || (normalize && !loud)) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const Clips c = Clips::ragged(n_clips, lens);
    const ChainArgs a{rate, frame, nr_db, nf_db, normalize, target_lufs, true_peak_dbtp, gain_db};
    int rc = chain_check(c, a);
    if (rc) return rc;
    ProcessSource src(pcm, device, c, a, loud, out_pcm);
    rc = png_run("process_spectrogram_png_ragged_pcm16", device, src, c, rate, rate_out, width, height, window, top_db, range_db, palette, out,
                 out_cap, png_offsets);
    return src.rc ? set_err(src.rc, src.err) : rc;
    BN_GUARD_END((void)0)
}

int bnhip_spectrogram_ragged_device(int device, const void* d_samples, int f32, int n_clips, const int* lens, int width, int height,
                                    const double* window, double top_db, double range_db, uint8_t* d_image, void* d_workspace,
                                    size_t workspace_bytes, void* hip_stream) {
    if (!d_samples || !d_image || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int rc = lens_check(n_clips, lens);
    if (rc) return rc;
    return device_run("spectrogram_ragged_device", "bnhip_spectrogram_ragged_workspace_size", device, d_samples, f32, Clips::ragged(n_clips, lens),
                      width, height, window, top_db, range_db, d_image, d_workspace, workspace_bytes, hip_stream);
    BN_GUARD_END((void)0)
}

}  // extern "C"
