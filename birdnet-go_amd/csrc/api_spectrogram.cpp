// C ABI of the detection-clip spectrogram images (bnhip_spectrogram_size, bnhip_spectrogram_pcm16, bnhip_spectrogram_device), of
// the render fused with the PNG encoder of api_png.cpp (bnhip_spectrogram_png_pcm16), which needs this file's window and rate tables,
// and of their forms for a ragged burst (bnhip_spectrogram_ragged_workspace_size, bnhip_spectrogram_ragged_pcm16,
// bnhip_spectrogram_png_ragged_pcm16, bnhip_spectrogram_ragged_device), the last also fed by the device FLAC decoder of flac_decode.h
// in place of the host's PCM (bnhip_flac_spectrogram_png), or by the processed-audio chain of process_chain.h behind it
// (bnhip_process_spectrogram_png_ragged_pcm16).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <numeric>

#include "api_oneshot.h"
#include "flac_decode.h"
#include "kernels.h"
#include "png.h"
#include "process_chain.h"
#include "resample.h"
#include "spectrogram.h"

namespace bnhip {
// (api_flac_decode.cpp)
int flacdec_read_infos(const uint8_t* streams, int n_streams, const uint64_t* offsets, std::vector<bnhip_flac_info>* infos);
int flacdec_burst_check(int n_streams, const bnhip_flac_info* infos, const uint64_t* offsets, size_t* pcm_samples);
}  // namespace bnhip

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
int spec_check(int n_clips, int n, int width, int height, const double* window, double top_db, double range_db) {
    if (n_clips <= 0) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    if (const int rc = clip_dims_check(n_clips, n)) return rc;
    return spec_image_check(width, height, window, top_db, range_db);
}
int spec_ragged_check(int n_clips, const int* lens, int width, int height, const double* window, double top_db, double range_db) {
    if (const int rc = ragged_lens_check(n_clips, lens)) return rc;
    return spec_image_check(width, height, window, top_db, range_db);
}

// What a host-pointer render holds under the table lock: the window table and, with a rate change, the phase table and the
// rendered length.
struct RenderTables { const SpecTable* tab = nullptr; const RateTable* rt = nullptr; int n_render = 0; };
int render_tables(const TableLock& lk, int device, int N, const double* window, bool resample, int n, int rate_in, int rate_out, RenderTables* t) {
    t->n_render = n;
    if (resample) {
        t->rt = rate_table(lk, device, rate_in, rate_out);
        if (!t->rt) return set_err(BNHIP_E_NOMEM, "device allocation failed (resampler phase table)");
        if (!t->rt->d) return set_err(BNHIP_E_UNSUPPORTED, "resample ratio needs a phase table larger than LDS");
        t->n_render = bnhip_resample_length(n, rate_in, rate_out);
        if (t->n_render < 1) return set_err(BNHIP_E_INVALID, "n must be at least 1");
    }
    t->tab = spec_table(lk, device, N, window);
    if (!t->tab) return set_err(BNHIP_E_NOMEM, "device allocation failed (spectrogram table)");
    return 0;
}
// d_pcm int16 [n_clips][n] -> d_img on the null stream; d_f32 [n_clips][n_render] is the resampler's output where there is a rate change
void render_enqueue(const RenderTables& t, const int16_t* d_pcm, float* d_f32, int n_clips, int n, int width, int height, double top_db,
                    double range_db, uint8_t* d_img) {
    const RateTable* rt = t.rt;
    if (rt) launch_resample(d_pcm, d_f32, rt->d, 1, 0, n_clips, n, t.n_render, rt->L, rt->M, rt->T, rt->half, 0, 0, nullptr);
    launch_spectrogram(rt ? (const void*)d_f32 : (const void*)d_pcm, rt ? 1 : 0, n_clips, t.n_render, width, height, t.tab->d, t.tab->wsum, top_db,
                       range_db, d_img, nullptr);
}


// The lengths a ragged burst is rendered at: lens itself, or with a rate change every clip's bnhip_resample_length (held to what
// ragged_lens_check asks of the input, so that the packed floats and their tiles stay inside the same limits).  -> 0 or a BNHIP_E_*
int ragged_render_lens(int n_clips, const int* lens, bool resample, int rate_in, int rate_out, std::vector<int>* lens_out) {
    if (!resample) return 0;
    if (rate_in <= 0 || rate_out < 0) return set_err(BNHIP_E_INVALID, "sample rates must be positive");
    lens_out->resize((size_t)n_clips);
    for (int c = 0; c < n_clips; c++) (*lens_out)[c] = bnhip_resample_length(lens[c], rate_in, rate_out);
    return ragged_lens_check(n_clips, lens_out->data());
}
// the device parts of a ragged host-pointer render, carved from the call's one block: packed PCM, images, the resampler's packed
// floats and the two kernels' tables
struct RaggedParts { size_t pcm_bytes, img_bytes, o_pcm, o_img, o_f32, o_rows, o_rtab; };
RaggedParts ragged_parts(DevCarve& cv, int n_clips, const int* lens, const std::vector<int>& lens_out, int width, int height) {
    RaggedParts r;
    r.pcm_bytes = ragged_total(n_clips, lens) * 2;
    r.img_bytes = (size_t)n_clips * height * width;
    r.o_pcm = cv.add(r.pcm_bytes); r.o_img = cv.add(r.img_bytes);
    r.o_f32 = cv.add(lens_out.empty() ? 0 : ragged_total(n_clips, lens_out.data()) * 4);
    r.o_rows = cv.add(spectrogram_ragged_table_bytes(n_clips));
    r.o_rtab = cv.add(lens_out.empty() ? 0 : resample_ragged_table_bytes(n_clips));
    return r;
}
// packed d_pcm -> d_img on the null stream, through the ragged resampler where there is a rate change (lens_out not empty)
void ragged_render_enqueue(const RenderTables& t, const DevCarve& cv, const RaggedParts& r, int n_clips, const int* lens,
                           const std::vector<int>& lens_out, int width, int height, double top_db, double range_db) {
    const RateTable* rt = t.rt;
    const int16_t* d_pcm = cv.at<int16_t>(r.o_pcm);
    float* d_f32 = cv.at<float>(r.o_f32);
    if (rt) launch_resample_ragged(d_pcm, d_f32, rt->d, n_clips, lens, lens_out.data(), rt->L, rt->M, rt->T, rt->half, cv.at<void>(r.o_rtab), nullptr);
    launch_spectrogram_ragged(rt ? (const void*)d_f32 : (const void*)d_pcm, rt ? 1 : 0, n_clips, rt ? lens_out.data() : lens, width, height,
                              t.tab->d, t.tab->wsum, top_db, range_db, cv.at<uint8_t>(r.o_img), cv.at<void>(r.o_rows), nullptr);
}

// Where the packed int16 clips of a ragged render come from: the host's PCM, or a decode on the device.  reserve() adds the source's
// own parts to the call's one block, fill() enqueues on the null stream what puts the clips at d_pcm, finish() runs after the
// call's synchronise.
struct RaggedSource {
    virtual void reserve(DevCarve&) {}
    virtual hipError_t fill(const DevCarve& cv, int16_t* d_pcm, size_t pcm_bytes) = 0;
    virtual hipError_t finish(const DevCarve&) { return hipSuccess; }
    virtual ~RaggedSource() {}
};
struct PcmSource : RaggedSource {
    const int16_t* pcm;
    explicit PcmSource(const int16_t* p) : pcm(p) {}
    hipError_t fill(const DevCarve&, int16_t* d_pcm, size_t pcm_bytes) override { return hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice); }
};
// FLAC streams in host memory: the compressed bytes are what crosses to the device, the clips are decoded where the render reads them
struct FlacSource : RaggedSource {
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
        launch_flacdec(d_in, flacdec_work(n_streams, infos.data(), offsets, cv.at<void>(o_ws)), d_pcm, pcm_bytes / 2,
                       cv.at<bnhip_flac_decode_result>(o_res), nullptr);
        return hipGetLastError();
    }
    hipError_t finish(const DevCarve& cv) override {
        return hipMemcpy(result, cv.at<void>(o_res), (size_t)n_streams * sizeof(bnhip_flac_decode_result), hipMemcpyDeviceToHost);
    }
};

// The host's PCM through the chain denoise -> normalise -> gain: the unprocessed clips are what crosses to the device, the
// processed ones are written where the render reads them and reach the host only if the caller asks for them
struct ProcessSource : RaggedSource {
    const int16_t* pcm;
    int device;
    ChainClips clips;
    ChainArgs args;
    bnhip_loudness* loud;
    int16_t* out_pcm;
    ChainParts parts;
    const int16_t* d_final = nullptr;
    int rc = 0;                              // the chain's own refusal, with its text: what the entry answers instead of a HIP error
    std::string err;
    ProcessSource(const int16_t* p, int dev, const ChainClips& c, const ChainArgs& a, bnhip_loudness* l, int16_t* o)
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

// The ragged render fused with the PNG encode, for any source: the body of bnhip_spectrogram_png_ragged_pcm16 and
// bnhip_flac_spectrogram_png after their own argument checks.
int png_ragged_run(const char* what, int device, RaggedSource& src, int n_clips, const int* lens, int rate_in, int rate_out, int width, int height,
                   const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out, size_t out_cap, uint64_t* offsets) {
    const int N = spec_ragged_check(n_clips, lens, width, height, window, top_db, range_db);
    if (N < 0) return N;
    const bool resample = rate_out != 0 && rate_out != rate_in;
    std::vector<int> lens_out;
    int rc = png_args_check(n_clips, width, height);
    if (!rc) rc = ragged_render_lens(n_clips, lens, resample, rate_in, rate_out, &lens_out);
    if (!rc) rc = png_cap_check(n_clips, width, height, out_cap);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    TableLock lk(g_tables.mu);
    RenderTables t;
    rc = render_tables(lk, device, N, window, resample, lens[0], rate_in, rate_out, &t);       // (its n_render is not used here)
    if (rc) return rc;
    const size_t cap = png_max_bytes(n_clips, width, height);
    DevCarve cv;
    const RaggedParts r = ragged_parts(cv, n_clips, lens, lens_out, width, height);
    const size_t o_bytes = cv.add(cap), o_off = cv.add(((size_t)n_clips + 1) * 8), o_ws = cv.add(png_workspace_bytes(n_clips, width, height));
    src.reserve(cv);
    DevBlocks b;
    cv.base = (char*)b.get(cv.bytes());
    uint8_t* d_bytes = cv.at<uint8_t>(o_bytes);
    unsigned long long* d_offsets = cv.at<unsigned long long>(o_off);
    if (b.he == hipSuccess) b.he = src.fill(cv, cv.at<int16_t>(r.o_pcm), r.pcm_bytes);
    if (b.he == hipSuccess) {
        ragged_render_enqueue(t, cv, r, n_clips, lens, lens_out, width, height, top_db, range_db);
        launch_png(cv.at<uint8_t>(r.o_img), png_work(n_clips, width, height, palette, cv.at<void>(o_ws)), d_bytes, cap, d_offsets, nullptr);
        b.he = hipGetLastError();
        lk.unlock();
        if (b.he == hipSuccess) b.he = png_fetch(d_offsets, d_bytes, n_clips, offsets, out);
        if (b.he == hipSuccess) b.he = src.finish(cv);
    }
    return b.he == hipSuccess ? BNHIP_OK : hip_fail(what, b);
}

}  // namespace

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
    if (!pcm || !image) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int N = spec_check(n_clips, n, width, height, window, top_db, range_db);
    if (N < 0) return N;
    const bool resample = rate_out != 0 && rate_out != rate_in;
    if (resample && (rate_in <= 0 || rate_out < 0)) return set_err(BNHIP_E_INVALID, "sample rates must be positive");
    int rc = use_device(device);
    if (rc) return rc;
    TableLock lk(g_tables.mu);
    RenderTables t;
    rc = render_tables(lk, device, N, window, resample, n, rate_in, rate_out, &t);
    if (rc) return rc;
    const size_t img_bytes = (size_t)n_clips * height * width;
    DevBlocks b;
    int16_t* d_pcm = (int16_t*)b.get((size_t)n_clips * n * 2);
    uint8_t* d_img = (uint8_t*)b.get(img_bytes);
    float* d_f32 = resample ? (float*)b.get((size_t)n_clips * t.n_render * 4) : nullptr;
    if (b.he == hipSuccess) b.he = hipMemcpy(d_pcm, pcm, (size_t)n_clips * n * 2, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        render_enqueue(t, d_pcm, d_f32, n_clips, n, width, height, top_db, range_db, d_img);
        b.he = hipGetLastError();
        lk.unlock();
        if (b.he == hipSuccess) b.he = hipMemcpy(image, d_img, img_bytes, hipMemcpyDeviceToHost);  // (the call's one synchronise)
    }
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("spectrogram_pcm16", b);
    BN_GUARD_END((void)0)
}

// bnhip_spectrogram_pcm16 with the PNG encoder (png.h) behind the render: the indices never leave the device.  One device block.
int bnhip_spectrogram_png_pcm16(int device, const int16_t* pcm, int n_clips, int n, int rate_in, int rate_out, int width, int height,
                                const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out, size_t out_cap,
                                uint64_t* offsets) {
    if (!pcm || !palette || !out || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    int rc = png_args_check(n_clips, width, height);
    if (rc) return rc;
    const int N = spec_check(n_clips, n, width, height, window, top_db, range_db);
    if (N < 0) return N;
    const bool resample = rate_out != 0 && rate_out != rate_in;
    if (resample && (rate_in <= 0 || rate_out < 0)) return set_err(BNHIP_E_INVALID, "sample rates must be positive");
    rc = png_cap_check(n_clips, width, height, out_cap);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    TableLock lk(g_tables.mu);
    RenderTables t;
    rc = render_tables(lk, device, N, window, resample, n, rate_in, rate_out, &t);
    if (rc) return rc;
    const size_t pcm_bytes = (size_t)n_clips * n * 2, cap = png_max_bytes(n_clips, width, height);
    DevCarve cv;
    const size_t o_pcm = cv.add(pcm_bytes), o_img = cv.add((size_t)n_clips * height * width);
    const size_t o_f32 = cv.add(resample ? (size_t)n_clips * t.n_render * 4 : 0), o_bytes = cv.add(cap), o_off = cv.add(((size_t)n_clips + 1) * 8);
    const size_t o_ws = cv.add(png_workspace_bytes(n_clips, width, height));
    DevBlocks b;
    cv.base = (char*)b.get(cv.bytes());
    int16_t* d_pcm = cv.at<int16_t>(o_pcm);
    uint8_t *d_img = cv.at<uint8_t>(o_img), *d_bytes = cv.at<uint8_t>(o_bytes);
    unsigned long long* d_offsets = cv.at<unsigned long long>(o_off);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_pcm, pcm, pcm_bytes, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        render_enqueue(t, d_pcm, resample ? cv.at<float>(o_f32) : nullptr, n_clips, n, width, height, top_db, range_db, d_img);
        launch_png(d_img, png_work(n_clips, width, height, palette, cv.at<void>(o_ws)), d_bytes, cap, d_offsets, nullptr);
        b.he = hipGetLastError();
        lk.unlock();
        if (b.he == hipSuccess) b.he = png_fetch(d_offsets, d_bytes, n_clips, offsets, out);
    }
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("spectrogram_png_pcm16", b);
    BN_GUARD_END((void)0)
}

int bnhip_spectrogram_device(int device, const void* d_samples, int f32, int n_clips, int n, int width, int height,
                             const double* window, double top_db, double range_db, uint8_t* d_image, void* hip_stream) {
    if (!d_samples || !d_image) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int N = spec_check(n_clips, n, width, height, window, top_db, range_db);
    if (N < 0) return N;
    int rc = use_device(device);
    if (rc) return rc;
    TableLock lk(g_tables.mu);
    const SpecTable* tab = spec_table(lk, device, N, window);
    if (!tab) return set_err(BNHIP_E_NOMEM, "device allocation failed (spectrogram table)");
    launch_spectrogram(d_samples, f32 != 0, n_clips, n, width, height, tab->d, tab->wsum, top_db, range_db, d_image,
                       reinterpret_cast<hipStream_t>(hip_stream));
    return launch_status("spectrogram_device");
    BN_GUARD_END((void)0)
}

// ---- ragged bursts: n_clips clips of lens[c] samples packed back to back (bnhip.h "Ragged bursts")

int bnhip_spectrogram_ragged_workspace_size(int n_clips, const int* lens, int width, int height, size_t* bytes) {
    if (!bytes) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    const int N = spec_ragged_check(n_clips, lens, width, height, nullptr, 0.0, 1.0);
    if (N < 0) return N;
    *bytes = spectrogram_ragged_table_bytes(n_clips);
    return BNHIP_OK;
}

int bnhip_spectrogram_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate_in, int rate_out, int width,
                                   int height, const double* window, double top_db, double range_db, uint8_t* image) {
    if (!pcm || !image) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int N = spec_ragged_check(n_clips, lens, width, height, window, top_db, range_db);
    if (N < 0) return N;
    const bool resample = rate_out != 0 && rate_out != rate_in;
    std::vector<int> lens_out;
    int rc = ragged_render_lens(n_clips, lens, resample, rate_in, rate_out, &lens_out);
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    TableLock lk(g_tables.mu);
    RenderTables t;
    rc = render_tables(lk, device, N, window, resample, lens[0], rate_in, rate_out, &t);       // (its n_render is not used here)
    if (rc) return rc;
    DevCarve cv;
    const RaggedParts r = ragged_parts(cv, n_clips, lens, lens_out, width, height);
    DevBlocks b;
    cv.base = (char*)b.get(cv.bytes());
    if (b.he == hipSuccess) b.he = hipMemcpy(cv.at<void>(r.o_pcm), pcm, r.pcm_bytes, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        ragged_render_enqueue(t, cv, r, n_clips, lens, lens_out, width, height, top_db, range_db);
        b.he = hipGetLastError();
        lk.unlock();
        if (b.he == hipSuccess) b.he = hipMemcpy(image, cv.at<void>(r.o_img), r.img_bytes, hipMemcpyDeviceToHost);  // (the call's one synchronise)
    }
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("spectrogram_ragged_pcm16", b);
    BN_GUARD_END((void)0)
}

int bnhip_spectrogram_png_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate_in, int rate_out, int width,
                                       int height, const double* window, double top_db, double range_db, const uint8_t* palette, uint8_t* out,
                                       size_t out_cap, uint64_t* offsets) {
    if (!pcm || !palette || !out || !offsets) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    PcmSource src(pcm);
    return png_ragged_run("spectrogram_png_ragged_pcm16", device, src, n_clips, lens, rate_in, rate_out, width, height, window, top_db, range_db,
                          palette, out, out_cap, offsets);
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
    return png_ragged_run("flac_spectrogram_png", device, src, n_streams, lens.data(), (int)src.infos[0].rate, rate_out, width, height, window,
                          top_db, range_db, palette, out, out_cap, png_offsets);
    BN_GUARD_END((void)0)
}

// bnhip_process_ragged_pcm16, then bnhip_spectrogram_png_ragged_pcm16 (with its resampler) in one call: the counterpart of
// ProcessedSpectrogramByID (internal/api/v2/media/media.go:1321), whose FFmpeg child (ffmpeg/process.go:212-251) feeds the
// spectrogram generator.  One device block, one synchronising fetch.
int bnhip_process_spectrogram_png_ragged_pcm16(int device, const int16_t* pcm, int n_clips, const int* lens, int rate, int frame, double nr_db,
                                               double nf_db, int normalize, double target_lufs, double true_peak_dbtp, double gain_db,
                                               int rate_out, int width, int height, const double* window, double top_db, double range_db,
                                               const uint8_t* palette, uint8_t* out, size_t out_cap, uint64_t* png_offsets,
                                               bnhip_loudness* loud, int16_t* out_pcm) {
    if (!pcm || !lens || !palette || !out || !png_offsets || (normalize && !loud)) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    ChainClips c;
    c.n_clips = n_clips; c.lens = lens;
    const ChainArgs a{rate, frame, nr_db, nf_db, normalize, target_lufs, true_peak_dbtp, gain_db};
    int rc = chain_check(c, a);
    if (rc) return rc;
    ProcessSource src(pcm, device, c, a, loud, out_pcm);
    rc = png_ragged_run("process_spectrogram_png_ragged_pcm16", device, src, n_clips, lens, rate, rate_out, width, height, window, top_db,
                        range_db, palette, out, out_cap, png_offsets);
    return src.rc ? set_err(src.rc, src.err) : rc;
    BN_GUARD_END((void)0)
}

int bnhip_spectrogram_ragged_device(int device, const void* d_samples, int f32, int n_clips, const int* lens, int width, int height,
                                    const double* window, double top_db, double range_db, uint8_t* d_image, void* d_workspace,
                                    size_t workspace_bytes, void* hip_stream) {
    if (!d_samples || !d_image || !d_workspace) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    BN_GUARD_BEGIN
    const int N = spec_ragged_check(n_clips, lens, width, height, window, top_db, range_db);
    if (N < 0) return N;
    int rc = workspace_check(d_workspace, workspace_bytes, spectrogram_ragged_table_bytes(n_clips), "bnhip_spectrogram_ragged_workspace_size");
    if (!rc) rc = use_device(device);
    if (rc) return rc;
    TableLock lk(g_tables.mu);
    const SpecTable* tab = spec_table(lk, device, N, window);
    if (!tab) return set_err(BNHIP_E_NOMEM, "device allocation failed (spectrogram table)");
    launch_spectrogram_ragged(d_samples, f32 != 0, n_clips, lens, width, height, tab->d, tab->wsum, top_db, range_db, d_image, d_workspace,
                              reinterpret_cast<hipStream_t>(hip_stream));
    return launch_status("spectrogram_ragged_device");
    BN_GUARD_END((void)0)
}

}  // extern "C"
