// C ABI of file analysis: whole recordings in, the top-k of every overlapping window (or the detection rows above a threshold) out,
// in one call - the windows are framed on the device (analyze.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "analyze.h"
#include "api_model.h"

using namespace bnhip;

static_assert(sizeof(bnhip_detection) == 16 && sizeof(DetRow) == 16, "a detection row is 16 bytes");

namespace bnhip {

// wav.frame_clips: p = 0; loop { remain = L - p; keep if first | remain >= clip | remain >= min_tail; stop if remain <= clip; p += hop }.
// Every window in front of the last one visited has remain > clip and is kept; the last one visited is window
// J = ceil((L - clip) / hop) (0 for L <= clip), which starts inside the recording because hop <= clip.
long long analyze_windows(const long long* lengths, int n_rec, int n_samples, int hop, long long min_tail, long long* first) {
    long long total = 0;
    first[0] = 0;
    for (int r = 0; r < n_rec; r++) {
        const long long L = lengths[r];
        const long long J = L > n_samples ? (L - n_samples + hop - 1) / hop : 0;
        const long long remain = L - J * hop;
        const bool keep = J == 0 || remain >= n_samples || remain >= min_tail;
        total += J + (keep ? 1 : 0);
        first[r + 1] = total;
    }
    return total;
}

}  // namespace bnhip

namespace {

constexpr size_t TOPK_LDS_MAX = 150 * 1024;             // the top-k kernel keeps one clip's confidences in LDS (api_predict.cpp)
constexpr long long ANALYZE_MAX_SAMPLES = (1ll << 36) - 1;

// the table arguments of all three entries; n_samples is the window (the model's clip)
int check_table(const int64_t* lengths, int n_recordings, int n_samples, int hop, int64_t min_tail) {
    if (!lengths) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_recordings < 1 || n_recordings > 65535) return set_err(BNHIP_E_INVALID, "n_recordings must be in [1, 65535]");
    if (n_samples < 1) return set_err(BNHIP_E_INVALID, "n_samples must be positive");
    if (hop < 1 || hop > n_samples) return set_err(BNHIP_E_INVALID, "hop must be in [1, n_samples]");
    if (min_tail < 0) return set_err(BNHIP_E_INVALID, "min_tail must not be negative");
    long long total = 0;
    for (int r = 0; r < n_recordings; r++) {
        if (lengths[r] < 1) return set_err(BNHIP_E_INVALID, "every recording needs at least one sample");
        if (lengths[r] > ANALYZE_MAX_SAMPLES - total) return set_err(BNHIP_E_INVALID, "burst of 2^36 samples or more");
        total += lengths[r];
    }
    return BNHIP_OK;
}

#define AN_HIP(call, what)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (ok && e_ != hipSuccess) { ok = false; err = std::string(what) + ": " + hipGetErrorString(e_); } \
    } while (0)

// bnhip_analyze_pcm_topk, and with `det` the detection rows behind it
int analyze(bnhip_model* m, const void* pcm, int bits, const int64_t* lengths, int n_recordings, int hop, int64_t min_tail, int activation,
            double sensitivity, int k, float* out_conf, int32_t* out_idx, bool det, float threshold, bnhip_detection* out_rows, size_t cap,
            size_t* n_out) {
    if (!m || !pcm || !lengths) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (det ? (!n_out || (cap && !out_rows)) : (!out_conf || !out_idx)) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (bits != 0 && bits != 16 && bits != 24 && bits != 32)
        return set_err(BNHIP_E_INVALID, "unsupported bit depth: " + std::to_string(bits) + " (supported: 0 = float32, 16, 24, 32)");
    if (k <= 0) return set_err(BNHIP_E_INVALID, "k must be positive");
    if (activation < 0 || activation > 2) return set_err(BNHIP_E_INVALID, "unknown activation");
    Engine& e = m->eng();
    if (int rc = check_table(lengths, n_recordings, e.n_samples, hop, min_tail)) return rc;
    if (m->engs.size() > 1) return set_err(BNHIP_E_INVALID, "file analysis runs on one device; use a single-device handle");
    if (e.device < 0) return set_err(BNHIP_E_INVALID, "plan-only model cannot run");
    if ((size_t)e.n_classes * 4 > TOPK_LDS_MAX) return set_err(BNHIP_E_UNSUPPORTED, "too many classes for the LDS top-k");
    std::vector<long long> table((size_t)n_recordings * 3 + 1);       // first[n + 1], then slot[n][2]
    long long* first = table.data();
    long long* slot = first + n_recordings + 1;
    std::vector<long long> len64(lengths, lengths + n_recordings);
    const long long W64 = analyze_windows(len64.data(), n_recordings, e.n_samples, hop, min_tail, first);
    if (W64 > INT_MAX) return set_err(BNHIP_E_INVALID, "more than INT_MAX windows");
    const int W = (int)W64, kk = std::min(k, e.n_classes);
    size_t block_bytes = 0;
    for (int r = 0; r < n_recordings; r++) {
        slot[2 * r] = (long long)block_bytes; slot[2 * r + 1] = lengths[r];
        block_bytes += analyze_slot_bytes(lengths[r], bits);
    }
    if (hipSetDevice(e.device) != hipSuccess) return set_err(BNHIP_E_RUNTIME, "hipSetDevice failed");
    // whatever an earlier asynchronous call still has queued on the engine's streams finishes first (as host_run does)
    e.sync_contexts();
    if (e.stream) hipStreamSynchronize(e.stream);
    // one allocation: recordings | tables | top-k confidences | top-k indices | detection scratch | row count | rows
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t table_bytes = table.size() * 8, tk_bytes = (size_t)W * kk * 4;
    const size_t rows_cap = det ? std::min(cap, (size_t)W * kk) : 0;
    const size_t o_table = up(block_bytes), o_conf = o_table + up(table_bytes), o_idx = o_conf + up(tk_bytes), o_scr = o_idx + up(tk_bytes);
    const size_t o_total = o_scr + (det ? up(detections_scratch_bytes(W)) : 0), o_rows = o_total + (det ? 256 : 0);
    const size_t all_bytes = o_rows + up(rows_cap * sizeof(DetRow));
    char* d = nullptr;
    if (hipMalloc((void**)&d, all_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(BNHIP_E_NOMEM, "device allocation failed (file analysis)");
    }
    bool ok = true;
    std::string err;
    const size_t sb = analyze_sample_bytes(bits);
    // the slots' zero fill, then one copy per recording into its slot
    AN_HIP(hipMemsetAsync(d, 0, o_table, e.stream), "memset");
    const char* src = static_cast<const char*>(pcm);
    for (int r = 0; ok && r < n_recordings; r++) {
        AN_HIP(hipMemcpyAsync(d + slot[2 * r], src, (size_t)lengths[r] * sb, hipMemcpyHostToDevice, e.stream), "H2D copy");
        src += (size_t)lengths[r] * sb;
    }
    AN_HIP(hipMemcpyAsync(d + o_table, table.data(), table_bytes, hipMemcpyHostToDevice, e.stream), "H2D copy");
    WinView view;
    view.first = reinterpret_cast<const long long*>(d + o_table);
    view.slot = view.first + n_recordings + 1;
    view.n_rec = n_recordings; view.hop = hop; view.w0 = 0;
    float* d_conf = reinterpret_cast<float*>(d + o_conf);
    int32_t* d_idx = reinterpret_cast<int32_t*>(d + o_idx);
    // the windows in chunks of max_batch, every chunk enqueued behind the previous one (as bnhip_range_heatmap runs its rows)
    for (int w0 = 0; ok && w0 < W; w0 += e.max_batch) {
        const int n = std::min(e.max_batch, W - w0);
        PcmSource ps;
        ps.samples = d; ps.bits = bits; ps.win = win_at(view, w0);
        ok = e.run(e.d_stage_in, n, e.d_stage_logits, nullptr, &err, ps);
        if (!ok) break;
        launch_activation(e.d_stage_logits, e.d_post_conf, n, e.n_classes, activation, sensitivity, e.stream);
        launch_topk(e.d_post_conf, n, e.n_classes, kk, d_conf + (size_t)w0 * kk, d_idx + (size_t)w0 * kk, e.stream);
    }
    unsigned long long total = 0;
    if (ok && det) {
        launch_detections(d_conf, d_idx, W, kk, threshold, view, d + o_scr, reinterpret_cast<DetRow*>(d + o_rows), rows_cap,
                          reinterpret_cast<unsigned long long*>(d + o_total), e.stream);
    }
    if (ok) AN_HIP(hipGetLastError(), "kernel launch");
    if (ok && det) {
        AN_HIP(hipMemcpyAsync(&total, d + o_total, 8, hipMemcpyDeviceToHost, e.stream), "D2H copy");
        AN_HIP(hipStreamSynchronize(e.stream), "file analysis");
        const size_t n_rows = (size_t)std::min<unsigned long long>(total, rows_cap);
        if (ok && n_rows) AN_HIP(hipMemcpyAsync(out_rows, d + o_rows, n_rows * sizeof(DetRow), hipMemcpyDeviceToHost, e.stream), "D2H copy");
    } else if (ok) {
        AN_HIP(hipMemcpyAsync(out_conf, d_conf, tk_bytes, hipMemcpyDeviceToHost, e.stream), "D2H copy");
        AN_HIP(hipMemcpyAsync(out_idx, d_idx, tk_bytes, hipMemcpyDeviceToHost, e.stream), "D2H copy");
    }
    {
        const hipError_t he = hipStreamSynchronize(e.stream);
        if (ok && he != hipSuccess) { ok = false; err = std::string("file analysis: ") + hipGetErrorString(he); }
    }
    hipFree(d);
    if (!ok) { (void)hipGetLastError(); e.mm_dirty = true; return set_err(BNHIP_E_RUNTIME, err); }
    if (det) *n_out = (size_t)total;
    return BNHIP_OK;
}

}  // namespace

extern "C" {

long long bnhip_analyze_windows(const int64_t* lengths, int n_recordings, int n_samples, int hop, int64_t min_tail, int64_t* first_window) {
    if (!first_window) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (int rc = check_table(lengths, n_recordings, n_samples, hop, min_tail)) return rc;
    BN_GUARD_BEGIN
    std::vector<long long> len64(lengths, lengths + n_recordings), first((size_t)n_recordings + 1);
    const long long W = analyze_windows(len64.data(), n_recordings, n_samples, hop, min_tail, first.data());
    std::copy(first.begin(), first.end(), first_window);
    return W;
    BN_GUARD_END((void)0)
}

int bnhip_analyze_pcm_topk(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                           int64_t min_tail, int activation, double sensitivity, int k, float* out_conf, int32_t* out_idx) {
    BN_GUARD_BEGIN
    return analyze(m, pcm, bits_per_sample, lengths, n_recordings, hop, min_tail, activation, sensitivity, k, out_conf, out_idx, false, 0.f,
                   nullptr, 0, nullptr);
    BN_GUARD_END((void)0)
}

int bnhip_analyze_pcm(bnhip_model* m, const void* pcm, int bits_per_sample, const int64_t* lengths, int n_recordings, int hop,
                      int64_t min_tail, int activation, double sensitivity, int k, float threshold, bnhip_detection* out, size_t cap,
                      size_t* n_out) {
    BN_GUARD_BEGIN
    return analyze(m, pcm, bits_per_sample, lengths, n_recordings, hop, min_tail, activation, sensitivity, k, nullptr, nullptr, true, threshold,
                   out, cap, n_out);
    BN_GUARD_END((void)0)
}

}  // extern "C"
