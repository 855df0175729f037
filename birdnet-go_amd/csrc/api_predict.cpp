// C ABI of the model handle's run entries: the predict and top-k families, the window assembler's tick, the range filter's
// heat-map grid and the debug fetch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "api_events.h"
#include "api_model.h"
#include "heatmap.h"
#include "hostpipe.h"
#include "windows.h"

using namespace bnhip;

namespace {

bool pcm_depth_known(int bits) { return bits == 16 || bits == 24 || bits == 32; }
// bytes of one clip on the host.  pcm_bits: 0 = float32 samples, 16 / 24 / 32 = little-endian PCM converted on the device
size_t clip_stride(const Engine& e, int pcm_bits) { return (size_t)e.n_samples * (pcm_bits ? (size_t)pcm_bits / 8 : 4); }
constexpr size_t TOPK_LDS_MAX = 150 * 1024;             // the top-k kernel keeps one clip's confidences in LDS
const char* const TOPK_LDS_TEXT = "too many classes for the LDS top-k";

// Clips [off, off + cnt) of a host call as one engine's job: `call` describes the whole call (src, pcm_bits and either logits /
// emb or topk / activation / sensitivity / out_conf / out_idx); every pointer moves to the shard's first clip.
HostJob shard_job(const Engine& e, const HostJob& call, int off, int cnt) {
    HostJob j = call;
    const size_t o = (size_t)off, kk = (size_t)std::min(call.topk, e.n_classes);
    j.src = (const char*)call.src + o * clip_stride(e, call.pcm_bits);
    j.n_clips = cnt;
    if (call.logits) j.logits = call.logits + o * e.n_classes;
    if (call.emb) j.emb = call.emb + o * e.emb_dim;
    if (call.out_conf) j.out_conf = call.out_conf + o * kk;
    if (call.out_idx) j.out_idx = call.out_idx + o * kk;
    return j;
}

// ---------------------------------------------------------------------------------------------- one engine, one shard
// The work itself - small calls straight through the engine, calls of >= 128 clips as chunks on alternating contexts fed
// from pinned staging - is hostpipe.cpp's host_run.
int predict_host(bnhip_model* m, const void* src, int pcm_bits, int n_clips, float* logits, float* emb) {
    if (!m || !src || !logits) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_clips <= 0) return set_err(BNHIP_E_INVALID, "n_clips must be positive");
    Engine& e0 = m->eng();
    if (e0.device < 0) return set_err(BNHIP_E_INVALID, "plan-only model cannot run");
    if (emb && !e0.emb_dim) return set_err(BNHIP_E_INVALID, "model has no embedding output");
    HostJob call;
    call.src = src; call.pcm_bits = pcm_bits; call.logits = logits; call.emb = emb;
    return shard_run(m, n_clips, [=](Engine& e, int off, int cnt, std::string& err) { return host_run(e, shard_job(e, call, off, cnt), err); });
}

int ensure_topk(Engine& e, int k, std::string& err) {
    if (k <= e.topk_cap) return BNHIP_OK;
    if (e.d_topk_conf) hipFree(e.d_topk_conf);
    if (e.d_topk_idx) hipFree(e.d_topk_idx);
    e.d_topk_conf = nullptr; e.d_topk_idx = nullptr; e.topk_cap = 0;
    if (hipMalloc((void**)&e.d_topk_conf, (size_t)e.max_batch * k * 4) != hipSuccess ||
        hipMalloc((void**)&e.d_topk_idx, (size_t)e.max_batch * k * 4) != hipSuccess) {
        if (e.d_topk_conf) { hipFree(e.d_topk_conf); e.d_topk_conf = nullptr; }
        err = "device allocation failed (top-k)";
        return BNHIP_E_NOMEM;
    }
    e.topk_cap = k;
    return BNHIP_OK;
}

// activation + top-k of logits that are already on the host (bnhip_postprocess_topk)
int post_topk_one(Engine& e, const float* logits, int n_clips, int activation, double sensitivity, int k, float* out_conf,
                  int32_t* out_idx, std::string& err) {
    if (hipSetDevice(e.device) != hipSuccess) { err = "hipSetDevice failed"; return BNHIP_E_RUNTIME; }
    const int n_classes = e.n_classes;
    int kk = std::min(k, n_classes);
    int rc = ensure_topk(e, kk, err);
    if (rc) return rc;
    for (int off = 0; off < n_clips; off += e.max_batch) {
        int n = std::min(e.max_batch, n_clips - off);
        hipError_t he = hipMemcpyAsync(e.d_stage_logits, logits + (size_t)off * n_classes, (size_t)n * n_classes * 4,
                                       hipMemcpyHostToDevice, e.stream);
        if (he != hipSuccess) { err = std::string("H2D copy: ") + hipGetErrorString(he); return BNHIP_E_RUNTIME; }
        launch_activation(e.d_stage_logits, e.d_post_conf, n, n_classes, activation, sensitivity, e.stream);
        launch_topk(e.d_post_conf, n, n_classes, kk, e.d_topk_conf, e.d_topk_idx, e.stream);
        hipMemcpyAsync(out_conf + (size_t)off * kk, e.d_topk_conf, (size_t)n * kk * 4, hipMemcpyDeviceToHost, e.stream);
        hipMemcpyAsync(out_idx + (size_t)off * kk, e.d_topk_idx, (size_t)n * kk * 4, hipMemcpyDeviceToHost, e.stream);
        he = hipStreamSynchronize(e.stream);
        if (he != hipSuccess) { err = std::string("top-k: ") + hipGetErrorString(he); return BNHIP_E_RUNTIME; }
    }
    return BNHIP_OK;
}

// pcm_bits as in clip_stride.  (The three top-k entries - this one, bnhip_postprocess_topk and the tick - check the same
// things in their own orders, which tests/test_cabi.py pins: the checks are not shared.)
int predict_topk_host(bnhip_model* m, const void* src, int pcm_bits, int n_clips, int activation, double sensitivity, int k,
                      float* out_conf, int32_t* out_idx) {
    if (!m || !src || !out_conf || !out_idx) return set_err(BNHIP_E_INVALID, "NULL argument");
    Engine& e = m->eng();
    if (n_clips <= 0 || k <= 0) return set_err(BNHIP_E_INVALID, "n_clips and k must be positive");
    if (activation < 0 || activation > 2) return set_err(BNHIP_E_INVALID, "unknown activation");
    if ((size_t)e.n_classes * 4 > TOPK_LDS_MAX) return set_err(BNHIP_E_UNSUPPORTED, TOPK_LDS_TEXT);
    if (e.device < 0) return set_err(BNHIP_E_INVALID, "plan-only model cannot run");
    HostJob call;
    call.src = src; call.pcm_bits = pcm_bits; call.topk = k; call.activation = activation; call.sensitivity = sensitivity;
    call.out_conf = out_conf; call.out_idx = out_idx;
    return shard_run(m, n_clips, [=](Engine& en, int off, int cnt, std::string& err) { return host_run(en, shard_job(en, call, off, cnt), err); });
}

}  // namespace

extern "C" {

int bnhip_predict_device(bnhip_model* m, const float* d_samples, int n_clips, float* d_logits, float* d_emb) {
    if (!m || !d_samples || !d_logits) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_clips <= 0) return set_err(BNHIP_E_INVALID, "n_clips must be positive");
    if (m->engs.size() > 1) return set_err(BNHIP_E_INVALID, "bnhip_predict_device: device pointers belong to one device; use a single-device handle");
    BN_GUARD_BEGIN
    Engine& e = m->eng();
    if (e.device < 0) return set_err(BNHIP_E_INVALID, "plan-only model cannot run");
    if (d_emb && !e.emb_dim) return set_err(BNHIP_E_INVALID, "model has no embedding output");
    if (hipSetDevice(e.device) != hipSuccess) return set_err(BNHIP_E_RUNTIME, "hipSetDevice failed");
    std::string err;
    for (int off = 0; off < n_clips; off += e.max_batch) {
        int n = std::min(e.max_batch, n_clips - off);
        if (!e.run_pipelined(d_samples + (size_t)off * e.n_samples, n, d_logits + (size_t)off * e.n_classes,
                             d_emb ? d_emb + (size_t)off * e.emb_dim : nullptr, &err))
            return set_err(BNHIP_E_RUNTIME, err);
    }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_predict(bnhip_model* m, const float* samples, int n_clips, float* logits, float* emb) {
    BN_GUARD_BEGIN
    return predict_host(m, samples, 0, n_clips, logits, emb);
    BN_GUARD_END((void)0)
}

int bnhip_predict_pcm16(bnhip_model* m, const int16_t* pcm, int n_clips, float* logits, float* emb) {
    BN_GUARD_BEGIN
    return predict_host(m, pcm, 16, n_clips, logits, emb);
    BN_GUARD_END((void)0)
}

int bnhip_predict_pcm(bnhip_model* m, const void* pcm, int bits_per_sample, int n_clips, float* logits, float* emb) {
    if (!pcm_depth_known(bits_per_sample)) return set_err(BNHIP_E_INVALID, "unsupported bit depth (supported: 16, 24, 32)");
    BN_GUARD_BEGIN
    return predict_host(m, pcm, bits_per_sample, n_clips, logits, emb);
    BN_GUARD_END((void)0)
}

int bnhip_postprocess_topk(bnhip_model* m, const float* logits, int n_clips, int n_classes, int activation,
                           double sensitivity, int k, float* out_conf, int32_t* out_idx) {
    if (!m || !logits || !out_conf || !out_idx) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    Engine& e = m->eng();
    if (n_clips <= 0 || k <= 0) return set_err(BNHIP_E_INVALID, "n_clips and k must be positive");
    if (e.device < 0) return set_err(BNHIP_E_INVALID, "plan-only model cannot run");
    if (n_classes != e.n_classes) return set_err(BNHIP_E_INVALID, "n_classes does not match the model");
    if (activation < 0 || activation > 2) return set_err(BNHIP_E_INVALID, "unknown activation");
    if ((size_t)n_classes * 4 > TOPK_LDS_MAX) return set_err(BNHIP_E_UNSUPPORTED, TOPK_LDS_TEXT);
    const int kk = std::min(k, n_classes);
    return shard_run(m, n_clips, [=](Engine& en, int off, int cnt, std::string& err) {
        return post_topk_one(en, logits + (size_t)off * n_classes, cnt, activation, sensitivity, k,
                             out_conf + (size_t)off * kk, out_idx + (size_t)off * kk, err);
    });
    BN_GUARD_END((void)0)
}

int bnhip_predict_topk(bnhip_model* m, const float* samples, int n_clips, int activation, double sensitivity, int k,
                       float* out_conf, int32_t* out_idx) {
    BN_GUARD_BEGIN
    return predict_topk_host(m, samples, 0, n_clips, activation, sensitivity, k, out_conf, out_idx);
    BN_GUARD_END((void)0)
}

int bnhip_predict_pcm_topk(bnhip_model* m, const void* pcm, int bits_per_sample, int n_clips, int activation, double sensitivity,
                           int k, float* out_conf, int32_t* out_idx) {
    BN_GUARD_BEGIN
    if (!pcm_depth_known(bits_per_sample))
        return set_err(BNHIP_E_INVALID, "unsupported bit depth: " + std::to_string(bits_per_sample) + " (supported: 16, 24, 32)");
    return predict_topk_host(m, pcm, bits_per_sample, n_clips, activation, sensitivity, k, out_conf, out_idx);
    BN_GUARD_END((void)0)
}

// Heat-map grid of one species (HeatmapInferenceService.ComputeGridWithBinding, internal/classifier/heatmap_service.go:143-420).
// Row g = wi * n_cells + c is [coords[2c], coords[2c+1], 1 + wi * stride]; the rows run in chunks of max_batch, every chunk
// enqueued on the engine's stream behind the previous one: the centres go up once, the [weeks][n_cells] result comes down once.
// Pruned tail (Engine::heatmap_pruned_step): the plan runs without its final dense step and k_heatmap_column computes the one
// column; any other plan runs whole and k_heatmap_gather takes the column from the logits.
int bnhip_range_heatmap(bnhip_model* m, const float* coords, int n_cells, int species, int stride, int total_weeks, float* result) {
    if (!m || !coords || !result) return set_err(BNHIP_E_INVALID, "NULL argument");
    if (n_cells <= 0 || stride <= 0 || total_weeks <= 0) return set_err(BNHIP_E_INVALID, "n_cells, stride and total_weeks must be positive");
    BN_GUARD_BEGIN
    Engine& e = m->eng();
    if (species < 0 || species >= e.n_classes)
        return set_err(BNHIP_E_INVALID, "species index " + std::to_string(species) + " out of range [0, " + std::to_string(e.n_classes) + ")");
    if (e.n_samples != 3)
        return set_err(BNHIP_E_INVALID, "range filter model must take 3 inputs (lat, lon, week), takes " + std::to_string(e.n_samples));
    if (m->engs.size() > 1) return set_err(BNHIP_E_INVALID, "bnhip_range_heatmap: a grid runs on one device; use a single-device handle");
    const int weeks = (total_weeks - 1) / stride + 1;                 // ceil(total_weeks / stride)
    if ((long long)weeks * n_cells > INT_MAX) return set_err(BNHIP_E_INVALID, "weeks * n_cells overflows");
    if (e.device < 0) return set_err(BNHIP_E_INVALID, "plan-only model cannot run");
    if (hipSetDevice(e.device) != hipSuccess) return set_err(BNHIP_E_RUNTIME, "hipSetDevice failed");
    const int total = weeks * n_cells;
    // whatever an earlier asynchronous call still has queued on the engine's streams finishes first (as host_run does)
    e.sync_contexts();
    if (e.stream) hipStreamSynchronize(e.stream);
    const size_t coord_floats = ((size_t)n_cells * 2 + 63) / 64 * 64;
    float* d_coords = nullptr;
    if (hipMalloc((void**)&d_coords, (coord_floats + (size_t)total) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(BNHIP_E_NOMEM, "device allocation failed (heat-map grid)");
    }
    float* d_res = d_coords + coord_floats;
    std::string err;
    hipError_t he = hipMemcpyAsync(d_coords, coords, (size_t)n_cells * 2 * 4, hipMemcpyHostToDevice, e.stream);
    bool ok = he == hipSuccess;
    if (!ok) err = std::string("H2D copy: ") + hipGetErrorString(he);
    const int pruned = e.heatmap_pruned_step();
    for (int g0 = 0; ok && g0 < total; g0 += e.max_batch) {
        const int n = std::min(e.max_batch, total - g0);
        launch_heatmap_rows(d_coords, n_cells, stride, g0, n, e.d_stage_in, e.stream);
        if (pruned >= 0) {
            const Step& s = e.steps[pruned];
            ok = e.run_head(pruned, e.d_stage_in, n, &err);
            const float* a = s.in0 == e.v_input ? e.d_stage_in : e.value_ptr(s.in0);
            if (ok) launch_heatmap_column(a, s.C, s.w0 + (size_t)species * s.C, s.w1 ? s.w1 + species : nullptr, s.act, n, d_res + g0, e.stream);
        } else {
            ok = e.run(e.d_stage_in, n, e.d_stage_logits, nullptr, &err);
            if (ok) launch_heatmap_gather(e.d_stage_logits, e.n_classes, species, n, d_res + g0, e.stream);
        }
    }
    if (ok && (he = hipGetLastError()) != hipSuccess) { ok = false; err = std::string("kernel launch: ") + hipGetErrorString(he); }
    if (ok && (he = hipMemcpyAsync(result, d_res, (size_t)total * 4, hipMemcpyDeviceToHost, e.stream)) != hipSuccess) {
        ok = false; err = std::string("D2H copy: ") + hipGetErrorString(he);
    }
    he = hipStreamSynchronize(e.stream);
    if (ok && he != hipSuccess) { ok = false; err = std::string("heat-map grid: ") + hipGetErrorString(he); }
    hipFree(d_coords);
    if (!ok) { e.mm_dirty = true; return set_err(BNHIP_E_RUNTIME, err); }
    return weeks;
    BN_GUARD_END((void)0)
}

// One tick: who is ready -> rows filled chunk by chunk under the device's work on the previous chunks -> top-k.  With a bank
// (bnhip_windows_predict_events) the top-k rows of every chunk also stay on the device, and the bank's call runs behind the last
// chunk on the model's stream: every refusal of the bank stage that can be known before the windows are taken is answered first.
static int windows_tick(bnhip_windows* w, bnhip_model* m, bnhip_event_bank* bank, int bits_per_sample, int activation, double sensitivity, int k,
                        int* sources, int* n_windows, float* out_conf, int32_t* out_idx, const void** batch, bnhip_event* events, size_t cap,
                        size_t* n_events) {
    bool begun = false;
    BN_GUARD_BEGIN
    Engine& e = m->eng();
    if (e.device < 0) return set_err(BNHIP_E_INVALID, "plan-only model cannot run");
    if ((size_t)e.n_classes * 4 > TOPK_LDS_MAX) return set_err(BNHIP_E_UNSUPPORTED, TOPK_LDS_TEXT);
    const size_t clip_bytes = clip_stride(e, bits_per_sample);
    if (w->a->window_bytes() != clip_bytes)
        return set_err(BNHIP_E_INVALID, "window size mismatch: assembler " + std::to_string(w->a->window_bytes()) + " bytes, model clip " +
                                        std::to_string(clip_bytes) + " bytes");
    bnhip::WindowAssembler& a = *w->a;
    const int kk = std::min(k, e.n_classes);
    float* d_keep_conf = nullptr;                           // the tick's rows on the device, for the bank
    int32_t* d_keep_idx = nullptr;
    std::unique_lock<std::mutex> feeding;
    if (bank) {
        if (m->engs.size() > 1) return set_err(BNHIP_E_INVALID, "bnhip_windows_predict_events: the bank lives on one device; use a single-device handle");
        if (event_bank_device(bank) != e.device) return set_err(BNHIP_E_INVALID, "model and event bank are on different devices");
        if (event_bank_k(bank) != kk)
            return set_err(BNHIP_E_INVALID, "the tick's rows hold " + std::to_string(kk) + " results, the event bank's " + std::to_string(event_bank_k(bank)));
        feeding = std::unique_lock<std::mutex>(event_bank_tick_mutex(bank));
        if (int rc = event_bank_rows(bank, (size_t)a.max_batch(), &d_keep_conf, &d_keep_idx)) return rc;
    }
    const int n = a.collect_begin(a.max_batch(), sources);
    begun = true;
    if (n == 0) { a.collect_end(); return BNHIP_OK; }       // "try again later"
    // every listed source gives up exactly one read, whatever happens to the device call: ranges the pipeline did not get to
    // (an error on the way) are consumed afterwards, as the reference's monitor has consumed its window before ProcessData fails
    std::vector<char> filled((size_t)n, 0);
    uint8_t* rows = w->batch;
    auto fill = [&a, &filled, rows, sources](int first, int cnt) {
        a.collect_rows(rows, sources, first, cnt);
        for (int r = first; r < first + cnt; r++) filled[(size_t)r] = 1;
    };
    HostJob call;
    call.src = rows; call.pcm_bits = bits_per_sample; call.topk = k; call.activation = activation; call.sensitivity = sensitivity;
    call.out_conf = out_conf; call.out_idx = out_idx;
    call.d_keep_conf = d_keep_conf; call.d_keep_idx = d_keep_idx;
    int rc = shard_run(m, n, [=](Engine& en, int off, int cnt, std::string& err) {
        HostJob j = shard_job(en, call, off, cnt);
        j.prepare = [=](int first, int c) { fill(off + first, c); };
        return host_run(en, j, err);
    });
    for (int r = 0; r < n;) {
        if (filled[(size_t)r]) { r++; continue; }
        int q = r;
        while (q < n && !filled[(size_t)q]) q++;
        fill(r, q - r);
        r = q;
    }
    a.collect_end();
    begun = false;
    *n_windows = n;
    if (rc == BNHIP_OK && bank) rc = bnhip_event_bank_process_device(bank, sources, n, d_keep_conf, d_keep_idx, events, cap, n_events, e.stream);
    return rc;
    BN_GUARD_END(if (begun) w->a->collect_end())
}

int bnhip_windows_predict_topk(bnhip_windows* w, bnhip_model* m, int bits_per_sample, int activation, double sensitivity, int k,
                               int* sources, int* n_windows, float* out_conf, int32_t* out_idx, const void** batch) {
    if (!w || !m || !sources || !n_windows || !out_conf || !out_idx) return set_err(BNHIP_E_INVALID, "NULL argument");
    *n_windows = 0;
    if (batch) *batch = w->batch;
    if (!pcm_depth_known(bits_per_sample))
        return set_err(BNHIP_E_INVALID, "unsupported bit depth: " + std::to_string(bits_per_sample) + " (supported: 16, 24, 32)");
    if (k <= 0) return set_err(BNHIP_E_INVALID, "n_clips and k must be positive");
    if (activation < 0 || activation > 2) return set_err(BNHIP_E_INVALID, "unknown activation");
    return windows_tick(w, m, nullptr, bits_per_sample, activation, sensitivity, k, sources, n_windows, out_conf, out_idx, batch, nullptr, 0, nullptr);
}

int bnhip_windows_predict_events(bnhip_windows* w, bnhip_model* m, bnhip_event_bank* bank, int bits_per_sample, int activation, double sensitivity,
                                 int k, int* sources, int* n_windows, float* out_conf, int32_t* out_idx, const void** batch, bnhip_event* events,
                                 size_t cap, size_t* n_events) {
    if (!w || !m || !bank || !sources || !n_windows || !out_conf || !out_idx || !n_events || (cap && !events))
        return set_err(BNHIP_E_INVALID, "NULL argument");
    *n_windows = 0;
    *n_events = 0;
    if (batch) *batch = w->batch;
    if (!pcm_depth_known(bits_per_sample))
        return set_err(BNHIP_E_INVALID, "unsupported bit depth: " + std::to_string(bits_per_sample) + " (supported: 16, 24, 32)");
    if (k <= 0) return set_err(BNHIP_E_INVALID, "n_clips and k must be positive");
    if (activation < 0 || activation > 2) return set_err(BNHIP_E_INVALID, "unknown activation");
    return windows_tick(w, m, bank, bits_per_sample, activation, sensitivity, k, sources, n_windows, out_conf, out_idx, batch, events, cap, n_events);
}

int bnhip_debug_fetch(bnhip_model* m, int tensor_index, int n_clips, float* out, size_t cap_floats) {
    if (!m || !out || m->eng().device < 0) return set_err(BNHIP_E_INVALID, "NULL argument or plan-only model");
    BN_GUARD_BEGIN
    Engine& e = m->eng();
    // tensor_index <= -2 names a plan value directly (value id = -tensor_index - 2: the "out_v" / "out2_v" of a describe()
    // step, which also covers internal scratch such as the squeeze-excite partial sums)
    int vid = -1;
    if (tensor_index <= -2) {
        vid = -tensor_index - 2;
        if (vid >= (int)e.vals.size()) return set_err(BNHIP_E_INVALID, "value id out of range");
    } else {
        auto it = e.tensor_value.find(tensor_index);
        if (it == e.tensor_value.end()) return set_err(BNHIP_E_INVALID, "tensor is not materialised by the plan (fused away)");
        vid = it->second;
    }
    const Value& v = e.vals[vid];
    if (v.external) return set_err(BNHIP_E_INVALID, "tensor is bound externally (graph input/logits)");
    size_t n = v.elems * (size_t)n_clips;
    if (n > cap_floats || n_clips > e.max_batch) return set_err(BNHIP_E_INVALID, "buffer too small");
    hipSetDevice(e.device);
    hipStreamSynchronize(e.stream);
    if (hipMemcpy(out, e.value_ptr(vid), n * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(BNHIP_E_RUNTIME, "debug fetch copy failed");
    return (int)v.elems;
    BN_GUARD_END((void)0)
}

}  // extern "C"
