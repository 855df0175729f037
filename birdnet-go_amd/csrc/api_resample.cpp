// C ABI of the resampler: the one-shot entries, the single-stream streaming handle and the multi-source bank.
#include <hip/hip_runtime.h>

#include <numeric>

#include "api_oneshot.h"
#include "kernels.h"
#include "resample.h"
#include "stream_bank.h"

using namespace bnhip;

// Streaming resampler state (Resampler, internal/audiocore/resample/resample.go:44-52): the polyphase filter's input
// history lives on the device between calls so that any chunking of a stream produces the samples of one call over the
// whole stream, bit for bit.
struct bnhip_resampler {
    int device = 0;
    ResamplePlan p;
    float* d_table = nullptr;
    float* d_work = nullptr;      // [hist | new chunk] as float32
    size_t work_cap = 0;          // floats
    void* d_in = nullptr;  size_t in_cap = 0;     // raw input staging (bytes)
    void* d_out = nullptr; size_t out_cap = 0;    // output staging (bytes)
    long long n_total = 0;        // input samples consumed so far
    long long i_next = 0;         // next output index
    long long n_base = 0;         // stream index of d_work[0]
    int n_hist = 0;               // valid history samples at the front of d_work
    hipStream_t stream = nullptr;
};

extern "C" {

// ------------------------------------------------------------------------------------------------ resampler
int bnhip_resample_length(int n_in, int rate_in, int rate_out) {
    if (n_in <= 0 || rate_in <= 0 || rate_out <= 0) return 0;
    return (int)resample_plan(rate_in, rate_out, nullptr).end(n_in);
}

static int resample_impl(int device, const void* in, bool pcm16, int n_clips, int n_in, int rate_in, int rate_out, void* out,
                         int n_out_cap, int* n_out) {
    if (!in || !out || n_clips <= 0 || n_in <= 0 || rate_in <= 0 || rate_out <= 0)
        return set_err(BNHIP_E_INVALID, "bad resample arguments");
    const int no = bnhip_resample_length(n_in, rate_in, rate_out);
    if (n_out) *n_out = no;
    if (no > n_out_cap) return set_err(BNHIP_E_INVALID, "destination buffer too small");     // resample.go:137-144
    const size_t esz = pcm16 ? 2 : 4;
    if (rate_in == rate_out) {                                                              // NewResampler returns nil: passthrough
        memcpy(out, in, (size_t)n_clips * n_in * esz);
        return BNHIP_OK;
    }
    int rc = use_device(device);
    if (rc) return rc;
    std::vector<float> table;
    const ResamplePlan p = resample_plan(rate_in, rate_out, &table);
    DevBlocks b;
    void* d_in = b.get((size_t)n_clips * n_in * esz);
    void* d_out = b.get((size_t)n_clips * no * esz);
    float* d_tab = (float*)b.get(table.size() * 4);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_in, in, (size_t)n_clips * n_in * esz, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) b.he = hipMemcpy(d_tab, table.data(), table.size() * 4, hipMemcpyHostToDevice);
    if (b.he == hipSuccess) {
        if (launch_resample(d_in, d_out, d_tab, pcm16, pcm16, n_clips, n_in, no, p.L, p.M, p.T, p.half, 0, 0, nullptr))
            return set_err(BNHIP_E_UNSUPPORTED, "resample ratio needs a phase table larger than LDS");
        b.he = hipMemcpy(out, d_out, (size_t)n_clips * no * esz, hipMemcpyDeviceToHost);
    }
    return b.he == hipSuccess ? BNHIP_OK : hip_fail("resample", b);
}

int bnhip_resample_f32(int device, const float* in, int n_clips, int n_in, int rate_in, int rate_out, float* out, int n_out_cap,
                       int* n_out) {
    BN_GUARD_BEGIN
    return resample_impl(device, in, false, n_clips, n_in, rate_in, rate_out, out, n_out_cap, n_out);
    BN_GUARD_END((void)0)
}

int bnhip_resample_pcm16(int device, const int16_t* in, int n_clips, int n_in, int rate_in, int rate_out, int16_t* out,
                         int n_out_cap, int* n_out) {
    BN_GUARD_BEGIN
    return resample_impl(device, in, true, n_clips, n_in, rate_in, rate_out, out, n_out_cap, n_out);
    BN_GUARD_END((void)0)
}

// ---- streaming form
static void resampler_free(bnhip_resampler* r) {
    if (!r) return;
    hipSetDevice(r->device);
    if (r->stream) { hipStreamSynchronize(r->stream); hipStreamDestroy(r->stream); }
    for (void* p : {(void*)r->d_table, (void*)r->d_work, r->d_in, r->d_out}) if (p) hipFree(p);
    delete r;
}

int bnhip_resampler_create(int device, int rate_in, int rate_out, bnhip_resampler** out) {
    if (!out) return set_err(BNHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (rate_in <= 0 || rate_out <= 0) return set_err(BNHIP_E_INVALID, "sample rates must be positive");
    if (rate_in == rate_out) return BNHIP_OK;            // NewResampler returns nil, nil: no resampling required (resample.go:58-60)
    bnhip_resampler* r = nullptr;
    BN_GUARD_BEGIN
    int rc = use_device(device);
    if (rc) return rc;
    std::vector<float> table;
    const ResamplePlan p = resample_plan(rate_in, rate_out, &table);
    if (!p.fits_lds()) return set_err(BNHIP_E_UNSUPPORTED, "resample ratio needs a phase table larger than LDS");
    r = new bnhip_resampler();
    r->device = device;
    r->p = p;
    hipError_t he = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipMalloc((void**)&r->d_table, table.size() * 4);
    if (he == hipSuccess) he = hipMemcpy(r->d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice);
    if (he != hipSuccess) { resampler_free(r); r = nullptr; return set_err(BNHIP_E_RUNTIME, std::string("resampler create: ") + hipGetErrorString(he)); }
    *out = r;
    return BNHIP_OK;
    BN_GUARD_END(resampler_free(r))
}

int bnhip_resampler_estimate(const bnhip_resampler* r, int n_in) {
    if (!r || n_in <= 0) return 0;
    return (int)r->p.estimate(n_in);
}

// a device staging buffer of at least `need` bytes, grown with room to spare; false: the allocation failed and the old one stays
static bool staging_grow(void** d, size_t* cap, size_t need) {
    if (need <= *cap) return true;
    const size_t c = std::max<size_t>(need * 2, 8192);
    void* nd = nullptr;
    if (hipMalloc(&nd, c) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (*d) hipFree(*d);
    *d = nd; *cap = c;
    return true;
}

// flush: 0 = emit what the inputs so far determine; 1 = end of stream (future inputs are zeros), then reset
static int resampler_run(bnhip_resampler* r, const void* in, bool pcm16, int n_in, void* out, int out_cap, int* n_out, int flush) {
    if (!r) return set_err(BNHIP_E_INVALID, "resampler is NULL");
    if (n_out) *n_out = 0;
    if (n_in < 0 || (n_in > 0 && !in) || !out) return set_err(BNHIP_E_INVALID, "bad resampler arguments");
    if (n_in == 0 && !flush) return BNHIP_OK;            // empty input: nothing written (resample.go:100-102)
    const long long n_after = r->n_total + n_in;
    const long long i_end = flush ? r->p.end(n_after) : r->p.ready(n_after);
    const long long cnt = i_end - r->i_next;
    // a too-small destination fails before the state advances (resample.go:137-144)
    if (cnt > out_cap || (!flush && bnhip_resampler_estimate(r, n_in) > out_cap))
        return set_err(BNHIP_E_INVALID, "destination buffer too small");
    hipSetDevice(r->device);
    const size_t esz = pcm16 ? 2 : 4;
    const size_t need = (size_t)r->n_hist + (size_t)n_in;
    const int n_work = r->n_hist + n_in;
    // what the next call still needs: the inputs from n0(i_end) - (T-1) on.  Computed up front so that every allocation
    // (including the staging the history compaction moves through) happens BEFORE any work is queued: a failure below
    // leaves n_total / i_next / n_hist / n_base exactly as they were ("fails before the state advances", resample.go:137-144).
    const long long keep_from = r->p.keep_from(i_end, r->n_base, n_after);
    const int drop = flush ? 0 : (int)(keep_from - r->n_base), keep = flush ? 0 : n_work - drop;
    if (need > r->work_cap) {
        size_t cap = std::max<size_t>(need * 2, 4096);
        float* nw = nullptr;
        if (hipMalloc((void**)&nw, cap * 4) != hipSuccess) { (void)hipGetLastError(); return set_err(BNHIP_E_NOMEM, "device allocation failed (resampler work buffer)"); }
        hipError_t hc = hipSuccess;
        if (r->n_hist) hc = hipMemcpyAsync(nw, r->d_work, (size_t)r->n_hist * 4, hipMemcpyDeviceToDevice, r->stream);
        if (hc == hipSuccess) hc = hipStreamSynchronize(r->stream);
        if (hc != hipSuccess) { hipFree(nw); return set_err(BNHIP_E_RUNTIME, std::string("resampler: ") + hipGetErrorString(hc)); }
        if (r->d_work) hipFree(r->d_work);
        r->d_work = nw; r->work_cap = cap;
    }
    // input staging; doubles as the bounce buffer of the (overlapping) history move, so it is sized for both
    const size_t in_need = std::max((size_t)n_in * esz, drop > 0 && keep > 0 ? (size_t)keep * 4 : (size_t)0);
    if (!staging_grow(&r->d_in, &r->in_cap, in_need)) return set_err(BNHIP_E_NOMEM, "device allocation failed (resampler input)");
    if (!staging_grow(&r->d_out, &r->out_cap, cnt > 0 ? (size_t)cnt * esz : 0)) return set_err(BNHIP_E_NOMEM, "device allocation failed (resampler output)");
    hipError_t he = hipSuccess;
    if (n_in > 0) {
        if (pcm16) {
            he = hipMemcpyAsync(r->d_in, in, (size_t)n_in * 2, hipMemcpyHostToDevice, r->stream);
            if (he == hipSuccess) launch_pcm_to_f32(r->d_in, 16, r->d_work + r->n_hist, (size_t)n_in, r->stream);   // float32(int16)/32768, resample.go:120-124
        } else {
            he = hipMemcpyAsync(r->d_work + r->n_hist, in, (size_t)n_in * 4, hipMemcpyHostToDevice, r->stream);
        }
    }
    if (he == hipSuccess && cnt > 0) {
        int lrc = launch_resample(r->d_work, r->d_out, r->d_table, 0, pcm16 ? 1 : 0, 1, n_work, (int)cnt, r->p.L, r->p.M, r->p.T, r->p.half,
                                  r->i_next, r->n_base, r->stream);
        if (lrc) { hipStreamSynchronize(r->stream); return set_err(BNHIP_E_UNSUPPORTED, "resample ratio needs a phase table larger than LDS"); }
        he = hipMemcpyAsync(out, r->d_out, (size_t)cnt * esz, hipMemcpyDeviceToHost, r->stream);
    }
    // history compaction (an overlapping move inside one buffer, bounced through the now idle input staging), queued behind
    // the resample kernel that still reads the old layout
    if (he == hipSuccess && drop > 0 && keep > 0) {
        he = hipMemcpyAsync(r->d_in, r->d_work + drop, (size_t)keep * 4, hipMemcpyDeviceToDevice, r->stream);
        if (he == hipSuccess) he = hipMemcpyAsync(r->d_work, r->d_in, (size_t)keep * 4, hipMemcpyDeviceToDevice, r->stream);
    }
    if (he == hipSuccess) he = hipStreamSynchronize(r->stream);
    if (he != hipSuccess) { (void)hipGetLastError(); return set_err(BNHIP_E_RUNTIME, std::string("resampler: ") + hipGetErrorString(he)); }
    // ---- commit: everything above succeeded
    if (n_out) *n_out = (int)cnt;
    if (flush) {                                          // back to the initial state: the next call starts a new stream
        r->n_total = 0; r->i_next = 0; r->n_base = 0; r->n_hist = 0;
        return BNHIP_OK;
    }
    r->n_total = n_after; r->i_next = i_end;
    r->n_hist = keep > 0 ? keep : 0;
    r->n_base = keep_from;
    return BNHIP_OK;
}

int bnhip_resampler_process_pcm16(bnhip_resampler* r, const int16_t* in, int n_in, int16_t* out, int out_cap, int* n_out) {
    BN_GUARD_BEGIN
    return resampler_run(r, in, true, n_in, out, out_cap, n_out, 0);
    BN_GUARD_END((void)0)
}
int bnhip_resampler_process_f32(bnhip_resampler* r, const float* in, int n_in, float* out, int out_cap, int* n_out) {
    BN_GUARD_BEGIN
    return resampler_run(r, in, false, n_in, out, out_cap, n_out, 0);
    BN_GUARD_END((void)0)
}
int bnhip_resampler_flush_pcm16(bnhip_resampler* r, int16_t* out, int out_cap, int* n_out) {
    BN_GUARD_BEGIN
    return resampler_run(r, nullptr, true, 0, out, out_cap, n_out, 1);
    BN_GUARD_END((void)0)
}
int bnhip_resampler_flush_f32(bnhip_resampler* r, float* out, int out_cap, int* n_out) {
    BN_GUARD_BEGIN
    return resampler_run(r, nullptr, false, 0, out, out_cap, n_out, 1);
    BN_GUARD_END((void)0)
}
void bnhip_resampler_destroy(bnhip_resampler* r) {
    try { resampler_free(r); } catch (...) {}
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ resampler bank
// The rate fan-out of BufferConsumer.Write (internal/analysis/buffer_consumer.go:105-210: one stateful Resampler per
// (source, non-native rate)) for every source of one (rate_in, rate_out) pair at once, one k_resample_bank launch per call.
// Each stream's filter history is a fixed pair of device slabs of H = T - 1 floats (keep_from = n0(i_end) - (T - 1) with
// n0(i_end) >= n_total bounds it): the launch reads one slab and writes the new tail into the other.
struct ResamplerStream {
    long long n_total = 0, i_next = 0, n_base = 0;
    int n_hist = 0;
};

struct bnhip_resampler_bank : StreamBank<ResamplerStream> {
    static constexpr const char* what = "resampler bank";
    ResamplePlan p;
    int H = 1;
    float* d_table = nullptr;
    float* d_hist = nullptr;            // [max_streams][2][H]
    ~bnhip_resampler_bank() { for (void* q : {(void*)d_table, (void*)d_hist}) if (q) hipFree(q); }

    template <class Deliver>
    int run(int n_frames, const int* streams, const int16_t* const* frames, const int* n_in, bool flush,
            long long out_cap, Deliver deliver) {
        std::vector<ResampleBankDesc> desc;
        int n_blocks = 0;
        auto plan = [&](std::vector<BankGroup>& groups, const std::vector<int>& frame_group, std::vector<long long>& cnt) -> int {
            // per-frame split: what ready() gives on the running n_total, frame after frame
            std::vector<long long> n_after(groups.size()), i_end(groups.size());
            for (size_t gi = 0; gi < groups.size(); gi++) {
                const auto& S = st[groups[gi].stream];
                n_after[gi] = S.n_total;
                i_end[gi] = S.i_next;
                groups[gi].run = flush || groups[gi].n_in > 0;      // streams with nothing to do (every frame empty) stay out of the launch
            }
            long long need = 0;
            for (int f = 0; f < n_frames; f++) {
                const int gi = frame_group[f];
                const long long e = flush ? p.end(n_after[gi]) : p.ready(n_after[gi] += n_in[f]);
                cnt[f] = e - i_end[gi];
                i_end[gi] = e;
                if (!flush) need += p.estimate(n_in[f]);
            }
            if (need > out_cap) return set_err(BNHIP_E_INVALID, "destination buffer too small");      // resample.go:137-144
            return BNHIP_OK;
        };
        auto describe = [&](const std::vector<BankGroup>& groups, long long in_total, long long out_total, BankBlob* hdr) -> int {
            long long blocks = 0;
            for (const BankGroup& g : groups) blocks += (g.n_out + 255) / 256 + 1;
            if (in_total > INT32_MAX / 2 || out_total > INT32_MAX / 2 || blocks > INT32_MAX / 2)
                return set_err(BNHIP_E_INVALID, "resampler bank call too large");
            desc.reserve(groups.size());
            for (const BankGroup& g : groups) {
                if (!g.run) continue;
                const auto& S = st[g.stream];
                ResampleBankDesc d{};
                d.n_base = S.n_base; d.i_next = S.i_next;
                if (!flush) {
                    d.keep_from = p.keep_from(S.i_next + g.n_out, S.n_base, S.n_total + g.n_in);
                    d.keep = (int)(S.n_total + g.n_in - d.keep_from);
                    if (d.keep > H) return set_err(BNHIP_E_RUNTIME, "internal error: resampler bank history exceeds its slab");
                }
                d.in_off = g.in_off; d.n_in = (int)g.n_in; d.n_hist = S.n_hist;
                d.hist_rd = (g.stream * 2 + S.parity) * H; d.hist_wr = (g.stream * 2 + (S.parity ^ 1)) * H;
                d.cnt = (int)g.n_out; d.out_off = g.out_off; d.block0 = n_blocks;
                n_blocks += (d.cnt + 255) / 256 + 1;
                desc.push_back(d);
            }
            hdr[0] = {desc.data(), desc.size() * sizeof(ResampleBankDesc)};
            return BNHIP_OK;
        };
        auto launch = [&](const uint8_t* d_hdr, const int16_t* d_pcm, int16_t* d_out) -> int {
            if (launch_resample_bank(reinterpret_cast<const ResampleBankDesc*>(d_hdr), (int)desc.size(), n_blocks, d_pcm, d_hist, d_out,
                                     d_table, p.L, p.M, p.T, p.half, stream))
                return set_err(BNHIP_E_UNSUPPORTED, "resample ratio needs a phase table larger than LDS");
            return BNHIP_OK;
        };
        auto commit = [&](const BankGroup& g, size_t k) {
            auto& S = st[g.stream];
            if (flush) { S.n_total = 0; S.i_next = 0; S.n_base = 0; S.n_hist = 0; return; }     // a new stream starts
            S.n_total += g.n_in; S.i_next += g.n_out;
            S.n_hist = desc[k].keep; S.n_base = desc[k].keep_from; S.parity ^= 1;
        };
        return bank_call(this, n_frames, streams, frames, n_in, flush, out_cap, plan, describe, launch, commit, deliver);
    }
};

extern "C" {

int bnhip_resampler_bank_create(int device, int rate_in, int rate_out, int max_streams, bnhip_resampler_bank** out) {
    if (!out) return set_err(BNHIP_E_INVALID, "out is NULL");
    *out = nullptr;
    if (rate_in <= 0 || rate_out <= 0) return set_err(BNHIP_E_INVALID, "sample rates must be positive");
    if (max_streams < 1 || max_streams > (1 << 20)) return set_err(BNHIP_E_INVALID, "max_streams must be in [1, 1048576]");
    if (rate_in == rate_out) return BNHIP_OK;            // NewResampler returns nil, nil: no resampling required (resample.go:58-60)
    BN_GUARD_BEGIN
    int rc = use_device(device);
    if (rc) return rc;
    std::vector<float> table;
    const ResamplePlan p = resample_plan(rate_in, rate_out, &table);
    if (!p.fits_lds()) return set_err(BNHIP_E_UNSUPPORTED, "resample ratio needs a phase table larger than LDS");
    return bank_create(device, max_streams, out, [&](bnhip_resampler_bank& b) {
        b.p = p;
        b.H = std::max(p.T - 1, 1);
        hipError_t he = hipMalloc((void**)&b.d_table, table.size() * 4);
        if (he == hipSuccess) he = hipMalloc((void**)&b.d_hist, (size_t)max_streams * 2 * b.H * 4);
        if (he == hipSuccess) he = hipMemcpy(b.d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice);
        return he;
    });
    BN_GUARD_END((void)0)
}

int bnhip_resampler_bank_add_stream(bnhip_resampler_bank* b, int* out_stream) { return bank_add_stream(b, out_stream); }
int bnhip_resampler_bank_remove_stream(bnhip_resampler_bank* b, int stream) { return bank_remove_stream(b, stream); }

int bnhip_resampler_bank_estimate(const bnhip_resampler_bank* b, int n_in) {
    if (!b || n_in <= 0) return 0;
    return (int)b->p.estimate(n_in);
}

int bnhip_resampler_bank_process_pcm16(bnhip_resampler_bank* b, int n_frames, const int* streams, const int16_t* const* frames,
                                       const int* n_in, int16_t* out, size_t out_cap, int* out_count) {
    return bank_to_buffer(b, n_frames, streams, frames, n_in, false, out, out_cap, out_count);
}

int bnhip_resampler_bank_flush_pcm16(bnhip_resampler_bank* b, int n, const int* streams, int16_t* out, size_t out_cap, int* out_count) {
    return bank_to_buffer(b, n, streams, nullptr, nullptr, true, out, out_cap, out_count);
}

int bnhip_windows_write_resampled(bnhip_windows* w, bnhip_resampler_bank* b, int n_frames, const int* streams, const int* sources,
                                  const int16_t* const* frames, const int* n_in) {
    return bank_to_rings(w, b, n_frames, streams, sources, frames, n_in);
}

void bnhip_resampler_bank_destroy(bnhip_resampler_bank* b) {
    try { bank_free(b); } catch (...) {}
}

}  // extern "C"
