// What the resampler, equalizer and sound level banks share.  Calls on a bank are serialised on its mutex and each one is one
// transaction on the bank's HIP stream: one H2D copy (the bank's headers, then the packed PCM16 of the streams that run), one
// launch, one D2H copy of the packed outputs and one synchronise.  A bank's outputs are elements of type Out (PCM16 samples for
// the resampler and equalizer banks, block sums for the sound level bank).  Each stream's device state is a pair of slabs: a
// launch reads slab `parity` and writes the other, and the host flips the parity in the commit, which runs only once everything
// succeeded - so a failed call changes no stream.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "api_common.h"
#include "windows.h"

namespace bnhip {

template <class State, class Out = int16_t>
struct StreamBank {
    using out_t = Out;
    struct Stream : State {
        bool live = false;
        int parity = 0;                 // slab read by the next call
    };
    std::mutex mu;                      // calls on one bank are serialised
    int device = 0;
    std::vector<Stream> st;
    hipStream_t stream = nullptr;
    uint8_t* h_stage = nullptr; void* d_stage = nullptr; size_t stage_cap = 0;   // headers | packed PCM16 (bytes)
    Out* h_out = nullptr; void* d_out = nullptr; size_t out_cap = 0;             // packed outputs (bytes)
    ~StreamBank() {                     // (bank_free has drained the stream)
        if (stream) hipStreamDestroy(stream);
        for (void* p : {d_stage, d_out}) if (p) hipFree(p);
        for (void* p : {(void*)h_stage, (void*)h_out}) if (p) hipHostFree(p);
    }
};

template <class B>
void bank_free(B* b) {
    if (!b) return;
    hipSetDevice(b->device);
    if (b->stream) hipStreamSynchronize(b->stream);
    delete b;                           // the destructors free the bank's buffers and its stream
    (void)hipGetLastError();
}

// a page-locked host buffer and its device twin of at least `need` bytes; the old pair is freed only once the new one exists
inline bool bank_grow(void** h, void** d, size_t* cap, size_t need) {
    if (need <= *cap) return true;
    const size_t c = std::max<size_t>(need + need / 2, 1 << 16);
    void *nh = nullptr, *nd = nullptr;
    if (hipHostMalloc(&nh, c, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipMalloc(&nd, c) != hipSuccess) { (void)hipGetLastError(); hipHostFree(nh); return false; }
    if (*h) hipHostFree(*h);
    if (*d) hipFree(*d);
    *h = nh; *d = nd; *cap = c;
    return true;
}

template <class B>
int bank_stream_check(const B* b, int s) {
    if (s >= 0 && (size_t)s < b->st.size() && b->st[s].live) return BNHIP_OK;
    return set_err(BNHIP_E_INVALID, std::string("no such ") + B::what + " stream: " + std::to_string(s));
}

// The rest of both creates, on the current device: the stream slots, the HIP stream, then alloc(bank) for the bank's own device
// buffers.  A failure frees the bank; *out is set only on success.
template <class B, class Alloc>
int bank_create(int device, int max_streams, B** out, Alloc alloc) {
    B* b = nullptr;
    BN_GUARD_BEGIN
    b = new B();
    b->device = device;
    b->st.resize(max_streams);
    hipError_t he = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = alloc(*b);
    if (he != hipSuccess) {
        (void)hipGetLastError();
        bank_free(b); b = nullptr;
        return set_err(he == hipErrorOutOfMemory ? BNHIP_E_NOMEM : BNHIP_E_RUNTIME, std::string(B::what) + " create: " + hipGetErrorString(he));
    }
    *out = b;
    return BNHIP_OK;
    BN_GUARD_END(bank_free(b))
}

template <class B>
int bank_add_stream(B* b, int* out_stream) {
    if (!b || !out_stream) return set_err(BNHIP_E_INVALID, "NULL argument");
    *out_stream = -1;
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    for (size_t s = 0; s < b->st.size(); s++) {
        if (b->st[s].live) continue;
        b->st[s] = typename B::Stream();               // fresh state: a reused slot starts a new stream
        b->st[s].live = true;
        *out_stream = (int)s;
        return BNHIP_OK;
    }
    return set_err(BNHIP_E_INVALID, std::string(B::what) + " is full (max_streams)");
    BN_GUARD_END((void)0)
}

template <class B>
int bank_remove_stream(B* b, int stream) {
    if (!b) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    if (int rc = bank_stream_check(b, stream)) return rc;
    b->st[stream].live = false;
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

// One stream's frames of a call.  The bank's plan decides whether the group runs on the device and whether its frames are
// handed back as they are; a group that runs has its inputs at in_off of the packed PCM16 and its outputs at out_off (in
// output elements) of the packed output.
struct BankGroup {
    int stream;
    long long n_in = 0, n_out = 0;      // samples of its frames, of their outputs
    bool run = false, pass = false;
    int in_off = 0, out_off = 0;
};

struct BankBlob { const void* p = nullptr; size_t bytes = 0; };

// One call on any bank: frames f = 0..n_frames-1 of streams[f] (a stream may appear several times; its frames are consumed
// in call order), or with flush the end of each listed stream (at most once each; no frames).  Checks everything, stages
// everything, runs, synchronises, commits, then hands frame f's outputs (in call order) to deliver(f, outputs, count).  Until
// the commit nothing of any stream changes.  Output counts and out_cap are in elements of the bank's out_t; the output buffer
// is sized in bytes.  The bank supplies
//   plan(groups, frame_group, cnt)          which groups run or pass, cnt[f] = frame f's output count (preset to its input
//                                           count), and its own checks; -> BNHIP_OK or an error
//   describe(groups, in_total, out_total, hdr)   with the offsets placed: its descriptors etc., staged as hdr[0] | hdr[1]
//                                           in front of the packed PCM16; -> BNHIP_OK or an error
//   launch(d_hdr, d_pcm, d_out)             d_out: out_t*; -> BNHIP_OK or an error (nothing was launched)
//   commit(group, k)                        the new state of the k-th group that ran
template <class B, class Plan, class Describe, class Launch, class Commit, class Deliver>
int bank_call(B* b, int n_frames, const int* streams, const int16_t* const* frames, const int* n_in, bool flush, long long out_cap,
              Plan plan, Describe describe, Launch launch, Commit commit, Deliver deliver) {
    using Out = typename B::out_t;
    constexpr size_t elem = sizeof(Out);
    if (n_frames < 0 || (n_frames > 0 && (!streams || (!flush && !n_in)))) return set_err(BNHIP_E_INVALID, std::string("bad ") + B::what + " arguments");
    std::vector<BankGroup> groups;
    std::vector<int> group_of(b->st.size(), -1), frame_group(n_frames);
    std::vector<long long> cnt(n_frames);
    for (int f = 0; f < n_frames; f++) {
        const int s = streams[f];
        if (int rc = bank_stream_check(b, s)) return rc;
        const long long n = flush ? 0 : n_in[f];
        if (n < 0) return set_err(BNHIP_E_INVALID, "negative frame length");
        if (n > 0 && (!frames || !frames[f])) return set_err(BNHIP_E_INVALID, "frame pointer is NULL");
        if (group_of[s] < 0) {
            group_of[s] = (int)groups.size();
            groups.push_back(BankGroup{s});
        } else if (flush) {
            return set_err(BNHIP_E_INVALID, "stream listed twice in one flush");
        }
        frame_group[f] = group_of[s];
        groups[group_of[s]].n_in += n;
        cnt[f] = n;
    }
    if (int rc = plan(groups, frame_group, cnt)) return rc;
    long long total = 0;
    for (int f = 0; f < n_frames; f++) {
        groups[frame_group[f]].n_out += cnt[f];
        total += cnt[f];
    }
    if (total > out_cap) return set_err(BNHIP_E_INVALID, "destination buffer too small");      // resample.go:137-144, convert/pcm.go:142-145
    long long in_total = 0, out_total = 0;
    int n_run = 0;
    for (BankGroup& g : groups) {
        if (!g.run) continue;
        g.in_off = (int)in_total;
        g.out_off = (int)out_total;
        in_total += g.n_in;
        out_total += g.n_out;
        n_run++;
    }
    BankBlob hdr[2];
    if (int rc = describe(groups, in_total, out_total, hdr)) return rc;
    if (n_run > 0) {
        hipSetDevice(b->device);
        const size_t hdr_bytes = hdr[0].bytes + hdr[1].bytes, stage_bytes = hdr_bytes + (size_t)in_total * 2;
        if (!bank_grow((void**)&b->h_stage, &b->d_stage, &b->stage_cap, stage_bytes))
            return set_err(BNHIP_E_NOMEM, std::string("allocation failed (") + B::what + " staging)");
        if (!bank_grow((void**)&b->h_out, &b->d_out, &b->out_cap, std::max<size_t>((size_t)out_total * elem, elem)))
            return set_err(BNHIP_E_NOMEM, std::string("allocation failed (") + B::what + " output)");
        memcpy(b->h_stage, hdr[0].p, hdr[0].bytes);
        if (hdr[1].bytes) memcpy(b->h_stage + hdr[0].bytes, hdr[1].p, hdr[1].bytes);
        int16_t* pk = reinterpret_cast<int16_t*>(b->h_stage + hdr_bytes);
        std::vector<long long> fill(groups.size(), 0);
        for (int f = 0; f < n_frames && !flush; f++) {
            const int gi = frame_group[f];
            if (n_in[f] <= 0 || !groups[gi].run) continue;
            memcpy(pk + groups[gi].in_off + fill[gi], frames[f], (size_t)n_in[f] * 2);
            fill[gi] += n_in[f];
        }
        const uint8_t* ds = static_cast<const uint8_t*>(b->d_stage);
        hipError_t he = hipMemcpyAsync(b->d_stage, b->h_stage, stage_bytes, hipMemcpyHostToDevice, b->stream);
        if (he == hipSuccess) {
            if (int rc = launch(ds, reinterpret_cast<const int16_t*>(ds + hdr_bytes), static_cast<Out*>(b->d_out))) {
                hipStreamSynchronize(b->stream);
                return rc;
            }
            he = hipGetLastError();
        }
        if (he == hipSuccess && out_total > 0)
            he = hipMemcpyAsync(b->h_out, b->d_out, (size_t)out_total * elem, hipMemcpyDeviceToHost, b->stream);
        const hipError_t hs = hipStreamSynchronize(b->stream);
        if (he == hipSuccess) he = hs;
        if (he != hipSuccess) { (void)hipGetLastError(); return set_err(BNHIP_E_RUNTIME, std::string(B::what) + ": " + hipGetErrorString(he)); }
    }
    // ---- commit: everything above succeeded
    for (size_t gi = 0, k = 0; gi < groups.size(); gi++)
        if (groups[gi].run) commit(groups[gi], k++);
    std::vector<long long> taken(groups.size(), 0);
    for (int f = 0; f < n_frames; f++) {
        const int gi = frame_group[f];
        const BankGroup& g = groups[gi];
        // (only the PCM16 banks pass frames through: there Out is int16_t)
        deliver(f, g.pass ? reinterpret_cast<const Out*>(frames ? frames[f] : nullptr) : b->h_out + g.out_off + taken[gi], (int)cnt[f]);
        taken[gi] += cnt[f];
    }
    return BNHIP_OK;
}

// The *_process_pcm16 / *_flush_pcm16 entries of a PCM16 bank (B::run: the bank's bank_call with its plan, describe, launch and
// commit): frame f's outputs packed into out in call order, their count in out_count[f]
template <class B>
int bank_to_buffer(B* b, int n_frames, const int* streams, const int16_t* const* frames, const int* n_in, bool flush, int16_t* out,
                   size_t out_cap, int* out_count) {
    if (!b || (n_frames > 0 && (!out || !out_count))) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(b->mu);
    long long pos = 0;
    return b->run(n_frames, streams, frames, n_in, flush, (long long)std::min<size_t>(out_cap, INT64_MAX),
                  [&](int f, const int16_t* p, int n) {
                      if (n > 0) memcpy(out + pos, p, (size_t)n * 2);
                      out_count[f] = n;
                      pos += n;
                  });
    BN_GUARD_END((void)0)
}

// The bnhip_windows_write_* entries: one ring write per frame, as BufferConsumer.Write's AnalysisBuffer.Write per frame (an
// empty result is a write too).  Every source is checked before the bank is locked; a source removed since then loses its frame
// as a missing buffer does in the reference (buffer_consumer.go:196-206).
template <class B>
int bank_to_rings(bnhip_windows* w, B* b, int n_frames, const int* streams, const int* sources, const int16_t* const* frames,
                  const int* n_in) {
    if (!w || !b || (n_frames > 0 && !sources)) return set_err(BNHIP_E_INVALID, "NULL argument");
    BN_GUARD_BEGIN
    for (int f = 0; f < n_frames; f++)
        if (!w->a->stats(sources[f], nullptr, nullptr, nullptr)) return set_err(BNHIP_E_INVALID, "no such source: " + std::to_string(sources[f]));
    std::lock_guard<std::mutex> lk(b->mu);
    return b->run(n_frames, streams, frames, n_in, false, INT64_MAX,
                  [&](int f, const int16_t* p, int n) { (void)w->a->write(sources[f], p, (size_t)n * 2); });
    BN_GUARD_END((void)0)
}

}  // namespace bnhip
