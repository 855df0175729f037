// The device plumbing of the one-shot clip entries (api_loudness.cpp, api_flac.cpp, api_spectrogram.cpp, api_ultrasonic.cpp and the
// one-shot half of api_resample.cpp): a cache of uploaded tables, a call's device blocks, the argument checks they share and the
// copies that bring byte streams back.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "api_common.h"
#include "ragged.h"

namespace bnhip {

// t on the current device; -> NULL on an allocation / copy failure, with the HIP error cleared
template <class T>
T* upload_table(const std::vector<T>& t) {
    T* d = nullptr;
    if (hipMalloc((void**)&d, t.size() * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (hipMemcpy(d, t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); hipFree(d); return nullptr; }
    return d;
}

// Device tables uploaded on first use and kept; the oldest of kCap entries leaves.  E holds a key, what the caller needs of the
// table besides, and the device pointer `d` (NULL where an entry has no table).  A caller holds a TableLock on `mu` from the lookup
// until its kernels are enqueued: hipFree waits for the device, so a table is never freed between a lookup and the launch that
// reads it, nor under a queued kernel.  (Two caches that one call consults share the first one's mu.)
using TableLock = std::unique_lock<std::mutex>;
template <class E>
struct TableCache {
    static constexpr size_t kCap = 32;
    std::mutex mu;
    std::vector<E> entries;
    // the entry `match` accepts, else the one `make` fills in (make -> false: nothing is kept, -> NULL)
    template <class Match, class Make>
    const E* find(const TableLock&, Match match, Make make) {
        for (const E& e : entries) if (match(e)) return &e;
        if (entries.size() >= kCap) { hipFree(entries.front().d); entries.erase(entries.begin()); }
        E e{};
        if (!make(e)) return nullptr;
        entries.push_back(std::move(e));
        return &entries.back();
    }
};

// The device blocks of one host-pointer call: the first failure sticks (later gets and the caller's `if (b.he == hipSuccess)` steps
// fall through), and every block is freed on every path out.
struct DevBlocks {
    std::vector<void*> p;
    hipError_t he = hipSuccess;
    bool nomem = false;
    void* get(size_t bytes) {
        void* d = nullptr;
        if (he == hipSuccess) he = hipMalloc(&d, bytes ? bytes : 1);
        if (he == hipErrorOutOfMemory) nomem = true;
        if (he == hipSuccess) p.push_back(d);
        return d;
    }
    ~DevBlocks() { for (void* d : p) hipFree(d); }
};

// The device parts of a host-pointer call: add() every part first (-> its handle), alloc() once, then at() each handle.  The parts
// of own_below (DEV_OWN_BLOCK) bytes and more are carved from one block at 256-byte alignment (what the device entries ask of a workspace), so a
// call makes one driver allocation however many large parts it has.  A smaller part is an allocation of its own: those the HIP
// runtime serves from blocks it keeps, with no driver call (1.4 us against 130 us and more from 2 MiB on, and a call on one 15 s
// clip is 0.26 ms slower with its 1.4 MB parts in one 3 MB block than with each on its own: DESIGN.md section 9, "One body per
// entry"), so a call whose parts are all small pays for none.
constexpr size_t DEV_OWN_BLOCK = (size_t)2 << 20;
struct DevCarve {
    std::vector<size_t> sizes;
    std::vector<char*> parts;
    size_t own_below = DEV_OWN_BLOCK;        // a part smaller than this is an allocation of its own (0: every part from the one block)
    size_t add(size_t bytes) { sizes.push_back(bytes ? bytes : 1); return sizes.size() - 1; }
    void alloc(DevBlocks& b) {
        auto al = [](size_t s) { return (s + 255) & ~(size_t)255; };
        size_t shared = 0;
        for (size_t s : sizes) if (s >= own_below) shared += al(s);
        char* next = shared ? (char*)b.get(shared) : nullptr;
        for (size_t s : sizes) {
            if (s < own_below) { parts.push_back((char*)b.get(s)); continue; }
            parts.push_back(next);
            if (next) next += al(s);
        }
    }
    template <class T> T* at(size_t part) const { return part < parts.size() ? (T*)parts[part] : nullptr; }
};

// b.he != hipSuccess: BNHIP_E_NOMEM for a failed allocation, else BNHIP_E_RUNTIME; the HIP error is cleared for the thread's next call
inline int hip_fail(const char* what, const DevBlocks& b) {
    (void)hipGetLastError();
    return set_err(b.nomem ? BNHIP_E_NOMEM : BNHIP_E_RUNTIME, std::string(what) + ": " + hipGetErrorString(b.he));
}

// after a launch on a caller's stream: -> BNHIP_OK or BNHIP_E_RUNTIME
inline int launch_status(const char* what) {
    const hipError_t he = hipGetLastError();
    if (he != hipSuccess) return set_err(BNHIP_E_RUNTIME, std::string(what) + ": " + hipGetErrorString(he));
    return BNHIP_OK;
}

// What every clip entry checks of its clips before any device is touched; -> 0 or a negative BNHIP_E_*.  A ragged burst's lengths
// are a host array, each >= 1; its clips are packed back to back at 64-bit offsets, and their total is held to STREAMINFO's 36 bits,
// which keeps every flat count of the kernels (frames, segments, true-peak tiles) inside a 31-bit grid.
constexpr long long RAGGED_MAX_SAMPLES = (1ll << 36) - 1;
inline int clips_check(const Clips& c) {
    if (c.n_clips < 1 || c.n_clips > 65535) return set_err(BNHIP_E_INVALID, "n_clips must be in [1, 65535]");
    if (!c.lens) return c.n < 1 ? set_err(BNHIP_E_INVALID, "n must be at least 1") : 0;
    long long total = 0;
    for (int i = 0; i < c.n_clips; i++) {
        if (c.lens[i] < 1) return set_err(BNHIP_E_INVALID, "every clip length must be at least 1");
        total += c.lens[i];
    }
    if (total > RAGGED_MAX_SAMPLES) return set_err(BNHIP_E_INVALID, "the clips' total length must be below 2^36 samples");
    return 0;
}
// a ragged entry's lens before they become a Clips, where NULL would say "uniform"; n_clips out of range is clips_check's to answer
inline int lens_check(int n_clips, const int* lens) {
    if (!lens && n_clips >= 1 && n_clips <= 65535) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    return 0;
}

// what an entry that returns byte streams copies back: the offsets first (that copy is the call's synchronise), then exactly
// offsets[n] bytes
inline hipError_t fetch_streams(const unsigned long long* d_offsets, const uint8_t* d_bytes, int n, uint64_t* offsets, uint8_t* out) {
    hipError_t he = hipMemcpy(offsets, d_offsets, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost);
    if (he == hipSuccess && offsets[n] > 0) he = hipMemcpy(out, d_bytes, (size_t)offsets[n], hipMemcpyDeviceToHost);
    return he;
}

// a device entry's caller-owned workspace against what `size_entry` (the bnhip_*_workspace_size to name) answers
inline int workspace_check(const void* d_workspace, size_t have, size_t need, const char* size_entry) {
    if (have < need) return set_err(BNHIP_E_INVALID, std::string("workspace smaller than ") + size_entry);
    if (((uintptr_t)d_workspace & 255) != 0) return set_err(BNHIP_E_INVALID, "workspace must be 256-byte aligned");
    return 0;
}

}  // namespace bnhip
