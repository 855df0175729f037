// The device plumbing of the one-shot clip entries (api_loudness.cpp, api_flac.cpp, api_spectrogram.cpp, api_ultrasonic.cpp and the
// one-shot half of api_resample.cpp): a cache of uploaded tables, a call's device blocks, and the argument checks they share.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "api_common.h"

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

// The parts of a call that takes all its device memory as one block: add() every part first (-> its offset, 256-byte aligned, what
// the device entries ask of a workspace), allocate bytes() once, then at() each offset.
struct DevCarve {
    size_t total = 0;
    char* base = nullptr;
    size_t add(size_t bytes) { const size_t off = total; total += ((bytes ? bytes : 1) + 255) & ~(size_t)255; return off; }
    size_t bytes() const { return total; }
    template <class T> T* at(size_t off) const { return base ? (T*)(base + off) : nullptr; }
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

// what every clip entry checks before any device is touched; -> 0 or a negative BNHIP_E_*
inline int clip_dims_check(int n_clips, int n) {
    if (n_clips < 1 || n_clips > 65535) return set_err(BNHIP_E_INVALID, "n_clips must be in [1, 65535]");
    if (n < 1) return set_err(BNHIP_E_INVALID, "n must be at least 1");
    return 0;
}

// A ragged burst's lengths (host array lens[n_clips], each >= 1) before any device is touched.  The clips are packed back to back at
// 64-bit offsets; the total is held to STREAMINFO's 36 bits, which keeps every flat count of the kernels (frames, segments, true-peak
// tiles) inside a 31-bit grid.
constexpr long long RAGGED_MAX_SAMPLES = (1ll << 36) - 1;
inline int ragged_lens_check(int n_clips, const int* lens) {
    if (n_clips < 1 || n_clips > 65535) return set_err(BNHIP_E_INVALID, "n_clips must be in [1, 65535]");
    if (!lens) return set_err(BNHIP_E_INVALID, "NULL/empty argument");
    long long total = 0;
    for (int c = 0; c < n_clips; c++) {
        if (lens[c] < 1) return set_err(BNHIP_E_INVALID, "every clip length must be at least 1");
        total += lens[c];
    }
    if (total > RAGGED_MAX_SAMPLES) return set_err(BNHIP_E_INVALID, "the clips' total length must be below 2^36 samples");
    return 0;
}
inline size_t ragged_total(int n_clips, const int* lens) {
    size_t total = 0;
    for (int c = 0; c < n_clips; c++) total += (size_t)lens[c];
    return total;
}

// a device entry's caller-owned workspace against what `size_entry` (the bnhip_*_workspace_size to name) answers
inline int workspace_check(const void* d_workspace, size_t have, size_t need, const char* size_entry) {
    if (have < need) return set_err(BNHIP_E_INVALID, std::string("workspace smaller than ") + size_entry);
    if (((uintptr_t)d_workspace & 255) != 0) return set_err(BNHIP_E_INVALID, "workspace must be 256-byte aligned");
    return 0;
}

}  // namespace bnhip
