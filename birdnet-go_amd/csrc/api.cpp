// C ABI of libbnhip.so, the library-wide part: version, the calling thread's last error, init / shutdown and pinned host
// allocation, and the helpers api_common.h declares.  The handle types have a unit each: api_windows.cpp, api_model.cpp,
// api_predict.cpp, api_ultrasonic.cpp, api_resample.cpp, api_eq.cpp, api_soundlevel.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>

#include "api_common.h"
#include "hostpipe.h"
#include "numa.h"

namespace {

thread_local std::string g_err;
std::mutex g_init_mu;
int g_devices = -1;     // -1 = not initialised

}  // namespace

namespace bnhip {

int set_err(int code, const std::string& msg) noexcept {
    try { g_err = msg; } catch (...) { g_err.clear(); }
    return code;
}

int device_count() {
    std::lock_guard<std::mutex> lk(g_init_mu);
    return g_devices;
}

int exception_error(std::string& text) noexcept {
    int code = BNHIP_E_RUNTIME;
    try {
        try { throw; }
        catch (const std::bad_alloc&) { code = BNHIP_E_NOMEM; text = "out of host memory"; }
        catch (const std::exception& ex) { text = std::string("internal error: ") + ex.what(); }
        catch (...) { text = "internal error: unknown exception"; }
    } catch (...) { text.clear(); }
    return code;
}

int guard_fail() noexcept {
    std::string text;
    const int code = exception_error(text);
    return set_err(code, text);
}

int use_device(int device) {
    int rc = bnhip_init(nullptr);
    if (rc) return rc;
    if (device < 0 || device >= device_count()) return set_err(BNHIP_E_INVALID, "device ordinal out of range");
    hipSetDevice(device);
    return BNHIP_OK;
}

int copy_out(const std::string& s, char* buf, size_t cap) {
    if (buf && cap) {
        size_t n = std::min(cap - 1, s.size());
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (int)s.size() + 1;
}

bool is_gfx950(int dev) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

}  // namespace bnhip

using namespace bnhip;

extern "C" {

const char* bnhip_version(void) { return "bnhip 0.2 (gfx950)"; }
const char* bnhip_last_error(void) { return g_err.c_str(); }
int bnhip_last_error_copy(char* buf, size_t cap) { return copy_out(g_err, buf, cap); }

int bnhip_init(int* n_devices) {
    BN_GUARD_BEGIN
    std::lock_guard<std::mutex> lk(g_init_mu);
    if (g_devices < 0) {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            if (n_devices) *n_devices = 0;
            return set_err(BNHIP_E_NO_DEVICE, std::string("no HIP device available: ") + hipGetErrorString(e));
        }
        int usable = 0;
        for (int d = 0; d < n; d++) if (is_gfx950(d)) usable++;
        if (!usable) {
            if (n_devices) *n_devices = 0;
            return set_err(BNHIP_E_NO_DEVICE, "no gfx950 (MI355X) device found; this library ships gfx950 code objects only");
        }
        g_devices = n;
    }
    if (n_devices) *n_devices = g_devices;
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

void bnhip_shutdown(void) {
    try {
        std::lock_guard<std::mutex> lk(g_init_mu);
        g_devices = -1;
    } catch (...) {}
}

int bnhip_host_alloc(size_t n_bytes, void** out) {
    BN_GUARD_BEGIN
    if (!out || !n_bytes) return set_err(BNHIP_E_INVALID, "bnhip_host_alloc: null output pointer or zero size");
    *out = nullptr;
    int rc = bnhip_init(nullptr);
    if (rc != BNHIP_OK) return rc;
    void* p = nullptr;
    // (round 6: from the NUMA node of the calling thread's current device when it has room - the buffer a Go classifier keeps per
    // model is read by that device's copy engines on every call; portable: pinned for every device of a multi-GPU handle)
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); cur = -1; }
    bnhip::NumaPrefer near_gpu(bnhip::device_numa_node(cur));
    hipError_t e = hipHostMalloc(&p, n_bytes, hipHostMallocPortable);
    if (e != hipSuccess) { (void)hipGetLastError(); return set_err(e == hipErrorOutOfMemory ? BNHIP_E_NOMEM : BNHIP_E_RUNTIME, std::string("pinned host allocation failed: ") + hipGetErrorString(e)); }
    *out = p;
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

int bnhip_host_free(void* p) {
    BN_GUARD_BEGIN
    if (!p) return BNHIP_OK;
    hipError_t e = hipHostFree(p);
    if (e != hipSuccess) { (void)hipGetLastError(); return set_err(BNHIP_E_INVALID, std::string("bnhip_host_free: not a bnhip_host_alloc pointer: ") + hipGetErrorString(e)); }
    return BNHIP_OK;
    BN_GUARD_END((void)0)
}

}  // extern "C"
