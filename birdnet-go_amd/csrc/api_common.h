// What the api*.cpp units share (internal to them; see include/bnhip.h for the interface itself).
//
// Every extern "C" entry point is exception-tight: the engine is C++ (std::vector / std::map / std::string), and an
// exception unwinding through a cgo frame aborts the host process, which would break the reference's rule for native
// backends - "never panic; any failure => fall back" (internal/classifier/model_openvino.go:227-230).  BN_GUARD turns
// std::bad_alloc into BNHIP_E_NOMEM and anything else into BNHIP_E_RUNTIME.
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>

#include "../../include/bnhip.h"

namespace bnhip {

class WindowAssembler;

// The calling thread's error text (what bnhip_last_error answers) and the device count live in api.cpp, once for the library.
int set_err(int code, const std::string& msg) noexcept;
int device_count();                                      // what bnhip_init found; -1 = not initialised
bool is_gfx950(int device);
// inside a catch block: the exception in flight -> its BNHIP_* code and text
int exception_error(std::string& text) noexcept;
int guard_fail() noexcept;                               // set_err of exception_error
// bnhip_init, then the ordinal checked and made current
int use_device(int device);
// the snprintf convention of the *_read / describe entries: s into buf[cap], -> the bytes a whole copy needs
int copy_out(const std::string& s, char* buf, size_t cap);

}  // namespace bnhip

#define BN_GUARD_BEGIN try {
#define BN_GUARD_END(fallback_stmt) } catch (...) { fallback_stmt; return bnhip::guard_fail(); }

// ---------------------------------------------------------------------------------------------- window assembler (row a3)
// (here because the tick entry and the banks' ring writers reach the assembler through it)
struct bnhip_windows {
    std::unique_ptr<bnhip::WindowAssembler> a;
    uint8_t* batch = nullptr;
    bool pinned = false;
};
