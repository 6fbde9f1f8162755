// What the host code of every translation unit of libmcpc.so shares, with no kernel behind it: the error string of mcpc_last_error
// and the ways an entry point fails.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <string>

#include "../../include/mcpc.h"

namespace mcpc {

inline thread_local std::string g_err;      // mcpc_last_error: ONE instance for the whole library (an inline variable), whichever unit fails

inline int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) return fail(MCPC_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

static inline int grid_for(size_t n, int block = 256) { return (int)std::min<size_t>((n + block - 1) / block, 4096); }

}  // namespace mcpc
