// hosterr.hip.h — host only, plain C++17: the thread's last error text (mfas_last_error) and fail(), which every MFAS_E* return goes
// through.  No HIP name: HIPCHK, which turns a hipError_t into fail(MFAS_EHIP, ...), stays with the HIP code (common.hip.h).
#pragma once
#include <string>

static thread_local std::string g_err;
inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
