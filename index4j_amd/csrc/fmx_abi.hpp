// fmx_abi.hpp — what every file of the C-ABI layer needs around its entry points: the error setter, the guard that keeps exceptions
// inside and the macro for a HIP runtime call.  Host code only: no .hip file includes it.
#pragma once

#include "../../include/fmx.h"

#include <exception>
#include <new>
#include <string>

namespace fmx {

// fmx_api.cpp: sets the calling thread's fmx_last_error and returns `code`.  With FMX_E_HIP the thread's last HIP error is taken
// off with the report, or the NEXT call's launchers — which ask hipGetLastError() after their launches — would report this call's
// failure as their own.
int api_fail(int code, const std::string &msg);

// The ABI never throws (an exception crossing into a JVM through JNI aborts it): every entry point that returns a status runs
// inside this guard.  What can throw in there: allocations sized by the caller's data, thread creation.
template <class F>
int guarded(F &&body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return api_fail(FMX_E_UNSUPPORTED, "out of host memory");
    } catch (const std::exception &e) {
        return api_fail(FMX_E_UNSUPPORTED, std::string("internal error: ") + e.what());
    }
}

}  // namespace fmx

// a HIP runtime call inside a function that returns an FMX_* code (the file that uses it includes <hip/hip_runtime.h>)
#define FMX_HIP_TRY(expr)                                                                                             \
    do {                                                                                                              \
        hipError_t e__ = (expr);                                                                                      \
        if (e__ != hipSuccess) return ::fmx::api_fail(FMX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)
