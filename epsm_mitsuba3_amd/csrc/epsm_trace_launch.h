// epsm_trace_launch.h -- the host side of an entry point, for every unit of the tracer's library: the workspace test and the
// checked launch.  Host code only (no kernel, no device function), so any unit may include it.
#pragma once

#include "epsm_common.h"

namespace epsm {

// a pass's workspace: there, 16-byte aligned and of `need` bytes at least
inline bool workspace_ok(const void *workspace, size_t bytes, size_t need) {
    return workspace && bytes >= need && !((uintptr_t) workspace & 15u);
}

// launch, hipGetLastError, hip_fail under the entry point's name
template <class Kernel, class... Params>
int launch_checked(const char *what, Kernel kernel, dim3 grid, unsigned threads, void *stream, Params... params) {
    hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, (hipStream_t) stream, params...);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? epsm_host::hip_fail(what, e) : EPSM_OK;
}

}  // namespace epsm
