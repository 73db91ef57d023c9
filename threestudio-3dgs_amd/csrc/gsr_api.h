// gsr_api.h — what the C ABI files (gsr_api.hip, gsr_api_image.hip, gsr_api_sugar.hip) share: the calling thread's
// error message and the argument-check helpers.  Host code only.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/gsr.h"
#include "gsr_kernels.h"

namespace gsr {

// what gsr_last_error() returns: one per thread, one in the library (defined in gsr_api.hip)
extern thread_local char g_err[512];

inline int fail(int code, const char* fmt, const char* what) {
  snprintf(g_err, sizeof(g_err), fmt, what);
  return code;
}
inline int invalid(const char* msg) { return fail(GSR_EINVAL, "%s", msg); }
inline int null_argument() { return invalid("null pointer argument"); }
inline int null_named(const char* name) { return fail(GSR_EINVAL, "null pointer argument: %s", name); }

#define GSR_HIP_CHECK(expr)                                                        \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) return fail(GSR_EHIP, "HIP error: %s", hipGetErrorString(e_)); \
  } while (0)

inline int last_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(GSR_EHIP, "HIP launch error: %s", hipGetErrorString(e));
  g_err[0] = 0;
  return GSR_OK;
}

// an empty problem: nothing to launch, no device touched
inline int nothing_to_do() {
  g_err[0] = 0;
  return GSR_OK;
}

// true, with the message set, when a workspace of `have` bytes does not hold `need`
inline bool workspace_too_small(size_t have, size_t need) {
  if (have < need) invalid("workspace too small");
  return have < need;
}

// any of the pointers is not n-byte aligned (n a power of two)
template <typename... Ptr>
inline bool misaligned(uintptr_t n, Ptr... p) {
  return (((uintptr_t)p | ...) & (n - 1)) != 0;
}

inline bool below_2_31(long long a, long long b) { return a * b < (1ll << 31); }
// a size argument of a sizer: negative counts size as empty
inline int at_least_0(int x) { return x < 0 ? 0 : x; }

}  // namespace gsr
