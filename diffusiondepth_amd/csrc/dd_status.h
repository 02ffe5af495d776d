// dd_status.h -- how the stateless operator units (dd_api_bn.cpp, dd_api_conv.cpp, dd_api_codec.cpp, dd_api_eval.cpp, dd_dcn.hip, dd_msda.hip)
// record a failed call: the return code, and a message behind the unit's dd_*_last_error.  Header-only.  Each unit defines ONE
//   thread_local ddstatus::LastError g_<unit>_err;
// of its own and hands out g_<unit>_err.text.c_str(): an error of one operator never shows through another's accessor.  (The handle-based ABI of
// dd_api.cpp keeps its message in the handle: h->fail / DD_HIP of dd_api_internal.h.)
#pragma once
#include "../../include/ddepth.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

namespace ddstatus __attribute__((visibility("hidden"))) {      // helpers of the units, not symbols of the library

struct LastError {
  std::string text;

  // records the printf-formatted message, returns `code`
  int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    text = buf;
    return code;
  }
};

// the pointers of a two-input convolution call: a, b in, `out` out, `ws` the workspace the 16-byte operand reads go to
inline int check_ptrs(LastError& err, const void* a, const void* b, const void* out, const void* ws) {
  if (!a || !b || !out || !ws) return err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (out == a || out == b) return err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  if (((uintptr_t)ws & 15) != 0) return err.fail(DD_ERR_INVALID_ARG, "the workspace must be 16-byte aligned");
  return DD_OK;
}

}  // namespace ddstatus

// returns DD_ERR_HIP from the calling function, with "<expr>: <hipGetErrorString>" in `err`, when the HIP call `expr` fails
#define DD_STATUS_HIP(err, expr)                                                                    \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess) return (err).fail(DD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e));    \
  } while (0)
