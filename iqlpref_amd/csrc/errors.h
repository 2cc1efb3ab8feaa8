// How an extern "C" entry point of include/iqlhip.h reports a failure: the status code is returned, the text
// goes into the calling thread's buffer (iqlhip_last_error).  Every file that defines entry points includes this.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/iqlhip.h"

namespace iqlhip {
// writes the message, returns `code` (the one buffer per thread is defined in api.hip)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
}  // namespace iqlhip

#define HIP_TRY(expr)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess)                                                                                 \
      return ::iqlhip::fail(IQLHIP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                            __LINE__);                                                                    \
  } while (0)
