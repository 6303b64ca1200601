// Error plumbing of the C ABI: the thread-local message behind svr_last_error() and the check-and-return macro.  Nothing
// from ROCm is included, so the file-format units (io_*.cpp) and capi.cpp build with any C++17 compiler.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "svr_hip.h"

namespace svr { void set_error(const char *fmt, ...); }  // capi.cpp

#define SVR_CHECK(cond, code, ...)      \
  do {                                  \
    if (!(cond)) {                      \
      svr::set_error(__VA_ARGS__);      \
      return (code);                    \
    }                                   \
  } while (0)
