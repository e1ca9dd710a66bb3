// The library's error state and version string (common.h declares err_buf and fail for every other file).
#include "common.h"

namespace rtpose {

char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

}  // namespace rtpose

extern "C" {

const char* rtpose_version(void) { return "rtpose_mi355x 0.1 (gfx950)"; }
const char* rtpose_last_error(void) { return rtpose::err_buf(); }

}  // extern "C"
