// Error plumbing and version for libfootprints_hip (see include/footprints_hip.h).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "footprints_hip.h"

static thread_local char g_err[512] = "";

int fp_set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int fp_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) return FP_OK;
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return (int)e;
}

// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), eight bytes per step through eight tables: the checksum of TFRecord framing
// (training/summary.py), taken over megabytes of PNG per log event on a thread that must not hold the interpreter lock.  `crc` is the
// value of the bytes before `data` (0 at the start), so a range may be fed in parts.
namespace {
struct Crc32cTables {
  uint32_t t[8][256];
  Crc32cTables() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0x82F63B78u : 0u);
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int j = 1; j < 8; ++j) t[j][i] = (t[j - 1][i] >> 8) ^ t[0][t[j - 1][i] & 0xffu];
  }
};
}  // namespace

extern "C" uint32_t fp_crc32c(uint32_t crc, const void* data, int64_t bytes) {
  static const Crc32cTables tab;
  const unsigned char* p = (const unsigned char*)data;
  uint32_t c = ~crc;
  if (!p || bytes <= 0) return crc;
  while (bytes >= 8) {
    const uint32_t lo = c ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    c = tab.t[7][lo & 0xffu] ^ tab.t[6][(lo >> 8) & 0xffu] ^ tab.t[5][(lo >> 16) & 0xffu] ^ tab.t[4][lo >> 24] ^ tab.t[3][p[4]] ^ tab.t[2][p[5]] ^
        tab.t[1][p[6]] ^ tab.t[0][p[7]];
    p += 8;
    bytes -= 8;
  }
  while (bytes-- > 0) c = (c >> 8) ^ tab.t[0][(c ^ *p++) & 0xffu];
  return ~c;
}

extern "C" int fp_version(void) { return 1; }
extern "C" const char* fp_last_error_string(void) { return g_err; }

