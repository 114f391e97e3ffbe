// Per-device "already done" words for one-time, per-device launch preparation (hipFuncSetAttribute grants of dynamic LDS
// above 64 KiB are a property of the (function, device) pair): a function-local `static bool done` would make the first
// device's grant hide the missing one on every other device of the process.  Racing writers store the same value.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

#include "gps_hip.h"

namespace gps_dev {

constexpr int kMaxDevices = 32;

inline int current_device() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) d = 0;
  return d;
}

// N words per device; row() = the calling thread's current device
template <typename T, int N>
struct PerDevice {
  T v[kMaxDevices][N] = {};
  T *row() { return v[current_device()]; }
};

// Opt a kernel into more than 64 KiB of dynamic LDS before a launch that wants `lds` bytes: unless this device's last
// grant for the kernel (`granted`, a PerDevice word of the call site) already covers it, ask for `ask` bytes (>= lds: the
// call site's policy, exactly `lds` or the 160 KiB of a CU) and record them.
inline int grant_lds(const void *kernel, size_t lds, size_t ask, size_t &granted) {
  if (lds > 64 * 1024 && lds > granted) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ask) != hipSuccess) return GPS_ERR_LAUNCH;
    granted = ask;
  }
  return GPS_OK;
}

}  // namespace gps_dev
