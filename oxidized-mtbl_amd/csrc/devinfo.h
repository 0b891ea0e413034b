// devinfo.h — immutable device properties the launch sizes need, cached per device.
//
// The library keeps no mutable state between calls (include/mtblx.h); the one process-wide data
// is this cache of what the hardware is (compute units, occupancy of a kernel), filled on first
// use per device.  Relaxed atomics: concurrent first calls from several host threads store the
// same value, and a device's entry never changes afterwards.
//
// One diagnostic seam sits on top (mtblx_debug_cu_limit, include/mtblx.h): a process-wide limit
// that can only LOWER what cu_count() answers, so that a test reaches the wrap-around trip of
// every capped launch at a small input.  The hardware value stays cached underneath; while a
// limit is set nothing derived from it is stored (Cache::get), so lifting it restores today's
// launches exactly.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace mtblx_dev {

constexpr int kMaxDevices = 64;

// the diagnostic limit (0: none); one relaxed load per launch
inline std::atomic<int>& cu_limit_word() {
  static std::atomic<int> w{0};
  return w;
}
inline int cu_limit() { return cu_limit_word().load(std::memory_order_relaxed); }

// compute units of the current device (256 on MI355X; 256 if the query fails), lowered to the
// diagnostic limit while one is set
inline int cu_count() {
  static std::atomic<int> cache[kMaxDevices];
  int dev = 0;
  (void)hipGetDevice(&dev);
  int v = (dev >= 0 && dev < kMaxDevices) ? cache[dev].load(std::memory_order_relaxed) : 0;
  if (v <= 0) {
    (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
    if (v <= 0) v = 256;
    if (dev >= 0 && dev < kMaxDevices) cache[dev].store(v, std::memory_order_relaxed);
  }
  const int lim = cu_limit();
  if (lim != 0) {
    const int cap = lim > 1 ? lim : 1;
    if (cap < v) v = cap;
  }
  return v;
}

// a per-device cached value computed by f() (e.g. an occupancy query): one Cache object per use.
// With a CU limit in force f() runs every time and its answer is not kept (it may depend on
// cu_count()); a limit that changes while f() runs keeps the answer out of the cache as well.
struct Cache {
  std::atomic<int> v[kMaxDevices] = {};
  template <class F>
  int get(F f) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= kMaxDevices || cu_limit() != 0) return f();
    int x = v[dev].load(std::memory_order_relaxed);
    if (x <= 0) {
      x = f();
      if (cu_limit() == 0) v[dev].store(x, std::memory_order_relaxed);
    }
    return x;
  }
};

}  // namespace mtblx_dev
