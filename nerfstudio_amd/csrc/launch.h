// Host side of the entry points, once: argument checks that several files share, the dynamic-LDS opt-in, the compute-unit
// count of the current device, the launch-grid guard. Host code only (needs the HIP runtime); not part of the C ABI.
#pragma once

#include "common.h"

namespace nsamd {

// ---- argument checks (no HIP runtime call) -------------------------------------------------------------------------------------
// M points given as explicit positions or as (origins, directions, t_bins) of rays with samples_per_ray samples each
inline int check_points(const nsamd_points& P, int64_t M) {
  if (M < 0) return NSAMD_ERR_INVALID_ARG;
  if (P.positions == nullptr && (P.origins == nullptr || P.directions == nullptr || P.t_bins == nullptr ||
                                 P.samples_per_ray <= 0 || M % P.samples_per_ray != 0))
    return NSAMD_ERR_INVALID_ARG;
  return NSAMD_OK;
}

// table sizes the kernels index with 32-bit arithmetic: 2 .. 2^28 entries per level
inline bool table_size_ok(const nsamd_grid& g) { return g.log2_table_size >= 1 && g.log2_table_size <= 28; }

inline int check_grid(const nsamd_grid& g) {
  return (g.num_levels > 0 && g.num_levels <= NSAMD_MAX_LEVELS && table_size_ok(g)) ? NSAMD_OK : NSAMD_ERR_UNSUPPORTED;
}

// n workgroups as the x extent of a launch grid
inline int grid_blocks(int64_t n, unsigned* blocks) {
  if (n > 0x7fffffffLL) return NSAMD_ERR_UNSUPPORTED;
  *blocks = (unsigned)n;
  return NSAMD_OK;
}

constexpr int kMaxCachedDevices = 64;  // per-device caches below; a device index beyond them is served uncached

inline bool device_properties(int* dev, hipDeviceProp_t* prop) {
  return hipGetDevice(dev) == hipSuccess && hipGetDeviceProperties(prop, *dev) == hipSuccess;
}

// Compute units of the CURRENT device (cached per device index); 256, uncached, where there is none — the workspace queries
// answer on a machine without a GPU too.
inline int device_cus() {
  static int cached[kMaxCachedDevices] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  const bool slot = dev >= 0 && dev < kMaxCachedDevices;
  if (slot && cached[dev] > 0) return cached[dev];
  hipDeviceProp_t prop;
  if (!device_properties(&dev, &prop)) return 256;
  const int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (slot) cached[dev] = cus;
  return cus;
}

// Dynamic LDS beyond 64 KiB is an opt-in per kernel and per device. One LdsOptIn per call site (a function-local static)
// remembers the devices on which its kernels have been opted in.
struct LdsOptIn {
  bool done[kMaxCachedDevices] = {};
};

inline bool lds_set_all() { return true; }
template <class Kernel, class... Rest>
bool lds_set_all(Kernel* kernel, size_t bytes, Rest... rest) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) ==
             hipSuccess &&
         lds_set_all(rest...);
}

// lds_opt_in(cache, kernel, bytes, kernel, bytes, ...): NSAMD_ERR_NO_DEVICE without a current device, NSAMD_ERR_LAUNCH when
// the runtime refuses a size (nothing is cached then: the next call asks again).
template <class... Pairs>
int lds_opt_in(LdsOptIn& cache, Pairs... kernel_bytes_pairs) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return NSAMD_ERR_NO_DEVICE;
  const bool slot = dev >= 0 && dev < kMaxCachedDevices;
  if (slot && cache.done[dev]) return NSAMD_OK;
  if (!lds_set_all(kernel_bytes_pairs...)) return NSAMD_ERR_LAUNCH;
  if (slot) cache.done[dev] = true;
  return NSAMD_OK;
}

}  // namespace nsamd
