// Host-side launch configuration that depends on the device: the dynamic-LDS cap of a kernel, how many of its
// workgroups a CU holds, and the CU count.  Every such decision in csrc/ goes through these three functions; each
// caches per device (obb_ctx is per device, and contexts of different host threads launch through the same kernels).
// One cache per process (inline, one definition across translation units), one mutex, held across the runtime call
// so that a key is queried exactly once.  Only the HIP runtime and the standard library: host-only programs include it.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <tuple>
#include <utility>

namespace obb {

struct LaunchCfgCache {
    std::mutex mu;
    std::map<std::pair<int, const void *>, size_t> dyn_lds;             // (device, kernel) -> cap already set
    std::map<std::tuple<int, const void *, int, size_t>, int> resident;  // (device, kernel, threads, lds) -> workgroups per CU
    std::map<int, int> ncu;                                              // device -> CU count
};

inline LaunchCfgCache &launchcfg_cache() {
    static LaunchCfgCache c;
    return c;
}

// Allows `fn` up to `bytes` of dynamic LDS on the current device (hipFuncAttributeMaxDynamicSharedMemorySize).  The runtime
// is called only when `bytes` exceeds what this (device, kernel) already holds; a failure is returned and not recorded.
inline hipError_t allow_dyn_lds(const void *fn, size_t bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    LaunchCfgCache &c = launchcfg_cache();
    std::lock_guard<std::mutex> lock(c.mu);
    size_t &have = c.dyn_lds[std::make_pair(dev, fn)];  // (0 when new)
    if (bytes <= have) return hipSuccess;
    if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)) != hipSuccess) return e;
    have = bytes;
    return hipSuccess;
}

// Workgroups of `fn` (`threads` wide, `lds` bytes of dynamic LDS) that one CU of the current device holds: the raw
// value of the occupancy query, which may be 0.
inline hipError_t resident_blocks(const void *fn, int threads, size_t lds, int *per_cu) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    LaunchCfgCache &c = launchcfg_cache();
    std::lock_guard<std::mutex> lock(c.mu);
    const auto key = std::make_tuple(dev, fn, threads, lds);
    auto it = c.resident.find(key);
    if (it == c.resident.end()) {
        int n = 0;
        if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds)) != hipSuccess) return e;
        it = c.resident.emplace(key, n).first;
    }
    *per_cu = it->second;
    return hipSuccess;
}

// CU count of the current device.  An error is the caller's to handle: there is no default.
inline hipError_t cu_count(int *ncu) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    LaunchCfgCache &c = launchcfg_cache();
    std::lock_guard<std::mutex> lock(c.mu);
    auto it = c.ncu.find(dev);
    if (it == c.ncu.end()) {
        int n = 0;
        if ((e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
        it = c.ncu.emplace(dev, n).first;
    }
    *ncu = it->second;
    return hipSuccess;
}

}  // namespace obb
