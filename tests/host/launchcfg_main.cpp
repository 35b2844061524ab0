// Host-only check of csrc/launchcfg.h: the four HIP entry points it uses are defined here as recorders with a settable
// "current device" (thread-local, as in HIP), so no HIP runtime is linked.  Exit status 0 = every assertion held.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -I<repo>/oriented-object-detection_amd/csrc -pthread launchcfg_main.cpp
#include "launchcfg.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

static thread_local int t_device = 0;
static std::atomic<int> n_attr{0}, n_occ{0}, n_ncu{0};
static std::atomic<int> fail_attr{0}, fail_occ{0}, fail_ncu{0}, fail_dev{0};  // the next call of that kind fails when > 0
static std::atomic<int> last_attr_bytes{0};

static bool take(std::atomic<int> &f) {
    int v = f.load();
    while (v > 0 && !f.compare_exchange_weak(v, v - 1)) {}
    return v > 0;
}

extern "C" {
hipError_t hipGetDevice(int *dev) {
    if (take(fail_dev)) return hipErrorNoDevice;
    *dev = t_device;
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute attr, int value) {
    if (attr != hipFuncAttributeMaxDynamicSharedMemorySize) return hipErrorInvalidValue;
    if (take(fail_attr)) return hipErrorInvalidDeviceFunction;
    ++n_attr;
    last_attr_bytes = value;
    return hipSuccess;
}
// distinct per device, kernel, block size and LDS size, so that a value cached under the wrong key shows
static int occ_value(int dev, const void *fn, int threads, size_t lds) { return 1 + dev * 1000 + (int)((uintptr_t)fn & 15) * 50 + threads / 64 + (int)(lds >> 10); }
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int *n, const void *fn, int threads, size_t lds) {
    if (take(fail_occ)) return hipErrorInvalidValue;
    ++n_occ;
    *n = occ_value(t_device, fn, threads, lds);
    return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t attr, int dev) {
    if (attr != hipDeviceAttributeMultiprocessorCount) return hipErrorInvalidValue;
    if (take(fail_ncu)) return hipErrorInvalidDevice;
    ++n_ncu;
    *v = 256 - 16 * dev;
    return hipSuccess;
}
}

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static char k_a, k_b, k_c, k_t[4];  // stand-ins for kernel addresses

int main() {
    using namespace obb;
    // allow_dyn_lds: once per (device, kernel); raised only by a larger size
    CHECK(allow_dyn_lds(&k_a, 80 * 1024) == hipSuccess && n_attr == 1 && last_attr_bytes == 80 * 1024);
    CHECK(allow_dyn_lds(&k_a, 80 * 1024) == hipSuccess && n_attr == 1);
    CHECK(allow_dyn_lds(&k_b, 80 * 1024) == hipSuccess && n_attr == 2);
    t_device = 1;
    CHECK(allow_dyn_lds(&k_a, 80 * 1024) == hipSuccess && n_attr == 3);
    CHECK(allow_dyn_lds(&k_a, 80 * 1024) == hipSuccess && n_attr == 3);
    t_device = 0;
    CHECK(allow_dyn_lds(&k_a, 40 * 1024) == hipSuccess && n_attr == 3);
    CHECK(allow_dyn_lds(&k_a, 0) == hipSuccess && n_attr == 3);
    CHECK(allow_dyn_lds(&k_a, 150 * 1024) == hipSuccess && n_attr == 4 && last_attr_bytes == 150 * 1024);
    CHECK(allow_dyn_lds(&k_a, 150 * 1024) == hipSuccess && allow_dyn_lds(&k_a, 100 * 1024) == hipSuccess && n_attr == 4);
    // a failure is returned, not cached, and the next call tries again
    fail_attr = 1;
    CHECK(allow_dyn_lds(&k_c, 96 * 1024) == hipErrorInvalidDeviceFunction && n_attr == 4);
    CHECK(allow_dyn_lds(&k_c, 96 * 1024) == hipSuccess && n_attr == 5);
    CHECK(allow_dyn_lds(&k_c, 96 * 1024) == hipSuccess && n_attr == 5);
    fail_attr = 1;  // a failed raise keeps the smaller size that holds
    CHECK(allow_dyn_lds(&k_c, 128 * 1024) == hipErrorInvalidDeviceFunction);
    CHECK(allow_dyn_lds(&k_c, 96 * 1024) == hipSuccess && n_attr == 5);
    CHECK(allow_dyn_lds(&k_c, 128 * 1024) == hipSuccess && n_attr == 6);
    fail_dev = 1;
    CHECK(allow_dyn_lds(&k_c, 160 * 1024) == hipErrorNoDevice && n_attr == 6);

    // resident_blocks: one query per (device, kernel, threads, lds), the raw value
    int v = -1, w = -1;
    CHECK(resident_blocks(&k_a, 256, 4096, &v) == hipSuccess && n_occ == 1 && v == occ_value(0, &k_a, 256, 4096));
    CHECK(resident_blocks(&k_a, 256, 4096, &w) == hipSuccess && n_occ == 1 && w == v);
    CHECK(resident_blocks(&k_a, 512, 4096, &w) == hipSuccess && n_occ == 2 && w == occ_value(0, &k_a, 512, 4096));
    CHECK(resident_blocks(&k_a, 256, 8192, &w) == hipSuccess && n_occ == 3 && w == occ_value(0, &k_a, 256, 8192));
    CHECK(resident_blocks(&k_b, 256, 4096, &w) == hipSuccess && n_occ == 4 && w == occ_value(0, &k_b, 256, 4096));
    t_device = 1;
    CHECK(resident_blocks(&k_a, 256, 4096, &w) == hipSuccess && n_occ == 5 && w == occ_value(1, &k_a, 256, 4096) && w != v);
    CHECK(resident_blocks(&k_a, 256, 4096, &w) == hipSuccess && n_occ == 5);
    t_device = 0;
    fail_occ = 1;
    w = -7;
    CHECK(resident_blocks(&k_c, 256, 4096, &w) == hipErrorInvalidValue && w == -7 && n_occ == 5);  // returned, nothing written
    CHECK(resident_blocks(&k_c, 256, 4096, &w) == hipSuccess && n_occ == 6 && w == occ_value(0, &k_c, 256, 4096));

    // cu_count: one query per device, errors returned and never defaulted
    int c0 = -1, c1 = -1;
    fail_ncu = 1;
    CHECK(cu_count(&c0) == hipErrorInvalidDevice && c0 == -1 && n_ncu == 0);
    CHECK(cu_count(&c0) == hipSuccess && c0 == 256 && n_ncu == 1);
    CHECK(cu_count(&c0) == hipSuccess && c0 == 256 && n_ncu == 1);
    t_device = 1;
    CHECK(cu_count(&c1) == hipSuccess && c1 == 240 && n_ncu == 2);
    CHECK(cu_count(&c1) == hipSuccess && c1 == 240 && n_ncu == 2);
    t_device = 0;
    fail_dev = 1;
    CHECK(cu_count(&c0) == hipErrorNoDevice);

    // 8 threads x 2 devices on fresh keys: the runtime is asked once per distinct key, whatever the interleaving
    t_device = 2;
    const int a0 = n_attr, o0 = n_occ, u0 = n_ncu;
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (int dev = 2; dev < 4; ++dev)
        for (int t = 0; t < 8; ++t)
            th.emplace_back([dev, &bad] {
                t_device = dev;
                for (int it = 0; it < 200; ++it)
                    for (int k = 0; k < 4; ++k) {
                        int n = 0, ncu = 0;
                        if (allow_dyn_lds(&k_t[k], 100 * 1024) != hipSuccess) ++bad;
                        for (size_t lds : {(size_t)1024, (size_t)2048, (size_t)3072})
                            if (resident_blocks(&k_t[k], 256, lds, &n) != hipSuccess || n != occ_value(dev, &k_t[k], 256, lds)) ++bad;
                        if (cu_count(&ncu) != hipSuccess || ncu != 256 - 16 * dev) ++bad;
                    }
            });
    for (auto &t : th) t.join();
    CHECK(bad == 0);
    CHECK(n_attr - a0 == 2 * 4);      // devices x kernels
    CHECK(n_occ - o0 == 2 * 4 * 3);   // devices x kernels x LDS sizes
    CHECK(n_ncu - u0 == 2);           // devices
    printf("launchcfg ok: %d attribute calls, %d occupancy queries, %d CU-count queries\n", n_attr.load(), n_occ.load(), n_ncu.load());
    return 0;
}
