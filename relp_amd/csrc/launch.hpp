// What the launch helpers of every kernel file share: the opt-in to more than 64 KB of dynamic LDS, the check behind a launch, the
// launch timer of the roofline measurement, and the step from a run-time pivot rule to a template argument.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <type_traits>

#include "../../include/relp_amd.h"
#include "device_memory.hpp"

namespace relp {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) acts on the CURRENT device's copy of a kernel, and a batch (relp_batch_create) may
// hold handles on several devices, created and driven by worker threads: one configuration per device, race-free.
struct PerDeviceOnce {
    std::atomic<unsigned long long> done{0};
    std::mutex mutex;
    template <class F>
    void run(F&& configure) {
        int device = 0;
        if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= 64) {  // (no bit to remember it by: configure every time)
            std::lock_guard<std::mutex> lock(mutex);
            configure();
            return;
        }
        const unsigned long long bit = 1ull << device;
        if (done.load(std::memory_order_acquire) & bit) return;
        std::lock_guard<std::mutex> lock(mutex);
        if (done.load(std::memory_order_relaxed) & bit) return;
        configure();
        done.fetch_or(bit, std::memory_order_release);
    }
};

inline void allow_full_lds(const void* kernel) {
    // dynamic + static LDS may reach the 160 KB of a CU; the attribute belongs to the kernel on the current device, so it is set
    // once per device to the maximum (not to the current LP's size: the last loaded handle would decide for every other one)
    hipFuncAttributes attr{};
    size_t fixed = 0;
    if (hipFuncGetAttributes(&attr, kernel) == hipSuccess) fixed = attr.sharedSizeBytes;
    const hipError_t err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024 - fixed));
    if (err != hipSuccess) {
        (void)hipGetLastError();  // not sticky: the launch itself reports a request that is too large
    }
}
// ... for every kernel of a list, once per device.  Only the ceiling: what a launch asks for is computed where it is launched.
template <class... Kernel>
void allow_full_lds_once(PerDeviceOnce& once, Kernel*... kernels) {
    once.run([&] { (allow_full_lds(reinterpret_cast<const void*>(kernels)), ...); });
}

// Behind a launch that is never part of a stream capture (lu.hip: launch_lu_pivot)
inline void check_launch(const char* what) {
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) throw DeviceError(std::string(what) + ": " + hipGetErrorString(err));
}

// Measurement hook (bench.py roofline leg): when armed, the NEXT launch of the named hot-loop kernel is bracketed by a
// start/stop event pair through hipExtLaunchKernelGGL, i.e. its own execution time inside the real pivot sequence.
struct LaunchTimer {
    int which = -1;  // 0 price (sparse or dense), 1 fused ftran/ratio, 2 update
    hipEvent_t start = nullptr, stop = nullptr;
};
extern thread_local LaunchTimer g_timer;  // (kernels.hip)
inline void arm_launch_timer(int which, hipEvent_t start, hipEvent_t stop) {
    g_timer.which = which;
    g_timer.start = start;
    g_timer.stop = stop;
}
#define RELP_LAUNCH(WHICH, KERNEL, GRID, BLOCK, LDS, STREAM, ...)                                            \
    do {                                                                                                     \
        if (g_timer.which == (WHICH)) {                                                                      \
            g_timer.which = -1;                                                                              \
            hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, (std::uint32_t)(LDS), STREAM, g_timer.start, g_timer.stop, 0, __VA_ARGS__); \
        } else {                                                                                             \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCK, LDS, STREAM, __VA_ARGS__);                               \
        }                                                                                                    \
    } while (0)

// relp_options.pivot_rule as a compile-time constant: `f` is a generic lambda, called with a std::integral_constant of the rule.
// Four-way for the kernels that implement every rule, two-way (steepest edge, else Dantzig) for those that only tell the two apart.
template <class F>
void with_pivot_rule(int rule, F&& f) {
    switch (rule) {
        case RELP_PIVOT_DANTZIG: f(std::integral_constant<int, RELP_PIVOT_DANTZIG>{}); break;
        case RELP_PIVOT_FIRST_PROFITABLE: f(std::integral_constant<int, RELP_PIVOT_FIRST_PROFITABLE>{}); break;
        case RELP_PIVOT_FIRST_PROFITABLE_MEMORY: f(std::integral_constant<int, RELP_PIVOT_FIRST_PROFITABLE_MEMORY>{}); break;
        default: f(std::integral_constant<int, RELP_PIVOT_STEEPEST_EDGE>{}); break;
    }
}
template <class F>
void with_steepest_edge_or_dantzig(int rule, F&& f) {
    if (rule == RELP_PIVOT_STEEPEST_EDGE) f(std::integral_constant<int, RELP_PIVOT_STEEPEST_EDGE>{});
    else f(std::integral_constant<int, RELP_PIVOT_DANTZIG>{});
}

}  // namespace relp
