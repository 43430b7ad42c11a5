// Host side of every kernel launch of libdifformer_hip.so: the one spelling for launch + status, the grid constructor, and the
// dynamic-LDS attribute.  Included at the end of dif_common.h (needs dif::fail / dif::launch_status); the variant selectors
// dif::with_flags / dif::with_int come with it.
#pragma once
#include <atomic>
#include "dif_select.h"

namespace dif {

// dim3 from the 64-bit counts the launchers compute (every one is checked or capped before it gets here)
inline dim3 grid_of(int64_t x, int64_t y = 1, int64_t z = 1) {
    return dim3(static_cast<unsigned>(x), static_cast<unsigned>(y), static_cast<unsigned>(z));
}

// Launch + post-launch check (hipGetLastError only, never synchronises).  The arguments convert to the kernel's parameter
// types as in a plain call.  `what` is the text of the error; several kernels of one entry point may share it.
template <typename... P, typename... A>
int launch(const char* what, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... args) {
    static_assert(sizeof...(P) == sizeof...(A), "dif::launch: argument count does not match the kernel's parameters");
    hipLaunchKernelGGL(kernel, grid, block, static_cast<unsigned>(lds), st, static_cast<A&&>(args)...);
    return launch_status(what);
}

// with_int's miss: an unlisted value is a programming error of the launcher, reported as DIF_E_SHAPE
inline auto no_variant(const char* who) {
    return [who](int v) { return fail(DIF_E_SHAPE, "%s: no kernel variant for %d", who, v); };
}

// Dynamic LDS above 64 KiB must be allowed per kernel and per device.  Success is remembered per (kernel instantiation, device):
// one hipFuncSetAttribute per kernel per process on a single device, nothing but hipGetDevice per launch after that.  A failure
// is never remembered -- the next call tries again.  `bytes` is the kernel's largest case, the same at every call.
template <auto Kernel>
int allow_lds(int bytes, const char* who) {
    constexpr int kDevices = 16;
    static std::atomic<bool> allowed[kDevices] = {};
    int dev = 0;
    hipError_t he = hipGetDevice(&dev);
    if (he != hipSuccess) return fail(static_cast<int>(he), "%s: LDS attribute: %s", who, hipGetErrorString(he));
    const bool slot = dev >= 0 && dev < kDevices;
    if (slot && allowed[dev].load(std::memory_order_acquire)) return 0;
    he = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (he != hipSuccess) return fail(static_cast<int>(he), "%s: LDS attribute: %s", who, hipGetErrorString(he));
    if (slot) allowed[dev].store(true, std::memory_order_release);
    return 0;
}

}  // namespace dif
