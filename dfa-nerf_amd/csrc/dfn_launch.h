// dfn_launch.h - host-side helpers of the kernel launchers
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
namespace dfn {
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device): a second device of the process needs it too.
// The kernel is the template ARGUMENT, so every kernel has a table of its own (a local static of a template on the kernel's
// TYPE would be shared by all kernels of one signature).  Host threads may race to the first call: the flags are atomic and
// setting the attribute twice is harmless.  A device id outside the table sets the attribute every time.
template <auto Kernel> hipError_t lds_limit(int bytes) {
    static std::atomic<bool> done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool slot = dev >= 0 && dev < 64;
    if (slot && done[dev].load(std::memory_order_acquire)) return hipSuccess;
    e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && slot) done[dev].store(true, std::memory_order_release);
    return e;
}
}  // namespace dfn
