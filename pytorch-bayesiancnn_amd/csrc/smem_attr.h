// Host-side helper shared by the kernels that need more dynamic LDS than the default limit (pconv_bf16.hip, pconv_bf16_lrt.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>

namespace {

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: `state` (one array per kernel instantiation)
// remembers the bytes granted on each device, so that a process driving several GPUs -- or several threads (relaxed atomics: a
// duplicated call is harmless) -- sets it wherever a launch needs it.
constexpr int kMaxDevices = 64;
struct SmemAttrState { std::atomic<int> bytes[kMaxDevices]; };
inline int ensure_dynamic_smem(const void* fn, int bytes, SmemAttrState& state) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
        return (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);       // (unknown device: every time)
    }
    if (state.bytes[dev].load(std::memory_order_relaxed) >= bytes) return 0;
    const hipError_t er = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (er != hipSuccess) return (int)er;
    state.bytes[dev].store(bytes, std::memory_order_relaxed);
    return 0;
}

}  // namespace
