// Host-side helpers shared by the kernels that need more dynamic LDS than the default limit (pconv_bf16.hip, pconv_bf16_lrt.hip):
// the per-device attribute, and the launch of the tiled bf16 GEMM kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>

#include "pconv_bf16_plan.h"

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

// The launch of one instantiation of a tiled bf16 GEMM kernel (pconv_bf16_kernel, its transposed form, pconv_bf16_lrt_kernel):
// KG k-groups x (WN x WM) waves (+ 4 staging waves with WS), WT weight tiles of 64 * WN rows per stage (LRT: W_mu and sigma^2).
template <auto Kernel, int WN, int WM, int KG, bool WS, int WT, class Args>
int launch_cfg(const Args& a, int64_t blocks, hipStream_t st) {
    using namespace bf16_plan;
    constexpr int kThreads = 64 * WN * WM * KG + (WS ? 256 : 0);
    constexpr int kStageB = (BK * (64 * WM + 32) + WT * 64 * WN * LDWB) * 2;
    constexpr int kSmem = KG * (WS ? 2 : 1) * kStageB + 4 * KCH * KG * 4;
    constexpr int kRed = (KG - 1) * 64 * (64 * WN * WM) * 4;      // (LRT: one moment at a time)
    static_assert(kRed <= KG * kStageB, "reduction buffer must fit in the stage memory");
    static_assert(kSmem <= 160 * 1024, "LDS");
    static_assert(WN * WM * 64 * 72 * 2 <= kStageB, "epilogue staging must fit in one stage");
    static_assert(kThreads <= 512, "256 registers per wave");
    static SmemAttrState attr_state;                              // (one per kernel instantiation)
    if (const int rc = ensure_dynamic_smem(reinterpret_cast<const void*>(Kernel), kSmem, attr_state)) return rc;
    hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3(kThreads), kSmem, st, a);
    return (int)hipGetLastError();
}

}  // namespace
