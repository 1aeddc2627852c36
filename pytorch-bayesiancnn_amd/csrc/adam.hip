// Multi-tensor Adam step for the (mu, rho) parameter pairs of the Bayesian layers (training extension):
// one launch updates up to 16 tensors.  Same update, in the same operation order, as torch.optim.Adam with
// amsgrad=False, weight_decay=0, maximize=False -- what main_bayesian.py:103 constructs:
//     m <- m + (g - m) * (1 - beta1)                     (lerp)
//     v <- v * beta2 + (1 - beta2) * g * g               (mul, addcmul)
//     p <- p - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),   bc1 = 1 - beta1^t, bc2 = 1 - beta2^t
// HBM traffic per element: 16 B read + 12 B written; purely bandwidth-bound.
// The argument checks, the chunk walk and the host-path scalars live in csrc/adam_plan.h (host only; bbb_adam_step_plan reports them).
// bbb_adam_step_ex is the same kernel body with compile-time switches: weight decay (L2: g <- g + wd p; decoupled: p <- p (1 - lr wd)
// before the update), an optional DEVICE clip coefficient (g <- coef g, from bbb_grad_norm_finish) and an optional DEVICE flag that makes
// the launch store nothing (a skipped non-finite step).  The gradient is only ever read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "adam_plan.h"

namespace {

constexpr int kThreads = adam_plan::kThreads;
constexpr int kChunk = adam_plan::kChunk;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct AdamArgs {
    bbb_adam_segment_t seg[BBB_MAX_SEGMENTS];
    int32_t chunk_begin[BBB_MAX_SEGMENTS + 1];
    int32_t nseg;
    float step_size, beta1, beta2, omb1, omb2, eps, sqrt_bc2;
    double lr_d, beta1_d, beta2_d;
    const float* step_dev;
    const float* lr_dev;       // optional DEVICE learning rate (captured graphs: schedulers change lr between replays)
};

// bbb_adam_step_ex: the same arguments plus weight decay and the device scalars of a clipped / guarded step
struct AdamArgsEx : AdamArgs {
    int32_t mode;              // adam_plan::PlanEx::mode: 0 no decay, 1 L2, 2 decoupled
    float wd32, decay;
    double wd_d;
    const float* coef_dev;     // optional DEVICE clip coefficient (bbb_grad_norm_finish): g <- coef g, one rounding
    const float* ok_dev;       // optional DEVICE 0.0 / 1.0: 0 = this step stores nothing
};

// One rounding each, whatever the contraction mode of the translation unit: the products and sums the contract states as separate
// roundings must not be fused into the update lines behind them (HIP's __fmul_rn / __fadd_rn are plain operators and can be).
__device__ inline float mul_rn(float x, float y) {
#pragma clang fp contract(off)
    return x * y;
}
__device__ inline float add_rn(float x, float y) {
#pragma clang fp contract(off)
    return x + y;
}

// ONE body for both entries.  kEx is a compile-time switch: without it the body is bbb_adam_step's as it always was; with it the
// extra operations sit in front of the unchanged update lines, each an exact identity when its option is neutral (coef 1, no decay).
template <class Args>
__global__ __launch_bounds__(kThreads) void adam_step_kernel(const Args a) {
    constexpr bool kEx = sizeof(Args) != sizeof(AdamArgs);
    const int chunk = blockIdx.x;
    float step_size = a.step_size, sqrt_bc2 = a.sqrt_bc2;
    [[maybe_unused]] float coef = 1.0f, decay = 1.0f;
    if constexpr (kEx) decay = a.decay;
    bool device_scalars = a.step_dev != nullptr;
    if constexpr (kEx) device_scalars = device_scalars || a.coef_dev != nullptr || a.ok_dev != nullptr;
    if (device_scalars) {              // captured graph: the step count lives on the device; one thread derives the scalars
        __shared__ float sc[5];
        if (threadIdx.x == 0) {
            if (a.step_dev != nullptr) {
                const double t = (double)*a.step_dev;
                const double lr = a.lr_dev != nullptr ? (double)*a.lr_dev : a.lr_d;
                sc[0] = (float)(lr / (1.0 - pow(a.beta1_d, t)));
                sc[1] = (float)sqrt(1.0 - pow(a.beta2_d, t));
                if constexpr (kEx) sc[2] = (float)(1.0 - lr * a.wd_d);
            } else {
                sc[0] = step_size;
                sc[1] = sqrt_bc2;
                if constexpr (kEx) sc[2] = decay;
            }
            if constexpr (kEx) {
                sc[3] = a.coef_dev != nullptr ? *a.coef_dev : 1.0f;
                sc[4] = a.ok_dev != nullptr ? *a.ok_dev : 1.0f;
            }
        }
        __syncthreads();
        step_size = sc[0];
        sqrt_bc2 = sc[1];
        if constexpr (kEx) {
            decay = sc[2];
            coef = sc[3];
            if (sc[4] == 0.0f) return;          // a skipped step: before the first store (block-uniform)
        }
    }
    int s = 0;
    while (s + 1 < a.nseg && chunk >= a.chunk_begin[s + 1]) ++s;
    const bbb_adam_segment_t sg = a.seg[s];
    const int64_t i0 = (int64_t)(chunk - a.chunk_begin[s]) * kChunk + (int64_t)threadIdx.x * 4;
    if (i0 >= sg.n) return;
    const int cnt = (sg.n - i0) >= 4 ? 4 : (int)(sg.n - i0);
    const bool vec = cnt == 4 && ((((uintptr_t)sg.param | (uintptr_t)sg.grad | (uintptr_t)sg.exp_avg | (uintptr_t)sg.exp_avg_sq) & 15u) == 0);
    float p[4], g[4], m[4], v[4];
    if (vec) {
        const f32x4 p4 = *reinterpret_cast<const f32x4*>(sg.param + i0), g4 = *reinterpret_cast<const f32x4*>(sg.grad + i0);
        const f32x4 m4 = *reinterpret_cast<const f32x4*>(sg.exp_avg + i0), v4 = *reinterpret_cast<const f32x4*>(sg.exp_avg_sq + i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) { p[j] = p4[j]; g[j] = g4[j]; m[j] = m4[j]; v[j] = v4[j]; }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = j < cnt;
            p[j] = ok ? sg.param[i0 + j] : 0.0f; g[j] = ok ? sg.grad[i0 + j] : 0.0f;
            m[j] = ok ? sg.exp_avg[i0 + j] : 0.0f; v[j] = ok ? sg.exp_avg_sq[i0 + j] : 0.0f;
        }
    }
    if constexpr (kEx) {               // explicit roundings (no contraction into the lines below): the contract states each one
        if (a.coef_dev != nullptr) {
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = mul_rn(coef, g[j]);
        }
        if (a.mode == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = add_rn(g[j], mul_rn(a.wd32, p[j]));
        } else if (a.mode == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = mul_rn(p[j], decay);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[j] = m[j] + (g[j] - m[j]) * a.omb1;
        v[j] = v[j] * a.beta2 + a.omb2 * g[j] * g[j];
        const float denom = __fdiv_rn(__fsqrt_rn(v[j]), sqrt_bc2) + a.eps;
        p[j] = p[j] - step_size * (m[j] / denom);
    }
    if (vec) {
        f32x4 p4, m4, v4;
#pragma unroll
        for (int j = 0; j < 4; ++j) { p4[j] = p[j]; m4[j] = m[j]; v4[j] = v[j]; }
        *reinterpret_cast<f32x4*>(sg.param + i0) = p4;
        *reinterpret_cast<f32x4*>(sg.exp_avg + i0) = m4;
        *reinterpret_cast<f32x4*>(sg.exp_avg_sq + i0) = v4;
    } else {
        for (int j = 0; j < cnt; ++j) { sg.param[i0 + j] = p[j]; sg.exp_avg[i0 + j] = m[j]; sg.exp_avg_sq[i0 + j] = v[j]; }
    }
}

template <class Args>
void fill_args(Args& a, const bbb_adam_segment_t* segs, int nseg, const adam_plan::Plan& p, double lr, double beta1, double beta2,
               const float* step_dev, const float* lr_dev) {
    for (int s = 0; s < nseg; ++s) a.seg[s] = segs[s];
    for (int s = 0; s <= BBB_MAX_SEGMENTS; ++s) a.chunk_begin[s] = p.chunk_begin[s];
    a.nseg = nseg;
    a.step_size = p.step_size; a.sqrt_bc2 = p.sqrt_bc2;
    a.beta1 = p.beta1; a.beta2 = p.beta2; a.omb1 = p.omb1; a.omb2 = p.omb2; a.eps = p.eps;
    a.lr_d = lr; a.beta1_d = beta1; a.beta2_d = beta2; a.step_dev = step_dev; a.lr_dev = lr_dev;
}

}  // namespace

extern "C" int bbb_adam_step(const bbb_adam_segment_t* segs, int nseg, double lr, double beta1, double beta2, double eps,
                             int64_t step, const float* step_dev, const float* lr_dev, void* stream) {
    adam_plan::Plan p;
    const int rc = adam_plan::plan(segs, nseg, lr, beta1, beta2, eps, step, step_dev, lr_dev, &p);
    if (rc != 0) return rc;
    AdamArgs a = {};
    fill_args(a, segs, nseg, p, lr, beta1, beta2, step_dev, lr_dev);
    hipLaunchKernelGGL(adam_step_kernel<AdamArgs>, dim3(p.chunks), dim3(kThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int bbb_adam_step_ex(const bbb_adam_segment_t* segs, int nseg, double lr, double beta1, double beta2, double eps,
                                double weight_decay, int decoupled, int64_t step, const float* step_dev, const float* lr_dev,
                                const float* coef_dev, const float* ok_dev, void* stream) {
    adam_plan::PlanEx p;
    const int rc = adam_plan::plan_ex(segs, nseg, lr, beta1, beta2, eps, weight_decay, decoupled, step, step_dev, lr_dev, coef_dev, ok_dev, &p);
    if (rc != 0) return rc;
    AdamArgsEx a = {};
    fill_args(a, segs, nseg, p.base, lr, beta1, beta2, step_dev, lr_dev);
    a.mode = p.mode; a.wd32 = p.wd32; a.decay = p.decay; a.wd_d = weight_decay; a.coef_dev = coef_dev; a.ok_dev = ok_dev;
    hipLaunchKernelGGL(adam_step_kernel<AdamArgsEx>, dim3(p.base.chunks), dim3(kThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// What bbb_adam_step launches for these arguments: the same plan, no launch, no device.  Out-pointers may be NULL; a refusal writes zeros.
extern "C" int bbb_adam_step_plan(const bbb_adam_segment_t* segs, int nseg, double lr, double beta1, double beta2, double eps,
                                  int64_t step, const float* step_dev, const float* lr_dev, int32_t* chunks, int32_t* chunk_begin,
                                  float* scalars, int32_t* vec) {
    adam_plan::Plan p;
    const int rc = adam_plan::plan(segs, nseg, lr, beta1, beta2, eps, step, step_dev, lr_dev, &p);
    if (chunks) *chunks = p.chunks;
    if (chunk_begin) for (int s = 0; s <= BBB_MAX_SEGMENTS; ++s) chunk_begin[s] = p.chunk_begin[s];
    if (scalars) {
        const float sc[7] = {p.step_size, p.sqrt_bc2, p.beta1, p.beta2, p.omb1, p.omb2, p.eps};
        for (int k = 0; k < 7; ++k) scalars[k] = sc[k];
    }
    if (vec) for (int s = 0; s < BBB_MAX_SEGMENTS; ++s) vec[s] = p.vec[s];
    return rc;
}

// The same for bbb_adam_step_ex: scalars[9] = the seven of bbb_adam_step_plan, then wd32 and decay; *mode: 0 no decay, 1 L2, 2 decoupled.
extern "C" int bbb_adam_step_ex_plan(const bbb_adam_segment_t* segs, int nseg, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, int decoupled, int64_t step, const float* step_dev, const float* lr_dev,
                                     const float* coef_dev, const float* ok_dev, int32_t* chunks, int32_t* chunk_begin, float* scalars,
                                     int32_t* vec, int32_t* mode) {
    adam_plan::PlanEx q;
    const int rc = adam_plan::plan_ex(segs, nseg, lr, beta1, beta2, eps, weight_decay, decoupled, step, step_dev, lr_dev, coef_dev, ok_dev, &q);
    const adam_plan::Plan& p = q.base;
    if (chunks) *chunks = p.chunks;
    if (chunk_begin) for (int s = 0; s <= BBB_MAX_SEGMENTS; ++s) chunk_begin[s] = p.chunk_begin[s];
    if (scalars) {
        const float sc[9] = {p.step_size, p.sqrt_bc2, p.beta1, p.beta2, p.omb1, p.omb2, p.eps, q.wd32, q.decay};
        for (int k = 0; k < 9; ++k) scalars[k] = sc[k];
    }
    if (vec) for (int s = 0; s < BBB_MAX_SEGMENTS; ++s) vec[s] = p.vec[s];
    if (mode) *mode = q.mode;
    return rc;
}
