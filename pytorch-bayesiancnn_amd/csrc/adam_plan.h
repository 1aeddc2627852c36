// Host-side launch plan of the multi-tensor Adam step (adam_step_kernel in csrc/adam.hip; the entry bbb_adam_step): the argument
// checks, the 1024-element chunks of every segment (chunk_begin[], the grid), the host-path scalars -- each formed in double and
// rounded to fp32 ONCE -- and, per segment, whether any thread can take the 16-byte path.  Plain C++17, no HIP headers: bbb_adam_step
// takes its launch shape and scalars from here, bbb_adam_step_plan reports them, and tests/host/adam_plan_check.cpp walks the plan
// under the sanitizers.
// plan_ex (bbb_adam_step_ex, bbb_adam_step_ex_plan) is plan() plus the weight-decay scalars and the checks of the two device scalars;
// tests/host/grad_norm_plan_check.cpp walks it.
#ifndef BBB_ADAM_PLAN_H
#define BBB_ADAM_PLAN_H

#include <math.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"

namespace adam_plan {

constexpr int kThreads = 256;
constexpr int kChunk = kThreads * 4;                 // elements of a block: 4 per thread
constexpr int64_t kMaxChunks = 0x7fffffffLL;         // gridDim.x, and the kernel's chunk index is an int

struct Plan {
    int32_t chunks;                                  // gridDim.x
    int32_t chunk_begin[BBB_MAX_SEGMENTS + 1];       // first chunk of segment s; [nseg .. 16] = chunks
    int32_t vec[BBB_MAX_SEGMENTS];                   // 1: the four pointers are jointly 16-byte aligned and n >= 4 (some thread moves a quad)
    int64_t step;                                    // the step the host scalars were formed at (1 when step_dev overrides a step <= 0)
    float step_size, sqrt_bc2, beta1, beta2, omb1, omb2, eps;
};

// A refusal leaves *p zeroed.  Addresses are only looked at, never read.
inline int plan(const bbb_adam_segment_t* segs, int nseg, double lr, double beta1, double beta2, double eps, int64_t step,
                const void* step_dev, const void* lr_dev, Plan* p) {
    *p = Plan{};
    if (segs == nullptr || nseg <= 0 || nseg > BBB_MAX_SEGMENTS || (step <= 0 && step_dev == nullptr)) return BBB_EINVAL;
    if (lr_dev != nullptr && step_dev == nullptr) return BBB_EINVAL;      // device-side lr goes with the device-side step count
    if ((((uintptr_t)step_dev | (uintptr_t)lr_dev) & 3u) != 0) return BBB_EALIGN;
    if (step <= 0) step = 1;
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return BBB_EINVAL;
    Plan q = {};
    int64_t chunks = 0;
    for (int s = 0; s < nseg; ++s) {
        const bbb_adam_segment_t& g = segs[s];
        if (g.param == nullptr || g.grad == nullptr || g.exp_avg == nullptr || g.exp_avg_sq == nullptr || g.n <= 0) return BBB_EINVAL;
        const uintptr_t bits = (uintptr_t)g.param | (uintptr_t)g.grad | (uintptr_t)g.exp_avg | (uintptr_t)g.exp_avg_sq;
        if ((bits & 3u) != 0) return BBB_EALIGN;
        q.chunk_begin[s] = (int32_t)chunks;
        const int64_t c = (g.n - 1) / kChunk + 1;    // ceil(n / 1024) without n + 1023, which overflows next to INT64_MAX
        if (c + chunks > kMaxChunks) return BBB_ESHAPE;
        chunks += c;
        q.vec[s] = ((bits & 15u) == 0 && g.n >= 4) ? 1 : 0;
    }
    for (int s = nseg; s <= BBB_MAX_SEGMENTS; ++s) q.chunk_begin[s] = (int32_t)chunks;
    q.chunks = (int32_t)chunks;
    q.step = step;
    // scalars in double on the host and rounded to fp32 once, as torch does with its Python-side hyper-parameters
    // (1 - 0.999 must become float(0.001), not 1.0f - 0.999f)
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    q.step_size = (float)(lr / bc1);
    q.sqrt_bc2 = (float)sqrt(bc2);
    q.beta1 = (float)beta1; q.beta2 = (float)beta2; q.omb1 = (float)(1.0 - beta1); q.omb2 = (float)(1.0 - beta2);
    q.eps = (float)eps;
    *p = q;
    return 0;
}

// The extended step (bbb_adam_step_ex): the same plan -- checks, chunk walk, vector rule and scalars are plan()'s own -- plus weight
// decay and the two optional device scalars of a clipped / guarded step.  mode 0: no decay (weight_decay == 0, either form: torch
// skips it too); 1: L2, g <- g + wd32 p; 2: decoupled, p <- p decay before the update.  wd32 = fp32(weight_decay); decay =
// fp32(1 - lr weight_decay) formed in double and rounded once (torch: param.mul_(1 - lr * weight_decay)); with lr_dev the kernel forms
// decay itself from the device rate.  Checks in this order: everything plan() checks, then coef_dev / ok_dev 4-byte aligned
// (BBB_EALIGN), then weight_decay >= 0 and not NaN (BBB_EINVAL).
struct PlanEx {
    Plan base;
    int32_t mode;
    float wd32, decay;
};

inline int plan_ex(const bbb_adam_segment_t* segs, int nseg, double lr, double beta1, double beta2, double eps, double weight_decay,
                   int decoupled, int64_t step, const void* step_dev, const void* lr_dev, const void* coef_dev, const void* ok_dev,
                   PlanEx* p) {
    *p = PlanEx{};
    Plan base;
    const int rc = plan(segs, nseg, lr, beta1, beta2, eps, step, step_dev, lr_dev, &base);
    if (rc != 0) return rc;
    if ((((uintptr_t)coef_dev | (uintptr_t)ok_dev) & 3u) != 0) return BBB_EALIGN;
    if (!(weight_decay >= 0.0)) return BBB_EINVAL;
    p->base = base;
    p->mode = weight_decay == 0.0 ? 0 : (decoupled ? 2 : 1);
    p->wd32 = (float)weight_decay;
    p->decay = (float)(1.0 - lr * weight_decay);
    return 0;
}

}  // namespace adam_plan

#endif
