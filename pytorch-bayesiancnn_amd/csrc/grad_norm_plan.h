// Host-side launch plan of the global gradient norm (csrc/grad_norm.hip; the entries bbb_grad_sumsq and bbb_grad_norm_finish): the
// argument checks with the codes of csrc/adam_plan.h, the 4096-element chunks of every segment (chunk_begin[], the grid; one float64
// partial per chunk, stored at partials[first + chunk]), and, per segment, whether the gradient can be read 16 bytes at a time.
// Plain C++17, no HIP headers: the launch entries take their shape from here, bbb_grad_sumsq_plan / bbb_grad_norm_finish_plan report
// it, and tests/host/grad_norm_plan_check.cpp walks it under the sanitizers.
#ifndef BBB_GRAD_NORM_PLAN_H
#define BBB_GRAD_NORM_PLAN_H

#include <math.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"

#if defined(__HIPCC__)
#define BBB_GRAD_NORM_HD __host__ __device__
#else
#define BBB_GRAD_NORM_HD
#endif

namespace grad_norm_plan {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;                       // four quads per thread, kThreads * 4 elements apart
constexpr int kChunk = kThreads * kPerThread;        // elements of a block: 4096 (AlexNet's parameters: about a thousand partials)
constexpr int64_t kMaxPartials = 0x7fffffffLL;       // gridDim.x, and the partial index is an int
constexpr double kNormEps = 1e-6;                    // torch.nn.utils.clip_grad_norm_: max_norm / (norm + 1e-6)

struct Plan {
    int32_t chunks;                                  // gridDim.x = partials written
    int32_t chunk_begin[BBB_MAX_SEGMENTS + 1];       // first chunk of segment s; [nseg .. 16] = chunks
    int32_t vec[BBB_MAX_SEGMENTS];                   // 1: grad is 16-byte aligned and n >= 4 (some thread loads a quad)
};

// Only grad and n of a segment are looked at (the other three pointers may be anything).  A refusal leaves *p zeroed.
inline int plan(const bbb_adam_segment_t* segs, int nseg, const void* partials, int64_t first, Plan* p) {
    *p = Plan{};
    if (segs == nullptr || nseg <= 0 || nseg > BBB_MAX_SEGMENTS || partials == nullptr || first < 0) return BBB_EINVAL;
    if (((uintptr_t)partials & 7u) != 0) return BBB_EALIGN;
    Plan q = {};
    int64_t chunks = 0;
    for (int s = 0; s < nseg; ++s) {
        const bbb_adam_segment_t& g = segs[s];
        if (g.grad == nullptr || g.n <= 0) return BBB_EINVAL;
        if (((uintptr_t)g.grad & 3u) != 0) return BBB_EALIGN;
        q.chunk_begin[s] = (int32_t)chunks;
        const int64_t c = (g.n - 1) / kChunk + 1;    // ceil(n / 4096) without n + 4095, which overflows next to INT64_MAX
        if (c > kMaxPartials - chunks || first > kMaxPartials - chunks - c) return BBB_ESHAPE;
        chunks += c;
        q.vec[s] = (((uintptr_t)g.grad & 15u) == 0 && g.n >= 4) ? 1 : 0;
    }
    for (int s = nseg; s <= BBB_MAX_SEGMENTS; ++s) q.chunk_begin[s] = (int32_t)chunks;
    q.chunks = (int32_t)chunks;
    *p = q;
    return 0;
}

// The finish launch: checks only (one block, whatever npartials is).
inline int finish_check(const void* partials, int64_t npartials, double max_norm, const void* norm_out, const void* coef_out,
                        const void* ok_out, const void* skipped_out) {
    if (partials == nullptr || norm_out == nullptr || npartials <= 0) return BBB_EINVAL;
    if (((uintptr_t)partials & 7u) != 0) return BBB_EALIGN;
    if ((((uintptr_t)norm_out | (uintptr_t)coef_out | (uintptr_t)ok_out | (uintptr_t)skipped_out) & 3u) != 0) return BBB_EALIGN;
    if (!(max_norm > 0.0)) return BBB_EINVAL;        // <= 0 or NaN; +inf = "norm only"
    if (npartials > kMaxPartials) return BBB_ESHAPE;
    return 0;
}

// The coefficient from the fp32 norm: torch's min(1, max_norm / (norm + 1e-6)) in double, rounded to fp32 once.  The comparison is
// written out: a NaN norm gives a NaN coefficient (fmin would return 1), an Inf norm gives 0, and "nothing clipped" is exactly 1.0f.
// max_norm = +inf is "norm only": 1 for every norm that is not NaN.
BBB_GRAD_NORM_HD inline float coefficient(float norm, double max_norm) {
    const double nd = (double)norm;
    if (nd != nd) return (float)nd;
    if (max_norm == INFINITY) return 1.0f;
    const double c = max_norm / (nd + kNormEps);
    return c < 1.0 ? (float)c : 1.0f;
}

}  // namespace grad_norm_plan

#endif
