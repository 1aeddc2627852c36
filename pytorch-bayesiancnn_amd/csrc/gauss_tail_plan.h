// Host-side launch plan of the Gaussian-likelihood tail on batch-innermost logits (csrc/gauss_tail.hip; the entries bbb_gauss_elbo_cb_fwd,
// bbb_gauss_elbo_cb_bwd, bbb_gauss_moments_cb and their *_plan twins): the argument checks in their documented order, the lanes of a
// block, the blocks and the LDS bytes.  Plain C++17, no HIP headers: the launches take their shape from here and from nowhere else, and
// tests/host/gauss_tail_plan_check.cpp walks it under the sanitizers.
#ifndef BBB_GAUSS_TAIL_PLAN_H
#define BBB_GAUSS_TAIL_PLAN_H

#include <stdint.h>

#include "../../include/bbb_hip.h"

namespace gauss_tail_plan {

constexpr int kThreads = 64;                          // images of a block (one per lane)
constexpr int kTile = 16;                             // target dimensions of one staged tile of y
constexpr int kPitch = kTile + 1;                     // floats between two images of the tile (odd: no bank conflicts)
constexpr int kLdsBytes = kThreads * kPitch * 4;      // the staged tile of y, static: 4352
constexpr int kLossThreads = 256;                     // the forward's second launch: ONE block adds LL [B] in a fixed order
constexpr int kMaxDraws = 512;
constexpr int kMaxChannels = 1024;
constexpr int kMoments = 5;                           // mean, epistemic, aleatoric, total [B][D]; log_density [B]

struct Shape {
    int draws, batch, channels, dims;                 // logits [draws][channels][batch], y [batch][dims]
    double noise_sigma;                               // read when channels == dims (homoscedastic) only
    float log_var_min, log_var_max;
    int mc, mean_over;                                // mc: 0 = logmeanexp, 1 = mean
};

struct Plan {
    int32_t threads;     // blockDim.x
    int32_t blocks;      // gridDim.x: 64 images each
    int32_t lds_bytes;   // static LDS of a block
    int32_t hetero;      // 1: channels == 2 * dims (the log-variance is the second half of the channels)
};

// BBB_EINVAL part that the three entries share (after their pointers): sizes, the form, the clamp, noise_sigma, mc, mean_over.
inline bool shape_valid(const Shape& s) {
    if (s.draws <= 0 || s.batch <= 0 || s.channels <= 0 || s.dims <= 0) return false;
    const bool hetero = (int64_t)s.channels == 2 * (int64_t)s.dims;
    if (!hetero && s.channels != s.dims) return false;
    if (!(s.log_var_min <= s.log_var_max)) return false;                       // (a NaN edge is refused too)
    if (!hetero && !(s.noise_sigma > 0.0 && s.noise_sigma <= 1.7976931348623157e308)) return false;
    if (s.mc != 0 && s.mc != 1) return false;
    return s.mean_over >= 0;
}

inline int finish(const Shape& s, uintptr_t all_pointers, Plan* p) {
    if ((all_pointers & 3u) != 0) return BBB_EALIGN;
    if (s.draws > kMaxDraws || s.channels > kMaxChannels || s.batch > INT32_MAX - (kThreads - 1)) return BBB_ESHAPE;
    p->threads = kThreads;
    p->blocks = (s.batch + kThreads - 1) / kThreads;
    p->lds_bytes = kLdsBytes;
    p->hetero = (int64_t)s.channels == 2 * (int64_t)s.dims ? 1 : 0;
    return 0;
}

// Order of the checks, the same in all three: BBB_EINVAL (a required pointer that is null; a size that is not positive; channels
// neither dims nor 2 * dims; log_var_min > log_var_max; homoscedastic with a noise_sigma that is not finite and positive; mc outside
// {0, 1}; mean_over < 0), BBB_EALIGN (a pointer, optional ones included, that is not a multiple of 4), BBB_ESHAPE (draws > 512,
// channels > 1024, a batch whose image index blockIdx.x * 64 + lane leaves int).
// Forward: logits, y, kl, ll_out, loss_out required; beta_dev optional.
inline int plan_fwd(const void* logits, const void* y, const void* kl, const void* beta_dev, const void* ll_out, const void* loss_out,
                    const Shape& s, Plan* p) {
    *p = Plan{};
    if (logits == nullptr || y == nullptr || kl == nullptr || ll_out == nullptr || loss_out == nullptr || !shape_valid(s))
        return BBB_EINVAL;
    return finish(s, (uintptr_t)logits | (uintptr_t)y | (uintptr_t)kl | (uintptr_t)beta_dev | (uintptr_t)ll_out | (uintptr_t)loss_out, p);
}

// Backward: logits, y, g_loss, g_logits required; beta_dev and g_kl optional.
inline int plan_bwd(const void* logits, const void* y, const void* g_loss, const void* beta_dev, const void* g_logits, const void* g_kl,
                    const Shape& s, Plan* p) {
    *p = Plan{};
    if (logits == nullptr || y == nullptr || g_loss == nullptr || g_logits == nullptr || !shape_valid(s)) return BBB_EINVAL;
    return finish(s, (uintptr_t)logits | (uintptr_t)y | (uintptr_t)g_loss | (uintptr_t)beta_dev | (uintptr_t)g_logits | (uintptr_t)g_kl, p);
}

// Moments: logits required; at least one output wanted; log_density (outs[4]) needs y.  s.mc and s.mean_over are 0.
inline int plan_moments(const void* logits, const void* y, const void* const outs[kMoments], const Shape& s, Plan* p) {
    *p = Plan{};
    uintptr_t any = 0;
    for (int i = 0; i < kMoments; ++i) any |= (uintptr_t)outs[i];
    if (logits == nullptr || any == 0 || (outs[4] != nullptr && y == nullptr) || !shape_valid(s)) return BBB_EINVAL;
    return finish(s, (uintptr_t)logits | (uintptr_t)y | any, p);
}

}  // namespace gauss_tail_plan

#endif
