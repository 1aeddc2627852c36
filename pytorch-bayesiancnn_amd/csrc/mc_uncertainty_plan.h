// Host-side launch plan of the batch-innermost uncertainty reduction (mc_uncertainty_cb_kernel in csrc/mc_uncertainty.hip; the entries
// bbb_mc_uncertainty_cb and bbb_mc_uncertainty_cb_plan): the argument checks, the largest number of draws one launch takes, the rows of
// the block, the blocks and the dynamic LDS bytes.  Plain C++17, no HIP headers: the launch takes its shape from here and
// tests/host/mc_uncertainty_plan_check.cpp walks it under the sanitizers.
#ifndef BBB_MC_UNCERTAINTY_PLAN_H
#define BBB_MC_UNCERTAINTY_PLAN_H

#include <stdint.h>

#include "../../include/bbb_hip.h"

namespace mc_uncertainty_plan {

constexpr int kThreads = 64;                          // images of a block (one per lane)
constexpr int kRows = 16;                             // rows of a block at most: draws in phase 1, classes in phase 2
constexpr int kOutputs = 7;                           // pred, p_mean, epistemic, aleatoric, entropy, expected_entropy, mutual_info
constexpr int kLdsBytesPerDraw = 3 * kThreads * 4;    // per (draw, image): the row's maximum (normalized: its softplus sum), its log
                                                      // partition and the entropy H[p_t] of the draw
constexpr int kLdsBytesReduce = 2 * kRows * kThreads * 4;   // per (row, image): the row's share of sum_c p_bar log p_bar and of the KL sum
constexpr int kMaxLdsBytes = 160 * 1024;              // LDS of a gfx950 workgroup
constexpr int kDefaultLdsBytes = 64 * 1024;           // dynamic LDS a launch may ask for without the per-kernel attribute
constexpr int kMaxDraws = (kMaxLdsBytes - kLdsBytesReduce) / kLdsBytesPerDraw;      // 202

struct Plan {
    int32_t rows;        // blockDim.y
    int32_t blocks;      // gridDim.x: 64 images each
    int32_t lds_bytes;   // dynamic LDS of the launch: draws * 768 + 8192
};

// Order of the checks: BBB_EINVAL (null logits, a size that is not positive, no output wanted), BBB_EALIGN (a pointer that is not a
// multiple of 4), BBB_ESHAPE (a batch whose image index blockIdx.x * 64 + lane leaves int, more draws than the LDS holds).
inline int plan(const void* logits, int draws, int batch, int classes, const void* const outs[kOutputs], Plan* p) {
    *p = Plan{};
    uintptr_t any = 0;
    for (int i = 0; i < kOutputs; ++i) any |= (uintptr_t)outs[i];
    if (logits == nullptr || draws <= 0 || batch <= 0 || classes <= 0 || any == 0) return BBB_EINVAL;
    if ((((uintptr_t)logits | any) & 3u) != 0) return BBB_EALIGN;
    if (batch > INT32_MAX - (kThreads - 1) || draws > kMaxDraws) return BBB_ESHAPE;
    const int mx = draws > classes ? draws : classes;
    p->rows = mx < kRows ? mx : kRows;
    p->blocks = (batch + kThreads - 1) / kThreads;
    p->lds_bytes = draws * kLdsBytesPerDraw + kLdsBytesReduce;
    return 0;
}

// ---- the backward (mc_uncertainty_cb_bwd_kernel; the entries bbb_mc_uncertainty_cb_bwd and bbb_mc_uncertainty_cb_bwd_plan) ----
// With the forward's p_mean as an input a (draw, image) pair needs nothing from any other pair: one thread per pair walks its C classes
// (compensated sums), blockDim = (64 images, 1), gridDim = (ceil(batch / 64), draws) -- bs = 512 with 15 draws is 120 workgroups where
// the forward has 8 -- no LDS, no barrier, no atomics.  The draw limit stays the forward's kMaxDraws: the design needs no smaller one,
// and a p_mean over more draws has no launch that could have written it.
constexpr int kUpstreams = 7;                         // w_pred, w_p_mean, w_epistemic, w_aleatoric [B][C]; w_entropy, w_expected_entropy,
                                                      // w_mutual_info [B]; NULL = zero
constexpr int kBwdRows = 1;                           // draws of a block
constexpr int kBwdLdsBytes = 0;

// Order of the checks: BBB_EINVAL (null logits, null p_mean, null d_logits, a size that is not positive, all seven upstream gradients
// null), BBB_EALIGN (a pointer that is not a multiple of 4), BBB_ESHAPE (a batch whose image index blockIdx.x * 64 + lane leaves int,
// more draws than kMaxDraws).  p->blocks is gridDim.x; gridDim.y = draws.
inline int plan_bwd(const void* logits, const void* p_mean, int draws, int batch, int classes, const void* const ups[kUpstreams],
                    const void* d_logits, Plan* p) {
    *p = Plan{};
    uintptr_t any = 0;
    for (int i = 0; i < kUpstreams; ++i) any |= (uintptr_t)ups[i];
    if (logits == nullptr || p_mean == nullptr || d_logits == nullptr || draws <= 0 || batch <= 0 || classes <= 0 || any == 0)
        return BBB_EINVAL;
    if ((((uintptr_t)logits | (uintptr_t)p_mean | (uintptr_t)d_logits | any) & 3u) != 0) return BBB_EALIGN;
    if (batch > INT32_MAX - (kThreads - 1) || draws > kMaxDraws) return BBB_ESHAPE;
    p->rows = kBwdRows;
    p->blocks = (batch + kThreads - 1) / kThreads;
    p->lds_bytes = kBwdLdsBytes;
    return 0;
}

}  // namespace mc_uncertainty_plan

#endif
