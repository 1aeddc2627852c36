// Host-side launch plan of the batch-innermost Monte-Carlo tail (mc_tail_cb_kernel in csrc/mc_tail.hip; the entries
// bbb_mc_tail_cb / _units / _units_step / _groups_step / _share_step): the argument checks, the draws an image reduces over at most
// (per_slice), the rows of the block (ny), the blocks and the dynamic LDS bytes.  Plain C++17, no HIP headers: mc_tail_launch takes
// its launch shape from here and tests/host/mc_tail_plan_check.cpp walks it under the sanitizers.
#ifndef BBB_MC_TAIL_PLAN_H
#define BBB_MC_TAIL_PLAN_H

#include <stdint.h>

#include "../../include/bbb_hip.h"

namespace mc_tail_plan {

constexpr int kCbThreads = 64;                       // images of a block (one per lane)
constexpr int kCbRows = 16;                          // rows of a block at most: draws in phase 1, classes in phase 2
constexpr int kMaxUnits = 4096;                      // slabs of one launch
constexpr int kLdsBytesPerSlice = kCbThreads * 4;    // one float per (local draw, image): log sum-exp of the draw's row (and, where
                                                     // both fit, as many bytes again for the row's maximum)
constexpr int kMaxLdsBytes = 160 * 1024;             // LDS of a gfx950 workgroup
constexpr int kDefaultLdsBytes = 64 * 1024;          // dynamic LDS a launch may ask for without the per-kernel attribute
constexpr int kMaxPerSlice = kMaxLdsBytes / kLdsBytesPerSlice;      // 640 draws reduced into one image
constexpr int kMaxPerSliceKeepMax = kMaxPerSlice / 2;               // up to 320 the row maxima stay in LDS too

struct Plan {
    int32_t per_slice;   // local draws an image reduces over, at most
    int32_t ny;          // blockDim.y
    int32_t blocks;      // gridDim.x: 64 images each
    int32_t keep_max;    // 1: the row maxima are kept in LDS behind the log sum-exps; 0: phase 2 of the kernel finds them again
    int32_t lds_bytes;   // dynamic LDS of the launch: per_slice * 256 for the log sum-exps, twice that with keep_max
};

// grp == 0: work units (unit u = unit_off + e: draw u / slices, batch slice u % slices); grp > 0: `slices` steps of grp draws each,
// the launch holding slabs goff .. goff + units - 1 of their draw-major enumeration.
inline int plan(const void* logits, const void* lse_out, const void* kl_in, const void* kl_out, const void* counter, int units, int slices,
                int unit_off, int batch_slice, int classes, int mean_over, int grp, int goff, Plan* p) {
    *p = Plan{};
    if ((kl_out != nullptr && kl_in == nullptr) || (((uintptr_t)kl_in | (uintptr_t)kl_out | (uintptr_t)counter) & 3u) != 0) return BBB_EINVAL;
    if (logits == nullptr || lse_out == nullptr || units <= 0 || slices <= 0 || unit_off < 0 || batch_slice <= 0 || classes <= 0 ||
        mean_over < 0 || units > kMaxUnits || grp < 0 || goff < 0 || (grp > 0 && (goff >= grp || (int64_t)grp * slices < (int64_t)units + goff)))
        return BBB_EINVAL;
    if ((((uintptr_t)logits | (uintptr_t)lse_out) & 3u) != 0) return BBB_EALIGN;
    const int64_t batch = (int64_t)batch_slice * slices;
    // (the kernel's image index blockIdx.x * 64 + lane, its slab bounds (step + 1) * grp and its unit count units - e0 + slices - 1
    // are ints)
    if (batch > INT32_MAX - (kCbThreads - 1) || (int64_t)grp * slices > INT32_MAX || (int64_t)units + slices > INT32_MAX) return BBB_ESHAPE;
    const int64_t per_slice = grp > 0 ? grp : ((int64_t)units + slices - 1) / slices;
    if (per_slice > kMaxPerSlice) return BBB_ESHAPE;          // more LDS than a workgroup has
    const int mx = per_slice > classes ? (int)per_slice : classes;
    p->per_slice = (int32_t)per_slice;
    p->ny = mx < kCbRows ? mx : kCbRows;
    p->blocks = (int32_t)((batch + kCbThreads - 1) / kCbThreads);
    p->keep_max = per_slice <= kMaxPerSliceKeepMax ? 1 : 0;
#ifdef BBB_TAIL_NEVER_KEEP_MAX       // timing experiments (profiles/tail_sweep_timing.py): phase 2 finds the maxima again at any draw count
    p->keep_max = 0;
#endif
    p->lds_bytes = (int32_t)per_slice * kLdsBytesPerSlice * (p->keep_max ? 2 : 1);
    return 0;
}

}  // namespace mc_tail_plan

#endif
