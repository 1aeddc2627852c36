// Host-side plan of the pooling launches of csrc/pool2d.hip and csrc/pool2d_bf16.hip: everything bbb_avgpool_chwn /
// bbb_avgpool_act_bwd_chwn / bbb_lrt_avgpool_act_bwd_chwn (fp32 planes: plan) and bbb_avgpool_chwn_bf16 / bbb_avgpool_act_bwd_chwn_bf16
// (bf16 planes: plan_bf16) decide before they touch a pointer or a stream -- the descriptor checks, the output map, the two grids.
// The launch entries and bbb_avgpool_plan / bbb_avgpool_bf16_plan call the same functions; the two plans are one function
// (plan_groups) at the image-group width of their 16-byte vectors, 4 fp32 or 8 bf16.
// Plain C++17, no HIP headers: tests/host/pool_plan_check.cpp walks this file under the sanitizers.
#ifndef BBB_POOL_PLAN_H
#define BBB_POOL_PLAN_H

#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "conv_desc_check.h"

namespace pool_plan {

using conv_desc_check::mul_cap;

constexpr int kThreads = 256;        // one thread per 16-byte group of images (4 fp32, 8 bf16)

struct Plan {
    int32_t ho, wo;                  // the output map, floor mode: (n + 2 pad - k) / stride + 1
    int32_t b4;                      // 16-byte groups per row of images (groups of `group` images: the names date from the fp32 plan)
    int64_t fwd_total4, bwd_total4;  // threads of the forward (one per output group) and of the backward (one per input group)
    int64_t fwd_blocks, bwd_blocks;  // their grids, kThreads threads per workgroup
};

// The checks, in this order (group = images per 16-byte vector).  BBB_EINVAL: a null descriptor, an unknown kind, a non-positive
// size, a negative padding, a count_include_pad that is neither 0 nor 1.  BBB_ESHAPE: batch % group != 0 (images move as 16-byte vectors); 2 * pad > k on an axis
// (torch's rule: with it every window holds a valid tap, so the divisor is never 0); a window larger than the padded map; a map
// whose padded extent leaves the int range; a grid that does not fit an int.  Last, BBB_EINVAL: a backward output pitch
// (out_plane_pitch, elements; 0 = dense) below one plane or not a multiple of group.
inline int plan_groups(const bbb_pool_desc_t* d, int64_t planes, int64_t out_plane_pitch, int group, Plan* p) {
    *p = Plan{};
    if (d == nullptr || d->kind != BBB_POOL_AVG) return BBB_EINVAL;
    if (planes <= 0 || d->h <= 0 || d->w <= 0 || d->batch <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride_h <= 0 || d->stride_w <= 0 ||
        d->pad_h < 0 || d->pad_w < 0 || (d->count_include_pad != 0 && d->count_include_pad != 1))
        return BBB_EINVAL;
    if (d->batch % group != 0) return BBB_ESHAPE;
    if (2 * (int64_t)d->pad_h > d->kh || 2 * (int64_t)d->pad_w > d->kw) return BBB_ESHAPE;
    const int64_t hp = (int64_t)d->h + 2 * (int64_t)d->pad_h, wp = (int64_t)d->w + 2 * (int64_t)d->pad_w;
    if (d->kh > hp || d->kw > wp) return BBB_ESHAPE;
    if (hp + d->kh > 0x7fffffffLL || wp + d->kw > 0x7fffffffLL) return BBB_ESHAPE;     // the kernels' row / column sums stay ints
    p->ho = (int32_t)((hp - d->kh) / d->stride_h + 1);
    p->wo = (int32_t)((wp - d->kw) / d->stride_w + 1);
    p->b4 = d->batch / group;
    p->fwd_total4 = mul_cap(planes, p->ho, p->wo, p->b4);
    p->bwd_total4 = mul_cap(planes, d->h, d->w, p->b4);
    if (p->fwd_total4 > 0x7fffffffLL * kThreads || p->bwd_total4 > 0x7fffffffLL * kThreads) return BBB_ESHAPE;
    p->fwd_blocks = (p->fwd_total4 + kThreads - 1) / kThreads;
    p->bwd_blocks = (p->bwd_total4 + kThreads - 1) / kThreads;
    if (out_plane_pitch != 0 && (out_plane_pitch < (int64_t)d->h * d->w * d->batch || out_plane_pitch % group != 0)) return BBB_EINVAL;
    return 0;
}

// fp32 planes: 4 images per 16-byte vector
inline int plan(const bbb_pool_desc_t* d, int64_t planes, int64_t out_plane_pitch, Plan* p) {
    return plan_groups(d, planes, out_plane_pitch, 4, p);
}

// bf16 planes: 8 images per 16-byte vector (batch % 8 != 0: BBB_ESHAPE; a pitch with % 8 != 0: BBB_EINVAL)
inline int plan_bf16(const bbb_pool_desc_t* d, int64_t planes, int64_t out_plane_pitch, Plan* p) {
    return plan_groups(d, planes, out_plane_pitch, 8, p);
}

}  // namespace pool_plan

#endif
