// Host-side plan of the pooling launches of csrc/pool2d.hip (fp32 planes: plan) and csrc/pool2d_bf16.hip (bf16 planes: plan_bf16),
// maximum and average: everything an entry decides before it touches a pointer or a stream -- the descriptor checks, the output
// map, the two grids -- and the kernel-argument block that follows from them.  The descriptor-taking average entries, the scalar
// maximum entries (bbb_maxpool_chwn, bbb_pool_act_bwd_chwn, bbb_lrt_pool_act_bwd_chwn, bbb_maxpool_chwn_bf16,
// bbb_pool_act_bwd_chwn_bf16: they build the BBB_POOL_MAX descriptor of their scalars, max_desc) and bbb_avgpool_plan /
// bbb_avgpool_bf16_plan call the same functions; the two plans are one function (plan_groups) at the image-group width of their
// 16-byte vectors, 4 fp32 or 8 bf16.
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
// size, a negative padding, a count_include_pad that is neither 0 nor 1; kind BBB_POOL_MAX with anything but what the maximum kernels
// implement -- a square window, one stride, no padding, count_include_pad 0.  BBB_ESHAPE: batch % group != 0 (images move as 16-byte vectors); 2 * pad > k on an axis
// (torch's rule: with it every window holds a valid tap, so the divisor is never 0); a window larger than the padded map; a map
// whose padded extent leaves the int range (average kind: the maximum kernels keep no such sums); a grid that does not fit an int.  Last, BBB_EINVAL: a backward output pitch
// (out_plane_pitch, elements; 0 = dense) below one plane or not a multiple of group.
inline int plan_groups(const bbb_pool_desc_t* d, int64_t planes, int64_t out_plane_pitch, int group, Plan* p) {
    *p = Plan{};
    if (d == nullptr || (d->kind != BBB_POOL_AVG && d->kind != BBB_POOL_MAX)) return BBB_EINVAL;
    if (planes <= 0 || d->h <= 0 || d->w <= 0 || d->batch <= 0 || d->kh <= 0 || d->kw <= 0 || d->stride_h <= 0 || d->stride_w <= 0 ||
        d->pad_h < 0 || d->pad_w < 0 || (d->count_include_pad != 0 && d->count_include_pad != 1))
        return BBB_EINVAL;
    const bool avg = d->kind == BBB_POOL_AVG;
    if (!avg && (d->kh != d->kw || d->stride_h != d->stride_w || d->pad_h != 0 || d->pad_w != 0 || d->count_include_pad != 0)) return BBB_EINVAL;
    if (d->batch % group != 0) return BBB_ESHAPE;
    if (2 * (int64_t)d->pad_h > d->kh || 2 * (int64_t)d->pad_w > d->kw) return BBB_ESHAPE;
    const int64_t hp = (int64_t)d->h + 2 * (int64_t)d->pad_h, wp = (int64_t)d->w + 2 * (int64_t)d->pad_w;
    if (d->kh > hp || d->kw > wp) return BBB_ESHAPE;
    if (avg && (hp + d->kh > 0x7fffffffLL || wp + d->kw > 0x7fffffffLL)) return BBB_ESHAPE;     // the kernels' row / column sums stay ints
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

// The BBB_POOL_MAX descriptor of the scalar entries' (h, w, batch, k, s).  A backward entry's k == 0 (no pooling: the activation
// alone) is PLANNED as the 1 x 1 window at stride 1 -- the same map, the same grid -- and still launched with k = 0: the kernels add
// nothing there (0.0f + g is not g for g = -0.0f).  Where two of an entry's rules are broken at once, the order above decides.
// One single-violation code did move: the plan bounds both grids whichever launch asks, where bbb_maxpool_chwn bounded the forward's
// alone -- a forward over more than 2^31 - 1 workgroups' worth of INPUT groups (over 8 TB) is BBB_ESHAPE now.
inline bbb_pool_desc_t max_desc(int h, int w, int batch, int k, int s, bool k0_is_none) {
    bbb_pool_desc_t d = {};
    const bool none = k0_is_none && k == 0;
    d.kind = BBB_POOL_MAX;
    d.h = h; d.w = w; d.batch = batch;
    d.kh = d.kw = none ? 1 : k;
    d.stride_h = d.stride_w = none ? 1 : s;
    return d;
}

// The descriptor-taking launch entries are the average pool's (there are no descriptor-taking maximum entries): any other kind is to
// them what it always was, an unknown kind -- the null descriptor every plan refuses with BBB_EINVAL.
inline const bbb_pool_desc_t* avg_only(const bbb_pool_desc_t* d) { return d != nullptr && d->kind == BBB_POOL_AVG ? d : nullptr; }

// The average kernels' argument block (the maximum kernels take their scalars one by one, as they always did).
struct PoolArgs {
    int H, W, Ho, Wo, Bg;        // Bg: 16-byte groups per row of images
    int kh, kw, sh, sw, ph, pw;
    int cip;                     // count_include_pad: divide by kh * kw, else by the taps inside the map
};

inline PoolArgs args_of(const bbb_pool_desc_t* d, const Plan& pl) {
    PoolArgs a;
    a.H = d->h; a.W = d->w; a.Ho = pl.ho; a.Wo = pl.wo; a.Bg = pl.b4;
    a.kh = d->kh; a.kw = d->kw; a.sh = d->stride_h; a.sw = d->stride_w; a.ph = d->pad_h; a.pw = d->pad_w;
    a.cip = d->count_include_pad;
    return a;
}

}  // namespace pool_plan

#endif
