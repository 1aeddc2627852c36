// What the pooling kernels of pool2d.hip (fp32 planes) and pool2d_bf16.hip (bf16 planes) share on the device: the rows a window
// covers, and for the backward passes of [activation -> pooling], whatever the pooling routes (pool_act_bwd_*: the first maximum;
// avgpool_act_bwd_*: every tap, divided): how the incoming gradient is read, and everything behind the routed gradient g_act -- the
// activation's derivative from the stored activated output, the padded-pitch store, on fp32 planes the LRT split into the gradients
// w.r.t. act_mu and act_var.  (The bf16 kernels keep their ends -- act', the one rounding, the store -- written out: as a shared
// device function the same lines compile to other, slower instructions, profiles/pool_home_notes.md.)  One thread per (plane, h, w, 16-byte group of images).
#ifndef BBB_POOL_ACT_BWD_CUH
#define BBB_POOL_ACT_BWD_CUH

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_pack.cuh"

namespace pool_bwd {

using bf16_pack::f32x4;
using bf16_pack::u32x4;

// the rows (columns) of the map that window o covers: [lo, hi), never empty (2 * pad <= k, pool_plan.h)
__device__ __forceinline__ void window(int o, int s, int p, int k, int n, int& lo, int& hi) {
    const int a = o * s - p;
    lo = a > 0 ? a : 0;
    hi = a + k < n ? a + k : n;
}

// The incoming gradient of 16-byte group idx.  g2 != NULL (an LRT layer below another one): it is g_out + 2 * xc * g2 -- the two
// input gradients of the layer above combined on the fly (bbb_lrt_glue mode 1's fmaf, bit for bit) instead of by a launch of its own
__device__ __forceinline__ f32x4 incoming(const float* __restrict__ g_out, const float* __restrict__ g2, const float* __restrict__ xc,
                                          int64_t xc_total4, int64_t idx) {
    f32x4 gv = reinterpret_cast<const f32x4*>(g_out)[idx];
    if (g2 != nullptr) {
        const f32x4 b4v = reinterpret_cast<const f32x4*>(g2)[idx], x4v = reinterpret_cast<const f32x4*>(xc)[idx % xc_total4];
#pragma unroll
        for (int u = 0; u < 4; ++u) gv[u] = fmaf(2.0f * x4v[u], b4v[u], gv[u]);
    }
    return gv;
}

// g_pre = g * act'(.) from the activated output `me` (group i of plane pl; plane4 = 16-byte groups per plane), stored densely or at
// out_pitch4; LRT layers (am != NULL): g_var = g_pre * (v - act_mu) / (2 act_var) with the pre-activation v recovered from `me`.
__device__ __forceinline__ void act_epilogue(const f32x4 g, const f32x4 me, int act, int64_t i, int64_t pl, int64_t plane4,
                                             int64_t out_pitch4, float* __restrict__ g_pre, const float* __restrict__ am,
                                             const float* __restrict__ av, float* __restrict__ g_var, int64_t mom_planes) {
    f32x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float d = 1.0f;
        if (act == 1) d = me[u] > 0.0f ? 1.0f : 0.0f;
        else if (act == 2) d = me[u] > 20.0f ? 1.0f : -expm1f(-me[u]);      // y = softplus(v) -> sigmoid(v) = 1 - exp(-y)
        o[u] = g[u] * d;
    }
    // out_pitch4 != 0: planes are written at that pitch (in 16-byte units) instead of densely -- see bbb_pool_act_bwd_chwn
    const int64_t oi = out_pitch4 ? pl * out_pitch4 + (i - pl * plane4) : i;
    reinterpret_cast<f32x4*>(g_pre)[oi] = o;
    if (am != nullptr) {
        const int64_t in_plane = i - pl * plane4;
        const int64_t mi = (pl % mom_planes) * plane4 + in_plane;
        const f32x4 a4 = reinterpret_cast<const f32x4*>(am)[mi];
        const f32x4 v4 = reinterpret_cast<const f32x4*>(av)[mi];
        f32x4 gv;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v = me[u];
            if (act == 2 && !(v > 20.0f)) v = v + logf(-expm1f(-v));
            const float t = (act != 0 && !(me[u] > 0.0f)) ? 0.0f : v - a4[u];        // sqrt(act_var) * eps
            gv[u] = (o[u] * t) / (2.0f * v4[u]);
        }
        reinterpret_cast<f32x4*>(g_var)[oi] = gv;
    }
}

// ---- bf16 planes: 8 images per 16-byte group, every value fp32 in registers ----

// The incoming gradient of group idx: fp32 (G_F32: two 16-byte vectors; the logits layer's, from bbb_elbo_cb_bwd) or bf16.
template <bool G_F32>
__device__ __forceinline__ void incoming8(const void* g_out, int64_t idx, float (&gv)[8]) {
    if (G_F32) {
        const f32x4* p = reinterpret_cast<const f32x4*>(g_out) + 2 * idx;
        const f32x4 a = p[0], b = p[1];
#pragma unroll
        for (int u = 0; u < 4; ++u) { gv[u] = a[u]; gv[4 + u] = b[u]; }
    } else {
        bf16_pack::unpack8(reinterpret_cast<const u32x4*>(g_out)[idx], gv);
    }
}

}  // namespace pool_bwd

#endif
