// Average pooling on batch-innermost planes ([planes][H][W][B], planes = draws * channels, B % 4 == 0), gfx950: nn.AvgPool2d in
// floor mode (any window, stride and padding with 2 * pad <= k, either divisor rule) and, as the window H/oh x W/ow with the same
// stride, nn.AdaptiveAvgPool2d on a map its output size divides -- the forward, and the backward of [activation -> pool] for the
// training nodes (BBB and LRT forms, the arithmetic behind the routing shared with the max-pool backward: pool_act_bwd.cuh).
// What every entry checks before it launches is pool_plan.h.  The same pool on bf16 planes (8 images per 16-byte group): pool2d_bf16.hip.
//
// Both kernels are bound by memory traffic (one pass over the larger of the two maps), one thread per 16-byte group of 4 images,
// rows of images read and written as whole vectors: fully coalesced on both sides.  The order of every sum depends on the window
// alone -- never on the plane count or the launch size -- so a draw computed alone, inside a many-draw launch or as a work unit is
// the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "pool_act_bwd.cuh"
#include "pool_plan.h"

namespace {

using pool_bwd::f32x4;

struct PoolArgs {
    int H, W, Ho, Wo, B4;
    int kh, kw, sh, sw, ph, pw;
    int cip;                     // count_include_pad: divide by kh * kw, else by the taps inside the map
};

// the rows (columns) of the map that window o covers: [lo, hi), never empty (2 * pad <= k, pool_plan.h)
__device__ __forceinline__ void window(int o, int s, int p, int k, int n, int& lo, int& hi) {
    const int a = o * s - p;
    lo = a > 0 ? a : 0;
    hi = a + k < n ? a + k : n;
}

// Forward: y(oh, ow) = (the valid taps of the window added in scan order, rows then columns, by plain fp32 adds) / divisor -- ONE
// IEEE division, torch's rule (no reciprocal: the quotient of an exactly representable sum is the correctly rounded average).
__global__ __launch_bounds__(256) void avgpool_chwn_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total4,
                                                           const PoolArgs p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int b4 = (int)(i % p.B4);
    int64_t t = i / p.B4;
    const int ow = (int)(t % p.Wo);
    t /= p.Wo;
    const int oh = (int)(t % p.Ho);
    const int64_t pl = t / p.Ho;
    int h0, h1, w0, w1;
    window(oh, p.sh, p.ph, p.kh, p.H, h0, h1);
    window(ow, p.sw, p.pw, p.kw, p.W, w0, w1);
    const f32x4* xp = reinterpret_cast<const f32x4*>(x) + pl * p.H * p.W * p.B4 + b4;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int a = h0; a < h1; ++a)
        for (int c = w0; c < w1; ++c) {
            const f32x4 v = xp[((int64_t)a * p.W + c) * p.B4];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += v[u];
        }
    const float div = (float)(p.cip ? p.kh * p.kw : (h1 - h0) * (w1 - w0));
    f32x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = acc[u] / div;
    reinterpret_cast<f32x4*>(y)[i] = o;
}

// Backward of [activation -> average pool], gather form (nothing is scattered: no atomics, a deterministic result), one thread per
// (plane, h, w, 4 images) of the layer's activated output y:
//   g_act(h, w) = sum over the windows (oh, ow) that contain (h, w), in ascending (oh, ow) order, of g_out(oh, ow) / divisor(oh, ow)
// with the windows along an axis ceil((h + ph - kh + 1) / sh) <= oh <= floor((h + ph) / sh), clipped to the output map; an element
// no window covers (k < s leaves gaps; rows and columns floor mode drops) receives 0.  Everything behind g_act -- act'(.) from y, the
// padded pitch, the LRT pair, the on-the-fly combine of the incoming gradient -- is pool_act_bwd_chwn_kernel's (pool_act_bwd.cuh).
__global__ __launch_bounds__(256) void avgpool_act_bwd_chwn_kernel(const float* __restrict__ g_out, const float* __restrict__ y,
                                                                   float* __restrict__ g_pre, int64_t total4, const PoolArgs p, int act,
                                                                   int64_t out_pitch4, const float* __restrict__ am,
                                                                   const float* __restrict__ av, float* __restrict__ g_var,
                                                                   int64_t mom_planes, const float* __restrict__ g2,
                                                                   const float* __restrict__ xc, int64_t xc_total4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int b4 = (int)(i % p.B4);
    int64_t t = i / p.B4;
    const int w = (int)(t % p.W);
    t /= p.W;
    const int h = (int)(t % p.H);
    const int64_t pl = t / p.H;
    const f32x4 me = reinterpret_cast<const f32x4*>(y)[i];
    const int64_t gbase = pl * p.Ho * p.Wo * p.B4 + b4;
    const int th = h + p.ph - p.kh + 1, tw = w + p.pw - p.kw + 1;
    const int oh_lo = th > 0 ? (th + p.sh - 1) / p.sh : 0, oh_hi = (h + p.ph) / p.sh < p.Ho - 1 ? (h + p.ph) / p.sh : p.Ho - 1;
    const int ow_lo = tw > 0 ? (tw + p.sw - 1) / p.sw : 0, ow_hi = (w + p.pw) / p.sw < p.Wo - 1 ? (w + p.pw) / p.sw : p.Wo - 1;
    f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        int h0, h1;
        window(oh, p.sh, p.ph, p.kh, p.H, h0, h1);
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
            int w0, w1;
            window(ow, p.sw, p.pw, p.kw, p.W, w0, w1);
            const float div = (float)(p.cip ? p.kh * p.kw : (h1 - h0) * (w1 - w0));
            const f32x4 go = pool_bwd::incoming(g_out, g2, xc, xc_total4, gbase + ((int64_t)oh * p.Wo + ow) * p.B4);
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] += go[u] / div;
        }
    }
    pool_bwd::act_epilogue(g, me, act, i, pl, (int64_t)p.H * p.W * p.B4, out_pitch4, g_pre, am, av, g_var, mom_planes);
}

PoolArgs args_of(const bbb_pool_desc_t* d, const pool_plan::Plan& pl) {
    PoolArgs a;
    a.H = d->h; a.W = d->w; a.Ho = pl.ho; a.Wo = pl.wo; a.B4 = pl.b4;
    a.kh = d->kh; a.kw = d->kw; a.sh = d->stride_h; a.sw = d->stride_w; a.ph = d->pad_h; a.pw = d->pad_w;
    a.cip = d->count_include_pad;
    return a;
}

int bwd_launch(const bbb_pool_desc_t* d, const float* g_out, const float* y, float* g_pre, int64_t planes, int act,
               int64_t out_plane_pitch, const float* am, const float* av, float* g_var, int64_t mom_planes, const float* g2,
               const float* xc, int64_t xc_planes, void* stream) {
    if (g_out == nullptr || y == nullptr || g_pre == nullptr || act < 0 || act > 2) return BBB_EINVAL;
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan(d, planes, out_plane_pitch, &pl)) return rc;
    if ((((uintptr_t)g_out | (uintptr_t)y | (uintptr_t)g_pre) & 15u) != 0) return BBB_EALIGN;
    if ((g2 == nullptr) != (xc == nullptr)) return BBB_EINVAL;
    if (g2 != nullptr) {
        if (xc_planes <= 0 || planes % xc_planes != 0) return BBB_EINVAL;
        if ((((uintptr_t)g2 | (uintptr_t)xc) & 15u) != 0) return BBB_EALIGN;
    }
    hipLaunchKernelGGL(avgpool_act_bwd_chwn_kernel, dim3((unsigned)pl.bwd_blocks), dim3(pool_plan::kThreads), 0, (hipStream_t)stream,
                       g_out, y, g_pre, pl.bwd_total4, args_of(d, pl), act, out_plane_pitch / 4, am, av, g_var, mom_planes, g2, xc,
                       g2 != nullptr ? xc_planes * pl.ho * pl.wo * pl.b4 : (int64_t)1);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int bbb_avgpool_plan(const bbb_pool_desc_t* d, int64_t planes, int64_t out_plane_pitch, int32_t* ho, int32_t* wo,
                                int64_t* fwd_blocks, int64_t* bwd_blocks) {
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan(d, planes, out_plane_pitch, &pl)) return rc;
    if (ho) *ho = pl.ho;
    if (wo) *wo = pl.wo;
    if (fwd_blocks) *fwd_blocks = pl.fwd_blocks;
    if (bwd_blocks) *bwd_blocks = pl.bwd_blocks;
    return 0;
}

extern "C" int bbb_avgpool_chwn(const bbb_pool_desc_t* d, const float* x, float* y, int64_t planes, void* stream) {
    if (x == nullptr || y == nullptr) return BBB_EINVAL;
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan(d, planes, 0, &pl)) return rc;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) != 0) return BBB_EALIGN;
    hipLaunchKernelGGL(avgpool_chwn_kernel, dim3((unsigned)pl.fwd_blocks), dim3(pool_plan::kThreads), 0, (hipStream_t)stream, x, y,
                       pl.fwd_total4, args_of(d, pl));
    return (int)hipGetLastError();
}

extern "C" int bbb_avgpool_act_bwd_chwn(const bbb_pool_desc_t* d, const float* g_out, const float* y, float* g_pre, int64_t planes,
                                        int act, int64_t out_plane_pitch, void* stream) {
    return bwd_launch(d, g_out, y, g_pre, planes, act, out_plane_pitch, nullptr, nullptr, nullptr, 1, nullptr, nullptr, 0, stream);
}

extern "C" int bbb_lrt_avgpool_act_bwd_chwn(const bbb_pool_desc_t* d, const float* g_out, const float* y, const float* act_mu,
                                            const float* act_var, float* g_mu, float* g_var, int64_t planes, int64_t moment_planes,
                                            int act, int64_t out_plane_pitch, const float* g_out2, const float* x_out, int64_t x_planes,
                                            void* stream) {
    if (act_mu == nullptr || act_var == nullptr || g_var == nullptr) return BBB_EINVAL;
    if (moment_planes <= 0 || planes % moment_planes != 0) return BBB_EINVAL;
    if ((((uintptr_t)act_mu | (uintptr_t)act_var | (uintptr_t)g_var) & 15u) != 0) return BBB_EALIGN;
    return bwd_launch(d, g_out, y, g_mu, planes, act, out_plane_pitch, act_mu, act_var, g_var, moment_planes, g_out2, x_out,
                      x_planes, stream);
}
