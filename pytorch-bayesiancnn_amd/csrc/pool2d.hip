// Pooling on batch-innermost planes ([planes][H][W][B], planes = draws * channels, B % 4 == 0), gfx950, maximum and average:
//   * nn.MaxPool2d(k, s) without padding in floor mode (the scalar entries bbb_maxpool_chwn, bbb_pool_act_bwd_chwn,
//     bbb_lrt_pool_act_bwd_chwn; the backward also with k = 0, the activation alone),
//   * nn.AvgPool2d in floor mode (any window, stride and padding with 2 * pad <= k, either divisor rule) and, as the window
//     H/oh x W/ow with the same stride, nn.AdaptiveAvgPool2d on a map its output size divides (the descriptor entries),
// each as the forward and as the backward of [activation -> pool] for the training nodes (BBB and LRT forms).  What every entry
// checks before it launches is pool_plan.h, one plan for both kinds; what the backward kernels share behind their routing is
// pool_act_bwd.cuh.  The same pools on bf16 planes (8 images per 16-byte group): pool2d_bf16.hip.  (The S3 / c8 S3 maximum pools
// stay with the split helpers they share with the GEMM epilogue: pconv_gemm.hip.)
//
// All kernels are bound by memory traffic (one pass over the larger of the two maps), one thread per 16-byte group of 4 images,
// rows of images read and written as whole vectors: fully coalesced on both sides.  The order of every sum depends on the window
// alone -- never on the plane count or the launch size -- so a draw computed alone, inside a many-draw launch or as a work unit is
// the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "bbb_common.cuh"
#include "pool_act_bwd.cuh"
#include "pool_plan.h"

namespace {

using pool_bwd::f32x4;
using pool_bwd::window;
using pool_plan::args_of;
using pool_plan::PoolArgs;

// maxpool over [planes][H][W][B] (planes = draws * channels), B innermost; 4 images per thread.
__global__ __launch_bounds__(256) void maxpool_chwn_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total4,
                                                           int H, int W, int Ho, int Wo, int B4, int k, int s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int b4 = (int)(i % B4);
    int64_t t = i / B4;
    const int ow = (int)(t % Wo);
    t /= Wo;
    const int oh = (int)(t % Ho);
    const int64_t pl = t / Ho;
    const f32x4* xp = reinterpret_cast<const f32x4*>(x) + ((pl * H + (int64_t)oh * s) * W + (int64_t)ow * s) * B4 + b4;
    f32x4 m = xp[0];
    for (int a = 0; a < k; ++a)
        for (int c = 0; c < k; ++c) {
            const f32x4 v = xp[((int64_t)a * W + c) * B4];
#pragma unroll
            for (int u = 0; u < 4; ++u) m[u] = bbb::max_nan(m[u], v[u]);
        }
    reinterpret_cast<f32x4*>(y)[i] = m;
}

// Backward of [activation -> MaxPool2d(k, s)] (or of the activation alone, k = 0) in the batch-innermost layout -- training
// extension.  Gather form, one thread per (plane, h, w, 4 images) of the layer's activated output y:
//   g_act(h, w) = sum over the pooling windows that contain (h, w) of g_out(window) if (h, w) is that window's FIRST maximum
//                 in scan order (torch's max_pool2d backward routes the gradient to the first argmax), else 0;
//   g_pre = g_act * act'(pre-activation), written from y alone: Softplus' = sigmoid(v) = 1 - exp(-y), ReLU' = [y > 0].
// Overlapping windows (k > s: Bayesian3Conv3FC pools 3x3 / 2) make up to ceil(k/s)^2 windows per element; nothing is
// scattered, so no atomics and a deterministic result.
// LRT layers (am != NULL): the layer's output was act(act_mu + sqrt(act_var) * eps), so besides g_pre (= the gradient w.r.t.
// act_mu) the same pass writes the gradient w.r.t. act_var, g_pre * (v - act_mu) / (2 act_var), with the pre-activation v
// recovered from the stored activated output (softplus: y + log(1 - exp(-y)); nothing flows where ReLU clipped).  act_mu /
// act_var hold mom_planes planes: all of them, or one draw's worth when every draw shares one pair of moments (first layer).
__global__ __launch_bounds__(256) void pool_act_bwd_chwn_kernel(const float* __restrict__ g_out, const float* __restrict__ y,
                                                                float* __restrict__ g_pre, int64_t total4, int H, int W, int Hp,
                                                                int Wp, int B4, int k, int s, int act, int64_t out_pitch4,
                                                                const float* __restrict__ am, const float* __restrict__ av,
                                                                float* __restrict__ g_var, int64_t mom_planes,
                                                                const float* __restrict__ g2, const float* __restrict__ xc,
                                                                int64_t xc_total4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    // (the incoming gradient and everything behind the routed gradient: pool_act_bwd.cuh, shared with the average-pool routing)
    auto incoming = [&](int64_t idx) { return pool_bwd::incoming(g_out, g2, xc, xc_total4, idx); };
    const int b4 = (int)(i % B4);
    int64_t t = i / B4;
    const int w = (int)(t % W);
    t /= W;
    const int h = (int)(t % H);
    const int64_t pl = t / H;
    const f32x4* yp = reinterpret_cast<const f32x4*>(y) + pl * H * W * B4 + b4;
    const f32x4 me = yp[((int64_t)h * W + w) * B4];
    f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
    if (k == 0) {
        g = incoming(i);
    } else {
        const int64_t gbase = pl * Hp * Wp * B4 + b4;
        // windows (ph, pw) with ph*s <= h < ph*s + k
        const int ph_lo = h - k + 1 > 0 ? (h - k + 1 + s - 1) / s : 0, ph_hi = h / s < Hp - 1 ? h / s : Hp - 1;
        const int pw_lo = w - k + 1 > 0 ? (w - k + 1 + s - 1) / s : 0, pw_hi = w / s < Wp - 1 ? w / s : Wp - 1;
        for (int ph = ph_lo; ph <= ph_hi; ++ph)
            for (int pw = pw_lo; pw <= pw_hi; ++pw) {
                // am I the first maximum of this window?  (an earlier element >= me, or a later one > me, disqualifies)
                bool first[4] = {true, true, true, true};
                const int my = (h - ph * s) * k + (w - pw * s);
                for (int a = 0; a < k; ++a)
                    for (int c = 0; c < k; ++c) {
                        const int idx = a * k + c;
                        if (idx == my) continue;
                        const f32x4 v = yp[((int64_t)(ph * s + a) * W + (pw * s + c)) * B4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) first[u] = first[u] && (idx < my ? v[u] < me[u] : v[u] <= me[u]);
                    }
                const f32x4 go = incoming(gbase + ((int64_t)ph * Wp + pw) * B4);
#pragma unroll
                for (int u = 0; u < 4; ++u) g[u] += first[u] ? go[u] : 0.0f;
            }
    }
    pool_bwd::act_epilogue(g, me, act, i, pl, (int64_t)H * W * B4, out_pitch4, g_pre, am, av, g_var, mom_planes);
}

// Forward: y(oh, ow) = (the valid taps of the window added in scan order, rows then columns, by plain fp32 adds) / divisor -- ONE
// IEEE division, torch's rule (no reciprocal: the quotient of an exactly representable sum is the correctly rounded average).
__global__ __launch_bounds__(256) void avgpool_chwn_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total4,
                                                           const PoolArgs p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const int b4 = (int)(i % p.Bg);
    int64_t t = i / p.Bg;
    const int ow = (int)(t % p.Wo);
    t /= p.Wo;
    const int oh = (int)(t % p.Ho);
    const int64_t pl = t / p.Ho;
    int h0, h1, w0, w1;
    window(oh, p.sh, p.ph, p.kh, p.H, h0, h1);
    window(ow, p.sw, p.pw, p.kw, p.W, w0, w1);
    const f32x4* xp = reinterpret_cast<const f32x4*>(x) + pl * p.H * p.W * p.Bg + b4;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int a = h0; a < h1; ++a)
        for (int c = w0; c < w1; ++c) {
            const f32x4 v = xp[((int64_t)a * p.W + c) * p.Bg];
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
    const int b4 = (int)(i % p.Bg);
    int64_t t = i / p.Bg;
    const int w = (int)(t % p.W);
    t /= p.W;
    const int h = (int)(t % p.H);
    const int64_t pl = t / p.H;
    const f32x4 me = reinterpret_cast<const f32x4*>(y)[i];
    const int64_t gbase = pl * p.Ho * p.Wo * p.Bg + b4;
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
            const f32x4 go = pool_bwd::incoming(g_out, g2, xc, xc_total4, gbase + ((int64_t)oh * p.Wo + ow) * p.Bg);
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] += go[u] / div;
        }
    }
    pool_bwd::act_epilogue(g, me, act, i, pl, (int64_t)p.H * p.W * p.Bg, out_pitch4, g_pre, am, av, g_var, mom_planes);
}

// The backward launch of either kind, BBB and LRT forms.  k: what a maximum descriptor's kernel is launched with -- its window, or 0
// for the activation alone, which the descriptor states as the 1 x 1 window (pool_plan::max_desc).
int bwd_launch(const bbb_pool_desc_t* d, int k, const float* g_out, const float* y, float* g_pre, int64_t planes, int act,
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
    const dim3 grid((unsigned)pl.bwd_blocks), blk(pool_plan::kThreads);
    const int64_t xc_total4 = g2 != nullptr ? xc_planes * pl.ho * pl.wo * pl.b4 : (int64_t)1;
    if (d->kind == BBB_POOL_MAX)
        hipLaunchKernelGGL(pool_act_bwd_chwn_kernel, grid, blk, 0, (hipStream_t)stream, g_out, y, g_pre, pl.bwd_total4, d->h, d->w, pl.ho,
                           pl.wo, pl.b4, k, d->stride_h, act, out_plane_pitch / 4, am, av, g_var, mom_planes, g2, xc, xc_total4);
    else
        hipLaunchKernelGGL(avgpool_act_bwd_chwn_kernel, grid, blk, 0, (hipStream_t)stream, g_out, y, g_pre, pl.bwd_total4, args_of(d, pl),
                           act, out_plane_pitch / 4, am, av, g_var, mom_planes, g2, xc, xc_total4);
    return (int)hipGetLastError();
}

// what the two LRT entries check before the launch's own checks
int lrt_check(const float* act_mu, const float* act_var, const float* g_var, int64_t planes, int64_t moment_planes) {
    if (act_mu == nullptr || act_var == nullptr || g_var == nullptr) return BBB_EINVAL;
    if (moment_planes <= 0 || planes % moment_planes != 0) return BBB_EINVAL;
    if ((((uintptr_t)act_mu | (uintptr_t)act_var | (uintptr_t)g_var) & 15u) != 0) return BBB_EALIGN;
    return 0;
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

extern "C" int bbb_maxpool_chwn(const float* x, float* y, int64_t planes, int h, int w, int batch, int k, int s, void* stream) {
    if (x == nullptr || y == nullptr) return BBB_EINVAL;
    const bbb_pool_desc_t d = pool_plan::max_desc(h, w, batch, k, s, false);
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan(&d, planes, 0, &pl)) return rc;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) != 0) return BBB_EALIGN;
    hipLaunchKernelGGL(maxpool_chwn_kernel, dim3((unsigned)pl.fwd_blocks), dim3(pool_plan::kThreads), 0, (hipStream_t)stream, x, y,
                       pl.fwd_total4, h, w, pl.ho, pl.wo, pl.b4, k, s);
    return (int)hipGetLastError();
}

extern "C" int bbb_pool_act_bwd_chwn(const float* g_out, const float* y, float* g_pre, int64_t planes, int h, int w, int batch,
                                     int k, int s, int act, int64_t out_plane_pitch, void* stream) {
    const bbb_pool_desc_t d = pool_plan::max_desc(h, w, batch, k, s, true);
    return bwd_launch(&d, k, g_out, y, g_pre, planes, act, out_plane_pitch, nullptr, nullptr, nullptr, 1, nullptr, nullptr, 0, stream);
}

extern "C" int bbb_lrt_pool_act_bwd_chwn(const float* g_out, const float* y, const float* act_mu, const float* act_var, float* g_mu,
                                         float* g_var, int64_t planes, int64_t moment_planes, int h, int w, int batch, int k, int s,
                                         int act, int64_t out_plane_pitch, const float* g_out2, const float* x_out, int64_t x_planes,
                                         void* stream) {
    if (const int rc = lrt_check(act_mu, act_var, g_var, planes, moment_planes)) return rc;
    const bbb_pool_desc_t d = pool_plan::max_desc(h, w, batch, k, s, true);
    return bwd_launch(&d, k, g_out, y, g_mu, planes, act, out_plane_pitch, act_mu, act_var, g_var, moment_planes, g_out2, x_out, x_planes,
                      stream);
}

extern "C" int bbb_avgpool_chwn(const bbb_pool_desc_t* d, const float* x, float* y, int64_t planes, void* stream) {
    if (x == nullptr || y == nullptr) return BBB_EINVAL;
    d = pool_plan::avg_only(d);
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan(d, planes, 0, &pl)) return rc;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) != 0) return BBB_EALIGN;
    hipLaunchKernelGGL(avgpool_chwn_kernel, dim3((unsigned)pl.fwd_blocks), dim3(pool_plan::kThreads), 0, (hipStream_t)stream, x, y,
                       pl.fwd_total4, args_of(d, pl));
    return (int)hipGetLastError();
}

extern "C" int bbb_avgpool_act_bwd_chwn(const bbb_pool_desc_t* d, const float* g_out, const float* y, float* g_pre, int64_t planes,
                                        int act, int64_t out_plane_pitch, void* stream) {
    return bwd_launch(pool_plan::avg_only(d), 0, g_out, y, g_pre, planes, act, out_plane_pitch, nullptr, nullptr, nullptr, 1, nullptr, nullptr, 0, stream);
}

extern "C" int bbb_lrt_avgpool_act_bwd_chwn(const bbb_pool_desc_t* d, const float* g_out, const float* y, const float* act_mu,
                                            const float* act_var, float* g_mu, float* g_var, int64_t planes, int64_t moment_planes,
                                            int act, int64_t out_plane_pitch, const float* g_out2, const float* x_out, int64_t x_planes,
                                            void* stream) {
    if (const int rc = lrt_check(act_mu, act_var, g_var, planes, moment_planes)) return rc;
    return bwd_launch(pool_plan::avg_only(d), 0, g_out, y, g_mu, planes, act, out_plane_pitch, act_mu, act_var, g_var, moment_planes, g_out2, x_out,
                      x_planes, stream);
}
