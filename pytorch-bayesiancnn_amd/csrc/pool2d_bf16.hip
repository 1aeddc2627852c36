// Pooling on batch-innermost bf16 planes ([planes][H][W][B] bf16, planes = draws * channels, B % 8 == 0), gfx950: the pools of the
// bf16 storage mode, maximum (bbb_maxpool_chwn_bf16, bbb_pool_act_bwd_chwn_bf16: scalar entries) and
// average (the descriptor entries; opt-in from Python, LaunchConfig.bf16_avgpool) -- pool2d.hip's forwards and backwards of
// [activation -> pool] with that file's window arithmetic on the storage rules of this mode: values are bf16 in memory, every
// comparison, sum and quotient is fp32, and a result is rounded to bf16 exactly once.  What every entry checks before it launches
// is pool_plan.h (plan_bf16); how the backward kernels read their incoming gradient is the bf16 section of pool_act_bwd.cuh.
//
// All kernels are bound by memory traffic, one thread per 16-byte group of 8 images, rows of images read and written as whole
// vectors, no LDS.  The order of every sum depends on the window alone -- never on the plane count or the launch size -- so a draw
// computed alone, inside a many-draw launch or as a work unit is the same bits.  There is no LRT form of the backward: bf16 LRT
// training does not exist.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/bbb_hip.h"
#include "pool_act_bwd.cuh"
#include "pool_plan.h"

namespace {

using namespace bf16_pack;
using pool_bwd::window;
using pool_plan::args_of;
using pool_plan::PoolArgs;

// maxpool over [planes][H][W][B] bf16, 8 images per thread (bf16 order = fp32 order of the widened values: exact)
__global__ __launch_bounds__(256) void maxpool_chwn_bf16_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y, int64_t total8,
                                                                int H, int W, int Ho, int Wo, int B8, int k, int s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int b8 = (int)(i % B8);
    int64_t t = i / B8;
    const int ow = (int)(t % Wo);
    t /= Wo;
    const int oh = (int)(t % Ho);
    const int64_t pl = t / Ho;
    const u32x4* xp = x + ((pl * H + (int64_t)oh * s) * W + (int64_t)ow * s) * B8 + b8;
    float m[8];
    {
        const u32x4 v = xp[0];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            m[2 * u] = __builtin_bit_cast(float, v[u] << 16);
            m[2 * u + 1] = __builtin_bit_cast(float, v[u] & 0xFFFF0000u);
        }
    }
    for (int a = 0; a < k; ++a)
        for (int c = 0; c < k; ++c) {
            const u32x4 v = xp[((int64_t)a * W + c) * B8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                m[2 * u] = fmaxf(m[2 * u], __builtin_bit_cast(float, v[u] << 16));
                m[2 * u + 1] = fmaxf(m[2 * u + 1], __builtin_bit_cast(float, v[u] & 0xFFFF0000u));
            }
        }
    u32x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        o[u] = (__builtin_bit_cast(uint32_t, m[2 * u]) >> 16) | (__builtin_bit_cast(uint32_t, m[2 * u + 1]) & 0xFFFF0000u);
    y[i] = o;
}

// g_pre = act'(y) * route(g) for 8 images per thread.  route: the sum (fp32, windows in scan order) of the incoming gradients of
// every pooling window whose FIRST maximum (torch's max_pool2d backward) is this element, compared on the stored bf16 values;
// act': ReLU [y > 0], Softplus 1 - exp(-y) (1 above the threshold 20), from the stored bf16 y.  One rounding to bf16 at the end
// (OUT_F32: the rounded values written as fp32, for the fp32 first-layer weight gradient).  G_F32: the incoming gradient is fp32
// (the logits layer's, from bbb_elbo_cb_bwd), else bf16.
template <bool G_F32, bool OUT_F32>
__global__ __launch_bounds__(256) void pool_act_bwd_bf16_kernel(const void* __restrict__ g_out, const u32x4* __restrict__ y,
                                                                void* __restrict__ g_pre, int64_t total8, int H, int W, int Hp, int Wp,
                                                                int B8, int k, int s, int act, int64_t out_pitch8) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int b8 = (int)(i % B8);
    int64_t t = i / B8;
    const int w = (int)(t % W);
    t /= W;
    const int h = (int)(t % H);
    const int64_t pl = t / H;
    const u32x4* yp = y + pl * H * W * B8 + b8;
    float me[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (y != nullptr) unpack8(yp[((int64_t)h * W + w) * B8], me);      // (no y: k == 0 and no activation -- a rounding only)
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k == 0) {
        pool_bwd::incoming8<G_F32>(g_out, i, g);
    } else {
        const int64_t gbase = pl * Hp * Wp * B8 + b8;
        const int ph_lo = h - k + 1 > 0 ? (h - k + 1 + s - 1) / s : 0, ph_hi = h / s < Hp - 1 ? h / s : Hp - 1;
        const int pw_lo = w - k + 1 > 0 ? (w - k + 1 + s - 1) / s : 0, pw_hi = w / s < Wp - 1 ? w / s : Wp - 1;
        for (int ph = ph_lo; ph <= ph_hi; ++ph)
            for (int pw = pw_lo; pw <= pw_hi; ++pw) {
                bool first[8] = {true, true, true, true, true, true, true, true};
                const int my = (h - ph * s) * k + (w - pw * s);
                for (int a = 0; a < k; ++a)
                    for (int c = 0; c < k; ++c) {
                        const int idx = a * k + c;
                        if (idx == my) continue;
                        float v[8];
                        unpack8(yp[((int64_t)(ph * s + a) * W + (pw * s + c)) * B8], v);
#pragma unroll
                        for (int u = 0; u < 8; ++u) first[u] = first[u] && (idx < my ? v[u] < me[u] : v[u] <= me[u]);
                    }
                float go[8];
                pool_bwd::incoming8<G_F32>(g_out, gbase + ((int64_t)ph * Wp + pw) * B8, go);
#pragma unroll
                for (int u = 0; u < 8; ++u) g[u] += first[u] ? go[u] : 0.0f;
            }
    }
    uint32_t r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float d = 1.0f;
        if (act == 1) d = me[u] > 0.0f ? 1.0f : 0.0f;
        else if (act == 2) d = me[u] > 20.0f ? 1.0f : -expm1f(-me[u]);      // y = softplus(v) -> sigmoid(v) = 1 - exp(-y)
        r[u] = f2bf(g[u] * d);
    }
    // out_pitch8 != 0: planes are written at that pitch (in 16-byte units of bf16) instead of densely
    const int64_t oi = out_pitch8 ? pl * out_pitch8 + (i - pl * (int64_t)H * W * B8) : i;
    if (OUT_F32) {
        f32x4* o = reinterpret_cast<f32x4*>(g_pre) + 2 * oi;
        o[0] = f32x4{bf2f(r[0]), bf2f(r[1]), bf2f(r[2]), bf2f(r[3])};
        o[1] = f32x4{bf2f(r[4]), bf2f(r[5]), bf2f(r[6]), bf2f(r[7])};
    } else {
        reinterpret_cast<u32x4*>(g_pre)[oi] = pack8(r);
    }
}

// Forward: y(oh, ow) = bf16(the valid taps of the window, each exact in fp32, added in scan order by plain fp32 adds / divisor):
// avgpool_chwn_kernel's sum and its ONE IEEE division, then the ONE rounding to storage.
__global__ __launch_bounds__(256) void avgpool_chwn_bf16_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y, int64_t total8,
                                                                const PoolArgs p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int b8 = (int)(i % p.Bg);
    int64_t t = i / p.Bg;
    const int ow = (int)(t % p.Wo);
    t /= p.Wo;
    const int oh = (int)(t % p.Ho);
    const int64_t pl = t / p.Ho;
    int h0, h1, w0, w1;
    window(oh, p.sh, p.ph, p.kh, p.H, h0, h1);
    window(ow, p.sw, p.pw, p.kw, p.W, w0, w1);
    const u32x4* xp = x + pl * p.H * p.W * p.Bg + b8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int a = h0; a < h1; ++a)
        for (int c = w0; c < w1; ++c) {
            float v[8];
            unpack8(xp[((int64_t)a * p.W + c) * p.Bg], v);
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += v[u];
        }
    const float div = (float)(p.cip ? p.kh * p.kw : (h1 - h0) * (w1 - w0));
    uint32_t r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) r[u] = f2bf(acc[u] / div);
    y[i] = pack8(r);
}

// Backward of [activation -> average pool], gather form (no atomics, a deterministic result), one thread per (plane, h, w, 8 images)
// of the layer's stored bf16 activated output y: avgpool_act_bwd_chwn_kernel's routing
//   g_act(h, w) = sum over the windows (oh, ow) that contain (h, w), in ascending (oh, ow) order, of g_out(oh, ow) / divisor(oh, ow)
// (windows along an axis: ceil((h + ph - kh + 1) / sh) <= oh <= floor((h + ph) / sh), clipped to the output map; an element no
// window covers receives 0) in fp32, then pool_act_bwd_bf16_kernel's end: act'(.) from the bf16 y, ONE rounding to bf16, the padded
// pitch.  G_F32: the incoming gradient is fp32, else bf16; OUT_F32: the rounded values are written as fp32.
template <bool G_F32, bool OUT_F32>
__global__ __launch_bounds__(256) void avgpool_act_bwd_bf16_kernel(const void* __restrict__ g_out, const u32x4* __restrict__ y,
                                                                   void* __restrict__ g_pre, int64_t total8, const PoolArgs p, int act,
                                                                   int64_t out_pitch8) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int b8 = (int)(i % p.Bg);
    int64_t t = i / p.Bg;
    const int w = (int)(t % p.W);
    t /= p.W;
    const int h = (int)(t % p.H);
    const int64_t pl = t / p.H;
    float me[8];
    unpack8(y[i], me);
    const int64_t gbase = pl * p.Ho * p.Wo * p.Bg + b8;
    const int th = h + p.ph - p.kh + 1, tw = w + p.pw - p.kw + 1;
    const int oh_lo = th > 0 ? (th + p.sh - 1) / p.sh : 0, oh_hi = (h + p.ph) / p.sh < p.Ho - 1 ? (h + p.ph) / p.sh : p.Ho - 1;
    const int ow_lo = tw > 0 ? (tw + p.sw - 1) / p.sw : 0, ow_hi = (w + p.pw) / p.sw < p.Wo - 1 ? (w + p.pw) / p.sw : p.Wo - 1;
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
        int h0, h1;
        window(oh, p.sh, p.ph, p.kh, p.H, h0, h1);
        for (int ow = ow_lo; ow <= ow_hi; ++ow) {
            int w0, w1;
            window(ow, p.sw, p.pw, p.kw, p.W, w0, w1);
            const float div = (float)(p.cip ? p.kh * p.kw : (h1 - h0) * (w1 - w0));
            float go[8];
            pool_bwd::incoming8<G_F32>(g_out, gbase + ((int64_t)oh * p.Wo + ow) * p.Bg, go);
#pragma unroll
            for (int u = 0; u < 8; ++u) g[u] += go[u] / div;
        }
    }
    uint32_t r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float d = 1.0f;
        if (act == 1) d = me[u] > 0.0f ? 1.0f : 0.0f;
        else if (act == 2) d = me[u] > 20.0f ? 1.0f : -expm1f(-me[u]);      // y = softplus(v) -> sigmoid(v) = 1 - exp(-y)
        r[u] = f2bf(g[u] * d);
    }
    // out_pitch8 != 0: planes are written at that pitch (in 16-byte units of bf16) instead of densely
    const int64_t oi = out_pitch8 ? pl * out_pitch8 + (i - pl * (int64_t)p.H * p.W * p.Bg) : i;
    if (OUT_F32) {
        f32x4* o = reinterpret_cast<f32x4*>(g_pre) + 2 * oi;
        o[0] = f32x4{bf2f(r[0]), bf2f(r[1]), bf2f(r[2]), bf2f(r[3])};
        o[1] = f32x4{bf2f(r[4]), bf2f(r[5]), bf2f(r[6]), bf2f(r[7])};
    } else {
        reinterpret_cast<u32x4*>(g_pre)[oi] = pack8(r);
    }
}

// launch(G_F32, OUT_F32) with the two storage flags of a bf16 backward as compile-time constants (std::bool_constant values)
template <typename L>
void with_bwd_flags(uint32_t flags, L&& launch) {
    const bool gf = (flags & BBB_BF16_BWD_G_F32) != 0, of = (flags & BBB_BF16_BWD_OUT_F32) != 0;
    if (gf && of) launch(std::true_type{}, std::true_type{});
    else if (gf) launch(std::true_type{}, std::false_type{});
    else if (of) launch(std::false_type{}, std::true_type{});
    else launch(std::false_type{}, std::false_type{});
}

// The backward launch of either kind.  k: what a maximum descriptor's kernel is launched with -- its window, or 0 for the activation
// (or, without y and act, the rounding) alone, which the descriptor states as the 1 x 1 window (pool_plan::max_desc).
int bwd_launch(const bbb_pool_desc_t* d, int k, const void* g_out, const void* y, void* g_pre, int64_t planes, int act,
               int64_t out_plane_pitch, uint32_t flags, void* stream) {
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan_bf16(d, planes, out_plane_pitch, &pl)) return rc;
    if ((((uintptr_t)g_out | (uintptr_t)y | (uintptr_t)g_pre) & 15u) != 0) return BBB_EALIGN;
    if (act < 0 || act > 2 || (flags & ~(BBB_BF16_BWD_G_F32 | BBB_BF16_BWD_OUT_F32)) != 0) return BBB_EINVAL;
    const u32x4* yv = reinterpret_cast<const u32x4*>(y);
    const dim3 grid((unsigned)pl.bwd_blocks), blk(pool_plan::kThreads);
    hipStream_t st = (hipStream_t)stream;
    const int64_t p8 = out_plane_pitch / 8;
    with_bwd_flags(flags, [&](auto gf, auto of) {
        constexpr bool G = decltype(gf)::value, O = decltype(of)::value;
        if (d->kind == BBB_POOL_MAX)
            hipLaunchKernelGGL((pool_act_bwd_bf16_kernel<G, O>), grid, blk, 0, st, g_out, yv, g_pre, pl.bwd_total4, d->h, d->w, pl.ho, pl.wo,
                               pl.b4, k, d->stride_h, act, p8);
        else
            hipLaunchKernelGGL((avgpool_act_bwd_bf16_kernel<G, O>), grid, blk, 0, st, g_out, yv, g_pre, pl.bwd_total4, args_of(d, pl), act, p8);
    });
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int bbb_avgpool_bf16_plan(const bbb_pool_desc_t* d, int64_t planes, int64_t out_plane_pitch, int32_t* ho, int32_t* wo,
                                     int64_t* fwd_blocks, int64_t* bwd_blocks) {
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan_bf16(d, planes, out_plane_pitch, &pl)) return rc;
    if (ho) *ho = pl.ho;
    if (wo) *wo = pl.wo;
    if (fwd_blocks) *fwd_blocks = pl.fwd_blocks;
    if (bwd_blocks) *bwd_blocks = pl.bwd_blocks;
    return 0;
}

extern "C" int bbb_maxpool_chwn_bf16(const void* x, void* y, int64_t planes, int h, int w, int batch, int k, int s, void* stream) {
    if (x == nullptr || y == nullptr) return BBB_EINVAL;
    const bbb_pool_desc_t d = pool_plan::max_desc(h, w, batch, k, s, false);
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan_bf16(&d, planes, 0, &pl)) return rc;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) != 0) return BBB_EALIGN;
    hipLaunchKernelGGL(maxpool_chwn_bf16_kernel, dim3((unsigned)pl.fwd_blocks), dim3(pool_plan::kThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const u32x4*>(x), reinterpret_cast<u32x4*>(y), pl.fwd_total4, h, w, pl.ho, pl.wo, pl.b4, k, s);
    return (int)hipGetLastError();
}

extern "C" int bbb_pool_act_bwd_chwn_bf16(const void* g_out, const void* y, void* g_pre, int64_t planes, int h, int w, int batch, int k,
                                          int s, int act, int64_t out_plane_pitch, uint32_t flags, void* stream) {
    if (g_out == nullptr || g_pre == nullptr || (y == nullptr && (k != 0 || act != 0))) return BBB_EINVAL;
    const bbb_pool_desc_t d = pool_plan::max_desc(h, w, batch, k, s, true);
    return bwd_launch(&d, k, g_out, y, g_pre, planes, act, out_plane_pitch, flags, stream);
}

extern "C" int bbb_avgpool_chwn_bf16(const bbb_pool_desc_t* d, const void* x, void* y, int64_t planes, void* stream) {
    if (x == nullptr || y == nullptr) return BBB_EINVAL;
    d = pool_plan::avg_only(d);
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan_bf16(d, planes, 0, &pl)) return rc;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) != 0) return BBB_EALIGN;
    hipLaunchKernelGGL(avgpool_chwn_bf16_kernel, dim3((unsigned)pl.fwd_blocks), dim3(pool_plan::kThreads), 0, (hipStream_t)stream,
                       reinterpret_cast<const u32x4*>(x), reinterpret_cast<u32x4*>(y), pl.fwd_total4, args_of(d, pl));
    return (int)hipGetLastError();
}

extern "C" int bbb_avgpool_act_bwd_chwn_bf16(const bbb_pool_desc_t* d, const void* g_out, const void* y, void* g_pre, int64_t planes,
                                             int act, int64_t out_plane_pitch, uint32_t flags, void* stream) {
    if (g_out == nullptr || y == nullptr || g_pre == nullptr) return BBB_EINVAL;
    return bwd_launch(pool_plan::avg_only(d), 0, g_out, y, g_pre, planes, act, out_plane_pitch, flags, stream);
}
