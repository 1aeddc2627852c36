// Pooling on batch-innermost bf16 planes ([planes][H][W][B] bf16, planes = draws * channels, B % 8 == 0), gfx950: the pools of the
// bf16 storage mode, maximum (bbb_maxpool_chwn_bf16, bbb_pool_act_bwd_chwn_bf16: scalar entries) and
// average (the descriptor entries; opt-in from Python, LaunchConfig.bf16_avgpool) -- pool2d.hip's forwards and backwards of
// [activation -> pool] with that file's window arithmetic on the storage rules of this mode: values are bf16 in memory, every
// comparison, sum and quotient is fp32, and a result is rounded to bf16 exactly once.  What every entry checks before it launches
// is pool_plan.h (plan_bf16); how the backward kernels read their incoming gradient is the bf16 section of pool_act_bwd.cuh.
//
// All kernels are bound by memory traffic, one thread per 16-byte group of 8 images, rows of images read and written as whole
// vectors, no LDS.  The order of every sum depends on the window alone -- never on the plane count or the launch size -- so a draw
// computed alone, inside a many-draw launch or as a work unit is the same bits.  The LRT form of the backward
// (bbb_lrt_pool_act_bwd_chwn_bf16: the activation side of a local-reparameterisation layer, input gradients only) regenerates the
// forward's noise element from the counter (that arithmetic, not the traffic, sets its time: profiles/bf16_lrt_input_grad_notes.md);
// there is no average-pool form of it, and bf16 LRT training does not exist.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/bbb_hip.h"
#include "bbb_common.cuh"
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
                m[2 * u] = bbb::max_nan(m[2 * u], __builtin_bit_cast(float, v[u] << 16));
                m[2 * u + 1] = bbb::max_nan(m[2 * u + 1], __builtin_bit_cast(float, v[u] & 0xFFFF0000u));
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

// The kernel arguments of the LRT backward below.
struct LrtBwdArgs {
    const void* g_out;           // [planes][Hp][Wp][B] bf16 (G_F32: fp32), the gradient w.r.t. the (pooled) output ...
    const u32x4* g2;             // ... or, g2 != NULL, d1 of the combine fmaf(2 * x_out, d2, d1): g2 = d2, xc = x_out (bf16, xc_total8
    const u32x4* xc;             //     16-byte groups: all planes, or one draw's worth)
    int64_t xc_total8;
    const u32x4* y;              // [planes][H][W][B] bf16, the stored activated output
    const f32x4* av;             // [mom_planes][H][W][B] fp32 act_var
    int64_t mom_planes;
    u32x4* g_mu;                 // [planes][H][W][B] bf16 (dense, or planes at out_pitch8 16-byte groups)
    u32x4* g_var;
    int64_t total;               // threads: planes * (H * W / PPT) * B8
    int H, W, Hp, Wp, B8, k, s, act, C;
    int64_t out_pitch8;
    uint32_t k0, k1, call0, stream_id;
    const uint32_t* call_dev;
    int b_off;
};

// Backward of [sample -> activation -> MaxPool2d(k, s)] (k = 0: no pool) of a local-reparameterisation layer on bf16 planes: the
// forward stored y = bf16(act(act_mu + sqrt(act_var) * eps)).  Gather form, one pass, fp32 in registers:
//   g_act = pool_act_bwd_bf16_kernel's routing (first maximum in scan order among the stored bf16 values) of the incoming gradient --
//           bf16, fp32 (G_F32: the logits layer's) or the on-the-fly combine fmaf(2 * x_out, d2, d1) of the layer above's two bf16
//           input gradients (pool_bwd::incoming's bf16 twin),
//   g_mu  = g_act * act'(y)                          (the gradient w.r.t. act_mu),
//   g_var = g_mu * eps / (2 * sqrt(act_var))         (the gradient w.r.t. act_var), from the fp32 g_mu,
// each rounded ONCE to bf16.  eps is the forward's element, REGENERATED from the counter -- the stored y is rounded, so the fp32
// kernel's y - act_mu would be a cancellation of rounded values: canonical NCHW index ((b + b_off) * C + n) * HW + pix of the
// pre-pool output, call call0 + *call_dev + draw (draw = plane / C), bbb::normal4(idx >> 2, ...) lane idx & 3, as
// lrt_sample_chwn_bf16_kernel and the epilogue of pconv_bf16_lrt.hip draw it.  One normal4 call yields four consecutive pixels of
// one (image, channel): a thread owns 8 images of PPT pixels -- PPT = 4 (H * W % 4 == 0: every value is used) or 1 (3 of 4 dropped).
template <bool G_F32, int PPT>
__global__ __launch_bounds__(256) void lrt_pool_act_bwd_bf16_kernel(const LrtBwdArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int HW = a.H * a.W, HWq = HW / PPT, B8 = a.B8, k = a.k, s = a.s;
    const int b8 = (int)(i % B8);
    int64_t t = i / B8;
    const int q = (int)(t % HWq);
    const int64_t pl = t / HWq;
    const int n = (int)(pl % a.C);
    const uint32_t call = a.call0 + (a.call_dev ? *a.call_dev : 0u) + (uint32_t)(pl / a.C);
    float z[8][4];                       // PPT == 4: image u's four pixels (idx0 % 4 == 0); PPT == 1: z[u][0] is image u's pixel
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const uint64_t idx0 = (uint64_t)(((int64_t)(8 * b8 + u + a.b_off) * a.C + n) * HW + (int64_t)q * PPT);
        bbb::normal4(idx0 >> 2, a.stream_id, call, a.k0, a.k1, z[u]);
        if (PPT == 1) {
            const int c = (int)(idx0 & 3);
            z[u][0] = c == 0 ? z[u][0] : c == 1 ? z[u][1] : c == 2 ? z[u][2] : z[u][3];
        }
    }
    const u32x4* yp = a.y + pl * HW * B8 + b8;
    const int64_t gbase = pl * a.Hp * a.Wp * B8 + b8;
    auto incoming = [&](int64_t idx, float (&gv)[8]) {
        pool_bwd::incoming8<G_F32>(a.g_out, idx, gv);
        if (!G_F32 && a.g2 != nullptr) {
            float d2[8], xo[8];
            unpack8(a.g2[idx], d2);
            unpack8(a.xc[idx % a.xc_total8], xo);
#pragma unroll
            for (int u = 0; u < 8; ++u) gv[u] = fmaf(2.0f * xo[u], d2[u], gv[u]);
        }
    };
    for (int j = 0; j < PPT; ++j) {
        const int pix = q * PPT + j;
        const int h = pix / a.W, w = pix - h * a.W;
        const int64_t in_plane = (int64_t)pix * B8 + b8;
        float me[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (a.y != nullptr) unpack8(yp[(int64_t)pix * B8], me);      // (no y: k == 0 and no activation -- the logits layer, fp32 output)
        float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (k == 0) {
            incoming(pl * HW * B8 + in_plane, g);
        } else {
            const int ph_lo = h - k + 1 > 0 ? (h - k + 1 + s - 1) / s : 0, ph_hi = h / s < a.Hp - 1 ? h / s : a.Hp - 1;
            const int pw_lo = w - k + 1 > 0 ? (w - k + 1 + s - 1) / s : 0, pw_hi = w / s < a.Wp - 1 ? w / s : a.Wp - 1;
            for (int ph = ph_lo; ph <= ph_hi; ++ph)
                for (int pw = pw_lo; pw <= pw_hi; ++pw) {
                    bool first[8] = {true, true, true, true, true, true, true, true};
                    const int my = (h - ph * s) * k + (w - pw * s);
                    for (int r = 0; r < k; ++r)
                        for (int c = 0; c < k; ++c) {
                            const int idx = r * k + c;
                            if (idx == my) continue;
                            float v[8];
                            unpack8(yp[((int64_t)(ph * s + r) * a.W + (pw * s + c)) * B8], v);
#pragma unroll
                            for (int u = 0; u < 8; ++u) first[u] = first[u] && (idx < my ? v[u] < me[u] : v[u] <= me[u]);
                        }
                    float go[8];
                    incoming(gbase + ((int64_t)ph * a.Wp + pw) * B8, go);
#pragma unroll
                    for (int u = 0; u < 8; ++u) g[u] += first[u] ? go[u] : 0.0f;
                }
        }
        const int64_t mi = (pl % a.mom_planes) * HW * B8 + in_plane;
        const f32x4 v0 = a.av[2 * mi], v1 = a.av[2 * mi + 1];
        uint32_t rm[8], rv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float d = 1.0f;
            if (a.act == 1) d = me[u] > 0.0f ? 1.0f : 0.0f;
            else if (a.act == 2) d = me[u] > 20.0f ? 1.0f : -expm1f(-me[u]);      // y = softplus(v) -> sigmoid(v) = 1 - exp(-y)
            const float gm = g[u] * d;
            const float eps = PPT == 1 ? z[u][0] : j == 0 ? z[u][0] : j == 1 ? z[u][1] : j == 2 ? z[u][2] : z[u][3];
            const float var = u < 4 ? v0[u & 3] : v1[u & 3];
            rm[u] = f2bf(gm);
            rv[u] = f2bf((gm * eps) * (0.5f * __builtin_amdgcn_rsqf(var)));      // g_mu * eps / (2 sqrt(act_var))
        }
        // out_pitch8 != 0: planes are written at that pitch (in 16-byte units of bf16) instead of densely
        const int64_t oi = (a.out_pitch8 ? pl * a.out_pitch8 : pl * HW * B8) + in_plane;
        a.g_mu[oi] = pack8(rm);
        a.g_var[oi] = pack8(rv);
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

extern "C" int bbb_lrt_pool_act_bwd_chwn_bf16(const void* g_out, const void* y, const float* act_var, void* g_mu, void* g_var,
                                              int64_t planes, int64_t moment_planes, int channels, int h, int w, int batch, int k, int s,
                                              int act, int64_t out_plane_pitch, const void* g_out2, const void* x_out, int64_t x_planes,
                                              uint64_t seed, uint32_t call0, const uint32_t* call_dev, uint32_t stream_id, int b_offset,
                                              uint32_t flags, void* stream) {
    if (g_out == nullptr || act_var == nullptr || g_mu == nullptr || g_var == nullptr || (y == nullptr && (k != 0 || act != 0)))
        return BBB_EINVAL;
    if (act < 0 || act > 2 || (flags & ~BBB_BF16_BWD_G_F32) != 0 || b_offset < 0) return BBB_EINVAL;
    if (channels <= 0 || planes <= 0 || planes % channels != 0 || moment_planes <= 0 || moment_planes % channels != 0 ||
        planes % moment_planes != 0)
        return BBB_EINVAL;
    const bool gf = (flags & BBB_BF16_BWD_G_F32) != 0;
    if ((g_out2 == nullptr) != (x_out == nullptr)) return BBB_EINVAL;
    if (g_out2 != nullptr && (gf || x_planes <= 0 || planes % x_planes != 0)) return BBB_EINVAL;      // (the combine is of bf16 gradients)
    const bbb_pool_desc_t d = pool_plan::max_desc(h, w, batch, k, s, true);
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan_bf16(&d, planes, out_plane_pitch, &pl)) return rc;
    if ((((uintptr_t)g_out | (uintptr_t)y | (uintptr_t)act_var | (uintptr_t)g_mu | (uintptr_t)g_var | (uintptr_t)g_out2 |
          (uintptr_t)x_out) & 15u) != 0)
        return BBB_EALIGN;
    const int64_t hw = (int64_t)h * w;
    // the canonical noise index ((b + b_offset) * channels + n) * hw + pix and the kernel's per-plane sizes stay in range
    if (hw > 0x7fffffffLL || pool_plan::mul_cap((int64_t)batch + b_offset, channels, hw) >= conv_desc_check::kCap) return BBB_ESHAPE;
    const int ppt = hw % 4 == 0 ? 4 : 1;
    LrtBwdArgs a = {};
    a.g_out = g_out; a.g2 = reinterpret_cast<const u32x4*>(g_out2); a.xc = reinterpret_cast<const u32x4*>(x_out);
    a.xc_total8 = g_out2 != nullptr ? x_planes * pl.ho * pl.wo * pl.b4 : (int64_t)1;
    a.y = reinterpret_cast<const u32x4*>(y); a.av = reinterpret_cast<const f32x4*>(act_var); a.mom_planes = moment_planes;
    a.g_mu = reinterpret_cast<u32x4*>(g_mu); a.g_var = reinterpret_cast<u32x4*>(g_var);
    a.total = pl.bwd_total4 / ppt;
    a.H = h; a.W = w; a.Hp = pl.ho; a.Wp = pl.wo; a.B8 = pl.b4; a.k = k; a.s = d.stride_h; a.act = act; a.C = channels;
    a.out_pitch8 = out_plane_pitch / 8;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.call0 = call0; a.stream_id = stream_id; a.call_dev = call_dev;
    a.b_off = b_offset;
    const dim3 grid((unsigned)((a.total + pool_plan::kThreads - 1) / pool_plan::kThreads)), blk(pool_plan::kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (gf) {
        if (ppt == 4) hipLaunchKernelGGL((lrt_pool_act_bwd_bf16_kernel<true, 4>), grid, blk, 0, st, a);
        else          hipLaunchKernelGGL((lrt_pool_act_bwd_bf16_kernel<true, 1>), grid, blk, 0, st, a);
    } else {
        if (ppt == 4) hipLaunchKernelGGL((lrt_pool_act_bwd_bf16_kernel<false, 4>), grid, blk, 0, st, a);
        else          hipLaunchKernelGGL((lrt_pool_act_bwd_bf16_kernel<false, 1>), grid, blk, 0, st, a);
    }
    return (int)hipGetLastError();
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
