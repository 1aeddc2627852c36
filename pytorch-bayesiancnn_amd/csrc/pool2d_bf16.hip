// Average pooling on batch-innermost bf16 planes ([planes][H][W][B] bf16, planes = draws * channels, B % 8 == 0), gfx950: the pool of
// the bf16 storage mode (opt-in from Python, LaunchConfig.bf16_avgpool) -- pool2d.hip's forward and the
// backward of [activation -> average pool] with that file's window arithmetic, on the storage rules of the bf16 max-pool pair
// (bbb_maxpool_chwn_bf16, bbb_pool_act_bwd_chwn_bf16): values are bf16 in memory, every sum and quotient is fp32, and a result is
// rounded to bf16 exactly once.  What every entry checks before it launches is pool_plan.h (plan_bf16).
//
// Both kernels are bound by memory traffic, one thread per 16-byte group of 8 images, rows of images read and written as whole
// vectors, no LDS.  The order of every sum depends on the window alone -- never on the plane count or the launch size -- so a draw
// computed alone, inside a many-draw launch or as a work unit is the same bits.  There is no LRT form of the backward: bf16 LRT
// training does not exist.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "pool_plan.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf2f(uint32_t bits16) { return __uint_as_float(bits16 << 16); }

__device__ __forceinline__ uint32_t f2bf(float v) {             // round to nearest even (v_cvt_pk_bf16_f32)
    return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v);
}

__device__ __forceinline__ void unpack8(const u32x4 v, float (&o)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[2 * j] = bf2f(v[j] & 0xFFFFu);
        o[2 * j + 1] = bf2f(v[j] >> 16);
    }
}

__device__ __forceinline__ u32x4 pack8(const uint32_t (&r)[8]) {
    return u32x4{r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16)};
}

struct PoolArgs {
    int H, W, Ho, Wo, B8;
    int kh, kw, sh, sw, ph, pw;
    int cip;                     // count_include_pad: divide by kh * kw, else by the taps inside the map
};

// the rows (columns) of the map that window o covers: [lo, hi), never empty (2 * pad <= k, pool_plan.h)
__device__ __forceinline__ void window(int o, int s, int p, int k, int n, int& lo, int& hi) {
    const int a = o * s - p;
    lo = a > 0 ? a : 0;
    hi = a + k < n ? a + k : n;
}

// Forward: y(oh, ow) = bf16(the valid taps of the window, each exact in fp32, added in scan order by plain fp32 adds / divisor):
// avgpool_chwn_kernel's sum and its ONE IEEE division, then the ONE rounding to storage.
__global__ __launch_bounds__(256) void avgpool_chwn_bf16_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y, int64_t total8,
                                                                const PoolArgs p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int b8 = (int)(i % p.B8);
    int64_t t = i / p.B8;
    const int ow = (int)(t % p.Wo);
    t /= p.Wo;
    const int oh = (int)(t % p.Ho);
    const int64_t pl = t / p.Ho;
    int h0, h1, w0, w1;
    window(oh, p.sh, p.ph, p.kh, p.H, h0, h1);
    window(ow, p.sw, p.pw, p.kw, p.W, w0, w1);
    const u32x4* xp = x + pl * p.H * p.W * p.B8 + b8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int a = h0; a < h1; ++a)
        for (int c = w0; c < w1; ++c) {
            float v[8];
            unpack8(xp[((int64_t)a * p.W + c) * p.B8], v);
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
    auto incoming = [&](int64_t idx, float (&gv)[8]) {
        if (G_F32) {
            const f32x4* q = reinterpret_cast<const f32x4*>(g_out) + 2 * idx;
            const f32x4 a = q[0], b = q[1];
#pragma unroll
            for (int u = 0; u < 4; ++u) { gv[u] = a[u]; gv[4 + u] = b[u]; }
        } else {
            unpack8(reinterpret_cast<const u32x4*>(g_out)[idx], gv);
        }
    };
    const int b8 = (int)(i % p.B8);
    int64_t t = i / p.B8;
    const int w = (int)(t % p.W);
    t /= p.W;
    const int h = (int)(t % p.H);
    const int64_t pl = t / p.H;
    float me[8];
    unpack8(y[i], me);
    const int64_t gbase = pl * p.Ho * p.Wo * p.B8 + b8;
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
            incoming(gbase + ((int64_t)oh * p.Wo + ow) * p.B8, go);
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
    const int64_t oi = out_pitch8 ? pl * out_pitch8 + (i - pl * (int64_t)p.H * p.W * p.B8) : i;
    if (OUT_F32) {
        f32x4* o = reinterpret_cast<f32x4*>(g_pre) + 2 * oi;
        o[0] = f32x4{bf2f(r[0]), bf2f(r[1]), bf2f(r[2]), bf2f(r[3])};
        o[1] = f32x4{bf2f(r[4]), bf2f(r[5]), bf2f(r[6]), bf2f(r[7])};
    } else {
        reinterpret_cast<u32x4*>(g_pre)[oi] = pack8(r);
    }
}

PoolArgs args_of(const bbb_pool_desc_t* d, const pool_plan::Plan& pl) {
    PoolArgs a;
    a.H = d->h; a.W = d->w; a.Ho = pl.ho; a.Wo = pl.wo; a.B8 = pl.b4;
    a.kh = d->kh; a.kw = d->kw; a.sh = d->stride_h; a.sw = d->stride_w; a.ph = d->pad_h; a.pw = d->pad_w;
    a.cip = d->count_include_pad;
    return a;
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

extern "C" int bbb_avgpool_chwn_bf16(const bbb_pool_desc_t* d, const void* x, void* y, int64_t planes, void* stream) {
    if (x == nullptr || y == nullptr) return BBB_EINVAL;
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
    pool_plan::Plan pl;
    if (const int rc = pool_plan::plan_bf16(d, planes, out_plane_pitch, &pl)) return rc;
    if ((((uintptr_t)g_out | (uintptr_t)y | (uintptr_t)g_pre) & 15u) != 0) return BBB_EALIGN;
    if (act < 0 || act > 2 || (flags & ~(BBB_BF16_BWD_G_F32 | BBB_BF16_BWD_OUT_F32)) != 0) return BBB_EINVAL;
    const bool gf = (flags & BBB_BF16_BWD_G_F32) != 0, of = (flags & BBB_BF16_BWD_OUT_F32) != 0;
    const u32x4* yv = reinterpret_cast<const u32x4*>(y);
    const dim3 grid((unsigned)pl.bwd_blocks), blk(pool_plan::kThreads);
    hipStream_t st = (hipStream_t)stream;
    const PoolArgs a = args_of(d, pl);
    const int64_t p8 = out_plane_pitch / 8;
    if (gf && of) hipLaunchKernelGGL((avgpool_act_bwd_bf16_kernel<true, true>), grid, blk, 0, st, g_out, yv, g_pre, pl.bwd_total4, a, act, p8);
    else if (gf) hipLaunchKernelGGL((avgpool_act_bwd_bf16_kernel<true, false>), grid, blk, 0, st, g_out, yv, g_pre, pl.bwd_total4, a, act, p8);
    else if (of) hipLaunchKernelGGL((avgpool_act_bwd_bf16_kernel<false, true>), grid, blk, 0, st, g_out, yv, g_pre, pl.bwd_total4, a, act, p8);
    else hipLaunchKernelGGL((avgpool_act_bwd_bf16_kernel<false, false>), grid, blk, 0, st, g_out, yv, g_pre, pl.bwd_total4, a, act, p8);
    return (int)hipGetLastError();
}
