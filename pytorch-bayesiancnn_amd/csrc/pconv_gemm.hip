// Pixel-major implicit GEMM for the Monte-Carlo ensemble path on gfx950: batch-innermost activations,
// padding taps never computed.
//
// Layout: activations are [draw][C][H][W][B] (B innermost, B % 4 == 0); weights stay in the reference's
// [draw][Cout][Cin][kh][kw].  One workgroup owns ONE output pixel (oh, ow), 64 output channels and BM images:
//     D[n][b] = sum over ci and over the kernel taps (r, q) that fall INSIDE the image for this pixel
//               W[n][ci][r][q] * X[ci][oh*s - p + r*d][ow*s - p + q*d][b]
// so the contraction length is K_eff = Cin * nr * nq (nr, nq = number of in-bounds taps per axis) instead of
// Cin*kh*kw.  On AlexNet/CIFAR the 2x2 and 4x4 feature maps make more than half of the im2col matrix padding
// zeros; skipping them halves the matrix-core work (7.07 instead of 14.11 GFLOP per draw at bs=512).
// Every X row of a tile is one contiguous run of BM floats (16-byte vector loads straight into LDS rows),
// every output row is contiguous in b: fully coalesced on both sides, no per-element im2col arithmetic.
//
// Matrix core: v_mfma_f32_32x32x2_f32 (exact fp32), weights as the "A" operand, X as "B" -> lanes = images.
// Workgroup = 256 threads = 4 waves, tile 64 (n) x BM (b) x 32 (k); register-staged double buffering;
// per-tile (k_eff -> weight offset, x row) tables computed by 32 lanes into LDS.
// Workgroups that share a weight tile (same draw, same 64 channels) are mapped to the same XCD (block id
// mod 8) so the tile stays in that XCD's private L2.
//
// LRT variant: second accumulator set for sigma^2 * x^2, epilogue act_mu + sqrt(1e-16 + act_var) * eps with eps
// indexed by the canonical NCHW element index (identical stream to the NCHW kernel and the oracle).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "bbb_common.cuh"
#include "pconv_args.h"
#include "pconv_body.cuh"
#include "pconv_bf16x3.cuh"
#include "pconv_plan.h"

namespace {

using namespace pconv;

template <int BM, bool LRT, bool ILV, bool SEQ = false>
__global__ __launch_bounds__(kThreads) void pconv_gemm_kernel(const PConvArgs p) {
    // ---- block -> work item; weight-tile sharers on one XCD ----
    // Work items (group g = (draw, channel tile), m-tile j) in g-major order are cut into 8 equal contiguous chunks,
    // one per XCD (workgroup id mod 8 is the XCD the dispatcher places it on): perfectly balanced, and the
    // workgroups that share a weight tile run on the same XCD at the same time.  (A wrong placement guess costs
    // L2 hits, never correctness.)
    const int bid = blockIdx.x;
    const int xcd = bid & 7;
    const int64_t item = (int64_t)xcd * p.per_xcd + (bid >> 3);
    const int64_t item_end = (int64_t)(xcd + 1) * p.per_xcd;
    if (item >= item_end || item >= (int64_t)p.G * p.Mtiles) return;
    pconv_item<BM, LRT, ILV, SEQ ? kSeq : kPlain>(p, item);
}

// The layer with its MaxPool2d(2, 2) (pconv_body.cuh, POOL): items are pooled pixels.
template <bool ILV>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void pconv_gemm_pool_kernel(const PConvArgs p) {
    const int bid = blockIdx.x;
    const int xcd = bid & 7;
    const int64_t item = (int64_t)xcd * p.per_xcd + (bid >> 3);
    const int64_t item_end = (int64_t)(xcd + 1) * p.per_xcd;
    if (item >= item_end || item >= (int64_t)p.G * p.Mtiles) return;
    pconv_item<128, false, ILV, kPool>(p, item);
}

// The pooled LRT layer: 64-image tiles, dual accumulators, the sampling epilogue per window pixel.
__global__ __launch_bounds__(kThreads) void pconv_gemm_pool_lrt_kernel(const PConvArgs p) {
    const int bid = blockIdx.x;
    const int xcd = bid & 7;
    const int64_t item = (int64_t)xcd * p.per_xcd + (bid >> 3);
    const int64_t item_end = (int64_t)(xcd + 1) * p.per_xcd;
    if (item >= item_end || item >= (int64_t)p.G * p.Mtiles) return;
    pconv_item<64, true, false, kPool>(p, item);
}

// Split contraction (pconv_body.cuh, SPLIT): block -> (item, k range).  The ksplit blocks of an item are consecutive, so they
// land on the same XCD chunk as their item's weight-tile sharers.
template <int BM, bool LRT, bool ILV>
__global__ __launch_bounds__(kThreads) void pconv_gemm_splitk_kernel(const PConvArgs p) {
    const int bid = blockIdx.x;
    const int xcd = bid & 7;
    const int64_t blk = (int64_t)xcd * p.per_xcd + (bid >> 3);
    const int64_t blk_end = (int64_t)(xcd + 1) * p.per_xcd;
    if (blk >= blk_end || blk >= (int64_t)p.G * p.Mtiles * p.ksplit) return;
    const int64_t item = blk / p.ksplit;
    pconv_item<BM, LRT, ILV, kSplit>(p, item, (int)(blk - item * p.ksplit));
}

// the descriptor checks (pconv_plan.h, describe) -> the kernel-argument block
int fill(const bbb_conv_desc_t* d, PConvArgs& a) {
    pconv_plan::Geom g;
    const int rc = pconv_plan::describe(d, &g);
    if (rc != 0) return rc;
    a.x_inv = g.x_inv;
    a.B = g.B; a.Cin = g.Cin; a.H = g.H; a.W = g.W; a.Cout = g.Cout; a.kh = g.kh; a.kw = g.kw;
    a.sh = g.sh; a.sw = g.sw; a.ph = g.ph; a.pw = g.pw; a.dh = g.dh; a.dw = g.dw;
    a.Ho = g.Ho; a.Wo = g.Wo; a.K = g.K; a.khkw = g.khkw; a.act = g.act; a.Kp = g.Kp;
    a.x_ds = g.x_ds; a.w_ds = g.w_ds; a.b_ds = g.b_ds; a.y_ds = g.y_ds;
    a.unit_div = g.unit_div; a.unit_off = g.unit_off; a.x_mod = g.x_mod; a.b_off = g.b_off;
    a.x_div = g.x_div; a.x_off = g.x_off; a.pool = g.pool; a.wtap = g.wtap;
    return 0;
}

// what the plan reads of a filled argument block
pconv_plan::Geom geom_of(const PConvArgs& a) {
    pconv_plan::Geom g = {};
    g.B = a.B; g.Cin = a.Cin; g.H = a.H; g.W = a.W; g.Cout = a.Cout; g.kh = a.kh; g.kw = a.kw;
    g.dh = a.dh; g.dw = a.dw; g.Ho = a.Ho; g.Wo = a.Wo; g.pool = a.pool;
    return g;
}

// Which kernel, which grid: pconv_plan.h (plan) decides -- the tile width, interleaved staging or not, the layer's split across
// workgroups or inside one, the pooled forms; this function starts what it names.
template <bool LRT>
int launch(PConvArgs& a, int draws, hipStream_t st) {
    using namespace pconv_plan;
    if (LRT && a.pool && (a.y_mu != nullptr || a.y_var != nullptr)) return BBB_EINVAL;    // the moments of unpooled pixels are not kept
    Plan pl;
    const int rc = plan(geom_of(a), draws, LRT, a.ksplit, a.part != nullptr, &pl);
    if (rc != 0) return rc;
    a.Ntiles = pl.Ntiles; a.G = pl.G; a.nbt = pl.nbt; a.Mtiles = pl.Mtiles; a.per_xcd = pl.per_xcd;
    const dim3 grid((unsigned)pl.blocks), block(kThreads);
    if constexpr (LRT) {
        switch (pl.form) {
            case kLrtPool:  hipLaunchKernelGGL(pconv_gemm_pool_lrt_kernel, grid, block, 0, st, a); break;
            case kLrtCross: hipLaunchKernelGGL((pconv_gemm_splitk_kernel<64, true, true>), grid, block, 0, st, a); break;
            case kLrtSeq64: hipLaunchKernelGGL((pconv_gemm_kernel<64, true, false, true>), grid, block, 0, st, a); break;
            case kLrt64Ilv: hipLaunchKernelGGL((pconv_gemm_kernel<64, true, true>), grid, block, 0, st, a); break;
            case kLrt64:    hipLaunchKernelGGL((pconv_gemm_kernel<64, true, false>), grid, block, 0, st, a); break;
            default: return BBB_EINVAL;
        }
    } else {
        switch (pl.form) {
            case kBbbPool:      hipLaunchKernelGGL((pconv_gemm_pool_kernel<false>), grid, block, 0, st, a); break;
            case kBbbCross:     hipLaunchKernelGGL((pconv_gemm_splitk_kernel<64, false, true>), grid, block, 0, st, a); break;
            case kBbbSeq128Ilv: hipLaunchKernelGGL((pconv_gemm_kernel<128, false, true, true>), grid, block, 0, st, a); break;
            case kBbbSeq128:    hipLaunchKernelGGL((pconv_gemm_kernel<128, false, false, true>), grid, block, 0, st, a); break;
            case kBbbSeq64Ilv:  hipLaunchKernelGGL((pconv_gemm_kernel<64, false, true, true>), grid, block, 0, st, a); break;
            case kBbbSeq64:     hipLaunchKernelGGL((pconv_gemm_kernel<64, false, false, true>), grid, block, 0, st, a); break;
            case kBbb128Ilv:    hipLaunchKernelGGL((pconv_gemm_kernel<128, false, true>), grid, block, 0, st, a); break;
            case kBbb128:       hipLaunchKernelGGL((pconv_gemm_kernel<128, false, false>), grid, block, 0, st, a); break;
            case kBbb64Ilv:     hipLaunchKernelGGL((pconv_gemm_kernel<64, false, true>), grid, block, 0, st, a); break;
            case kBbb64:        hipLaunchKernelGGL((pconv_gemm_kernel<64, false, false>), grid, block, 0, st, a); break;
            default: return BBB_EINVAL;
        }
    }
    return (int)hipGetLastError();
}

}  // namespace

namespace {
using pconv_plan::kTicketBytes;

// The layer's split (pconv_plan.h: canonical_ksplit, split_scratch_bytes) applied to one launch's argument block.
int split_setup(PConvArgs& a, int draws, bool lrt, int k_split, void* scratch, int64_t scratch_bytes) {
    if (k_split <= 1) return 0;
    const pconv_plan::Geom g = geom_of(a);
    if (k_split != pconv_plan::canonical_ksplit(g)) return BBB_EINVAL;   // the split is the layer's, not the caller's choice
    a.ksplit = k_split;
    const int64_t need = pconv_plan::split_scratch_bytes(g, draws, lrt, k_split);
    if (need > 0 && scratch != nullptr) {
        if (scratch_bytes < need || (((uintptr_t)scratch) & 255u) != 0) return BBB_EINVAL;
        a.tickets = static_cast<int32_t*>(scratch);
        a.part = reinterpret_cast<float*>(static_cast<char*>(scratch) + kTicketBytes);
    }
    return 0;
}
}  // namespace

extern "C" int bbb_conv2d_chwn_plan(const bbb_conv_desc_t* d, int lrt, int k_split, int has_scratch, int32_t* form, int32_t* bm,
                                    int32_t* ilv, int64_t* items, int64_t* blocks) {
    pconv_plan::Geom g;
    int rc = pconv_plan::describe(d, &g);
    if (rc != 0) return rc;
    if (lrt && (d->w_draw_stride != 0 || d->b_draw_stride != 0)) return BBB_EINVAL;     // as bbb_lrt_conv2d_chwn_splitk_fwd
    pconv_plan::Plan pl;
    if ((rc = pconv_plan::plan(g, d->draws, lrt != 0, k_split, has_scratch != 0, &pl)) != 0) return rc;
    if (form) *form = pl.form;
    if (bm) *bm = pl.bm;
    if (ilv) *ilv = pl.ilv;
    if (items) *items = pl.items;
    if (blocks) *blocks = pl.blocks;
    return 0;
}

extern "C" int64_t bbb_conv2d_chwn_splitk_scratch(const bbb_conv_desc_t* d, int lrt, int32_t* k_split) {
    PConvArgs a = {};
    if (k_split) *k_split = 1;
    if (fill(d, a) != 0) return 0;
    const pconv_plan::Geom g = geom_of(a);
    const int s = pconv_plan::canonical_ksplit(g);
    if (k_split) *k_split = s;
    return pconv_plan::split_scratch_bytes(g, d->draws, lrt != 0, s);
}

extern "C" int bbb_conv2d_chwn_splitk_fwd(const bbb_conv_desc_t* d, const float* x, const float* w, const float* bias, float* y,
                                          int k_split, void* scratch, int64_t scratch_bytes, void* stream) {
    PConvArgs a = {};
    int rc = fill(d, a);
    if (rc != 0) return rc;
    if (x == nullptr || w == nullptr || y == nullptr) return BBB_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) != 0 || (((uintptr_t)w | (uintptr_t)bias) & 3u) != 0) return BBB_EALIGN;
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    if ((rc = split_setup(a, d->draws, false, k_split, scratch, scratch_bytes)) != 0) return rc;
    return launch<false>(a, d->draws, (hipStream_t)stream);
}

extern "C" int bbb_conv2d_chwn_fwd(const bbb_conv_desc_t* d, const float* x, const float* w, const float* bias, float* y,
                                   void* stream) {
    PConvArgs a = {};
    const int rc = fill(d, a);
    if (rc != 0) return rc;
    if (x == nullptr || w == nullptr || y == nullptr) return BBB_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) != 0 || (((uintptr_t)w | (uintptr_t)bias) & 3u) != 0) return BBB_EALIGN;
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    return launch<false>(a, d->draws, (hipStream_t)stream);
}

// bbb_conv2d_chwn_fwd with the contraction on the 16-bit matrix pipe at fp32 accuracy, range-free (pconv_bf16x3.cuh)
extern "C" int bbb_conv2d_chwn_bf16x3_fwd(const bbb_conv_desc_t* d, const void* x, const float* w, const float* bias, void* y,
                                          uint32_t flags, void* stream) {
    PConvArgs a = {};
    const int rc = fill(d, a);
    if (rc != 0) return rc;
    if (x == nullptr || w == nullptr || y == nullptr || (flags & ~3u) != 0 || a.pool || a.wtap) return BBB_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) != 0 || (((uintptr_t)w | (uintptr_t)bias) & 3u) != 0) return BBB_EALIGN;
    const bool xs3 = (flags & BBB_S3_IN) != 0, ys3 = (flags & BBB_S3_OUT) != 0;
    if ((xs3 || ys3) && d->batch % 8 != 0) return BBB_ESHAPE;           // S3 rows move as 16-byte vectors of 8 bf16
    a.x = static_cast<const float*>(x); a.w = w; a.bias = bias; a.y = static_cast<float*>(y);
    a.x_ps = (int64_t)a.Cin * a.H * a.W * a.B;
    a.y_ps = (int64_t)a.Cout * a.Ho * a.Wo * a.B;
    if (ys3) a.y_ds = 3 * a.y_ps;
    if (xs3 && (d->x_draw_stride != 0 && d->x_draw_stride < 3 * a.x_ps)) return BBB_EINVAL;
    // 128 images per workgroup (measured: the 256-image form -- 2 workgroups per CU, half the workgroups -- is slower on four of
    // the six launches of the metric step, profiles/r04_notes.md); the grid is the fp32 forward's (pconv_plan.h)
    constexpr int kMT = 1;
    pconv_plan::Plan pl = {};
    if (const int rc = pconv_plan::channel_groups(a.Cout, d->draws, &pl)) return rc;
    if (const int rc = pconv_plan::item_grid(a.B, (int64_t)a.Ho * a.Wo, 128 * kMT, &pl)) return rc;
    a.Ntiles = pl.Ntiles; a.G = pl.G; a.nbt = pl.nbt; a.Mtiles = pl.Mtiles; a.per_xcd = pl.per_xcd;
    const dim3 grid((unsigned)pl.blocks), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (xs3 && ys3)      hipLaunchKernelGGL((pconv_bf16x3_kernel<kMT, true, true>), grid, block, 0, st, a);
    else if (xs3)        hipLaunchKernelGGL((pconv_bf16x3_kernel<kMT, true, false>), grid, block, 0, st, a);
    else if (ys3)        hipLaunchKernelGGL((pconv_bf16x3_kernel<kMT, false, true>), grid, block, 0, st, a);
    else                 hipLaunchKernelGGL((pconv_bf16x3_kernel<kMT, false, false>), grid, block, 0, st, a);
    return (int)hipGetLastError();
}

namespace {
// S3 helpers: 8 images (16 bytes per plane) per thread
typedef uint32_t s3_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void s3_join(const s3_u32x4 h, const s3_u32x4 m, const s3_u32x4 l, float (&v)[8]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {        // hi + mid is exact (16 significant bits), + lo gives back the fp32 value exactly
        v[2 * c] = (__builtin_bit_cast(float, h[c] << 16) + __builtin_bit_cast(float, m[c] << 16)) + __builtin_bit_cast(float, l[c] << 16);
        v[2 * c + 1] = (__builtin_bit_cast(float, h[c] & 0xFFFF0000u) + __builtin_bit_cast(float, m[c] & 0xFFFF0000u)) +
                       __builtin_bit_cast(float, l[c] & 0xFFFF0000u);
    }
}

__device__ __forceinline__ void s3_cut(const float (&v)[8], s3_u32x4& h, s3_u32x4& m, s3_u32x4& l) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint32_t a0, a1, a2;
        split3_pair(f32x2{v[2 * c], v[2 * c + 1]}, a0, a1, a2);
        h[c] = a0; m[c] = a1; l[c] = a2;
    }
}

// MaxPool2d(k, s) on S3 planes: x [slabs][3][C][H][W][B] -> y [slabs][3][C][Ho][Wo][B]; values are joined (exact), compared as
// fp32 and cut again (exact), so the result is the S3 form of what maxpool_chwn_kernel computes on the fp32 tensor.
// SQ (the LRT chain of pconv_c8x3): slabs hold SIX planes -- the values' pieces, then the pieces of their squares; the maximum is
// taken over the values and the squares are those of the pooled values (what the next LRT layer's second contraction reads).
template <bool SQ>
__global__ __launch_bounds__(256) void maxpool_s3_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y,
                                                         int64_t total8, int C, int H, int W, int Ho, int Wo, int B8, int k, int s) {
    constexpr int NPL = SQ ? 6 : 3;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int b8 = (int)(i % B8);
    int64_t t = i / B8;
    const int ow = (int)(t % Wo);
    t /= Wo;
    const int oh = (int)(t % Ho);
    t /= Ho;
    const int c = (int)(t % C);
    const int64_t slab = t / C;
    const int64_t xps = (int64_t)C * H * W * B8, yps = (int64_t)C * Ho * Wo * B8;     // plane strides in 16-byte units
    const s3_u32x4* xp = reinterpret_cast<const s3_u32x4*>(x) + slab * NPL * xps + (((int64_t)c * H + (int64_t)oh * s) * W + (int64_t)ow * s) * B8 + b8;
    float best[8];
    for (int a = 0; a < k; ++a)
        for (int q = 0; q < k; ++q) {
            const int64_t o = ((int64_t)a * W + q) * B8;
            float v[8];
            s3_join(xp[o], xp[o + xps], xp[o + 2 * xps], v);
#pragma unroll
            for (int u = 0; u < 8; ++u) best[u] = (a == 0 && q == 0) ? v[u] : bbb::max_nan(best[u], v[u]);
        }
    s3_u32x4 h, m, l;
    s3_cut(best, h, m, l);
    s3_u32x4* yp = reinterpret_cast<s3_u32x4*>(y) + slab * NPL * yps + (((int64_t)c * Ho + oh) * Wo + ow) * B8 + b8;
    yp[0] = h; yp[yps] = m; yp[2 * yps] = l;
    if constexpr (SQ) {
#pragma unroll
        for (int u = 0; u < 8; ++u) best[u] = bbb::mul_rn(best[u], best[u]);      // (the rounded fp32 square: no fma contraction into the cut)
        s3_cut(best, h, m, l);
        yp[3 * yps] = h; yp[4 * yps] = m; yp[5 * yps] = l;
    }
}

// fp32 [slabs][n] <-> S3 [slabs][3][n] (n % 8 == 0): test / boundary helpers
__global__ __launch_bounds__(256) void s3_from_f32_kernel(const float* __restrict__ x, unsigned short* __restrict__ y, int64_t n8, int64_t slabs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8 * slabs) return;
    const int64_t slab = i / n8, j = i - slab * n8;
    const f32x4* xp = reinterpret_cast<const f32x4*>(x) + (slab * n8 + j) * 2;
    const f32x4 a = xp[0], b = xp[1];
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    s3_u32x4 h, m, l;
    s3_cut(v, h, m, l);
    s3_u32x4* yp = reinterpret_cast<s3_u32x4*>(y) + slab * 3 * n8 + j;
    yp[0] = h; yp[n8] = m; yp[2 * n8] = l;
}

__global__ __launch_bounds__(256) void s3_to_f32_kernel(const unsigned short* __restrict__ x, float* __restrict__ y, int64_t n8, int64_t slabs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8 * slabs) return;
    const int64_t slab = i / n8, j = i - slab * n8;
    const s3_u32x4* xp = reinterpret_cast<const s3_u32x4*>(x) + slab * 3 * n8 + j;
    float v[8];
    s3_join(xp[0], xp[n8], xp[2 * n8], v);
    f32x4* yp = reinterpret_cast<f32x4*>(y) + (slab * n8 + j) * 2;
    yp[0] = f32x4{v[0], v[1], v[2], v[3]};
    yp[1] = f32x4{v[4], v[5], v[6], v[7]};
}
}  // namespace

namespace {
int maxpool_s3_launch(const void* x, void* y, int64_t slabs, int channels, int h, int w, int batch, int k, int s, bool sq, void* stream) {
    if (x == nullptr || y == nullptr || slabs <= 0 || channels <= 0 || h <= 0 || w <= 0 || batch <= 0 || k <= 0 || s <= 0) return BBB_EINVAL;
    if (batch % 8 != 0 || h < k || w < k) return BBB_ESHAPE;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) != 0) return BBB_EALIGN;
    const int ho = (h - k) / s + 1, wo = (w - k) / s + 1;
    const int64_t total8 = slabs * channels * ho * wo * (batch / 8);
    const int64_t blocks = (total8 + 255) / 256;
    if (blocks > 0x7fffffffLL) return BBB_ESHAPE;
    if (sq) hipLaunchKernelGGL(maxpool_s3_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, static_cast<const unsigned short*>(x),
                               static_cast<unsigned short*>(y), total8, channels, h, w, ho, wo, batch / 8, k, s);
    else    hipLaunchKernelGGL(maxpool_s3_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, static_cast<const unsigned short*>(x),
                               static_cast<unsigned short*>(y), total8, channels, h, w, ho, wo, batch / 8, k, s);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int bbb_maxpool_chwn_s3(const void* x, void* y, int64_t slabs, int channels, int h, int w, int batch, int k, int s, void* stream) {
    return maxpool_s3_launch(x, y, slabs, channels, h, w, batch, k, s, false, stream);
}

extern "C" int bbb_maxpool_chwn_s3sq(const void* x, void* y, int64_t slabs, int channels, int h, int w, int batch, int k, int s, void* stream) {
    return maxpool_s3_launch(x, y, slabs, channels, h, w, batch, k, s, true, stream);
}

extern "C" int bbb_s3_convert(const void* src, void* dst, int64_t slabs, int64_t n, int to_s3, void* stream) {
    if (src == nullptr || dst == nullptr || slabs <= 0 || n <= 0) return BBB_EINVAL;
    if (n % 8 != 0) return BBB_ESHAPE;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15u) != 0) return BBB_EALIGN;
    const int64_t blocks = (slabs * (n / 8) + 255) / 256;
    if (blocks > 0x7fffffffLL) return BBB_ESHAPE;
    if (to_s3) hipLaunchKernelGGL(s3_from_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, static_cast<const float*>(src),
                                  static_cast<unsigned short*>(dst), n / 8, slabs);
    else       hipLaunchKernelGGL(s3_to_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                                  static_cast<const unsigned short*>(src), static_cast<float*>(dst), n / 8, slabs);
    return (int)hipGetLastError();
}

extern "C" int bbb_lrt_conv2d_chwn_splitk_fwd(const bbb_conv_desc_t* d, const float* x, const float* w_mu, const float* w_var,
                                              const float* b_mu, const float* b_var, float* y, float* act_mu_out,
                                              float* act_var_out, const float* eps_ext, uint64_t seed, uint32_t call0,
                                              uint32_t stream_id, int sample, const uint32_t* call_dev, int k_split,
                                              void* scratch, int64_t scratch_bytes, void* stream) {
    PConvArgs a = {};
    int rc = fill(d, a);
    if (rc != 0) return rc;
    if (k_split > 1 && (rc = split_setup(a, d->draws, true, k_split, scratch, scratch_bytes)) != 0) return rc;
    if (x == nullptr || w_mu == nullptr || w_var == nullptr || y == nullptr) return BBB_EINVAL;
    if ((b_mu == nullptr) != (b_var == nullptr)) return BBB_EINVAL;
    if (d->w_draw_stride != 0 || d->b_draw_stride != 0) return BBB_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)y) & 15u) != 0) return BBB_EALIGN;
    if ((((uintptr_t)w_mu | (uintptr_t)w_var | (uintptr_t)b_mu | (uintptr_t)b_var | (uintptr_t)act_mu_out |
          (uintptr_t)act_var_out | (uintptr_t)eps_ext) & 3u) != 0)
        return BBB_EALIGN;
    a.x = x; a.w = w_mu; a.w2 = w_var; a.bias = b_mu; a.bias2 = b_var; a.y = y;
    a.y_mu = act_mu_out; a.y_var = act_var_out; a.eps_ext = eps_ext;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.call0 = call0; a.stream_id = stream_id;
    a.sample = sample ? 1 : 0;
    a.call_dev = call_dev;
    return launch<true>(a, d->draws, (hipStream_t)stream);
}

extern "C" int bbb_lrt_conv2d_chwn_fwd(const bbb_conv_desc_t* d, const float* x, const float* w_mu, const float* w_var,
                                       const float* b_mu, const float* b_var, float* y, float* act_mu_out,
                                       float* act_var_out, const float* eps_ext, uint64_t seed, uint32_t call0,
                                       uint32_t stream_id, int sample, const uint32_t* call_dev, void* stream) {
    return bbb_lrt_conv2d_chwn_splitk_fwd(d, x, w_mu, w_var, b_mu, b_var, y, act_mu_out, act_var_out, eps_ext, seed, call0, stream_id,
                                          sample, call_dev, 1, nullptr, 0, stream);
}
