// Host-side plan of bbb_conv2d_fwd / bbb_lrt_conv2d_fwd (csrc/conv_gemm.hip): the reference-layout implicit GEMM
//     D[n][m] = sum_k W[n][k] * X[k][m],      m = (b, oh, ow), k = (ci, r, q),
// everything the two entries decide before they touch a pointer or a stream -- the checks, the instantiation
// conv_gemm_kernel<BM, LRT, LINEAR> and the grid.  The launch entries and bbb_conv2d_fwd_plan call the same function.
// Plain C++17, no HIP headers: tests/host/conv_gemm_plan_check.cpp walks this file under the sanitizers.
#ifndef BBB_CONV_GEMM_PLAN_H
#define BBB_CONV_GEMM_PLAN_H

#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "conv_desc_check.h"

namespace conv_gemm_plan {

using conv_desc_check::mul_cap;

constexpr int kTileN = 64;           // output channels per workgroup
constexpr int kBkBbb = 32;           // k per LDS tile
constexpr int kBkLrt = 16;           // ... of the LRT form, which stages two weight tiles
constexpr int64_t kWideBlocks = 3 * 256;   // the 128-pixel tile from three workgroups per CU on

struct Plan {
    int32_t ho, wo;                  // the output map
    int32_t M, K;                    // pixels (b, oh, ow) of a draw; contraction length cin * kh * kw
    int64_t y_ds;                    // elements between the output slabs of two draws
    int32_t bm;                      // pixels per workgroup: 64 | 128
    int32_t linear;                  // 1: x is read as the [M][K] row-major matrix it is (1 x 1 taps on a 1 x 1 map, no padding)
    int32_t bk;                      // k per LDS tile: 32 | 16 (LRT)
    int32_t k_tiles;                 // ceil(K / bk): trips of the double-buffered loop
    int32_t grid[3];                 // (pixel tiles, channel tiles, draws): each fits an int
};

// What a launch entry found on its operands; the plan query passes none.
struct Operands {
    bool null_operand = false;       // x, w (w_mu, w_var) or y is NULL
    bool half_a_bias = false;        // LRT: b_mu without b_var, or the reverse
    uintptr_t address_bits = 0;      // OR of every operand's address, the optional ones included
};

// The checks, in this order.
//   BBB_EINVAL  a null descriptor; a non-positive size, stride or dilation, a negative padding; act outside 0..2; a work-unit or
//               steps-per-launch field, b_offset, w_row_pitch, pool or w_tap_major that is not 0 (batch-innermost entries only)
//   BBB_ESHAPE  a kernel larger than the padded map; batch * ho * wo, cin * kh * kw or cin * h * w past 2^31 - 1 (pixel, k and
//               per-image offsets are int32); h + pad_h + dil_h * kh or its width twin at or beyond 0x7000 (a tap's row and
//               column offsets travel as two 16-bit halves, 0x7fff marking a k past K)
//   BBB_EINVAL  a NULL x, w or y; LRT: half a bias, a weight or bias draw stride (the slabs share one pair of moments)
//   BBB_EALIGN  an operand that is not 4-byte aligned
inline int plan(const bbb_conv_desc_t* d, bool lrt, const Operands& o, Plan* p) {
    *p = Plan{};
    if (d == nullptr) return BBB_EINVAL;
    using namespace conv_desc_check;
    if (!positive_geometry(d) || d->act < 0 || d->act > 2) return BBB_EINVAL;
    if (unit_fields(d, kNothing) != 0 || d->w_row_pitch != 0 || d->pool != 0 || d->w_tap_major != 0) return BBB_EINVAL;
    int32_t ho = 0, wo = 0;
    if (const int rc = out_map(d, &ho, &wo)) return rc;
    const int64_t M = mul_cap(d->batch, ho, wo);
    const int64_t K = mul_cap(d->cin, d->kh, d->kw);
    if (M > 0x7fffffffLL || K > 0x7fffffffLL) return BBB_ESHAPE;
    if (mul_cap(d->cin, d->h, d->w) > 0x7fffffffLL) return BBB_ESHAPE;
    if ((int64_t)d->h + d->pad_h + (int64_t)d->dil_h * d->kh >= 0x7000 || (int64_t)d->w + d->pad_w + (int64_t)d->dil_w * d->kw >= 0x7000)
        return BBB_ESHAPE;
    if (o.null_operand) return BBB_EINVAL;
    if (lrt && (o.half_a_bias || d->w_draw_stride != 0 || d->b_draw_stride != 0)) return BBB_EINVAL;
    if ((o.address_bits & 3u) != 0) return BBB_EALIGN;
    p->ho = ho; p->wo = wo; p->M = (int32_t)M; p->K = (int32_t)K;
    p->y_ds = mul_cap(d->batch, d->cout, ho, wo);
    p->linear = d->h == 1 && d->w == 1 && d->kh == 1 && d->kw == 1 && d->pad_h == 0 && d->pad_w == 0;
    p->bk = lrt ? kBkLrt : kBkBbb;
    p->k_tiles = (int32_t)((K + p->bk - 1) / p->bk);
    // Smaller pixel tile when the 128-wide grid would not give every CU a few blocks.  (64-bit throughout: M + 127 and
    // cout + 63 leave the int range for descriptors the checks above admit.)
    const int64_t n_tiles = ((int64_t)d->cout + kTileN - 1) / kTileN;
    const int64_t blocks128 = mul_cap((M + 127) / 128, n_tiles, d->draws);
    p->bm = blocks128 >= kWideBlocks ? 128 : 64;
    p->grid[0] = (int32_t)((M + p->bm - 1) / p->bm);
    p->grid[1] = (int32_t)n_tiles;
    p->grid[2] = d->draws;
    return 0;
}

}  // namespace conv_gemm_plan

#endif
