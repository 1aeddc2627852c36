// Host-side plan of bbb_first_layer_dgrad_bf16 (csrc/input_grad_bf16.hip): the contraction half of a first layer's input gradient
// on bf16 operands,
//     D[(ci, r, q)][n] = sum over k = (e, co) of w[k][(ci, r, q)] * g_pre[k][n],      n = (ho, wo, b),
// everything the entry decides before it touches a pointer or a stream -- the checks, the tile, the grid -- and the kernel-argument
// block that follows from them.  The launch entry and bbb_first_layer_dgrad_bf16_plan call the same function.
// Plain C++17, no HIP headers: tests/host/input_grad_bf16_plan_check.cpp walks this file under the sanitizers.
#ifndef BBB_INPUT_GRAD_BF16_PLAN_H
#define BBB_INPUT_GRAD_BF16_PLAN_H

#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "conv_desc_check.h"

namespace input_grad_bf16_plan {

using conv_desc_check::mul_cap;

constexpr int kThreads = 256;        // four waves
constexpr int kTileN = 128;          // columns (ho, wo, b) per workgroup
constexpr int kChunk = 32;           // rows (e, co) staged per step: two 32x32x16 MFMA k steps
constexpr uint32_t kFlags = BBB_BF16_BWD_G_F32 | BBB_BF16_W_TAP_MAJOR;

struct Plan {
    int32_t ho, wo;                  // the layer's output map = g_pre's
    int32_t M;                       // contraction length E * cout
    int32_t J, Kp;                   // rows of D = cin * kh * kw; the weight rows' pitch, J rounded up to 8
    int64_t ncols;                   // ho * wo * batch: the columns that are read, contracted and written
    int32_t tile_j;                  // rows of D per workgroup: 32 (J <= 32) | 64 -- a function of J alone
    int32_t k_chunks;                // ceil(M / kChunk): the contraction is never split, every workgroup walks all of them in order
    int32_t j_tiles;
    int64_t n_tiles, items;          // items = j_tiles * n_tiles, the j tiles of one column tile next to each other ...
    int32_t per_xcd;                 // ... and dealt to the 8 XCDs in runs of per_xcd (workgroup b is item (b & 7) * per_xcd + (b >> 3)):
    int64_t blocks;                  // the j tiles that read one tile of g_pre share an L2; blocks = 8 * per_xcd
};

// The checks, in this order.  ptr_rc: what the launch entry found on its operand pointers (0; BBB_EINVAL: one is null; BBB_EALIGN:
// one is not 16-byte aligned) -- the plan query passes 0.
//   BBB_EINVAL  a null descriptor or operand; a flag bit other than BBB_BF16_BWD_G_F32 | BBB_BF16_W_TAP_MAJOR; a non-positive size,
//               stride or dilation, a negative padding; a field the LAYER does not have (x_draw_stride, b_draw_stride, act, the work
//               unit / steps-per-launch fields, b_offset, w_row_pitch, pool, w_tap_major) that is not 0; a w_draw_stride other than
//               cout * Kp (the rows of sample_weights_bf16, read in place); tap-major rows with cin % 8 != 0
//   BBB_EALIGN  an operand that is not 16-byte aligned; g_row_pitch % 8 != 0; d_row_pitch % 4 != 0
//   BBB_ESHAPE  a kernel larger than the padded map; batch % 8 != 0; a pitch below ho * wo * batch; cin * kh * kw, E * cout,
//               E * cout * g_row_pitch, E * cout * Kp or cin * kh * kw * d_row_pitch past 2^31 - 1 (element offsets fit 32 bits, as
//               the forward's); a grid that does not fit an int
inline int plan(const bbb_conv_desc_t* d, int64_t g_row_pitch, int64_t d_row_pitch, uint32_t flags, int ptr_rc, Plan* p) {
    *p = Plan{};
    if (d == nullptr || ptr_rc == BBB_EINVAL || (flags & ~kFlags) != 0) return BBB_EINVAL;
    if (!conv_desc_check::positive_geometry(d)) return BBB_EINVAL;
    if (d->x_draw_stride != 0 || d->b_draw_stride != 0 || d->act != 0 || d->w_row_pitch != 0 || d->pool != 0 || d->w_tap_major != 0)
        return BBB_EINVAL;
    if (const int rc = conv_desc_check::unit_fields(d, conv_desc_check::kNothing)) return rc;
    const int64_t J = mul_cap(d->cin, d->kh, d->kw);
    const int64_t Kp = J > 0x7fffffffLL - 7 ? conv_desc_check::kCap : (J + 7) & ~(int64_t)7;
    if (d->w_draw_stride != mul_cap(d->cout, Kp)) return BBB_EINVAL;
    if ((flags & BBB_BF16_W_TAP_MAJOR) != 0 && d->cin % 8 != 0) return BBB_EINVAL;
    if (ptr_rc == BBB_EALIGN || g_row_pitch % 8 != 0 || d_row_pitch % 4 != 0) return BBB_EALIGN;
    int32_t ho = 0, wo = 0;
    if (const int rc = conv_desc_check::out_map(d, &ho, &wo)) return rc;
    if (d->batch % 8 != 0) return BBB_ESHAPE;
    const int64_t ncols = mul_cap(ho, wo, d->batch);
    if (g_row_pitch < ncols || d_row_pitch < ncols) return BBB_ESHAPE;
    const int64_t M = mul_cap(d->draws, d->cout);
    if (J > 0x7fffffffLL || M > 0x7fffffffLL || mul_cap(M, g_row_pitch) > 0x7fffffffLL || mul_cap(M, Kp) > 0x7fffffffLL ||
        mul_cap(J, d_row_pitch) > 0x7fffffffLL)
        return BBB_ESHAPE;
    p->ho = ho; p->wo = wo;
    p->M = (int32_t)M; p->J = (int32_t)J; p->Kp = (int32_t)Kp;
    p->ncols = ncols;
    p->tile_j = J <= 32 ? 32 : 64;
    p->k_chunks = (int32_t)((M + kChunk - 1) / kChunk);
    p->j_tiles = (int32_t)((J + p->tile_j - 1) / p->tile_j);
    p->n_tiles = (ncols + kTileN - 1) / kTileN;
    p->items = mul_cap(p->j_tiles, p->n_tiles);
    if (p->items > 0x7fffffffLL || conv_desc_check::xcd_grid(p->items, &p->per_xcd, &p->blocks) != 0) {
        *p = Plan{};                     // (a refusal leaves no plan behind)
        return BBB_ESHAPE;
    }
    return 0;
}

// The kernel's argument block.
struct Args {
    const void* g;                   // [M][g_pitch] bf16, or fp32 holding bf16 values
    const uint16_t* w;               // [M][Kp] bf16
    float* dcol;                     // [J][d_pitch]
    int M, J, Kp, cin, khkw, j_tiles, k_chunks, tap_major, per_xcd;
    int64_t ncols, g_pitch, d_pitch, items;
};

inline Args args_of(const bbb_conv_desc_t* d, const Plan& pl, int64_t g_row_pitch, int64_t d_row_pitch, uint32_t flags) {
    Args a = {};
    a.M = pl.M; a.J = pl.J; a.Kp = pl.Kp; a.cin = d->cin; a.khkw = d->kh * d->kw; a.j_tiles = pl.j_tiles; a.k_chunks = pl.k_chunks;
    a.tap_major = (flags & BBB_BF16_W_TAP_MAJOR) != 0;
    a.per_xcd = pl.per_xcd; a.items = pl.items;
    a.ncols = pl.ncols; a.g_pitch = g_row_pitch; a.d_pitch = d_row_pitch;
    return a;
}

}  // namespace input_grad_bf16_plan

#endif
