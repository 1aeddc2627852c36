// First-layer input gradient of the bf16 training backward (bbb_hip/fast_train.py: _MCForwardBF16): the contraction over (draw,
// channel) on bf16 operands,
//     D[(ci, r, q)][n] = sum over k = (e, co) of w[k][(ci, r, q)] * g_pre[k][n],      n = (ho, wo, b),
// on v_mfma_f32_32x32x16_bf16 with fp32 accumulation and an fp32 result that is never rounded; bbb_input_grad_col2im
// (csrc/input_grad.hip) then folds D onto the input pixels, unchanged.
//
// Both operands are read where they are.  The contraction index k is the ROW of both -- w is sample_weights_bf16's [E][cout][Kp]
// rows, g_pre the (draw, channel) planes at their pitch -- so for the MFMA, whose lanes want 8 consecutive k of one row / column,
// k is strided in memory on both sides.  Staging does the turn in registers: a thread loads 8 consecutive k for two neighbouring
// columns (one 4-byte load per k for bf16, one 8-byte load for an fp32 g_pre whose values are bf16-representable: the high half of
// the word IS the bf16 value), packs each column's 8 values into one 16-byte vector and writes it to an LDS image [column][k] whose
// rows the MFMA lanes read back with one ds_read_b128 each.  No transposed copy of the weights, no bf16 copy of an fp32 g_pre.
//
// A workgroup owns tile_j rows of D (32 | 64, a function of cin*kh*kw alone) and 128 columns and walks ALL of k in ascending chunks
// of 32: the contraction is never split, so an element of D is the same number whatever else shares the launch, and a column's
// result does not depend on the other columns.  Tails are masked on both operands: k >= E*cout, rows of D >= cin*kh*kw and
// columns >= ho*wo*batch are staged as zeros and never read from memory (the pad columns of a padded g_pre pitch are not read
// either); only rows < cin*kh*kw and columns < ho*wo*batch of D are written.  The row tiles of one column tile read the same
// tile of g_pre: they are neighbours in the item order, and the items are dealt to the 8 XCDs in runs, so they meet in one L2
// (g_pre is fetched from memory about once, not once per row tile).  The plan, the checks and their order: input_grad_bf16_plan.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "input_grad_bf16_plan.h"

namespace {

using namespace input_grad_bf16_plan;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kLdsPitch = kChunk + 8;        // bf16 per LDS row: 80 bytes, 16-byte aligned, rows spread over the banks

// 8 values (k ascending) of one column, one per low half of v[i], as the 16-byte vector of the LDS image
__device__ __forceinline__ u32x4 pack_k8(const uint32_t (&v)[8]) {
    return u32x4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
}

template <int TJ, bool GF32>
__global__ __launch_bounds__(kThreads) void first_dgrad_bf16_kernel(const Args a) {
    constexpr int WJ = TJ / 32;                  // waves along the rows of D
    constexpr int WN = 4 / WJ;                   // waves along the columns
    constexpr int NT = kTileN / (32 * WN);       // 32-column MFMA tiles per wave
    __shared__ __attribute__((aligned(16))) uint16_t As[TJ * kLdsPitch];          // [row of D][k]
    __shared__ __attribute__((aligned(16))) uint16_t Bs[kTileN * kLdsPitch];      // [column][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // workgroup -> item: the 8 XCDs take workgroups round robin, so XCD x walks items x * per_xcd ...: the j tiles that read one
    // tile of g_pre run next to each other on ONE XCD and share its L2
    const int64_t item = (int64_t)(blockIdx.x & 7) * a.per_xcd + (blockIdx.x >> 3);
    if (item >= a.items) return;                 // (the whole workgroup, before any barrier)
    const int j0 = (int)(item % a.j_tiles) * TJ;
    const int64_t n0 = (item / a.j_tiles) * kTileN;

    // staging roles.  g_pre: every thread one (column pair, k octet) -- a wave's loads of one k run along 128 columns.
    const int g_oct = tid >> 6;
    const int64_t gn = n0 + 2 * lane;
    const bool g_ok = gn < a.ncols;              // (ncols is a multiple of 8: a pair is inside or outside as a whole)
    // weights: the first 2 * TJ threads one (row pair of D, k octet) each; a row of D is a COLUMN of the weight rows -- j itself,
    // or (tap, ci) -> tap * cin + ci for tap-major rows
    const bool w_thread = tid < 2 * TJ;
    const int w_pair = tid % (TJ / 2), w_oct = tid / (TJ / 2);
    int w_col[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = j0 + 2 * w_pair + i;
        w_col[i] = (!w_thread || j >= a.J) ? -1 : a.tap_major ? (j % a.khkw) * a.cin + j / a.khkw : j;
    }

    uint32_t g_lo[8], g_hi[8], w_lo[8], w_hi[8];
    auto load = [&](int c) {
        const int kg = c * kChunk + 8 * g_oct;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = kg + i;
            g_lo[i] = 0u; g_hi[i] = 0u;
            if (g_ok && k < a.M) {
                const int64_t off = (int64_t)k * a.g_pitch + gn;
                if (GF32) {
                    const u32x2 v = *reinterpret_cast<const u32x2*>(static_cast<const float*>(a.g) + off);
                    g_lo[i] = v.x >> 16; g_hi[i] = v.y >> 16;
                } else {
                    const uint32_t v = *reinterpret_cast<const uint32_t*>(static_cast<const uint16_t*>(a.g) + off);
                    g_lo[i] = v & 0xFFFFu; g_hi[i] = v >> 16;
                }
            }
        }
        const int kw_ = c * kChunk + 8 * w_oct;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = kw_ + i;
            const bool in = w_thread && k < a.M;
            const int64_t row = (int64_t)k * a.Kp;
            w_lo[i] = (in && w_col[0] >= 0) ? (uint32_t)a.w[row + w_col[0]] : 0u;
            w_hi[i] = (in && w_col[1] >= 0) ? (uint32_t)a.w[row + w_col[1]] : 0u;
        }
    };

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int wj = wave % WJ, wn = wave / WJ;
    const int fr = lane & 31, fh = lane >> 5;        // the MFMA operand maps: lane (r, h) holds k = 8h .. 8h + 7 of row / column r
    load(0);
    for (int c = 0; c < a.k_chunks; ++c) {
        __syncthreads();                             // the previous chunk's fragments have been read
        *reinterpret_cast<u32x4*>(&Bs[(2 * lane) * kLdsPitch + 8 * g_oct]) = pack_k8(g_lo);
        *reinterpret_cast<u32x4*>(&Bs[(2 * lane + 1) * kLdsPitch + 8 * g_oct]) = pack_k8(g_hi);
        if (w_thread) {
            *reinterpret_cast<u32x4*>(&As[(2 * w_pair) * kLdsPitch + 8 * w_oct]) = pack_k8(w_lo);
            *reinterpret_cast<u32x4*>(&As[(2 * w_pair + 1) * kLdsPitch + 8 * w_oct]) = pack_k8(w_hi);
        }
        __syncthreads();
        if (c + 1 < a.k_chunks) load(c + 1);         // in flight beside the MFMAs below
#pragma unroll
        for (int s = 0; s < kChunk / 16; ++s) {
            const bf16x8 fa = *reinterpret_cast<const bf16x8*>(&As[(wj * 32 + fr) * kLdsPitch + 16 * s + 8 * fh]);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bf16x8 fb = *reinterpret_cast<const bf16x8*>(&Bs[((wn * NT + t) * 32 + fr) * kLdsPitch + 16 * s + 8 * fh]);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[t], 0, 0, 0);
            }
        }
    }

    // C / D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int64_t n = n0 + (wn * NT + t) * 32 + fr;
        if (n >= a.ncols) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + wj * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
            if (j < a.J) a.dcol[(int64_t)j * a.d_pitch + n] = acc[t][r];
        }
    }
}

}  // namespace

extern "C" int bbb_first_layer_dgrad_bf16_plan(const bbb_conv_desc_t* d, int64_t g_row_pitch, int64_t d_row_pitch, uint32_t flags,
                                               int32_t* tile_j, int32_t* tile_n, int32_t* k_chunks, int64_t* blocks) {
    Plan pl;
    if (const int rc = plan(d, g_row_pitch, d_row_pitch, flags, 0, &pl)) return rc;
    if (tile_j) *tile_j = pl.tile_j;
    if (tile_n) *tile_n = kTileN;
    if (k_chunks) *k_chunks = pl.k_chunks;
    if (blocks) *blocks = pl.blocks;
    return 0;
}

extern "C" int bbb_first_layer_dgrad_bf16(const bbb_conv_desc_t* d, const void* g_pre, int64_t g_row_pitch, const void* w, float* dcol,
                                          int64_t d_row_pitch, uint32_t flags, void* stream) {
    int ptr_rc = 0;
    if (g_pre == nullptr || w == nullptr || dcol == nullptr) ptr_rc = BBB_EINVAL;
    else if ((((uintptr_t)g_pre | (uintptr_t)w | (uintptr_t)dcol) & 15u) != 0) ptr_rc = BBB_EALIGN;
    Plan pl;
    if (const int rc = plan(d, g_row_pitch, d_row_pitch, flags, ptr_rc, &pl)) return rc;
    Args a = args_of(d, pl, g_row_pitch, d_row_pitch, flags);
    a.g = g_pre; a.w = static_cast<const uint16_t*>(w); a.dcol = dcol;
    const dim3 grid((unsigned)pl.blocks), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    const bool gf32 = (flags & BBB_BF16_BWD_G_F32) != 0;
    if (pl.tile_j == 64) {
        if (gf32) hipLaunchKernelGGL((first_dgrad_bf16_kernel<64, true>), grid, block, 0, st, a);
        else      hipLaunchKernelGGL((first_dgrad_bf16_kernel<64, false>), grid, block, 0, st, a);
    } else {
        if (gf32) hipLaunchKernelGGL((first_dgrad_bf16_kernel<32, true>), grid, block, 0, st, a);
        else      hipLaunchKernelGGL((first_dgrad_bf16_kernel<32, false>), grid, block, 0, st, a);
    }
    return (int)hipGetLastError();
}
