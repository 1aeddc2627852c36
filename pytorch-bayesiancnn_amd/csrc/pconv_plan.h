// Host-side launch plan of the batch-innermost fp32 implicit GEMM (csrc/pconv_gemm.hip, csrc/pconv_body.cuh): the descriptor
// checks, the layer's split of its contraction, and which of the fifteen launch forms a launch takes -- tile width, staging
// interleaved or not, the split across workgroups or inside one, the pooled forms -- with its item count and grid; the same tile
// rule applied to the transposed launch (dgrad_plan: csrc/pconv_dgrad.hip) and to the grid of bbb_conv2d_chwn_bf16x3_fwd.  What
// every family checks on a descriptor comes from conv_desc_check.h.  Plain C++17, no HIP headers: launch<LRT>() takes its kernel
// and grid from here, bbb_conv2d_chwn_plan / bbb_conv2d_chwn_dgrad_plan report them, and tests/host/pconv_plan_check.cpp walks
// this file under the sanitizers.
#ifndef BBB_PCONV_PLAN_H
#define BBB_PCONV_PLAN_H

#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "conv_desc_check.h"

// launches of more 64-image items than this run the in-workgroup form of a layer's split (measured, profiles/r03_notes.md
// section 2 and r04_notes.md: above ~400 items the cross-workgroup form only adds partial-tile traffic; LRT items carry two
// accumulator sets and their in-workgroup form runs at 3 waves per SIMD, so the crossover sits higher)
#ifndef PCONV_ILV_MAX
#define PCONV_ILV_MAX 12000          // launches of at most this many items interleave their staging loads with the MFMAs (see plan())
#endif
#ifndef PCONV_SPLIT_MAX
#define PCONV_SPLIT_MAX 384
#endif

namespace pconv_plan {

using conv_desc_check::mul_cap;
using conv_desc_check::xcd_grid;

constexpr int kBN = 64;                           // output channels per item (pconv::BN)
constexpr int kBK = 32;                           // contraction elements per k tile (pconv::BK)
constexpr int64_t kTicketBytes = 16384;           // arrival counters of up to 4096 items
constexpr int64_t split_max_items(bool lrt) { return lrt ? 512 : PCONV_SPLIT_MAX; }

// The launch forms = the kernel instantiations launch<LRT>() can start (BBB_FP32_FORM_* of include/bbb_hip.h, ops.FP32_FORMS).
enum Form : int32_t {
    kBbb64Ilv = 0,      // pconv_gemm_kernel<64, false, true>
    kBbb64 = 1,         // pconv_gemm_kernel<64, false, false>
    kBbb128Ilv = 2,     // pconv_gemm_kernel<128, false, true>
    kBbb128 = 3,        // pconv_gemm_kernel<128, false, false>
    kBbbSeq64Ilv = 4,   // pconv_gemm_kernel<64, false, true, true>
    kBbbSeq64 = 5,      // pconv_gemm_kernel<64, false, false, true>
    kBbbSeq128Ilv = 6,  // pconv_gemm_kernel<128, false, true, true>
    kBbbSeq128 = 7,     // pconv_gemm_kernel<128, false, false, true>
    kBbbCross = 8,      // pconv_gemm_splitk_kernel<64, false, true>
    kBbbPool = 9,       // pconv_gemm_pool_kernel<false>
    kLrt64Ilv = 10,     // pconv_gemm_kernel<64, true, true>
    kLrt64 = 11,        // pconv_gemm_kernel<64, true, false>
    kLrtSeq64 = 12,     // pconv_gemm_kernel<64, true, false, true>
    kLrtCross = 13,     // pconv_gemm_splitk_kernel<64, true, true>
    kLrtPool = 14,      // pconv_gemm_pool_lrt_kernel
    kForms = 15
};

// What fill() of pconv_gemm.hip copies into the kernel-argument block.
struct Geom {
    int32_t B, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo;
    int32_t K, Kp, khkw, act;
    int32_t unit_div, unit_off, x_mod, b_off, x_div, x_off, pool, wtap;
    uint32_t x_inv;
    int64_t x_ds, w_ds, b_ds, y_ds;
};

struct Plan {
    int32_t form;       // Form
    int32_t bm;         // images per item: 64 | 128
    int32_t ilv;        // staging loads interleaved with the MFMAs
    int32_t nbt;        // image tiles per pixel
    int32_t Mtiles;     // (pixel, image tile) pairs per (draw, channel tile) group; pooled forms: pooled pixels
    int32_t Ntiles, G;  // channel tiles; (draw, channel tile) groups
    int32_t per_xcd;    // items (cross form: blocks of work) per XCD chunk
    int64_t items;      // work items of the launch
    int64_t blocks;     // workgroups of the launch
};

// The limits of 32-bit buffer offsets into one draw's slabs, for a launch that writes an ho x wo map; -> PConvArgs::x_inv
inline int slab_limits(const bbb_conv_desc_t* d, int32_t ho, int32_t wo, uint32_t* x_inv) {
    if (mul_cap(d->cin, d->h, d->w) > 0x7fffffffLL || mul_cap(d->cin, d->kh, d->kw) > 0x7fffffffLL) return BBB_ESHAPE;
    // per-draw slabs are addressed through 32-bit buffer offsets
    const int64_t x_bytes = mul_cap(d->cin, d->h, d->w, (int64_t)d->batch * 4);
    if (x_bytes > 0xFFFE0000LL || mul_cap(d->cout, ho, wo, (int64_t)d->batch * 4) > 0xFFFE0000LL ||
        mul_cap((int64_t)d->cout + 64, d->cin, d->kh, (int64_t)d->kw * 4) > 0x3FFFFFFFLL || (int64_t)d->batch * 4 > 0x0FFFFFFFLL)
        return BBB_ESHAPE;
    *x_inv = (0xFFFFFFF0u - ((uint32_t)d->batch + 512u) * 4u) & ~15u;   /* a ragged last tile reaches < 512 columns past the row */
    return x_bytes > (int64_t)*x_inv ? BBB_ESHAPE : 0;
}

// The descriptor checks of every batch-innermost fp32 forward entry, in the order the entries have always made them.
inline int describe(const bbb_conv_desc_t* d, Geom* g) {
    if (d == nullptr) return BBB_EINVAL;
    *g = Geom{};
    if (!conv_desc_check::positive_geometry(d) || d->act < 0 || d->act > 2) return BBB_EINVAL;
    if (d->batch % 4 != 0) return BBB_ESHAPE;        // batch-innermost rows are moved as 16-byte vectors
    int32_t ho = 0, wo = 0;
    if (const int rc = conv_desc_check::out_map(d, &ho, &wo)) return rc;
    if (const int rc = slab_limits(d, ho, wo, &g->x_inv)) return rc;
    g->B = d->batch; g->Cin = d->cin; g->H = d->h; g->W = d->w; g->Cout = d->cout; g->kh = d->kh; g->kw = d->kw;
    g->sh = d->stride_h; g->sw = d->stride_w; g->ph = d->pad_h; g->pw = d->pad_w; g->dh = d->dil_h; g->dw = d->dil_w;
    g->Ho = ho; g->Wo = wo; g->K = d->cin * d->kh * d->kw; g->khkw = d->kh * d->kw; g->act = d->act;
    if (d->w_row_pitch < 0 || (d->w_row_pitch > 0 && d->w_row_pitch < g->K)) return BBB_EINVAL;
    g->Kp = d->w_row_pitch > 0 ? d->w_row_pitch : g->K;
    if (mul_cap((int64_t)d->cout + 64, g->Kp, 4) > 0x3FFFFFFFLL) return BBB_ESHAPE;
    g->x_ds = d->x_draw_stride; g->w_ds = d->w_draw_stride; g->b_ds = d->b_draw_stride;
    g->y_ds = (int64_t)d->cout * ho * wo * d->batch;
    if (d->b_offset < 0 || conv_desc_check::unit_fields(d, conv_desc_check::kUnitsAndSteps) != 0) return BBB_EINVAL;
    g->unit_div = d->unit_div; g->unit_off = d->unit_div > 1 ? d->unit_off : 0; g->x_mod = d->x_unit_mod; g->b_off = d->b_offset;
    g->x_div = d->x_unit_div; g->x_off = d->x_unit_off;
    if (d->pool != 0 && d->pool != 1) return BBB_EINVAL;
    g->pool = d->pool;
    if (d->w_tap_major != 0 && d->w_tap_major != 1) return BBB_EINVAL;
    g->wtap = d->w_tap_major;
    if (g->pool) {
        if ((ho & 1) || (wo & 1)) return BBB_EINVAL;
        g->y_ds = (int64_t)d->cout * (ho / 2) * (wo / 2) * d->batch;
    }
    return 0;
}

// The split of a LAYER's contraction: a function of the layer's geometry ONLY (not of the batch, the number of draws or how a
// step is partitioned), so that every launch that computes an output element of this layer -- one draw alone, a 10-draw
// launch, a work unit of a sharded step, one of G steps per launch, a batch-parallel shard -- adds the same partial sums in the
// same order (cross-workgroup SPLIT form for small launches, in-workgroup SEQ form otherwise: same bits).
// Which layers: few (pixel, 64-channel tile) groups and a long contraction -- a draw of such a layer is a handful of workgroups
// each walking a long serial k loop (AlexNet conv4: 4 pixels x 4 tiles, 48 k tiles; conv5: 4 x 2, 32 tiles; measured one draw,
// bs 512: 42 -> 28 us and 28 -> 17 us with four ranges, profiles/r03_notes.md section 2).  Layers with more groups (conv2: 48, conv3:
// 24) fill the chip from a few hundred images on and keep the plain chain.
inline int canonical_ksplit(const Geom& a) {
    const int ntl = (a.Cout + kBN - 1) / kBN;
    const int64_t groups = (int64_t)a.Ho * a.Wo * ntl;
    if (groups > 16) return 1;
    // longest contraction of any pixel, in 32-k tiles (taps that can fall inside the image)
    const int nr = a.kh < (a.H - 1) / a.dh + 1 ? a.kh : (a.H - 1) / a.dh + 1;
    const int nq = a.kw < (a.W - 1) / a.dw + 1 ? a.kw : (a.W - 1) / a.dw + 1;
    const int tiles = (int)(((int64_t)a.Cin * nr * nq + kBK - 1) / kBK);        // (<= Cin * kh * kw, which describe() holds below 2^31)
    if (tiles < 16) return 1;
    const int s = tiles / 8;                                             // >= 8 tiles per range
    return s > 4 ? 4 : s;
}

// Scratch bytes the cross-workgroup form of this launch needs (0: the launch is too large for it and runs the SEQ form).
inline int64_t split_scratch_bytes(const Geom& a, int draws, bool lrt, int s) {
    if (s <= 1) return 0;
    const int ntl = (a.Cout + kBN - 1) / kBN;
    // (split layers have at most 16 pixel x channel-tile groups; image tiles < 2^26, draws < 2^31: the product stays in 64 bits)
    const int64_t items = (int64_t)a.Ho * a.Wo * ntl * ((a.B + 63) / 64) * draws;
    if (items > split_max_items(lrt)) return 0;
    // tickets live in a FIXED region at the start of the scratch (split launches have < 512 items), so that launches of
    // different sizes sharing one scratch buffer never put partial tiles where another launch expects zeroed tickets
    return kTicketBytes + items * s * (lrt ? 2 : 1) * 64 * 64 * 4;
}

// ---- the pieces the forward's plain branch, the transposed launch (dgrad_plan) and bbb_conv2d_chwn_bf16x3_fwd share ----
// channel tiles and (draw, channel tile) groups
inline int channel_groups(int cout, int draws, Plan* p) {
    p->Ntiles = (cout + kBN - 1) / kBN;
    const int64_t G = (int64_t)p->Ntiles * draws;
    if (G > 0x7fffffffLL) return BBB_ESHAPE;
    p->G = (int32_t)G;
    return 0;
}

// tile choice: 128 images per workgroup (two accumulator chains per wave) unless that leaves fewer than 3
// workgroups per CU, then 64.  A 256-image tile (64x64 per wave) exists but measured 5-10 % slower on every
// AlexNet layer (3 instead of 4 workgroups per CU); the launcher never selects it.
// LRT stages two weight tiles and keeps two accumulator sets: 64-wide only.
inline int image_tile(int B, int64_t pixels, int64_t G, bool lrt) {
    // (the slab limits hold Ho * Wo * B below 2^30 and G is below 2^31: the item counts stay inside 64 bits)
    const int64_t nb128 = pixels * ((B + 127) / 128) * G;
    if (lrt || nb128 < 768) return 64;               // (round 3 re-measured 600 / 300: conv4 +10 %, conv5 +25 % slower with 128)
    // an image axis that 128-wide tiles would pad by >= 25 % and 64-wide ones by less (192 = the input channels of conv3's
    // role-swapped weight gradient: 256 against 192): 64.  Same sums per element either way.
    const int64_t pad128 = ((int64_t)B + 127) / 128 * 128, pad64 = ((int64_t)B + 63) / 64 * 64;
    return (pad128 * 4 >= (int64_t)B * 5 && pad64 < pad128) ? 64 : 128;
}

// nbt, Mtiles, items, the grid and the interleave choice of a launch of bm-image items (p->G set by channel_groups)
inline int item_grid(int B, int64_t pixels, int bm, Plan* p) {
    p->bm = bm;
    p->nbt = (B + bm - 1) / bm;
    const int64_t mt = pixels * p->nbt;
    if (mt > 0x7fffffffLL) return BBB_ESHAPE;
    p->Mtiles = (int32_t)mt;
    p->items = (int64_t)p->G * mt;
    // staging loads interleaved with the MFMAs (ILV): round 1 measured it a loss beyond ~1.5 rounds of workgroups; re-measured in
    // round 3 on the current kernel (profiles/r03_notes.md section 3) it is a 1-2 % gain up to ~12k items, one or three steps in flight
    p->ilv = p->items <= PCONV_ILV_MAX;
    return xcd_grid(p->items, &p->per_xcd, &p->blocks);
}

// The form of one launch.  k_split: what the caller passed (<= 1: no split; otherwise it must be the layer's plan);
// has_scratch: the caller gave scratch for the cross-workgroup form (it is used only when split_scratch_bytes() is not 0).
inline int plan(const Geom& a, int draws, bool lrt, int k_split, bool has_scratch, Plan* p) {
    *p = Plan{};
    int ksplit = 0;
    if (k_split > 1) {
        if (k_split != canonical_ksplit(a)) return BBB_EINVAL;               // the split is the layer's, not the caller's choice
        ksplit = k_split;
    }
    const bool part = ksplit > 1 && has_scratch && split_scratch_bytes(a, draws, lrt, ksplit) > 0;
    if (const int rc = channel_groups(a.Cout, draws, p)) return rc;
    const int64_t G = p->G;
    const int64_t pixels = (int64_t)a.Ho * a.Wo;
    if (a.pool) {
        // one item per POOLED pixel, 128-image tiles (LRT: 64) (the callers fuse large launches only)
        if (ksplit > 1) return BBB_EINVAL;
        p->bm = lrt ? 64 : 128;
        p->nbt = (a.B + p->bm - 1) / p->bm;
        const int64_t mtp = (pixels / 4) * p->nbt;
        const int64_t itp = G * mtp;
        if (mtp > 0x7fffffffLL || itp > 0x7fffffffLL - 8) return BBB_ESHAPE;
        p->Mtiles = (int32_t)mtp;
        // staging loads up front (ILV = false): with the running maximum in 32 more accumulation registers this form fits four
        // workgroups per CU (60 + 64 registers) and the interleaved one does not (82 + 64: three; measured 492-494 us against 480-482
        // for conv1 of the metric step, profiles/r04_notes.md section 7)
        p->ilv = 0;
        p->form = lrt ? kLrtPool : kBbbPool;
        p->items = itp;
        return xcd_grid(itp, &p->per_xcd, &p->blocks);
    }
    const int64_t items64 = pixels * ((a.B + 63) / 64) * G;
    const bool cross = part && items64 <= split_max_items(lrt);
    const int bm = cross ? 64 : image_tile(a.B, pixels, G, lrt);
    if (const int rc = item_grid(a.B, pixels, bm, p)) return rc;
    const int64_t items = p->items;
    if (cross) {
        // the layer's split contraction ACROSS workgroups: a launch this small cannot fill the chip otherwise
        if (items * ksplit > 0x7fffffffLL) return BBB_EINVAL;
        p->ilv = 1;
        p->form = lrt ? kLrtCross : kBbbCross;
        return xcd_grid(items * ksplit, &p->per_xcd, &p->blocks);
    }
    const bool ilv = p->ilv != 0;
    if (ksplit > 1) {
        // the same summation order inside ONE workgroup per item (pconv_body.cuh, SEQ): no scratch, no extra traffic
        if (!lrt && bm == 128) {
            // (88-100 VGPRs + 64 accumulation registers = three workgroups per CU; held to four by amdgpu_waves_per_eu the
            // prefetched tile spills around the range folds and the launch is 4-9 % slower: profiles/r04_notes.md section 4)
            p->ilv = ilv;
            p->form = ilv ? kBbbSeq128Ilv : kBbbSeq128;
            return 0;
        }
        const bool ilv_seq = ilv && !lrt;        // LRT: the interleaved form needs 172 registers (2 waves per SIMD), the plain one 161 (3)
        p->ilv = ilv_seq;
        p->form = lrt ? kLrtSeq64 : ilv_seq ? kBbbSeq64Ilv : kBbbSeq64;
        return 0;
    }
    p->ilv = ilv;
    if (lrt) p->form = ilv ? kLrt64Ilv : kLrt64;
    else if (bm == 128) p->form = ilv ? kBbb128Ilv : kBbb128;
    else p->form = ilv ? kBbb64Ilv : kBbb64;
    return 0;
}

// ---- bbb_conv2d_chwn_dgrad: the transposed launch (csrc/pconv_dgrad.hip) ----
// d describes the stride-1 launch on the flipped weights (its h x w is g's map); the layer's stride travels as the upsampling
// factors and out_h x out_w is dx's map.  The entry's checks in the order it has always made them, then the forward's own tile
// rule: image_tile() and item_grid() of the plain form, never LRT, never a split contraction (p->form stays 0: the entry picks
// pconv_dgrad_kernel<bm, ilv>).  ptr_rc: what the entry's operand-pointer checks found (0 | BBB_EINVAL | BBB_EALIGN), returned at
// their place in the order.
inline int dgrad_plan(const bbb_conv_desc_t* d, int up_h, int up_w, int out_h, int out_w, int ptr_rc, uint32_t* x_inv, Plan* p) {
    *p = Plan{};
    if (d == nullptr) return BBB_EINVAL;
    if (!conv_desc_check::positive_geometry(d) || up_h <= 0 || up_w <= 0 || out_h <= 0 || out_w <= 0) return BBB_EINVAL;
    if (d->stride_h != 1 || d->stride_w != 1) return BBB_EINVAL;
    if (up_h == 1 && up_w == 1) return BBB_EINVAL;          // a stride-1 layer's gradient is bbb_conv2d_chwn_fwd: one way to compute it
    if (d->act != 0 || d->pool != 0 || d->w_tap_major != 0 || d->w_row_pitch != 0 ||
        conv_desc_check::unit_fields(d, conv_desc_check::kNothing) != 0)
        return BBB_EINVAL;
    if (d->x_draw_stride < 0 || d->w_draw_stride < 0) return BBB_EINVAL;
    if (d->batch % 4 != 0) return BBB_ESHAPE;
    // (out_h, out_w) must be a map whose forward (padding p = d (k - 1) - q >= 0, stride up) gives exactly the g map of d
    const int64_t fph = (int64_t)d->dil_h * (d->kh - 1) - d->pad_h, fpw = (int64_t)d->dil_w * (d->kw - 1) - d->pad_w;
    if (fph < 0 || fpw < 0) return BBB_ESHAPE;
    int32_t gh = 0, gw = 0;
    if (conv_desc_check::out_axis(out_h, fph, d->dil_h, d->kh, up_h, &gh) != 0 ||
        conv_desc_check::out_axis(out_w, fpw, d->dil_w, d->kw, up_w, &gw) != 0 || gh != d->h || gw != d->w)
        return BBB_ESHAPE;
    if (const int rc = slab_limits(d, out_h, out_w, x_inv)) return rc;
    if (ptr_rc != 0) return ptr_rc;
    if (const int rc = channel_groups(d->cout, d->draws, p)) return rc;
    const int64_t pixels = (int64_t)out_h * out_w;
    return item_grid(d->batch, pixels, image_tile(d->batch, pixels, p->G, false), p);
}

}  // namespace pconv_plan

#endif
