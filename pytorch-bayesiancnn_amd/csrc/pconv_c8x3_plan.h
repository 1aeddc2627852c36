// Host-side launch plan of the split-bf16 contraction over MFMA-ready operands (csrc/pconv_c8x3.hip): everything
// bbb_conv2d_c8x3_fwd / bbb_lrt_conv2d_c8x3_fwd decide before they touch a pointer or a stream -- the flag word, the descriptor
// checks, the zero-border window, the slab limits, the tile rule -- and which of the 20 kernel instantiations the launch starts
// (BBB_C8X3_FORM_* of include/bbb_hip.h, ops.C8X3_FORMS).  The launch entries and bbb_conv2d_c8x3_plan call the same two functions.
// Plain C++17, no HIP headers: tests/host/c8x3_plan_check.cpp walks this file under the sanitizers.
#ifndef BBB_PCONV_C8X3_PLAN_H
#define BBB_PCONV_C8X3_PLAN_H

#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "conv_desc_check.h"

namespace c8x3_plan {

using conv_desc_check::mul_cap;

constexpr int kForms = 20;

// the flag word, decoded
struct Flags {
    bool of32, pool, lrt;
    int nt_force;                // 0 | 2 | 3 | 4
    uint32_t word;
};

struct Plan {
    int32_t form;                // BBB_C8X3_FORM_*
    int32_t nt, mt;              // 32-channel tiles per workgroup (2 | 3 | 4); 32-image fragments per wave (1 | 2)
    int32_t images_per_wg;       // 128 * mt (pooled: 32 * mt)
    int32_t Ntiles, G, nbt, Mtiles, per_xcd;
    int64_t items, blocks;
    // the geometry the entry copies into the kernel-argument block
    int32_t ho, wo, K;
    int32_t vh0, vh1, vw0, vw1;  // rows / columns of the input that are not declared all-zero
    int64_t x_ps, y_ps, y_ds;    // elements per input / output plane, per output slab
};

constexpr int form_of(int nt, int mt, bool of32, bool pool, bool lrt) {
    return lrt ? (of32 ? BBB_C8X3_FORM_LRT_F32 : BBB_C8X3_FORM_LRT_S3) : ((nt - 2) * 2 + (mt - 1)) * 3 + (pool ? 2 : of32 ? 1 : 0);
}

// The checks that come before the LRT entry looks at the alignment of its second operand pair: the flag word, the fields this
// family leaves alone, and what the LRT form gives up.  All BBB_EINVAL.
inline int decode(const bbb_conv_desc_t* d, uint32_t flags, bool lrt, Flags* f) {
    *f = Flags{};
    constexpr uint32_t kKnown = BBB_C8X3_OUT_F32 | BBB_C8X3_TILE128 | BBB_C8X3_TILE256 | BBB_C8X3_POOL | BBB_C8X3_NT_MASK | BBB_C8X3_ZERO_MASK;
    if (d == nullptr || (flags & ~kKnown) != 0 || ((flags & BBB_C8X3_TILE128) && (flags & BBB_C8X3_TILE256))) return BBB_EINVAL;
    if (!conv_desc_check::positive_geometry(d) || d->act < 0 || d->act > 2 || d->pool != 0 || d->w_row_pitch != 0 || d->w_tap_major != 0)
        return BBB_EINVAL;
    f->word = flags;
    f->lrt = lrt;
    f->of32 = (flags & BBB_C8X3_OUT_F32) != 0;
    f->pool = (flags & BBB_C8X3_POOL) != 0;
    f->nt_force = (int)((flags & BBB_C8X3_NT_MASK) >> BBB_C8X3_NT_SHIFT);
    if (f->nt_force == 1 || f->nt_force > 4 || (f->pool && f->of32)) return BBB_EINVAL;
    // LRT: one (mu, sigma^2) weight pair for every slab; 64-channel tiles; pooling is a launch of its own (bbb_maxpool_c8s3_sq)
    if (lrt && (f->pool || (f->nt_force != 0 && f->nt_force != 2) || d->w_draw_stride != 0 || d->b_draw_stride != 0)) return BBB_EINVAL;
    return 0;
}

// The rest, in the order the launcher has always made its checks.  ptr_rc: what the entry's pointer-alignment check found
// (0 | BBB_EALIGN), returned at its place in that order.
inline int plan(const bbb_conv_desc_t* d, const Flags& f, int ptr_rc, Plan* p) {
    *p = Plan{};
    const int sets = f.lrt ? 2 : 1;
    if (d->cin % 16 != 0 || d->batch % 4 != 0 || (!f.of32 && d->cout % 8 != 0)) return BBB_ESHAPE;
    if (const int rc = conv_desc_check::out_map(d, &p->ho, &p->wo)) return rc;
    // the pooled form: no padding (the four pixels of a window walk the same taps), even output height and width
    if (f.pool && (d->pad_h != 0 || d->pad_w != 0 || p->ho % 2 != 0 || p->wo % 2 != 0)) return BBB_ESHAPE;
    if (ptr_rc != 0) return ptr_rc;
    {   // rows / columns of the input the caller declares all-zero (BBB_C8X3_ZERO_* nibbles of flags)
        const int lh = (int)((f.word >> 8) & 15u), lw = (int)((f.word >> 12) & 15u), th = (int)((f.word >> 16) & 15u), tw = (int)((f.word >> 20) & 15u);
        if (lh + th >= d->h || lw + tw >= d->w) return BBB_EINVAL;
        p->vh0 = lh; p->vh1 = d->h - th; p->vw0 = lw; p->vw1 = d->w - tw;
    }
    p->x_ps = mul_cap(d->cin, d->h, d->w, d->batch);
    p->y_ps = mul_cap(d->cout, p->ho, p->wo, d->batch) / (f.pool ? 4 : 1);
    const int64_t K = mul_cap(d->cin, d->kh, d->kw);
    // slabs are addressed through 32-bit buffer offsets (three -- LRT: six -- planes of 2-byte elements, or fp32 outputs)
    if (mul_cap(6 * sets, p->x_ps) >= 0x3FFF0000LL || mul_cap(6 * sets, p->y_ps) >= 0x3FFF0000LL ||
        mul_cap((int64_t)d->cout + 128, K, 4) >= 0x3FFF0000LL)
        return BBB_ESHAPE;
    p->K = (int32_t)K;
    if (d->x_draw_stride != 0 && d->x_draw_stride < 3 * sets * p->x_ps) return BBB_EINVAL;
    if (d->w_draw_stride % 4 != 0 || (!f.of32 && d->b_draw_stride % 4 != 0) || d->x_draw_stride % 8 != 0) return BBB_EALIGN;
    p->y_ds = f.of32 ? p->y_ps : 3 * sets * p->y_ps;
    if (const int rc = conv_desc_check::unit_fields(d, conv_desc_check::kUnitsAndSteps)) return rc;
    const int64_t pixels = (int64_t)p->ho * p->wo / (f.pool ? 4 : 1);
    // Tile shape (the MFMA sequence per output element, hence every output bit, does not depend on it).  Channels per workgroup
    // 32 * NT: NT = 2 unless forced -- wider tiles halve the image fragments' trips through the vector memory path per matrix
    // instruction but hold 96 / 128 accumulation registers (two waves per SIMD instead of three), and measured slower on every
    // AlexNet layer but conv3 (profiles/r06_notes.md: conv2 504 / 515 / 603 us for NT = 2 / 3 / 4 at 40 slabs).  Images per wave
    // 32 * MT: 64, or 32 when the launch would otherwise leave the chip less than ~two rounds of workgroups.
    const int nt = f.nt_force ? f.nt_force : 2;
    int mt = 2;
    const int64_t bm2 = (f.pool ? 32 : 128) * 2;
    const int64_t items2 = mul_cap(d->draws, (d->cout + 32 * nt - 1) / (32 * nt), pixels, (d->batch + bm2 - 1) / bm2);
    if (f.word & BBB_C8X3_TILE128) mt = 1;
    else if (f.word & BBB_C8X3_TILE256) mt = 2;
    else if (d->batch <= bm2 / 2 || items2 < 1024) mt = 1;
    if (f.lrt) mt = 1;                                           // two accumulator sets: 32 images per wave
    const int bnw = 32 * nt, bm = (f.pool ? 32 : 128) * mt;
    p->nt = nt; p->mt = mt; p->images_per_wg = bm;
    p->Ntiles = (d->cout + bnw - 1) / bnw;
    const int64_t G = (int64_t)p->Ntiles * d->draws;
    if (G > 0x7fffffffLL) return BBB_ESHAPE;
    p->G = (int32_t)G;
    p->nbt = (d->batch + bm - 1) / bm;
    const int64_t mtiles = pixels * p->nbt;
    if (mtiles > 0x7fffffffLL) return BBB_ESHAPE;
    p->Mtiles = (int32_t)mtiles;
    p->items = G * mtiles;
    p->form = form_of(nt, mt, f.of32, f.pool, f.lrt);
    return conv_desc_check::xcd_grid(p->items, &p->per_xcd, &p->blocks);
}

}  // namespace c8x3_plan

#endif
