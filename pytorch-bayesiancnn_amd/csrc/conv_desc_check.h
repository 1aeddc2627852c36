// The one statement of the checks every entry makes on a bbb_conv_desc_t (include/bbb_hip.h) before it looks at anything of its
// own: positive sizes, the output map, the work-unit fields, and the two pieces of guarded arithmetic the launchers share (a
// capped product and the grid of a launch dealt to the 8 XCDs).  Nothing family-specific lives here: which fields an entry admits,
// its slab limits and its tile rule stay in the family's plan header (pconv_plan.h, pconv_bf16_plan.h, pconv_c8x3_plan.h).
// Plain C++17, no HIP headers, like the plan headers, so the host programs under tests/host walk it under the sanitizers.
#ifndef BBB_CONV_DESC_CHECK_H
#define BBB_CONV_DESC_CHECK_H

#include <stdint.h>

#include "../../include/bbb_hip.h"

namespace conv_desc_check {

// a * b for positive factors, capped far above every limit it is compared with (no signed overflow on absurd descriptors)
constexpr int64_t kCap = (int64_t)1 << 62;
inline int64_t mul_cap(int64_t a, int64_t b) { return a > kCap / b ? kCap : a * b; }
inline int64_t mul_cap(int64_t a, int64_t b, int64_t c, int64_t e = 1) { return mul_cap(mul_cap(mul_cap(a, b), c), e); }

// the map itself: images, input channels, the input map, taps, strides, padding, dilation
inline bool positive_map(const bbb_conv_desc_t* d) {
    return d->batch > 0 && d->cin > 0 && d->h > 0 && d->w > 0 && d->kh > 0 && d->kw > 0 && d->stride_h > 0 && d->stride_w > 0 &&
           d->pad_h >= 0 && d->pad_w >= 0 && d->dil_h > 0 && d->dil_w > 0;
}
// ... and what a launch adds: output channels and slabs
inline bool positive_geometry(const bbb_conv_desc_t* d) { return positive_map(d) && d->cout > 0 && d->draws > 0; }

// One axis of the output map, o = (n + 2 pad - dil (k - 1) - 1) / stride + 1, in 64 bits (n + 2 pad and dil (k - 1) of a hostile
// descriptor leave the int range).  A kernel that reaches past the padded input is refused: C's division rounds a negative
// numerator towards zero, which for a stride above 1 would name one output row where there is none.
inline int out_axis(int64_t n, int64_t pad, int64_t dil, int64_t k, int64_t stride, int32_t* o) {
    const int64_t num = n + 2 * pad - dil * (k - 1) - 1;
    if (num < 0) return BBB_ESHAPE;
    const int64_t v = num / stride + 1;
    if (v > 0x7fffffffLL) return BBB_ESHAPE;
    *o = (int32_t)v;
    return 0;
}

inline int out_map(const bbb_conv_desc_t* d, int32_t* ho, int32_t* wo) {
    if (out_axis(d->h, d->pad_h, d->dil_h, d->kh, d->stride_h, ho) != 0) return BBB_ESHAPE;
    return out_axis(d->w, d->pad_w, d->dil_w, d->kw, d->stride_w, wo);
}

// The work-unit fields (unit_div, unit_off, x_unit_mod) and the steps-per-launch fields (x_unit_div, x_unit_off), by what an
// entry admits.  kNothing: all of them and b_offset are zero (the dgrad entries, conv_gemm).  kSteps: steps per launch, no work
// units (the bf16 LRT entry).  kUnitsAndSteps: either, never both (the batch-innermost forwards).
enum Admits { kNothing, kSteps, kUnitsAndSteps };
inline int unit_fields(const bbb_conv_desc_t* d, Admits admits) {
    if (admits == kNothing)
        return (d->unit_div != 0 || d->unit_off != 0 || d->x_unit_mod != 0 || d->x_unit_div != 0 || d->x_unit_off != 0 || d->b_offset != 0)
                   ? BBB_EINVAL : 0;
    if (admits == kSteps) {
        if (d->unit_div > 1 || d->unit_off != 0 || d->x_unit_mod != 0) return BBB_EINVAL;
    } else {
        if (d->unit_div < 0 || d->unit_off < 0 || d->x_unit_mod < 0) return BBB_EINVAL;
        if (d->unit_div > 1 && d->unit_off >= d->unit_div) return BBB_EINVAL;          // passed reduced modulo S
        if (d->x_unit_mod > 0 && d->x_unit_mod != d->unit_div) return BBB_EINVAL;
    }
    if (d->x_unit_div < 0 || d->x_unit_off < 0 || (d->x_unit_div > 1 && (d->unit_div > 1 || d->x_unit_off >= d->x_unit_div)) ||
        (d->x_unit_div <= 1 && d->x_unit_off != 0))
        return BBB_EINVAL;
    return 0;
}

// `items` work items dealt to the 8 XCDs in chunks of per_xcd: the grid is 8 * per_xcd workgroups and must fit an int
inline int xcd_grid(int64_t items, int32_t* per_xcd, int64_t* blocks) {
    const int64_t per = (items + 7) / 8;
    if (8 * per > 0x7fffffffLL) return BBB_ESHAPE;
    *per_xcd = (int32_t)per;
    *blocks = 8 * per;
    return 0;
}

}  // namespace conv_desc_check

#endif
