// Host-only walk of the launch plan of the split-bf16 contraction over MFMA-ready operands (csrc/pconv_c8x3_plan.h) for
// tests/test_c8x3_plan_cpu.py, which builds this file with -fsanitize=address,undefined: decode() and plan() over a seeded sweep of
// ordinary layers, over launches on both sides of the two thresholds of the tile rule (items2 = 1024, B = bm2 / 2), and over
// descriptors at the integer limits (2^31 - 1 in each field in turn, padding and dilation included; draws x channel tiles past
// 2^31).  Checks the plan's invariants and prints how often each form and each refusal came up, and a checksum of everything returned.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../pytorch-bayesiancnn_amd/csrc/pconv_c8x3_plan.h"

namespace {

using namespace c8x3_plan;

uint64_t state = 0x9E3779B97F4A7C15ull, sum = 0xcbf29ce484222325ull;
uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
int pick(const int* v, int n) { return v[rnd() % (uint32_t)n]; }
void mix(int64_t v) { sum = (sum ^ (uint64_t)v) * 0x100000001b3ull; }

long counts[4];        // ok / EINVAL / EALIGN / ESHAPE
long forms[kForms];
long mt_reason[5];     // flag, LRT, B <= bm2 / 2, items2 < 1024, neither

void fail(const char* what, long i) {
    printf("invariant broken: %s (case %ld)\n", what, i);
    exit(1);
}

int walk(const bbb_conv_desc_t* d, uint32_t flags, bool lrt, long i, Plan* out = nullptr) {
    Flags f;
    Plan p;
    int rc = decode(d, flags, lrt, &f);
    if (rc == 0) rc = plan(d, f, 0, &p);
    mix(rc);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
    if (rc != 0) return rc;
    if (out) *out = p;
    if (p.form < 0 || p.form >= kForms) fail("form range", i);
    forms[p.form] += 1;
    mix(p.form); mix(p.nt); mix(p.mt); mix(p.images_per_wg); mix(p.Ntiles); mix(p.G); mix(p.nbt); mix(p.Mtiles); mix(p.per_xcd);
    mix(p.items); mix(p.blocks); mix(p.ho); mix(p.wo); mix(p.K); mix(p.vh0); mix(p.vh1); mix(p.vw0); mix(p.vw1); mix(p.x_ps); mix(p.y_ps); mix(p.y_ds);
    if (p.blocks != 8 * (int64_t)p.per_xcd || p.blocks < p.items || p.blocks >= p.items + 8 || p.blocks > 0x7fffffffLL) fail("grid", i);
    if (p.items != (int64_t)p.G * p.Mtiles || p.items <= 0 || p.G != (int64_t)p.Ntiles * d->draws) fail("items", i);
    if ((int64_t)p.Ntiles * 32 * p.nt < d->cout || (int64_t)(p.Ntiles - 1) * 32 * p.nt >= d->cout) fail("channel tiles", i);
    if ((int64_t)p.nbt * p.images_per_wg < d->batch || (int64_t)(p.nbt - 1) * p.images_per_wg >= d->batch) fail("image tiles", i);
    if (p.nt < 2 || p.nt > 4 || p.mt < 1 || p.mt > 2 || p.images_per_wg != (f.pool ? 32 : 128) * p.mt) fail("tile", i);
    if (f.nt_force && p.nt != f.nt_force) fail("forced nt", i);
    if ((flags & BBB_C8X3_TILE128) && p.mt != 1) fail("forced 128", i);
    if ((flags & BBB_C8X3_TILE256) && !lrt && p.mt != 2) fail("forced 256", i);
    const int want = lrt ? (f.of32 ? BBB_C8X3_FORM_LRT_F32 : BBB_C8X3_FORM_LRT_S3) : ((p.nt - 2) * 2 + (p.mt - 1)) * 3 + (f.pool ? 2 : f.of32 ? 1 : 0);
    if (p.form != want || (lrt && (p.nt != 2 || p.mt != 1 || f.pool))) fail("form", i);
    if (p.ho <= 0 || p.wo <= 0 || p.K != d->cin * d->kh * d->kw || p.vh0 < 0 || p.vh0 >= p.vh1 || p.vh1 > d->h || p.vw0 < 0 || p.vw0 >= p.vw1 || p.vw1 > d->w) fail("geometry", i);
    if (p.Mtiles != (int64_t)p.ho * p.wo / (f.pool ? 4 : 1) * p.nbt) fail("pixel tiles", i);
    // why MT is what it is
    const int64_t bm2 = f.pool ? 64 : 256;
    const int64_t items2 = (int64_t)d->draws * ((d->cout + 32 * p.nt - 1) / (32 * p.nt)) * ((int64_t)p.ho * p.wo / (f.pool ? 4 : 1)) * ((d->batch + bm2 - 1) / bm2);
    const int why = (flags & (BBB_C8X3_TILE128 | BBB_C8X3_TILE256)) ? 0 : lrt ? 1 : d->batch <= bm2 / 2 ? 2 : items2 < 1024 ? 3 : 4;
    mt_reason[why] += 1;
    if (why >= 1 && p.mt != (why == 4 ? 2 : 1)) fail("tile rule", i);
    return 0;
}

bbb_conv_desc_t base(int B, int cin, int h, int w, int cout, int k, int draws) {
    bbb_conv_desc_t d = {};
    d.batch = B; d.cin = cin; d.h = h; d.w = w; d.cout = cout; d.kh = d.kw = k;
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1;
    d.draws = draws;
    return d;
}

}  // namespace

int main() {
    long cases = 0;
    // (a) ordinary layers, every field and flag varied, refusals mixed in
    for (long i = 0; i < 60000; ++i, ++cases) {
        bbb_conv_desc_t d = base(4 * (1 + (int)(rnd() % 130)), 16 * (1 + (int)(rnd() % 8)), 1 + (int)(rnd() % 24), 1 + (int)(rnd() % 24),
                                 8 * (1 + (int)(rnd() % 40)), 1 + (int)(rnd() % 5), 1 + (int)(rnd() % 40));
        d.kw = rnd() % 4 ? d.kh : 1 + (int)(rnd() % 5);
        d.stride_h = 1 + (int)(rnd() % 2); d.stride_w = 1 + (int)(rnd() % 2);
        d.dil_h = 1 + (int)(rnd() % 2); d.dil_w = 1 + (int)(rnd() % 2);
        d.pad_h = (int)(rnd() % 4); d.pad_w = (int)(rnd() % 4);
        d.act = (int)(rnd() % 3);
        const bool lrt = rnd() % 5 == 0;
        uint32_t flags = 0;
        if (rnd() % 4 == 0) { flags |= BBB_C8X3_OUT_F32; d.cout += (int)(rnd() % 8); }
        if (rnd() % 2) flags |= rnd() % 2 ? BBB_C8X3_TILE128 : BBB_C8X3_TILE256;
        if (rnd() % 4 == 0) { flags |= BBB_C8X3_POOL; if (rnd() % 4) d.pad_h = d.pad_w = 0; }
        if (rnd() % 2) flags |= (uint32_t)(2 + rnd() % 3) << BBB_C8X3_NT_SHIFT;
        if (rnd() % 8 == 0) flags |= BBB_C8X3_ZERO_LEAD_H(rnd() % 3) | BBB_C8X3_ZERO_LEAD_W(rnd() % 3) | BBB_C8X3_ZERO_TRAIL_H(rnd() % 3) | BBB_C8X3_ZERO_TRAIL_W(rnd() % 3);
        if (rnd() % 30 == 0) flags |= 1u << (24 + rnd() % 8);
        if (rnd() % 30 == 0) flags |= BBB_C8X3_TILE128 | BBB_C8X3_TILE256;
        if (rnd() % 30 == 0) flags |= 1u << BBB_C8X3_NT_SHIFT;
        if (!lrt || rnd() % 8 == 0) { d.w_draw_stride = 4 * (int64_t)(rnd() % 1000); d.b_draw_stride = rnd() % 16 ? d.cout / 4 * 4 : 3; }
        if (rnd() % 2) d.x_draw_stride = (lrt ? 6 : 3) * (int64_t)d.cin * d.h * d.w * d.batch - (rnd() % 40 == 0 ? 8 : 0);
        if (rnd() % 6 == 0) { d.unit_div = 1 + (int)(rnd() % 4); d.unit_off = (int)(rnd() % 5); d.x_unit_mod = rnd() % 2 ? d.unit_div : (int)(rnd() % 3); }
        else if (rnd() % 6 == 0) { d.x_unit_div = (int)(rnd() % 5); d.x_unit_off = (int)(rnd() % 4); }
        if (rnd() % 25 == 0) d.batch += 1 + (int)(rnd() % 3);
        if (rnd() % 25 == 0) d.cin += 8;
        if (rnd() % 40 == 0) d.pool = 1;
        if (rnd() % 40 == 0) d.w_tap_major = 1;
        if (rnd() % 40 == 0) d.w_row_pitch = d.cin;
        walk(rnd() % 2000 == 0 ? nullptr : &d, flags, lrt, i);
    }
    // (b) both sides of the tile rule's thresholds: B at bm2 / 2 and bm2 / 2 + 4, draws that put items2 at 1023 / 1024 / 1025
    for (long i = 0; i < 40000; ++i, ++cases) {
        const bool pool = rnd() % 3 == 0;
        const int bm2 = pool ? 64 : 256;
        static const int images[] = {-4, 0, 4, 8, 128, 260, 516};
        const int B = bm2 / 2 + pick(images, 7);
        const int px = 2 * (1 + (int)(rnd() % 4)), cout = 8 * (1 + (int)(rnd() % 30));
        bbb_conv_desc_t d = base(B < 4 ? 4 : B, 16, px + (pool ? 2 : 0), px + (pool ? 2 : 0), cout, pool ? 3 : 1, 1);
        const int64_t per = (int64_t)((cout + 63) / 64) * (px * px / (pool ? 4 : 1)) * ((d.batch + bm2 - 1) / bm2);
        d.draws = (int)((1024 + per - 1) / per) + (int)(rnd() % 3) - 1;
        if (d.draws < 1) d.draws = 1;
        Plan p;
        if (walk(&d, pool ? BBB_C8X3_POOL : 0, false, i, &p) != 0) fail("a threshold case was refused", i);
        const int64_t items2 = per * d.draws;
        if (p.mt != ((d.batch <= bm2 / 2 || items2 < 1024) ? 1 : 2)) fail("threshold", i);
    }
    // (c) the integer limits: 2^31 - 1 (and other edge values) in each field in turn, then in random pairs
    static const int ints[] = {1, 2, 3, 4, 8, 16, 64, 0x7fff, 0x8000, 0x10000, 0x3fffffff, 0x40000000, 0x7ffffff0, 0x7ffffffc, 0x7fffffff, 0, -1, -0x7fffffff - 1};
    for (long i = 0; i < 60000; ++i, ++cases) {
        bbb_conv_desc_t d = base(8, 16, 6, 6, 16, 3, 2);
        d.pad_h = d.pad_w = 1;
        int* f[] = {&d.batch, &d.cin, &d.h, &d.w, &d.cout, &d.kh, &d.kw, &d.stride_h, &d.stride_w, &d.pad_h, &d.pad_w, &d.dil_h, &d.dil_w, &d.draws,
                    &d.w_row_pitch, &d.unit_div, &d.unit_off, &d.x_unit_mod, &d.x_unit_div, &d.x_unit_off, &d.b_offset, &d.act, &d.pool};
        if (i < 23 * 18) *f[i / 18] = ints[i % 18];
        else for (int r = 0; r < 1 + (int)(rnd() % 3); ++r) *f[rnd() % 23] = pick(ints, 18);
        if (rnd() % 4 == 0) d.x_draw_stride = pick(ints, 18);
        if (rnd() % 4 == 0) d.w_draw_stride = (int64_t)pick(ints, 18) * 4;
        const uint32_t flags = rnd() % 4 ? (rnd() % 2 ? BBB_C8X3_OUT_F32 : 0) : rnd();
        walk(&d, flags, rnd() % 4 == 0, i);
    }
    {   // draws x channel tiles past 2^31: refused, not wrapped
        bbb_conv_desc_t d = base(8, 16, 1, 1, 72, 1, 0x7fffffff);
        if (walk(&d, 0, false, -1) != BBB_ESHAPE) fail("draws x channel tiles past 2^31 taken", -1);
        d.draws = 0x3ffffffc;                   // two 64-channel tiles: 2^31 - 8 groups, one pixel tile each -> the grid just fits
        if (walk(&d, 0, false, -2) != 0) fail("2^31 - 8 groups refused", -2);
        d.cout = 136;                           // three tiles
        if (walk(&d, 0, false, -3) != BBB_ESHAPE) fail("3 x (2^30 - 4) groups taken", -3);
        cases += 3;
    }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld forms", cases, counts[0], counts[1], counts[2], counts[3]);
    for (int f = 0; f < kForms; ++f) printf(" %ld", forms[f]);
    printf(" reasons %ld %ld %ld %ld %ld", mt_reason[0], mt_reason[1], mt_reason[2], mt_reason[3], mt_reason[4]);
    printf(" checksum %016llx\n", (unsigned long long)sum);
    return 0;
}
