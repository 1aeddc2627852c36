// Host-only walk of the fp32 implicit GEMM's launch plan (csrc/pconv_plan.h) for tests/test_pconv_sweep_cpu.py, which builds this
// file with -fsanitize=address,undefined: describe(), canonical_ksplit(), split_scratch_bytes() and plan() over seeded descriptors
// placed around every threshold of the plan (767 / 768 items of 128 images, 384 / 385 and 512 / 513 items of a split layer,
// 12000 / 12001 items, 15 / 16 / 23 / 24 / 31 / 32 k tiles, 16 / 17 groups, the "128 declined" image counts) and over descriptors whose
// fields sit near the 32-bit limits (every count inside the plan must be guarded, not overflow).  Checks the plan's own invariants
// and prints how often each form and each refusal came up, and a checksum of everything returned.  The same descriptors also go
// through the pieces that share the header: the transposed launch's plan (dgrad_plan, on the stride-1 descriptor derived from each
// forward one and on the hostile ones as they are), the grid bbb_conv2d_chwn_bf16x3_fwd takes (128-image tiles) and the functions of
// csrc/conv_desc_check.h.  `pconv_plan_check dump` prints one line per plan() call instead -- the case, the return code and the
// plan's fields -- so that two builds of this file against two versions of the header can be compared line by line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/bbb_hip.h"
#include "../../pytorch-bayesiancnn_amd/csrc/pconv_plan.h"

namespace {

using namespace pconv_plan;

uint64_t state = 0x9E3779B97F4A7C15ull, sum = 0xcbf29ce484222325ull;
uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
int pick(const int* v, int n) { return v[rnd() % (uint32_t)n]; }
void mix(int64_t v) { sum = (sum ^ (uint64_t)v) * 0x100000001b3ull; }

long counts[4];        // ok / EINVAL / EALIGN / ESHAPE over all calls
long forms[kForms];
long dgrad[2];         // transposed launches planned / refused
bool dump = false;

void tally(int rc) {
    mix(rc);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
}

void fail(const char* what, long i) {
    printf("invariant broken: %s (case %ld)\n", what, i);
    exit(1);
}

void walk(const bbb_conv_desc_t* d, long i) {
    Geom g;
    const int rd = describe(d, &g);
    tally(rd);
    if (rd != 0) return;
    if (g.Ho <= 0 || g.Wo <= 0 || (int64_t)g.Ho * g.Wo * g.B > ((int64_t)1 << 30) || g.K <= 0 || g.Kp < g.K) fail("describe", i);
    const int ks = canonical_ksplit(g);
    if (ks < 1 || ks > 4) fail("k_split range", i);
    mix(ks);
    for (int lrt = 0; lrt < 2; ++lrt)
        for (int scratch = 0; scratch < 2; ++scratch)
            for (int k = 0; k < 3; ++k) {
                const int k_split = k == 0 ? 1 : k == 1 ? ks : ks + 1;
                const int64_t need = split_scratch_bytes(g, d->draws, lrt != 0, k_split);
                if (need < 0 || (need > 0 && need < kTicketBytes)) fail("scratch bytes", i);
                mix(need);
                Plan p;
                const int rc = plan(g, d->draws, lrt != 0, k_split, scratch != 0, &p);
                tally(rc);
                if (dump)
                    printf("%ld %d%d%d rc %d form %d bm %d ilv %d nbt %d Mtiles %d Ntiles %d G %d per_xcd %d items %lld blocks %lld\n", i, lrt, scratch, k,
                           rc, rc ? -1 : p.form, rc ? 0 : p.bm, rc ? 0 : p.ilv, rc ? 0 : p.nbt, rc ? 0 : p.Mtiles, rc ? 0 : p.Ntiles, rc ? 0 : p.G,
                           rc ? 0 : p.per_xcd, rc ? 0LL : (long long)p.items, rc ? 0LL : (long long)p.blocks);
                if (k == 2 && rc != BBB_EINVAL) fail("a split that is not the layer's was taken", i);
                if (rc != 0) continue;
                forms[p.form] += 1;
                mix(p.form); mix(p.bm); mix(p.ilv); mix(p.nbt); mix(p.Mtiles); mix(p.Ntiles); mix(p.G); mix(p.per_xcd); mix(p.items); mix(p.blocks);
                const bool split = k_split > 1, cross = p.form == kBbbCross || p.form == kLrtCross, pool = p.form == kBbbPool || p.form == kLrtPool;
                if ((p.form >= kLrt64Ilv) != (lrt != 0)) fail("form of the other kernel", i);
                if (p.bm != 64 && p.bm != 128) fail("tile", i);
                if (lrt && p.bm != 64) fail("LRT tile", i);
                if (p.nbt != (g.B + p.bm - 1) / p.bm || p.Ntiles != (g.Cout + 63) / 64 || p.G != (int64_t)p.Ntiles * d->draws) fail("tiles", i);
                if (p.items != (int64_t)p.G * p.Mtiles || p.items <= 0) fail("items", i);
                if (p.blocks % 8 != 0 || p.blocks != 8 * (int64_t)p.per_xcd || p.blocks > 0x7fffffffLL) fail("grid", i);
                if (p.blocks < p.items * (cross ? k_split : 1) || p.blocks >= p.items * (cross ? k_split : 1) + 8) fail("grid size", i);
                if (pool != (g.pool != 0) || (pool && (split || p.ilv))) fail("pooled form", i);
                if (cross && (!split || !scratch || p.items > split_max_items(lrt != 0) || need == 0 || !p.ilv)) fail("cross form", i);
                if (!cross && split && scratch && need > 0) fail("cross form not taken", i);
                const bool seq = p.form >= kBbbSeq64Ilv && p.form <= kBbbSeq128 ? true : p.form == kLrtSeq64;
                if (seq != (split && !cross)) fail("SEQ form", i);
                if (!cross && !pool && !(lrt && seq) && (p.ilv != 0) != (p.items <= PCONV_ILV_MAX)) fail("interleave", i);
            }
}

#ifdef BBB_CONV_DESC_CHECK_H
// the pieces that share the header with plan(): every one of them on every descriptor of the walk
void check_grid(const Plan& p, int B, int64_t pixels, int draws, int cout, const char* what, long i) {
    if (p.bm != 64 && p.bm != 128) fail(what, i);
    if (p.Ntiles != (cout + 63) / 64 || p.G != (int64_t)p.Ntiles * draws || p.nbt != (B + p.bm - 1) / p.bm || p.Mtiles != pixels * p.nbt) fail(what, i);
    if (p.items != (int64_t)p.G * p.Mtiles || p.items <= 0 || p.blocks != 8 * (int64_t)p.per_xcd || p.blocks < p.items || p.blocks >= p.items + 8 ||
        p.blocks > 0x7fffffffLL || (p.ilv != 0) != (p.items <= PCONV_ILV_MAX))
        fail(what, i);
}

void walk_dgrad(const bbb_conv_desc_t* g, int up_h, int up_w, int out_h, int out_w, long i) {
    Plan p;
    uint32_t x_inv = 0;
    const int rc = dgrad_plan(g, up_h, up_w, out_h, out_w, 0, &x_inv, &p);
    mix(rc);
    dgrad[rc != 0] += 1;
    for (int ptr_rc = BBB_EALIGN; ptr_rc <= BBB_EINVAL; ++ptr_rc) {        // the pointer checks' code comes back at its place or not at all
        Plan q;
        const int rq = dgrad_plan(g, up_h, up_w, out_h, out_w, ptr_rc, &x_inv, &q);
        if (rq != ptr_rc && rq != rc) fail("dgrad pointer code", i);
        if (rc == 0 && rq != ptr_rc) fail("dgrad pointer code dropped", i);
    }
    if (rc != 0) return;
    const int64_t pixels = (int64_t)out_h * out_w;
    check_grid(p, g->batch, pixels, g->draws, g->cout, "dgrad grid", i);
    if (p.form != 0 || p.bm != image_tile(g->batch, pixels, p.G, false)) fail("dgrad tile", i);
    // the forward launch of the same pixels, channels, images and draws (1 x 1 taps over dx's map) takes the same tile and grid
    Geom f = {};
    f.B = g->batch; f.Cin = 4; f.H = f.Ho = out_h; f.W = f.Wo = out_w; f.Cout = g->cout; f.kh = f.kw = f.dh = f.dw = 1;
    Plan fp;
    if (plan(f, g->draws, false, 1, false, &fp) != 0 || fp.bm != p.bm || fp.ilv != p.ilv || fp.items != p.items || fp.blocks != p.blocks ||
        fp.per_xcd != p.per_xcd)
        fail("dgrad plan is not the forward's", i);
    mix(p.bm); mix(p.ilv); mix(p.items); mix(p.blocks); mix(x_inv);
}

void walk_shared(const bbb_conv_desc_t* d, long i) {
    using namespace conv_desc_check;
    if (d == nullptr) {
        walk_dgrad(nullptr, 2, 2, 8, 8, i);
        return;
    }
    int32_t ho = -1, wo = -1;
    const bool pos = positive_geometry(d);
    if (pos && !positive_map(d)) fail("positive_geometry without positive_map", i);
    if (pos) {
        const int rc = out_map(d, &ho, &wo);
        mix(rc); mix(ho); mix(wo);
        const int64_t nh = (int64_t)d->h + 2 * (int64_t)d->pad_h - (int64_t)d->dil_h * (d->kh - 1) - 1;
        const int64_t nw = (int64_t)d->w + 2 * (int64_t)d->pad_w - (int64_t)d->dil_w * (d->kw - 1) - 1;
        const bool reach = nh < 0 || nw < 0;                                                   // the kernel reaches past the padded input
        const bool wide = nh >= 0x7fffffffLL * d->stride_h || nw >= 0x7fffffffLL * d->stride_w;   // the map leaves int
        if ((rc != 0) != (reach || wide) || (rc != 0 && rc != BBB_ESHAPE)) fail("out_map refuses the over-reaching kernels and the maps that leave int", i);
        if (rc == 0 && (ho <= 0 || wo <= 0)) fail("out_map", i);
        mix(mul_cap(d->cin, d->h, d->w, d->batch));
    }
    const int u0 = unit_fields(d, kNothing), u1 = unit_fields(d, kSteps), u2 = unit_fields(d, kUnitsAndSteps);
    mix(u0); mix(u1); mix(u2);
    if ((u0 != 0 && u0 != BBB_EINVAL) || (u1 != 0 && u1 != BBB_EINVAL) || (u2 != 0 && u2 != BBB_EINVAL)) fail("unit_fields code", i);
    if (u0 == 0 && (u1 != 0 || u2 != 0)) fail("all-zero unit fields are admitted everywhere", i);
    if (u1 == 0 && d->unit_div >= 0 && u2 != 0) fail("steps are admitted where units and steps are", i);
    int32_t per = 0;
    int64_t blocks = 0;
    if (xcd_grid(0x7ffffff8LL, &per, &blocks) != 0 || blocks != 0x7ffffff8LL || xcd_grid(0x7ffffff9LL, &per, &blocks) != BBB_ESHAPE ||
        xcd_grid(kCap, &per, &blocks) != BBB_ESHAPE || mul_cap(kCap, 0x7fffffff) != kCap || mul_cap(3, 5, 7, 11) != 1155)
        fail("xcd_grid / mul_cap", i);
    // the grid of bbb_conv2d_chwn_bf16x3_fwd: the descriptor checks of the fp32 forward, then 128-image items
    Geom g;
    if (describe(d, &g) == 0) {
        Plan p = {};
        int rc = channel_groups(g.Cout, d->draws, &p);
        if (rc == 0) rc = item_grid(g.B, (int64_t)g.Ho * g.Wo, 128, &p);
        mix(rc);
        if (rc == 0) check_grid(p, g.B, (int64_t)g.Ho * g.Wo, d->draws, g.Cout, "bf16x3 grid", i);
        if (rc == 0 && p.bm != 128) fail("bf16x3 tile", i);
    }
    // the transposed launch: the hostile descriptor as it is, and -- where d is a strided forward layer -- the stride-1 descriptor of
    // its input gradient (g's map = d's output map, padding dil (k - 1) - pad, the stride as the upsampling factors, dx = d's input map)
    walk_dgrad(d, d->stride_h, d->stride_w, d->h, d->w, i);
    const int64_t qh = (int64_t)d->dil_h * (d->kh - 1) - d->pad_h, qw = (int64_t)d->dil_w * (d->kw - 1) - d->pad_w;
    if (pos && ho > 0 && wo > 0 && qh >= 0 && qw >= 0 && qh <= 0x7fffffffLL && qw <= 0x7fffffffLL) {
        bbb_conv_desc_t t = {};
        t.batch = d->batch; t.cin = d->cout; t.h = ho; t.w = wo; t.cout = d->cin; t.kh = d->kh; t.kw = d->kw;
        t.stride_h = t.stride_w = 1; t.pad_h = (int32_t)qh; t.pad_w = (int32_t)qw; t.dil_h = d->dil_h; t.dil_w = d->dil_w;
        t.draws = d->draws;
        walk_dgrad(&t, d->stride_h, d->stride_w, d->h, d->w, i);
    }
}
#else
void walk_shared(const bbb_conv_desc_t*, long) {}
#endif

bbb_conv_desc_t base(int B, int cin, int h, int w, int cout, int k, int draws) {
    bbb_conv_desc_t d = {};
    d.batch = B; d.cin = cin; d.h = h; d.w = w; d.cout = cout; d.kh = d.kw = k;
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1;
    d.draws = draws;
    d.x_draw_stride = (int64_t)((uint64_t)cin * (uint64_t)h * (uint64_t)w * (uint64_t)B);     // (never looked at by the plan)
    return d;
}

}  // namespace

int main(int argc, char** argv) {
    dump = argc > 1 && argv[1][0] == 'd';
    long cases = 0;
    static const int tiles[] = {1, 8, 15, 16, 17, 23, 24, 25, 31, 32, 33, 48}, images[] = {4, 60, 64, 68, 128, 132, 192, 204, 208, 256, 260, 308, 324, 408, 412, 512};
    static const int item_edges[] = {383, 384, 385, 511, 512, 513, 766, 767, 768, 769, 11999, 12000, 12001, 24000, 24001};
    // (a) layers around the split's rule: `groups` pixels x channel tiles, `t` k tiles; launches with item counts at every edge
    for (long i = 0; i < 60000; ++i, ++cases) {
        const int t = pick(tiles, 12), B = pick(images, 16);
        const int cin = 32 * t - (int)(rnd() % 3 == 0 ? rnd() % 32 : 0);
        const int px = 1 + (int)(rnd() % 18), ntl = 1 + (int)(rnd() % 3);
        const int per = px * ((B + 63) / 64) * ntl;
        const int target = pick(item_edges, 15);
        const int draws = rnd() % 4 ? (target + per - 1) / per + (int)(rnd() % 3) - 1 : 1 + (int)(rnd() % 40);
        bbb_conv_desc_t d = base(B, cin, px, 1, 64 * ntl - (int)(rnd() % 64), 1, draws < 1 ? 1 : draws);
        if (rnd() % 8 == 0) { d.kh = 3; d.pad_h = 1; d.cin = (cin + 2) / 3; }
        if (rnd() % 16 == 0) { d.h = 2 * px; d.w = 2; d.pool = 1; }
        walk(&d, i);
        walk_shared(&d, i);
    }
    // (b) ordinary layers, every field varied, refusals mixed in
    for (long i = 0; i < 60000; ++i, ++cases) {
        bbb_conv_desc_t d = base(4 * (1 + (int)(rnd() % 130)), 1 + (int)(rnd() % 300), 1 + (int)(rnd() % 40), 1 + (int)(rnd() % 40),
                                 1 + (int)(rnd() % 300), 1 + (int)(rnd() % 7), 1 + (int)(rnd() % 60));
        d.kw = 1 + (int)(rnd() % 7);
        d.stride_h = 1 + (int)(rnd() % 3); d.stride_w = 1 + (int)(rnd() % 3);
        d.pad_h = (int)(rnd() % 5); d.pad_w = (int)(rnd() % 5);
        d.dil_h = 1 + (int)(rnd() % 2); d.dil_w = 1 + (int)(rnd() % 2);
        d.act = (int)(rnd() % 3);
        d.pool = rnd() % 4 == 0;
        d.w_tap_major = rnd() % 4 == 0;
        if (rnd() % 6 == 0) { d.unit_div = 1 + (int)(rnd() % 4); d.unit_off = (int)(rnd() % 5); d.x_unit_mod = rnd() % 2 ? d.unit_div : (int)(rnd() % 3); }
        else if (rnd() % 6 == 0) { d.x_unit_div = (int)(rnd() % 5); d.x_unit_off = (int)(rnd() % 4); }
        if (rnd() % 20 == 0) d.batch += 1 + (int)(rnd() % 3);
        if (rnd() % 20 == 0) d.w_row_pitch = d.cin * d.kh * d.kw + (int)(rnd() % 9) - 2;
        if (rnd() % 40 == 0) d.b_offset = (int)(rnd() % 3) - 1;
        if (rnd() % 40 == 0) d.act = 3;
        const bbb_conv_desc_t* dp = rnd() % 2000 == 0 ? nullptr : &d;
        walk(dp, i);
        walk_shared(dp, i);
    }
    // (c) the integer limits: every size from {small, near 2^15, near 2^31}
    static const int ints[] = {1, 2, 3, 4, 7, 64, 65, 0x7fff, 0x8000, 0x10000, 0x3fffffff, 0x40000000, 0x7ffffffc, 0x7fffffff, 0, -1, -0x7fffffff - 1};
    for (long i = 0; i < 80000; ++i, ++cases) {
        const int n = rnd() % 3 ? 8 : 17;             // mostly small fields with one or two large ones
        bbb_conv_desc_t d = base(pick(ints, n), pick(ints, n), pick(ints, n), pick(ints, n), pick(ints, n), pick(ints, n), pick(ints, n));
        int* f[] = {&d.batch, &d.cin, &d.h, &d.w, &d.cout, &d.kh, &d.kw, &d.stride_h, &d.stride_w, &d.pad_h, &d.pad_w, &d.dil_h, &d.dil_w, &d.draws,
                    &d.w_row_pitch, &d.unit_div, &d.unit_off, &d.x_unit_div, &d.b_offset};
        for (int r = 0; r < 1 + (int)(rnd() % 3); ++r) *f[rnd() % 19] = pick(ints, 17);
        if (rnd() % 2) d.batch = d.batch / 4 * 4;
        d.pool = rnd() % 8 == 0;
        walk(&d, i);
        walk_shared(&d, i);
    }
    if (dump) return 0;
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld forms", cases, counts[0], counts[1], counts[2], counts[3]);
    for (int f = 0; f < kForms; ++f) printf(" %ld", forms[f]);
    printf(" checksum %016llx dgrad %ld %ld\n", (unsigned long long)sum, dgrad[0], dgrad[1]);
    return 0;
}
