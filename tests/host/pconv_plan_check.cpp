// Host-only walk of the fp32 implicit GEMM's launch plan (csrc/pconv_plan.h) for tests/test_pconv_sweep_cpu.py, which builds this
// file with -fsanitize=address,undefined: describe(), canonical_ksplit(), split_scratch_bytes() and plan() over seeded descriptors
// placed around every threshold of the plan (767 / 768 items of 128 images, 384 / 385 and 512 / 513 items of a split layer,
// 12000 / 12001 items, 15 / 16 / 23 / 24 / 31 / 32 k tiles, 16 / 17 groups, the "128 declined" image counts) and over descriptors whose
// fields sit near the 32-bit limits (every count inside the plan must be guarded, not overflow).  Checks the plan's own invariants
// and prints how often each form and each refusal came up, and a checksum of everything returned.
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

bbb_conv_desc_t base(int B, int cin, int h, int w, int cout, int k, int draws) {
    bbb_conv_desc_t d = {};
    d.batch = B; d.cin = cin; d.h = h; d.w = w; d.cout = cout; d.kh = d.kw = k;
    d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1;
    d.draws = draws;
    d.x_draw_stride = (int64_t)((uint64_t)cin * (uint64_t)h * (uint64_t)w * (uint64_t)B);     // (never looked at by the plan)
    return d;
}

}  // namespace

int main() {
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
        walk(rnd() % 2000 == 0 ? nullptr : &d, i);
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
    }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld forms", cases, counts[0], counts[1], counts[2], counts[3]);
    for (int f = 0; f < kForms; ++f) printf(" %ld", forms[f]);
    printf(" checksum %016llx\n", (unsigned long long)sum);
    return 0;
}
