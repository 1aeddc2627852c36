// Host-only walk of the plan of bbb_conv2d_fwd / bbb_lrt_conv2d_fwd (csrc/conv_gemm_plan.h) for tests/test_host_cpu.py, which builds
// this file with -fsanitize=address,undefined.  Ordinary layers next to the 768-workgroup threshold of the pixel tile with every
// refusal mixed in, then descriptors at the integer limits (edge values in each field in turn, then in random groups).  For every
// plan that is taken the invariants the kernel relies on are checked: the tiles cover the output exactly once, the k tiles cover the
// contraction, the tile rule, what the int32 and 16-bit fields of the kernel hold.  Prints how often each code came up, how often
// each of the eight instantiations, and a checksum of everything returned.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../pytorch-bayesiancnn_amd/csrc/conv_gemm_plan.h"

namespace {

using namespace conv_gemm_plan;

uint64_t state = 0x9E3779B97F4A7C15ull, sum = 0xcbf29ce484222325ull;
uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
void mix(int64_t v) { sum = (sum ^ (uint64_t)v) * 0x100000001b3ull; }

long counts[4];        // ok / EINVAL / EALIGN / ESHAPE
long forms[8];         // (bm == 128) * 4 + lrt * 2 + linear

void fail(const char* what, long i) {
    printf("invariant broken: %s (case %ld)\n", what, i);
    exit(1);
}

void axis(int64_t n, int64_t k, int64_t s, int64_t p, int64_t dl, int64_t o, long i) {
    const int64_t reach = dl * (k - 1) + 1;
    if (o < 1 || (o - 1) * s + reach > n + 2 * p || o * s + reach <= n + 2 * p) fail("output map", i);
}

void invariants(const bbb_conv_desc_t* d, bool lrt, const Plan& p, long i) {
    axis(d->h, d->kh, d->stride_h, d->pad_h, d->dil_h, p.ho, i);
    axis(d->w, d->kw, d->stride_w, d->pad_w, d->dil_w, p.wo, i);
    if (p.M != (int64_t)d->batch * p.ho * p.wo || p.K != (int64_t)d->cin * d->kh * d->kw) fail("M or K", i);
    if (p.y_ds != (int64_t)p.M * d->cout) fail("output slab", i);
    if ((int64_t)d->cin * d->h * d->w > 0x7fffffffLL) fail("per-image offsets leave int32", i);
    // a tap's offsets r * dil_h and q * dil_w travel in 16-bit halves next to 0x7fff, and ih0 + r * dil_h is compared unsigned
    if ((int64_t)(d->kh - 1) * d->dil_h >= 0x7000 || (int64_t)(d->kw - 1) * d->dil_w >= 0x7000) fail("tap offsets leave 15 bits", i);
    if (p.bk != (lrt ? 16 : 32)) fail("bk", i);
    if ((int64_t)p.k_tiles * p.bk < p.K || (int64_t)(p.k_tiles - 1) * p.bk >= p.K || p.k_tiles < 1) fail("k tiles", i);
    const int64_t n_tiles = ((int64_t)d->cout + 63) / 64;
    const int64_t blocks128 = conv_desc_check::mul_cap(((int64_t)p.M + 127) / 128, n_tiles, d->draws);
    if (p.bm != (blocks128 >= 768 ? 128 : 64)) fail("tile rule", i);
    if ((int64_t)p.grid[0] * p.bm < p.M || (int64_t)(p.grid[0] - 1) * p.bm >= p.M) fail("pixel tiles", i);
    if ((int64_t)p.grid[1] * 64 < d->cout || (int64_t)(p.grid[1] - 1) * 64 >= d->cout) fail("channel tiles", i);
    if (p.grid[2] != d->draws || p.grid[0] < 1 || p.grid[1] < 1) fail("grid", i);
    const bool lin = d->h == 1 && d->w == 1 && d->kh == 1 && d->kw == 1 && d->pad_h == 0 && d->pad_w == 0;
    if ((p.linear != 0) != lin) fail("linear", i);
    if (lin && (p.ho != 1 || p.wo != 1 || p.M != d->batch || p.K != d->cin)) fail("linear: x is not [M][K]", i);
    if (lrt && (d->w_draw_stride != 0 || d->b_draw_stride != 0)) fail("LRT with a draw stride", i);
}

int walk(const bbb_conv_desc_t* d, bool lrt, const Operands& o, long i) {
    Plan p;
    const int rc = plan(d, lrt, o, &p);
    mix(rc);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
    if (rc == 0) {
        mix(p.ho); mix(p.wo); mix(p.M); mix(p.K); mix(p.y_ds); mix(p.bm); mix(p.linear); mix(p.bk); mix(p.k_tiles);
        mix(p.grid[0]); mix(p.grid[1]); mix(p.grid[2]);
        forms[(p.bm == 128) * 4 + lrt * 2 + (p.linear != 0)] += 1;
        invariants(d, lrt, p, i);
    } else if (p.bm != 0 || p.grid[0] != 0 || p.k_tiles != 0) {
        fail("a refusal leaves a plan behind", i);
    }
    return rc;
}

bbb_conv_desc_t layer(int B, int cin, int h, int w, int cout, int kh, int kw, int s, int pd, int dl, int E) {
    bbb_conv_desc_t d = {};
    d.batch = B; d.cin = cin; d.h = h; d.w = w; d.cout = cout; d.kh = kh; d.kw = kw;
    d.stride_h = d.stride_w = s; d.pad_h = d.pad_w = pd; d.dil_h = d.dil_w = dl; d.draws = E;
    return d;
}

void expect(int got, int want, const char* what, long i) {
    if (got != want) fail(what, i);
}

}  // namespace

int main() {
    long cases = 0;
    static const int targets[] = {1, 50, 766, 767, 768, 769, 1535, 1536, 3000};
    // (a) ordinary layers (a fifth of them linear), draws chosen next to the tile rule's threshold, refusals mixed in
    for (long i = 0; i < 120000; ++i, ++cases) {
        const bool linear = rnd() % 5 == 0, lrt = rnd() % 2;
        const int kh = linear ? 1 : 1 + (int)(rnd() % 5), kw = linear ? 1 : 1 + (int)(rnd() % 5);
        bbb_conv_desc_t d = layer(1 + (int)(rnd() % 300), 1 + (int)(rnd() % (linear ? 600 : 40)), linear ? 1 : 1 + (int)(rnd() % 33),
                                  linear ? 1 : 1 + (int)(rnd() % 33), 1 + (int)(rnd() % 200), kh, kw, 1, 0, 1, 1);
        if (!linear) {
            d.stride_h = 1 + (int)(rnd() % 3); d.stride_w = 1 + (int)(rnd() % 3);
            d.pad_h = (int)(rnd() % 4); d.pad_w = (int)(rnd() % 4);
            d.dil_h = 1 + (int)(rnd() % 2); d.dil_w = 1 + (int)(rnd() % 2);
        }
        {   // draws next to the threshold, where the map exists
            Plan p;
            if (plan(&d, false, Operands(), &p) == 0) {
                const int64_t per = ((int64_t)p.M + 127) / 128 * p.grid[1];
                const int64_t t = targets[rnd() % 9];
                d.draws = (int)((t + per - 1) / per) + (int)(rnd() % 3) - 1;
                if (d.draws < 1) d.draws = 1;
            }
        }
        if (!lrt && rnd() % 2) { d.x_draw_stride = (int64_t)d.batch * d.cin * d.h * d.w; d.w_draw_stride = (int64_t)d.cout * d.cin * kh * kw; d.b_draw_stride = d.cout; }
        Operands o;
        o.address_bits = 4096;
        d.act = (int)(rnd() % 3);
        if (rnd() % 40 == 0) d.act = rnd() % 2 ? 3 : -1;
        if (rnd() % 40 == 0) d.draws = 0;
        if (rnd() % 40 == 0) d.pad_w = -1;
        if (rnd() % 40 == 0) d.stride_h = 0;
        if (rnd() % 40 == 0) d.kh = d.h + 2 * d.pad_h + 2;
        if (rnd() % 60 == 0) d.unit_div = 2;
        if (rnd() % 60 == 0) d.unit_off = 1;
        if (rnd() % 60 == 0) d.x_unit_mod = 2;
        if (rnd() % 60 == 0) d.x_unit_div = 2;
        if (rnd() % 60 == 0) d.x_unit_off = 1;
        if (rnd() % 60 == 0) d.b_offset = 8;
        if (rnd() % 60 == 0) d.w_row_pitch = 64;
        if (rnd() % 60 == 0) d.pool = 1;
        if (rnd() % 60 == 0) d.w_tap_major = 1;
        if (lrt && rnd() % 30 == 0) d.w_draw_stride = 64;
        if (lrt && rnd() % 30 == 0) d.b_draw_stride = 64;
        if (rnd() % 30 == 0) o.null_operand = true;
        if (lrt && rnd() % 30 == 0) o.half_a_bias = true;
        if (rnd() % 30 == 0) o.address_bits |= 1 + rnd() % 3;
        walk(rnd() % 2000 == 0 ? nullptr : &d, lrt, o, i);
    }
    // (b) the integer limits
    static const int ints[] = {1, 2, 3, 31, 32, 33, 64, 127, 128, 0x6fff, 0x7000, 0x7fff, 0x8000, 0x10000, 0x3fffffff, 0x40000000,
                               0x7fffff80, 0x7fffffc0, 0x7fffffff, 0, -1, -0x7fffffff - 1};
    const int n_ints = (int)(sizeof(ints) / sizeof(ints[0]));
    for (long i = 0; i < 80000; ++i, ++cases) {
        bbb_conv_desc_t d = layer(8, 3, 9, 13, 12, 2, 3, 2, 1, 1, 2);
        int* f[] = {&d.batch, &d.cin, &d.h, &d.w, &d.cout, &d.kh, &d.kw, &d.stride_h, &d.stride_w, &d.pad_h, &d.pad_w, &d.dil_h, &d.dil_w,
                    &d.draws, &d.act};
        if (i < 15 * n_ints) *f[i / n_ints] = ints[i % n_ints];
        else for (int r = 0; r < 1 + (int)(rnd() % 3); ++r) *f[rnd() % 15] = ints[rnd() % n_ints];
        if (rnd() % 4 == 0) { d.h = d.w = d.kh = d.kw = 1; d.pad_h = d.pad_w = 0; }       // linear: batch and cin up to 2^31 - 1 are admitted
        walk(&d, rnd() % 2, Operands(), i);
    }
    {   // hand-worked
        Plan p;
        Operands none, null_op, half, odd;
        null_op.null_operand = true; half.half_a_bias = true; odd.address_bits = 4098;
        bbb_conv_desc_t d = layer(7, 3, 17, 17, 130, 3, 3, 1, 1, 1, 16);      // 7 * 17 * 17 = 2023 pixels: 16 x 3 x 16 = 768 workgroups of 128
        if (plan(&d, false, none, &p) != 0 || p.M != 2023 || p.K != 27 || p.bm != 128 || p.linear != 0 || p.bk != 32 || p.k_tiles != 1 ||
            p.grid[0] != 16 || p.grid[1] != 3 || p.grid[2] != 16)
            fail("the hand-worked plan at the threshold", -1);
        d.draws = 15;                                                          // 720 < 768: the 64-pixel tile, 32 x 3 x 15
        if (plan(&d, true, none, &p) != 0 || p.bm != 64 || p.bk != 16 || p.k_tiles != 2 || p.grid[0] != 32 || p.grid[2] != 15)
            fail("the hand-worked plan below the threshold", -2);
        d = layer(2023, 70, 1, 1, 130, 1, 1, 1, 0, 1, 16);
        if (plan(&d, true, none, &p) != 0 || p.linear != 1 || p.bm != 128 || p.k_tiles != 5 || p.M != 2023 || p.K != 70) fail("linear", -3);
        d.pad_w = 1;                                                           // a padded 1 x 1 map is a convolution: 1 x 3 pixels
        if (plan(&d, true, none, &p) != 0 || p.linear != 0 || p.wo != 3) fail("padded 1 x 1 map", -4);
        // the order of the checks
        d = layer(8, 3, 9, 13, 12, 2, 3, 2, 1, 1, 2);
        expect(plan(&d, false, null_op, &p), BBB_EINVAL, "a NULL operand", -5);
        expect(plan(&d, true, half, &p), BBB_EINVAL, "half a bias", -6);
        expect(plan(&d, false, half, &p), 0, "half a bias is an LRT matter", -7);
        expect(plan(&d, false, odd, &p), BBB_EALIGN, "alignment", -8);
        d.w_draw_stride = 72;
        expect(plan(&d, false, none, &p), 0, "BBB weights per draw", -9);
        expect(plan(&d, true, odd, &p), BBB_EINVAL, "LRT draw stride comes before alignment", -10);
        d.kh = 12;                                                             // 9 + 2 - 11 - 1 < 0
        expect(plan(&d, false, null_op, &p), BBB_ESHAPE, "the descriptor comes before the operands", -11);
        d.act = 3;
        expect(plan(&d, false, null_op, &p), BBB_EINVAL, "EINVAL of the descriptor comes before its ESHAPE", -12);
        // 0x7000: h + pad_h + dil_h * kh
        d = layer(1, 1, 0x6ffe, 1, 1, 1, 1, 1, 0, 1, 1);
        expect(walk(&d, false, none, -13), 0, "h + kh = 0x6fff refused", -13);
        d.h = 0x6fff;
        expect(walk(&d, false, none, -14), BBB_ESHAPE, "h + kh = 0x7000 taken", -14);
        // int32 limits: M = 2^31 - 1 is admitted and planned in 64 bits; M = 2^31 is not
        d = layer(0x7fffffff, 1, 1, 1, 0x7fffffff, 1, 1, 1, 0, 1, 0x7fffffff);
        if (walk(&d, false, none, -15) != 0) fail("M = cout = draws = 2^31 - 1 refused", -15);
        plan(&d, false, none, &p);
        if (p.bm != 128 || p.grid[0] != 0x1000000 || p.grid[1] != 0x2000000) fail("the grid at the int limit", -15);
        d = layer(0x10000, 1, 0x6000, 1, 1, 1, 1, 1, 0, 1, 1);                  // 2^16 * 0x6000 = 3 * 2^29 pixels
        expect(walk(&d, false, none, -16), 0, "M = 3 * 2^29 refused", -16);
        d.batch = 0x20000;
        expect(walk(&d, false, none, -17), BBB_ESHAPE, "M = 3 * 2^30 taken", -17);
        d = layer(1, 0x10000, 0x4000, 2, 1, 1, 1, 1, 0, 1, 1);                  // cin * h * w = 2^31
        expect(walk(&d, false, none, -18), BBB_ESHAPE, "cin * h * w = 2^31 taken", -18);
        cases += 18;
    }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld forms", cases, counts[0], counts[1], counts[2], counts[3]);
    for (int i = 0; i < 8; ++i) printf(" %ld", forms[i]);
    printf(" checksum %016llx\n", (unsigned long long)sum);
    return 0;
}
