// Host-only walk of the plan of bbb_first_layer_dgrad_bf16 (csrc/input_grad_bf16_plan.h) for tests/test_bf16_input_grad_cpu.py, which
// builds this file with -fsanitize=address,undefined.  Ordinary first layers with every refusal mixed in, then descriptors at the
// integer limits (edge values in each field in turn, then in random groups; pitches up to 2^62).  For every plan that is taken the
// invariants the kernel relies on are checked: the tiles cover D exactly once, the workgroups dealt to the 8 XCDs cover the tiles, every offset the kernel forms fits 32 bits, the grid
// fits an int.  Prints how often each code came up, how often each tile, and a checksum of everything returned.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../pytorch-bayesiancnn_amd/csrc/input_grad_bf16_plan.h"

namespace {

using namespace input_grad_bf16_plan;

uint64_t state = 0x9E3779B97F4A7C15ull, sum = 0xcbf29ce484222325ull;
uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
void mix(int64_t v) { sum = (sum ^ (uint64_t)v) * 0x100000001b3ull; }

long counts[4];        // ok / EINVAL / EALIGN / ESHAPE
long tiles[2];         // tile_j 32 / 64

void fail(const char* what, long i) {
    printf("invariant broken: %s (case %ld)\n", what, i);
    exit(1);
}

void axis(int64_t n, int64_t k, int64_t s, int64_t p, int64_t dl, int64_t o, long i) {
    const int64_t reach = dl * (k - 1) + 1;
    if (o < 1 || (o - 1) * s + reach > n + 2 * p || o * s + reach <= n + 2 * p) fail("output map", i);
}

void invariants(const bbb_conv_desc_t* d, int64_t gp, int64_t dp, uint32_t flags, const Plan& p, long i) {
    axis(d->h, d->kh, d->stride_h, d->pad_h, d->dil_h, p.ho, i);
    axis(d->w, d->kw, d->stride_w, d->pad_w, d->dil_w, p.wo, i);
    if (p.M != (int64_t)d->draws * d->cout || p.J != (int64_t)d->cin * d->kh * d->kw) fail("M or J", i);
    if (p.Kp % 8 != 0 || p.Kp < p.J || p.Kp >= p.J + 8 || d->w_draw_stride != (int64_t)d->cout * p.Kp) fail("row pitch", i);
    if (p.ncols != (int64_t)p.ho * p.wo * d->batch || p.ncols % 8 != 0 || gp < p.ncols || dp < p.ncols) fail("columns", i);
    if (gp % 8 != 0 || dp % 4 != 0) fail("pitch alignment", i);
    if (p.tile_j != (p.J <= 32 ? 32 : 64)) fail("tile rule", i);
    if ((int64_t)p.j_tiles * p.tile_j < p.J || (int64_t)(p.j_tiles - 1) * p.tile_j >= p.J) fail("j tiles", i);
    if (p.n_tiles * kTileN < p.ncols || (p.n_tiles - 1) * kTileN >= p.ncols) fail("n tiles", i);
    if ((int64_t)p.k_chunks * kChunk < p.M || (int64_t)(p.k_chunks - 1) * kChunk >= p.M) fail("k chunks", i);
    if (p.items != p.j_tiles * p.n_tiles || p.items < 1) fail("items", i);
    if (p.blocks != 8 * (int64_t)p.per_xcd || p.blocks < p.items || p.blocks - 8 >= p.items || p.blocks > 0x7fffffffLL) fail("grid", i);
    if ((int64_t)p.M * gp > 0x7fffffffLL || (int64_t)p.M * p.Kp > 0x7fffffffLL || (int64_t)p.J * dp > 0x7fffffffLL) fail("32-bit offsets", i);
    if ((flags & BBB_BF16_W_TAP_MAJOR) != 0 && d->cin % 8 != 0) fail("tap-major rows without cin % 8", i);
    const Args a = args_of(d, p, gp, dp, flags);
    if (a.items != p.items || a.per_xcd != p.per_xcd) fail("kernel arguments: the grid", i);
    if ((int64_t)a.khkw * a.cin != p.J || a.g_pitch != gp || a.d_pitch != dp || a.k_chunks != p.k_chunks) fail("kernel arguments", i);
}

int walk(const bbb_conv_desc_t* d, int64_t gp, int64_t dp, uint32_t flags, int ptr_rc, long i) {
    Plan p;
    const int rc = plan(d, gp, dp, flags, ptr_rc, &p);
    mix(rc);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
    if (rc == 0) {
        mix(p.ho); mix(p.wo); mix(p.M); mix(p.J); mix(p.Kp); mix(p.ncols); mix(p.tile_j); mix(p.k_chunks); mix(p.j_tiles); mix(p.n_tiles);
        mix(p.items); mix(p.blocks);
        tiles[p.tile_j == 64] += 1;
        invariants(d, gp, dp, flags, p, i);
    } else if (p.blocks != 0 || p.tile_j != 0) {
        fail("a refusal leaves a plan behind", i);
    }
    return rc;
}

bbb_conv_desc_t layer(int B, int cin, int h, int w, int cout, int kh, int kw, int s, int pd, int dl, int E) {
    bbb_conv_desc_t d = {};
    d.batch = B; d.cin = cin; d.h = h; d.w = w; d.cout = cout; d.kh = kh; d.kw = kw;
    d.stride_h = d.stride_w = s; d.pad_h = d.pad_w = pd; d.dil_h = d.dil_w = dl; d.draws = E;
    d.w_draw_stride = (int64_t)cout * (((int64_t)cin * kh * kw + 7) & ~(int64_t)7);
    return d;
}

int64_t cols(const bbb_conv_desc_t& d) {      // a row of g_pre where the descriptor has one, else any multiple of 8
    if (d.stride_h <= 0 || d.stride_w <= 0 || d.batch <= 0) return 8;
    const int64_t ho = ((int64_t)d.h + 2 * (int64_t)d.pad_h - (int64_t)d.dil_h * ((int64_t)d.kh - 1) - 1) / d.stride_h + 1;
    const int64_t wo = ((int64_t)d.w + 2 * (int64_t)d.pad_w - (int64_t)d.dil_w * ((int64_t)d.kw - 1) - 1) / d.stride_w + 1;
    return ho > 0 && wo > 0 ? conv_desc_check::mul_cap(ho, wo, d.batch) : 8;
}

}  // namespace

int main() {
    long cases = 0;
    // (a) ordinary first layers (a fifth of them linear: 1 x 1 taps on a 1 x 1 map), refusals mixed in
    for (long i = 0; i < 60000; ++i, ++cases) {
        const bool linear = rnd() % 5 == 0;
        const int k = linear ? 1 : 1 + (int)(rnd() % 11);
        bbb_conv_desc_t d = layer(8 * (1 + (int)(rnd() % 64)), linear ? 4 * (1 + (int)(rnd() % 200)) : 1 + (int)(rnd() % 9), linear ? 1 : 1 + (int)(rnd() % 32),
                                  linear ? 1 : 1 + (int)(rnd() % 32), 1 + (int)(rnd() % 96), k, k, 1 + (int)(rnd() % 4),
                                  linear ? 0 : (int)(rnd() % (k + 1)), 1 + (int)(rnd() % 2), 1 + (int)(rnd() % 10));
        if (!linear && rnd() % 3 == 0) { d.kw = 1 + (int)(rnd() % 5); d.w_draw_stride = (int64_t)d.cout * (((int64_t)d.cin * d.kh * d.kw + 7) & ~(int64_t)7); }
        uint32_t flags = rnd() % 2 ? BBB_BF16_BWD_G_F32 : 0;
        if (d.cin % 8 == 0 && rnd() % 2) flags |= BBB_BF16_W_TAP_MAJOR;
        int64_t gp = cols(d) + 8 * (int64_t)(rnd() % 3 ? 0 : rnd() % 9), dp = cols(d) + 4 * (int64_t)(rnd() % 3 ? 0 : rnd() % 9);
        int ptr_rc = 0;
        if (rnd() % 25 == 0) d.batch += 1 + (int)(rnd() % 7);
        if (rnd() % 25 == 0) d.kh = d.h + 2 * d.pad_h + 2;
        if (rnd() % 30 == 0) flags |= 4u << (rnd() % 8);
        if (rnd() % 30 == 0) flags |= BBB_BF16_W_TAP_MAJOR;
        if (rnd() % 30 == 0) gp += 4;
        if (rnd() % 30 == 0) dp += 2;
        if (rnd() % 30 == 0) gp = cols(d) - 8;
        if (rnd() % 30 == 0) dp = cols(d) - 4;
        if (rnd() % 30 == 0) d.w_draw_stride += 8;
        if (rnd() % 40 == 0) d.act = 1;
        if (rnd() % 40 == 0) d.x_draw_stride = 8;
        if (rnd() % 40 == 0) d.unit_div = 2;
        if (rnd() % 40 == 0) d.draws = 0;
        if (rnd() % 40 == 0) d.pad_w = -1;
        if (rnd() % 30 == 0) ptr_rc = rnd() % 2 ? BBB_EINVAL : BBB_EALIGN;
        walk(rnd() % 2000 == 0 ? nullptr : &d, gp, dp, flags, ptr_rc, i);
    }
    // (b) the integer limits
    static const int ints[] = {1, 2, 3, 8, 16, 32, 33, 64, 0x7fff, 0x8000, 0x10000, 0x3fffffff, 0x40000000, 0x7ffffff8, 0x7fffffff, 0, -1,
                               -0x7fffffff - 1};
    static const int64_t bigs[] = {8, 64, 1000, 0x7ffffff8LL, 0x80000000LL, (int64_t)1 << 40, (int64_t)1 << 62, 0x7ffffffffffffff8LL, 0, -8};
    for (long i = 0; i < 60000; ++i, ++cases) {
        bbb_conv_desc_t d = layer(8, 3, 9, 13, 12, 2, 3, 2, 1, 1, 2);
        int* f[] = {&d.batch, &d.cin, &d.h, &d.w, &d.cout, &d.kh, &d.kw, &d.stride_h, &d.stride_w, &d.pad_h, &d.pad_w, &d.dil_h, &d.dil_w, &d.draws};
        if (i < 14 * 18) *f[i / 18] = ints[i % 18];
        else for (int r = 0; r < 1 + (int)(rnd() % 3); ++r) *f[rnd() % 14] = ints[rnd() % 18];
        if (rnd() % 2) {     // keep the rows' pitch right where the sizes allow it, so that the later checks are reached
            const int64_t J = conv_desc_check::mul_cap(d.cin > 0 ? d.cin : 1, d.kh > 0 ? d.kh : 1, d.kw > 0 ? d.kw : 1);
            if (J < ((int64_t)1 << 30) && d.cout > 0) d.w_draw_stride = d.cout * ((J + 7) & ~(int64_t)7);
        }
        const int64_t gp = rnd() % 3 ? cols(d) : bigs[rnd() % 10], dp = rnd() % 3 ? cols(d) : bigs[rnd() % 10];
        walk(&d, gp, dp, rnd() % 4, 0, i);
    }
    {   // hand-worked
        Plan p;
        bbb_conv_desc_t d = layer(8, 3, 9, 13, 12, 2, 3, 2, 1, 1, 2);       // stride 2, pad 1: 5 x 7 pixels, J = 18, Kp = 24, M = 24
        if (plan(&d, 280, 280, 0, 0, &p) != 0 || p.ho != 5 || p.wo != 7 || p.ncols != 280 || p.J != 18 || p.Kp != 24 || p.M != 24 ||
            p.tile_j != 32 || p.k_chunks != 1 || p.j_tiles != 1 || p.n_tiles != 3 || p.items != 3 || p.per_xcd != 1 || p.blocks != 8)
            fail("the hand-worked plan", -1);
        d = layer(512, 3, 32, 32, 64, 11, 11, 4, 5, 1, 10);                 // AlexNet conv1 at 32 x 32: 8 x 8 pixels, J = 363
        if (plan(&d, 32768 + 32, 32768, BBB_BF16_BWD_G_F32, 0, &p) != 0 || p.tile_j != 64 || p.j_tiles != 6 || p.n_tiles != 256 || p.k_chunks != 20)
            fail("AlexNet conv1", -2);
        // the order: a null operand before the flags' successor checks, alignment before shape
        d = layer(12, 3, 9, 13, 12, 2, 3, 2, 1, 1, 2);                      // batch % 8 != 0 ...
        if (plan(&d, 420, 422, 0, 0, &p) != BBB_EALIGN) fail("EALIGN comes before ESHAPE", -3);      // ... and a D pitch % 4 != 0
        if (plan(&d, 420, 420, 8, BBB_EALIGN, &p) != BBB_EINVAL) fail("EINVAL comes before EALIGN", -4);
        if (plan(&d, 424, 420, 0, 0, &p) != BBB_ESHAPE) fail("batch % 8", -5);
        // 32-bit limits: M * g_row_pitch at the edge
        d = layer(8, 4, 1, 1, 1 << 10, 1, 1, 1, 0, 1, 1 << 10);            // M = 2^20
        d.w_draw_stride = (int64_t)(1 << 10) * 8;
        if (walk(&d, 2040, 8, 0, 0, -6) != 0) fail("M * pitch = 2^31 - 2^23 refused", -6);
        if (walk(&d, 2048, 8, 0, 0, -7) != BBB_ESHAPE) fail("M * pitch = 2^31 taken", -7);
        cases += 7;
    }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld tile32 %ld tile64 %ld checksum %016llx\n", cases, counts[0], counts[1], counts[2],
           counts[3], tiles[0], tiles[1], (unsigned long long)sum);
    return 0;
}
