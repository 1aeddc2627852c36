// Host-only walk of the bf16 launch plans (csrc/pconv_bf16_plan.h) for tests/test_bf16_plan_cpu.py, which builds this file with
// -fsanitize=undefined: the three plans over a seeded sweep of ordinary geometries and over descriptors whose dimensions sit near
// INT32_MAX / 2 (every product inside the plans must be guarded, not overflow).  Prints a checksum of everything the plans return.
// `bf16_plan_check dump` prints one line per walk() instead -- whether the kernel reaches past the padded input, then each plan's
// return code and fields -- so that two builds of this file against two versions of the header can be compared line by line.
#include <stdint.h>
#include <stdio.h>

#include "../../include/bbb_hip.h"
#include "../../pytorch-bayesiancnn_amd/csrc/pconv_bf16_plan.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull, sum = 0xcbf29ce484222325ull;
uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
int pick(const int* v, int n) { return v[rnd() % (uint32_t)n]; }
void mix(int64_t v) { sum = (sum ^ (uint64_t)v) * 0x100000001b3ull; }

long counts[4];   // ok / EINVAL / EALIGN / ESHAPE over all plan calls
bool dump = false;
long walks = 0;

void tally(int rc) {
    mix(rc);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
}

void walk(const bbb_conv_desc_t& d, uint32_t flags, int up_h, int up_w, int out_h, int out_w) {
    bf16_plan::FwdPlan f;
    int rc = bf16_plan::fwd_plan(&d, flags, 0, &f);
    tally(rc);
    if (dump) {
        const bool reach = (int64_t)d.h + 2 * (int64_t)d.pad_h < (int64_t)d.dil_h * (d.kh - 1) + 1 ||
                           (int64_t)d.w + 2 * (int64_t)d.pad_w < (int64_t)d.dil_w * (d.kw - 1) + 1;
        printf("%ld reach %d fwd %d form %d shape %d kgs %d ws %d blocks %lld", walks++, reach, rc, rc ? -1 : f.form, rc ? 0 : f.tile.shape,
               rc ? 0 : f.tile.kgs, rc ? 0 : (int)f.tile.ws, rc ? 0LL : (long long)f.blocks);
    }
    if (rc == 0) {
        mix(f.form); mix(f.tile.shape); mix(f.tile.kgs); mix(f.tile.ws); mix(f.blocks); mix(f.smem_bytes); mix(f.y_ds); mix(f.nt); mix(f.ks);
        mix(f.f.Ntiles); mix(f.f.G); mix(f.f.nbt); mix(f.f.Mtiles); mix(f.f.per_xcd); mix(f.f.px_run); mix(f.f.pool); mix(f.f.y_c8);
        mix(f.f.y_f32); mix(f.g.ho); mix(f.g.wo); mix(f.g.K); mix(f.g.Kp); mix(f.g.x_inv);
    }
    bf16_plan::DgradPlan g;
    rc = bf16_plan::dgrad_plan(&d, up_h, up_w, out_h, out_w, flags & BBB_BF16_W_TAP_MAJOR, 0, &g);
    tally(rc);
    if (dump) printf(" dgrad %d shape %d kgs %d ws %d blocks %lld", rc, rc ? 0 : g.tile.shape, rc ? 0 : g.tile.kgs, rc ? 0 : (int)g.tile.ws, rc ? 0LL : (long long)g.grid.blocks);
    if (rc == 0) {
        mix(g.tile.shape); mix(g.tile.kgs); mix(g.tile.ws); mix(g.tstep_h); mix(g.tstep_w); mix(g.grid.blocks); mix(g.grid.Mtiles);
        mix(g.grid.G); mix(g.grid.per_xcd);
    }
    bf16_plan::LrtPlan l;
    rc = bf16_plan::lrt_plan(&d, &l);
    tally(rc);
    if (dump) printf(" lrt %d shape %d kgs %d ws %d\n", rc, rc ? 0 : l.tile.shape, rc ? 0 : l.tile.kgs, rc ? 0 : (int)l.tile.ws);
    if (rc == 0) {
        mix(l.tile.shape); mix(l.tile.kgs); mix(l.tile.ws);
        bf16_plan::Geom geom;
        bf16_plan::TileGrid t;
        rc = bf16_plan::slab_limits(&d, l.ho, l.wo, bf16_plan::kLrtLimits, &geom);
        if (rc == 0) rc = bf16_plan::tile_grid(l.tile.shape, l.work, &t);
        tally(rc);
        if (rc == 0) { mix(t.blocks); mix(t.Mtiles); mix(t.G); }
    }
}

}  // namespace

int main(int argc, char** argv) {
    dump = argc > 1 && argv[1][0] == 'd';
    static const int batches[] = {8, 16, 24, 64, 128, 136, 200, 256, 264, 512}, taps[] = {1, 3, 5, 11}, strides[] = {1, 1, 2, 4};
    static const int pools[] = {0, 0, 0, 1, (3 << 8) | 2, (2 << 8) | 2, (3 << 8) | 3};
    static const uint32_t flagset[] = {0, 1, 2, 3, 2 | 4, 2 | 4 | 8, 8, 4};
    long cases = 0;
    for (int i = 0; i < 60000; ++i, ++cases) {
        bbb_conv_desc_t d = {};
        d.batch = pick(batches, 10);
        d.cin = i % 3 == 0 ? 1 + (int)(rnd() % 1040) : (i % 3 == 1 ? 8 * (1 + (int)(rnd() % 64)) : 1 + (int)(rnd() % 40));
        d.h = 1 + (int)(rnd() % 32); d.w = 1 + (int)(rnd() % 32);
        d.cout = rnd() % 4 == 0 ? 1 + (int)(rnd() % 16) : 1 + (int)(rnd() % 512);
        d.kh = pick(taps, 4); d.kw = rnd() % 4 == 0 ? pick(taps, 4) : d.kh;
        d.stride_h = pick(strides, 4); d.stride_w = pick(strides, 4);
        d.dil_h = 1 + (int)(rnd() % 2); d.dil_w = 1 + (int)(rnd() % 2);
        d.pad_h = (int)(rnd() % (uint32_t)(d.dil_h * (d.kh - 1) + 1)); d.pad_w = (int)(rnd() % (uint32_t)(d.dil_w * (d.kw - 1) + 1));
        d.draws = 1 + (int)(rnd() % 64);
        d.act = (int)(rnd() % 3);
        d.pool = pick(pools, 7);
        const uint32_t flags = flagset[rnd() % 8];
        const int up_h = 1 + (int)(rnd() % 4), up_w = 1 + (int)(rnd() % 4);
        // an input map whose forward (stride up) gives d's map, most of the time
        const int64_t fph = (int64_t)d.dil_h * (d.kh - 1) - d.pad_h, fpw = (int64_t)d.dil_w * (d.kw - 1) - d.pad_w;
        int64_t out_h = (int64_t)(d.h - 1) * up_h + 1 + (int64_t)d.dil_h * (d.kh - 1) - 2 * fph + (int)(rnd() % (uint32_t)up_h);
        int64_t out_w = (int64_t)(d.w - 1) * up_w + 1 + (int64_t)d.dil_w * (d.kw - 1) - 2 * fpw + (int)(rnd() % (uint32_t)up_w);
        walk(d, flags, up_h, up_w, out_h < 1 ? 1 : (int)out_h, out_w < 1 ? 1 : (int)out_w);
        bbb_conv_desc_t s = d;              // the transposed launch's own descriptor: stride 1, nothing else set
        s.stride_h = s.stride_w = 1; s.act = 0; s.pool = 0;
        walk(s, flags, up_h, up_w, out_h < 1 ? 1 : (int)out_h, out_w < 1 ? 1 : (int)out_w);
    }
    // the extremes: every field from {small, near INT32_MAX / 2, INT32_MAX}
    static const int big[] = {1, 2, 8, 0x3FFFFFF8, 0x40000000, 0x7FFFFFF8, 0x7FFFFFFF};
    static const int mid[] = {1, 3, 64, 1 << 12, 1 << 20, 0x3FFFFFFF, 0x7FFFFFFF};
    for (int i = 0; i < 60000; ++i, ++cases) {
        bbb_conv_desc_t d = {};
        d.batch = pick(big, 7); d.cin = pick(mid, 7); d.h = pick(mid, 7); d.w = pick(mid, 7); d.cout = pick(mid, 7);
        d.kh = pick(mid, 5); d.kw = pick(mid, 5);
        d.stride_h = pick(mid, 7); d.stride_w = pick(mid, 7); d.dil_h = pick(mid, 7); d.dil_w = pick(mid, 7);
        d.pad_h = pick(mid, 7) - 1; d.pad_w = pick(mid, 7) - 1;
        d.draws = pick(mid, 7);
        d.pool = pick(pools, 7);
        if (i % 2) { d.stride_h = d.stride_w = 1; d.pool = 0; }
        if (i % 4 == 3) { d.kh = d.kw = 1 + (int)(rnd() % 3); d.dil_h = d.dil_w = 1; d.pad_h = d.pad_w = 0; d.h = pick(mid, 4); d.w = pick(mid, 4); }
        walk(d, flagset[rnd() % 8], pick(mid, 7), pick(mid, 7), pick(mid, 7), pick(mid, 7));
    }
    // wide maps on the pooled forms: the strip searches walk the pooled row
    for (int i = 0; i < 64; ++i, ++cases) {
        bbb_conv_desc_t d = {};
        d.batch = 8; d.cin = 1 + i % 3; d.h = 2 + i % 5; d.w = (1 << (10 + i % 12)) + i; d.cout = 1 + i % 40;
        d.kh = d.kw = 1 + i % 3; d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1; d.draws = 1 + i % 7;
        d.pool = i % 2 ? 1 : (3 << 8) | 2;
        walk(d, 0, 2, 2, 4, 4);
    }
    if (dump) return 0;
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld checksum %016llx\n", cases, counts[0], counts[1], counts[2], counts[3],
           (unsigned long long)sum);
    return 0;
}
