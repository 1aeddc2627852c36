// Host-only walk of the plan of the average-pool launches on bf16 planes (csrc/pool_plan.h: plan_bf16, 16-byte groups of 8 images)
// for tests/test_bf16_avgpool_cpu.py, which builds this file with -fsanitize=address,undefined.  plan_bf16() and, beside it on the
// same descriptor, plan(): the two are one function at two group widths, so everything that does not depend on the width must come
// out the same -- the code of every refusal that is not about the batch or the pitch, the output map -- and what does depend on it
// must differ exactly as the width says.  Ordinary geometries with every refusal mixed in, then descriptors at the integer limits
// (edge values in each field in turn, then in random pairs; plane counts and pitches up to 2^62).  Prints how often each code came
// up (of plan_bf16) and a checksum of everything returned.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../pytorch-bayesiancnn_amd/csrc/pool_plan.h"

namespace {

using namespace pool_plan;

uint64_t state = 0xD1B54A32D192ED03ull, sum = 0xcbf29ce484222325ull;
uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
void mix(int64_t v) { sum = (sum ^ (uint64_t)v) * 0x100000001b3ull; }

long counts[4];        // ok / EINVAL / EALIGN / ESHAPE
long both_ok, only4;   // both widths take the descriptor / only the 4-wide plan does

void fail(const char* what, long i) {
    printf("invariant broken: %s (case %ld)\n", what, i);
    exit(1);
}

// one axis: the map is floor mode's and the first and the last window reach into the map
void axis(int64_t n, int64_t k, int64_t s, int64_t p, int64_t o, long i) {
    if (o < 1 || (o - 1) * s + k > n + 2 * p || o * s + k <= n + 2 * p) fail("output map", i);
    if (-p + k <= 0 || (o - 1) * s - p >= n) fail("a window without a valid tap", i);
}

void invariants(const bbb_pool_desc_t* d, int64_t planes, int64_t pitch, const Plan& p, int group, long i) {
    axis(d->h, d->kh, d->stride_h, d->pad_h, p.ho, i);
    axis(d->w, d->kw, d->stride_w, d->pad_w, p.wo, i);
    if ((int64_t)p.b4 * group != d->batch) fail("image groups", i);
    if (p.fwd_total4 != planes * p.ho * p.wo * p.b4 || p.bwd_total4 != planes * d->h * d->w * p.b4) fail("threads", i);
    if (p.fwd_blocks * kThreads < p.fwd_total4 || (p.fwd_blocks - 1) * kThreads >= p.fwd_total4 || p.fwd_blocks > 0x7fffffffLL)
        fail("forward grid", i);
    if (p.bwd_blocks * kThreads < p.bwd_total4 || (p.bwd_blocks - 1) * kThreads >= p.bwd_total4 || p.bwd_blocks > 0x7fffffffLL)
        fail("backward grid", i);
    if (pitch != 0 && (pitch % group != 0 || pitch < (int64_t)d->h * d->w * d->batch)) fail("pitch", i);
}

int walk(const bbb_pool_desc_t* d, int64_t planes, int64_t pitch, long i) {
    Plan p8, p4;
    const int rc = plan_bf16(d, planes, pitch, &p8), rc4 = plan(d, planes, pitch, &p4);
    mix(rc); mix(rc4);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
    if (rc == 0) {
        mix(p8.ho); mix(p8.wo); mix(p8.b4); mix(p8.fwd_total4); mix(p8.bwd_total4); mix(p8.fwd_blocks); mix(p8.bwd_blocks);
        invariants(d, planes, pitch, p8, 8, i);
    }
    if (rc4 == 0) invariants(d, planes, pitch, p4, 4, i);
    if (rc == 0 && rc4 == 0) {
        both_ok += 1;
        if (p8.ho != p4.ho || p8.wo != p4.wo || 2 * p8.b4 != p4.b4 || 2 * p8.fwd_total4 != p4.fwd_total4 ||
            2 * p8.bwd_total4 != p4.bwd_total4)
            fail("the widths disagree about the map or the groups", i);
    } else if (rc == 0) {
        // 8-wide only: half the threads may fit a grid that the 4-wide count overflows; nothing else separates them this way
        if (rc4 != BBB_ESHAPE || d->batch % 8 != 0) fail("taken 8-wide, refused 4-wide for another reason than the grid", i);
    } else if (rc4 == 0) {
        only4 += 1;
        if (!((rc == BBB_ESHAPE && d->batch % 8 != 0) || (rc == BBB_EINVAL && pitch % 8 != 0)))
            fail("taken 4-wide, refused 8-wide for another reason than batch % 8 or pitch % 8", i);
    } else if (rc != rc4) {
        // both refuse: the order of the checks is shared, so the codes differ only where the batch check (ESHAPE) comes first
        // 8-wide and something later refuses 4-wide, or where twice the threads overflow the 4-wide grid (ESHAPE) and the 8-wide plan
        // goes on to refuse the pitch (EINVAL)
        const bool batch_first = rc == BBB_ESHAPE && d->batch % 8 != 0 && d->batch % 4 == 0;
        const bool grid_first = rc4 == BBB_ESHAPE && rc == BBB_EINVAL && d->batch % 8 == 0 && pitch != 0;
        if (!batch_first && !grid_first) fail("the widths refuse with different codes", i);
    }
    return rc;
}

bbb_pool_desc_t base(int h, int w, int B, int k, int s, int p) {
    bbb_pool_desc_t d = {};
    d.kind = BBB_POOL_AVG;
    d.h = h; d.w = w; d.batch = B; d.kh = d.kw = k; d.stride_h = d.stride_w = s; d.pad_h = d.pad_w = p;
    d.count_include_pad = 1;
    return d;
}

}  // namespace

int main() {
    long cases = 0;
    // (a) ordinary geometries, every field varied, refusals mixed in (batches: multiples of 4, so half of them are not 8-wide)
    for (long i = 0; i < 60000; ++i, ++cases) {
        bbb_pool_desc_t d = base(1 + (int)(rnd() % 40), 1 + (int)(rnd() % 40), 4 * (1 + (int)(rnd() % 130)), 1 + (int)(rnd() % 7),
                                 1 + (int)(rnd() % 5), 0);
        if (rnd() % 4 != 0) d.batch = (d.batch + 7) / 8 * 8;
        if (rnd() % 3 == 0) d.kw = 1 + (int)(rnd() % 7);
        if (rnd() % 3 == 0) d.stride_w = 1 + (int)(rnd() % 5);
        d.pad_h = (int)(rnd() % (d.kh / 2 + 1)); d.pad_w = (int)(rnd() % (d.kw / 2 + 1));
        d.count_include_pad = (int)(rnd() % 2);
        int64_t planes = 1 + rnd() % 4000, pitch = 0;
        if (rnd() % 4 == 0) pitch = (int64_t)d.h * d.w * d.batch + 4 * (int64_t)(rnd() % 16);
        if (rnd() % 20 == 0) d.pad_h = d.kh / 2 + 1;
        if (rnd() % 20 == 0) d.pad_w = d.kw / 2 + 1;
        if (rnd() % 25 == 0) d.batch += 1 + (int)(rnd() % 7);
        if (rnd() % 25 == 0) d.kh = d.h + 2 * d.pad_h + 1;
        if (rnd() % 40 == 0) d.kind = (int)(rnd() % 4);
        if (rnd() % 40 == 0) d.count_include_pad = 2;
        if (rnd() % 40 == 0) d.pad_w = -1;
        if (rnd() % 40 == 0) planes = 0;
        if (rnd() % 40 == 0) pitch = (int64_t)d.h * d.w * d.batch - 8;
        if (rnd() % 40 == 0) pitch += 2;
        walk(rnd() % 2000 == 0 ? nullptr : &d, planes, pitch, i);
    }
    // (b) the integer limits: edge values in each field in turn, then in random pairs, with plane counts and pitches to match
    static const int ints[] = {1, 2, 3, 4, 8, 16, 64, 0x7fff, 0x8000, 0x10000, 0x3fffffff, 0x40000000, 0x7ffffff0, 0x7ffffff8, 0x7fffffff, 0, -1,
                               -0x7fffffff - 1};
    static const int64_t bigs[] = {1, 2, 1000, 0x7fffffffLL, 0x80000000LL, (int64_t)1 << 40, (int64_t)1 << 62, 0x7fffffffffffffffLL, 0, -1};
    for (long i = 0; i < 60000; ++i, ++cases) {
        bbb_pool_desc_t d = base(9, 7, 8, 3, 2, 1);
        int* f[] = {&d.kind, &d.h, &d.w, &d.batch, &d.kh, &d.kw, &d.stride_h, &d.stride_w, &d.pad_h, &d.pad_w, &d.count_include_pad};
        if (i < 11 * 18) *f[i / 18] = ints[i % 18];
        else for (int r = 0; r < 1 + (int)(rnd() % 3); ++r) *f[1 + rnd() % 10] = ints[rnd() % 18];
        const int64_t planes = rnd() % 3 ? 1 + rnd() % 8 : bigs[rnd() % 10];
        const int64_t pitch = rnd() % 4 ? 0 : bigs[rnd() % 10];
        walk(&d, planes, pitch, i);
    }
    {   // hand-worked: the width is the only difference
        bbb_pool_desc_t d = base(9, 7, 12, 3, 2, 1);
        Plan p;
        if (plan_bf16(&d, 6, 0, &p) != BBB_ESHAPE || plan(&d, 6, 0, &p) != 0) fail("batch 12", -1);
        d = base(9, 7, 8, 3, 2, 1);
        if (plan_bf16(&d, 6, 508, &p) != BBB_EINVAL || plan(&d, 6, 508, &p) != 0) fail("pitch 508", -2);   // 504 = one plane; 508 % 8 = 4
        if (plan_bf16(&d, 6, 512, &p) != 0 || p.ho != 5 || p.wo != 4 || p.b4 != 1 || p.fwd_blocks != 1 || p.bwd_blocks != 2)
            fail("the hand-worked plan", -3);                                                          // 120 and 378 threads
        // the grids at the edge of an int: 2^31 - 1 workgroups are taken, one more is refused
        d = base(1, 1, 8, 1, 1, 0);
        if (walk(&d, 0x7fffffffLL * 256, 0, -4) != 0) fail("2^31 - 1 workgroups refused", -4);
        if (walk(&d, 0x7fffffffLL * 256 + 1, 0, -5) != BBB_ESHAPE) fail("2^31 workgroups taken", -5);
        d = base(0x7fffffff, 1, 8, 2, 1, 1);                // h + 2 pad + k past the int range
        if (walk(&d, 1, 0, -6) != BBB_ESHAPE) fail("a padded extent past 2^31 taken", -6);
        cases += 6;
    }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld both %ld only4 %ld checksum %016llx\n", cases, counts[0], counts[1],
           counts[2], counts[3], both_ok, only4, (unsigned long long)sum);
    return 0;
}
