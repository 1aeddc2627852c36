// Host-only walk of the plan of the pooling launches (csrc/pool_plan.h) for tests/test_avgpool_cpu.py, which builds this file
// with -fsanitize=address,undefined: plan() over a seeded sweep of ordinary geometries with every refusal mixed in, and over
// descriptors at the integer limits (2^31 - 1 and other edge values in each field in turn, then in random pairs; plane counts and
// pitches up to 2^62).  Checks the plan's invariants -- the output map is floor mode's, every window holds a valid tap, the grids
// cover their threads and fit an int -- and prints how often each code came up and a checksum of everything returned.
// Then the maximum kind: over seeded (planes, h, w, batch, k, s, pitch) at both group widths, the plan of pool_plan::max_desc against
// a restatement of the checks the scalar maximum entries made themselves before the plan took them over (old_fwd: bbb_maxpool_chwn
// and its bf16 twin; old_bwd: pool_act_bwd_launch and bbb_pool_act_bwd_chwn_bf16) -- the same code whenever at most one rule is
// broken, the same map and grid whenever the plan succeeds -- and the BBB_POOL_MAX descriptors the plan must refuse.
// `pool_plan_check dump` prints one line per average-kind walk() instead (the descriptor, then code, map and grids of both group
// widths): two versions of the header are compared by diffing it, so that part uses nothing newer than plan / plan_bf16 and the
// maximum part is compiled where the header has the kind.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../pytorch-bayesiancnn_amd/csrc/pool_plan.h"

namespace {

using namespace pool_plan;

uint64_t state = 0x9E3779B97F4A7C15ull, sum = 0xcbf29ce484222325ull;
uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
void mix(int64_t v) { sum = (sum ^ (uint64_t)v) * 0x100000001b3ull; }

long counts[4];        // ok / EINVAL / EALIGN / ESHAPE
bool dump = false;

void fail(const char* what, long i) {
    printf("invariant broken: %s (case %ld)\n", what, i);
    exit(1);
}

// one axis: the map is floor mode's and the first and the last window reach into the map
void axis(int64_t n, int64_t k, int64_t s, int64_t p, int64_t o, long i) {
    if (o < 1 || (o - 1) * s + k > n + 2 * p || o * s + k <= n + 2 * p) fail("output map", i);
    if (-p + k <= 0 || (o - 1) * s - p >= n) fail("a window without a valid tap", i);
}

int walk(const bbb_pool_desc_t* d, int64_t planes, int64_t pitch, long i) {
    Plan p;
    const int rc = plan(d, planes, pitch, &p);
    if (dump) {
        if (d != nullptr && d->kind == BBB_POOL_AVG) {
            Plan q;
            const int rq = plan_bf16(d, planes, pitch, &q);
            printf("%d %d %d %d %d %d %d %d %d %d planes %lld pitch %lld", d->h, d->w, d->batch, d->kh, d->kw, d->stride_h, d->stride_w,
                   d->pad_h, d->pad_w, d->count_include_pad, (long long)planes, (long long)pitch);
            printf(" f32 %d %d %d %lld %lld", rc, p.ho, p.wo, (long long)p.fwd_blocks, (long long)p.bwd_blocks);
            printf(" bf16 %d %d %d %lld %lld\n", rq, q.ho, q.wo, (long long)q.fwd_blocks, (long long)q.bwd_blocks);
        }
        return rc;
    }
    mix(rc);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
    if (rc != 0) return rc;
    mix(p.ho); mix(p.wo); mix(p.b4); mix(p.fwd_total4); mix(p.bwd_total4); mix(p.fwd_blocks); mix(p.bwd_blocks);
    axis(d->h, d->kh, d->stride_h, d->pad_h, p.ho, i);
    axis(d->w, d->kw, d->stride_w, d->pad_w, p.wo, i);
    if (p.b4 * 4 != d->batch) fail("image groups", i);
    if (p.fwd_total4 != planes * p.ho * p.wo * p.b4 || p.bwd_total4 != planes * d->h * d->w * p.b4) fail("threads", i);
    if (p.fwd_blocks * kThreads < p.fwd_total4 || (p.fwd_blocks - 1) * kThreads >= p.fwd_total4 || p.fwd_blocks > 0x7fffffffLL)
        fail("forward grid", i);
    if (p.bwd_blocks * kThreads < p.bwd_total4 || (p.bwd_blocks - 1) * kThreads >= p.bwd_total4 || p.bwd_blocks > 0x7fffffffLL)
        fail("backward grid", i);
    if (pitch != 0 && (pitch % 4 != 0 || pitch < (int64_t)d->h * d->w * d->batch)) fail("pitch", i);
    return 0;
}

bbb_pool_desc_t base(int h, int w, int B, int k, int s, int p) {
    bbb_pool_desc_t d = {};
    d.kind = BBB_POOL_AVG;
    d.h = h; d.w = w; d.batch = B; d.kh = d.kw = k; d.stride_h = d.stride_w = s; d.pad_h = d.pad_w = p;
    d.count_include_pad = 1;
    return d;
}

#ifdef BBB_POOL_MAX
// ---- the maximum kind against the scalar entries' former checks ----
long nviol;            // how many of an entry's rules the last old_* call found broken

// bbb_maxpool_chwn (group 4) / bbb_maxpool_chwn_bf16 (group 8), pointers aside
int old_fwd(int64_t planes, int h, int w, int batch, int k, int s, int group, int* ho, int* wo, int64_t* blocks) {
    const bool sizes = planes <= 0 || h <= 0 || w <= 0 || batch <= 0 || k <= 0 || s <= 0;
    nviol = (planes <= 0) + (h <= 0) + (w <= 0) + (batch <= 0) + (k <= 0) + (s <= 0);
    if (sizes) return BBB_EINVAL;
    nviol = (batch % group != 0) + (h < k) + (w < k);
    if (nviol) return BBB_ESHAPE;
    *ho = (h - k) / s + 1; *wo = (w - k) / s + 1;
    const int64_t total = planes * *ho * *wo * (batch / group);
    *blocks = (total + 255) / 256;
    return *blocks > 0x7fffffffLL ? BBB_ESHAPE : 0;
}

// pool_act_bwd_launch (group 4) / bbb_pool_act_bwd_chwn_bf16 (group 8), pointers, activation and flags aside
int old_bwd(int64_t planes, int h, int w, int batch, int k, int s, int64_t pitch, int group, int* hp, int* wp, int64_t* blocks) {
    const int size_v = (planes <= 0) + (h <= 0) + (w <= 0) + (batch <= 0) + (k < 0) + (k > 0 && s <= 0);
    nviol = size_v;
    if (size_v) return BBB_EINVAL;
    const int shape_v = (batch % group != 0) + (k > 0 && h < k) + (k > 0 && w < k);
    const int pitch_v = pitch != 0 ? (pitch < (int64_t)h * w * batch) + (pitch % group != 0) : 0;
    nviol = shape_v + pitch_v;
    if (shape_v) return BBB_ESHAPE;
    if (pitch_v) return BBB_EINVAL;
    *hp = k > 0 ? (h - k) / s + 1 : h; *wp = k > 0 ? (w - k) / s + 1 : w;
    const int64_t total = planes * h * w * (batch / group);
    *blocks = (total + 255) / 256;
    return *blocks > 0x7fffffffLL ? BBB_ESHAPE : 0;
}

long max_cases, max_ok, max_single, max_multi;

void max_case(int64_t planes, int h, int w, int batch, int k, int s, int64_t pitch, int group, long i) {
    const auto planner = group == 4 ? plan : plan_bf16;
    for (int bwd = 0; bwd < 2; ++bwd) {
        int ho = 0, wo = 0;
        int64_t blocks = 0;
        const int want = bwd ? old_bwd(planes, h, w, batch, k, s, pitch, group, &ho, &wo, &blocks)
                             : old_fwd(planes, h, w, batch, k, s, group, &ho, &wo, &blocks);
        const bbb_pool_desc_t d = max_desc(h, w, batch, k, s, bwd != 0);
        Plan p;
        const int rc = planner(&d, planes, bwd ? pitch : 0, &p);
        mix(rc);
        max_cases += 1;
        if (nviol <= 1 && rc != want) fail(bwd ? "maximum backward: the code of a single violation" : "maximum forward: the code of a single violation", i);
        if ((rc == 0) != (want == 0)) fail("maximum: taken by one, refused by the other", i);
        if (want != 0) { (nviol <= 1 ? max_single : max_multi) += 1; continue; }
        max_ok += 1;
        if (p.ho != ho || p.wo != wo || p.b4 != batch / group) fail("maximum: the map", i);
        if ((bwd ? p.bwd_blocks : p.fwd_blocks) != blocks) fail("maximum: the grid", i);
        if ((bwd ? p.bwd_total4 : p.fwd_total4) != (bwd ? planes * h * w : planes * ho * wo) * (batch / group)) fail("maximum: threads", i);
    }
}

void max_walk() {
    for (long i = 0; i < 40000; ++i) {
        const int group = rnd() % 2 ? 4 : 8;
        int64_t planes = 1 + rnd() % 3000;
        int h = 1 + (int)(rnd() % 12), w = rnd() % 3 ? h : 1 + (int)(rnd() % 12), batch = group * (1 + (int)(rnd() % 40));
        int k = (int)(rnd() % 6), s = 1 + (int)(rnd() % 4);                 // k = 0, k > h, k < s all come up
        int64_t pitch = 0;
        if (rnd() % 3 == 0) pitch = (int64_t)h * w * batch + group * (int64_t)(rnd() % 16);
        if (rnd() % 12 == 0) batch += 1 + (int)(rnd() % (group - 1));       // not a multiple of the group
        if (rnd() % 12 == 0) k = (h > w ? h : w) + 1;
        if (rnd() % 30 == 0) pitch = (int64_t)h * w * batch - group;        // below one plane
        if (rnd() % 30 == 0) pitch += group / 2;                            // not a multiple of the group
        if (rnd() % 40 == 0) s = -(int)(rnd() % 2);
        if (rnd() % 40 == 0) k = -1;
        if (rnd() % 40 == 0) planes = 0;
        if (rnd() % 40 == 0) h = 0;
        if (rnd() % 60 == 0) batch = 0;
        max_case(planes, h, w, batch, k, s, pitch, group, i);
    }
    // the grid at the edge of an int, as the entries drew it
    max_case(0x7fffffffLL * 256, 1, 1, 4, 1, 1, 0, 4, -10);
    max_case(0x7fffffffLL * 256 + 1, 1, 1, 8, 0, 1, 0, 8, -11);
    // what the maximum kernels do not implement is not a maximum descriptor
    bbb_pool_desc_t good = max_desc(9, 7, 8, 3, 2, false);
    Plan p;
    if (plan(&good, 6, 0, &p) != 0 || plan_bf16(&good, 6, 0, &p) != 0 || p.ho != 4 || p.wo != 3) fail("a plain maximum descriptor", -12);
    bbb_pool_desc_t d = good; d.pad_h = 1;
    if (plan(&d, 6, 0, &p) != BBB_EINVAL) fail("maximum with a padding taken", -13);
    d = good; d.pad_w = 1;
    if (plan_bf16(&d, 6, 0, &p) != BBB_EINVAL) fail("maximum with a padding taken", -14);
    d = good; d.kw = 2;
    if (plan(&d, 6, 0, &p) != BBB_EINVAL) fail("a rectangular maximum window taken", -15);
    d = good; d.stride_w = 1;
    if (plan(&d, 6, 0, &p) != BBB_EINVAL) fail("maximum with two strides taken", -16);
    d = good; d.count_include_pad = 1;
    if (plan(&d, 6, 0, &p) != BBB_EINVAL) fail("maximum with count_include_pad taken", -17);
    if (avg_only(&good) != nullptr || avg_only(nullptr) != nullptr) fail("avg_only", -18);
    {   // the one code that moved (pool_plan.h): a forward whose own grid fits while the grid over its input does not
        int ho, wo;
        int64_t blocks;
        const int64_t planes = 0x7fffffffLL * 100;
        if (old_fwd(planes, 2, 2, 4, 2, 2, 4, &ho, &wo, &blocks) != 0) fail("the forward's own grid", -20);
        d = max_desc(2, 2, 4, 2, 2, false);
        if (plan(&d, planes, 0, &p) != BBB_ESHAPE) fail("a forward over an input grid past an int taken", -20);
    }
    // no sums in the maximum kernels: a map at the end of the int range is what it was to the scalar entries
    max_case(1, 0x7fffffff, 1, 4, 1, 1, 0, 4, -19);
}
#endif

}  // namespace

int main(int argc, char** argv) {
    dump = argc > 1 && argv[1][0] == 'd';
    long cases = 0;
    // (a) ordinary geometries, every field varied, refusals mixed in
    for (long i = 0; i < 60000; ++i, ++cases) {
        bbb_pool_desc_t d = base(1 + (int)(rnd() % 40), 1 + (int)(rnd() % 40), 4 * (1 + (int)(rnd() % 130)), 1 + (int)(rnd() % 7),
                                 1 + (int)(rnd() % 5), 0);
        if (rnd() % 3 == 0) d.kw = 1 + (int)(rnd() % 7);
        if (rnd() % 3 == 0) d.stride_w = 1 + (int)(rnd() % 5);
        d.pad_h = (int)(rnd() % (d.kh / 2 + 1)); d.pad_w = (int)(rnd() % (d.kw / 2 + 1));
        d.count_include_pad = (int)(rnd() % 2);
        int64_t planes = 1 + rnd() % 4000, pitch = 0;
        if (rnd() % 4 == 0) pitch = (int64_t)d.h * d.w * d.batch + 4 * (int64_t)(rnd() % 16);
        if (rnd() % 20 == 0) d.pad_h = d.kh / 2 + 1;
        if (rnd() % 20 == 0) d.pad_w = d.kw / 2 + 1;
        if (rnd() % 25 == 0) d.batch += 1 + (int)(rnd() % 3);
        if (rnd() % 25 == 0) d.kh = d.h + 2 * d.pad_h + 1;
        if (rnd() % 40 == 0) d.kind = (int)(rnd() % 4);
        if (rnd() % 40 == 0) d.count_include_pad = 2;
        if (rnd() % 40 == 0) d.pad_w = -1;
        if (rnd() % 40 == 0) planes = 0;
        if (rnd() % 40 == 0) pitch = (int64_t)d.h * d.w * d.batch - 4;
        if (rnd() % 40 == 0) pitch += 2;
        walk(rnd() % 2000 == 0 ? nullptr : &d, planes, pitch, i);
    }
    // (b) the integer limits: edge values in each field in turn, then in random pairs, with plane counts and pitches to match
    static const int ints[] = {1, 2, 3, 4, 8, 16, 64, 0x7fff, 0x8000, 0x10000, 0x3fffffff, 0x40000000, 0x7ffffff0, 0x7ffffffc, 0x7fffffff, 0, -1,
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
    {   // the grids at the edge of an int: 2^31 - 1 workgroups are taken, one more is refused
        bbb_pool_desc_t d = base(1, 1, 4, 1, 1, 0);
        if (walk(&d, 0x7fffffffLL * 256, 0, -1) != 0) fail("2^31 - 1 workgroups refused", -1);
        if (walk(&d, 0x7fffffffLL * 256 + 1, 0, -2) != BBB_ESHAPE) fail("2^31 workgroups taken", -2);
        d = base(0x7fffffff, 1, 4, 2, 1, 1);                // h + 2 pad + k past the int range
        if (walk(&d, 1, 0, -3) != BBB_ESHAPE) fail("a padded extent past 2^31 taken", -3);
        cases += 3;
    }
    if (dump) return 0;
#ifdef BBB_POOL_MAX
    max_walk();
#endif
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld checksum %016llx", cases, counts[0], counts[1], counts[2], counts[3],
           (unsigned long long)sum);
#ifdef BBB_POOL_MAX
    printf(" max_cases %ld max_ok %ld max_single %ld max_multi %ld", max_cases, max_ok, max_single, max_multi);
#endif
    printf("\n");
    return 0;
}
