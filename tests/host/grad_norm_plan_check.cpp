// Host-only walk of the gradient-norm launch plan (csrc/grad_norm_plan.h) and of the extended Adam plan (adam_plan::plan_ex in
// csrc/adam_plan.h) for tests/test_adam_ex_cpu.py, which builds this file with -fsanitize=address,undefined: a seeded sweep of ordinary
// segment lists with now and then one bad argument, every refusal by name (and that it leaves the plan zeroed), n next to the chunk
// limit and to INT64_MAX, `first` at its ends, the finish launch's checks, the coefficient at its special values, and plan_ex held to
// plan() plus its own two checks.  Each answer is compared with a restatement in 128-bit arithmetic that cannot overflow.  Prints
// the case counts per return code and a checksum of everything the plans return.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bbb_hip.h"
#include "../../pytorch-bayesiancnn_amd/csrc/adam_plan.h"
#include "../../pytorch-bayesiancnn_amd/csrc/grad_norm_plan.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull, sum = 0xcbf29ce484222325ull;
uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
void mix(int64_t v) { sum = (sum ^ (uint64_t)v) * 0x100000001b3ull; }
void mixf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    mix(u);
}

long counts[4];   // ok / EINVAL / EALIGN / ESHAPE

void fail(const char* what, long i) {
    printf("invariant broken: %s (case %ld)\n", what, i);
    exit(1);
}

void count(int rc, long i) {
    if (rc != 0 && rc != BBB_EINVAL && rc != BBB_EALIGN && rc != BBB_ESHAPE) fail("return code", i);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
    mix(rc);
}

struct Args {
    uint64_t grad[BBB_MAX_SEGMENTS + 1];     // addresses are only looked at, never read
    uint64_t other[BBB_MAX_SEGMENTS + 1];    // param / exp_avg / exp_avg_sq: NOT looked at by the norm plan
    int64_t n[BBB_MAX_SEGMENTS + 1];
    int nseg;
    bool null_segs;
    uint64_t partials;
    int64_t first;
};

float* at(uint64_t a) { return reinterpret_cast<float*>(a); }

int want_code(const Args& a) {
    if (a.null_segs || a.nseg <= 0 || a.nseg > BBB_MAX_SEGMENTS || a.partials == 0 || a.first < 0) return BBB_EINVAL;
    if ((a.partials & 7u) != 0) return BBB_EALIGN;
    unsigned __int128 chunks = 0;
    for (int s = 0; s < a.nseg; ++s) {
        if (a.grad[s] == 0 || a.n[s] <= 0) return BBB_EINVAL;
        if ((a.grad[s] & 3u) != 0) return BBB_EALIGN;
        chunks += ((unsigned __int128)a.n[s] + 4095) / 4096;
        if (chunks + (unsigned __int128)a.first > 0x7fffffffu) return BBB_ESHAPE;
    }
    return 0;
}

int walk(const Args& a, long i) {
    bbb_adam_segment_t segs[BBB_MAX_SEGMENTS + 1];
    for (int s = 0; s <= BBB_MAX_SEGMENTS; ++s) {
        segs[s].param = at(a.other[s]); segs[s].exp_avg = at(a.other[s]); segs[s].exp_avg_sq = at(a.other[s]);
        segs[s].grad = at(a.grad[s]);
        segs[s].n = a.n[s];
    }
    grad_norm_plan::Plan p;
    memset(&p, 0x5a, sizeof p);
    const int rc = grad_norm_plan::plan(a.null_segs ? nullptr : segs, a.nseg, at(a.partials), a.first, &p);
    count(rc, i);
    if (rc != want_code(a)) fail("not the code of the restated checks", i);
    if (rc != 0) {
        static const grad_norm_plan::Plan zero = {};
        if (memcmp(&p, &zero, sizeof p) != 0) fail("a refused plan is not zeroed", i);
        return rc;
    }
    int64_t chunks = 0;
    for (int s = 0; s < a.nseg; ++s) {
        if (p.chunk_begin[s] != chunks) fail("chunk_begin", i);
        const int64_t c = a.n[s] / 4096 + (a.n[s] % 4096 != 0);
        if (c < 1 || (c - 1) * 4096 >= a.n[s] || c * 4096 < a.n[s]) fail("chunks of a segment", i);
        chunks += c;
        if (p.vec[s] != (((a.grad[s] & 15u) == 0 && a.n[s] >= 4) ? 1 : 0)) fail("vec", i);
        mix(p.chunk_begin[s]); mix(p.vec[s]);
    }
    if (p.chunks != chunks || chunks + a.first > INT32_MAX || p.chunks < a.nseg) fail("chunks", i);
    for (int s = a.nseg; s <= BBB_MAX_SEGMENTS; ++s)
        if (p.chunk_begin[s] != p.chunks) fail("chunk_begin behind the last segment", i);
    for (int s = a.nseg; s < BBB_MAX_SEGMENTS; ++s)
        if (p.vec[s] != 0) fail("vec behind the last segment", i);
    mix(p.chunks);
    return 0;
}

Args ordinary(int nseg) {
    Args a = {};
    a.nseg = nseg;
    for (int s = 0; s <= BBB_MAX_SEGMENTS; ++s) { a.grad[s] = 0x20000; a.other[s] = 0x10000; a.n[s] = 100; }
    a.partials = 0x70000;
    return a;
}

void expect(const Args& a, int want, const char* what, long i) {
    if (walk(a, i) != want) fail(what, i);
}

void expect_finish(int got, int want, const char* what, long i) {
    count(got, i);
    if (got != want) fail(what, i);
}

uint32_t fbits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// plan_ex = plan() and two more checks behind it
void walk_ex(double lr, double wd, int decoupled, int64_t step, uint64_t step_dev, uint64_t lr_dev, uint64_t coef_dev, uint64_t ok_dev, int nseg,
             int64_t n0, long i) {
    bbb_adam_segment_t segs[BBB_MAX_SEGMENTS];
    for (int s = 0; s < BBB_MAX_SEGMENTS; ++s) {
        segs[s].param = at(0x10000); segs[s].grad = at(0x20000); segs[s].exp_avg = at(0x30000); segs[s].exp_avg_sq = at(0x40000);
        segs[s].n = s == 0 ? n0 : 100 + s;
    }
    adam_plan::Plan base;
    const int rb = adam_plan::plan(segs, nseg, lr, 0.9, 0.999, 1e-8, step, at(step_dev), at(lr_dev), &base);
    adam_plan::PlanEx p;
    memset(&p, 0x5a, sizeof p);
    const int rc = adam_plan::plan_ex(segs, nseg, lr, 0.9, 0.999, 1e-8, wd, decoupled, step, at(step_dev), at(lr_dev), at(coef_dev), at(ok_dev), &p);
    count(rc, i);
    int want = rb;
    if (want == 0 && ((coef_dev | ok_dev) & 3u) != 0) want = BBB_EALIGN;
    if (want == 0 && !(wd >= 0.0)) want = BBB_EINVAL;
    if (rc != want) fail("plan_ex: not plan()'s code followed by its own checks", i);
    if (rc != 0) {
        static const adam_plan::PlanEx zero = {};
        if (memcmp(&p, &zero, sizeof p) != 0) fail("a refused plan_ex is not zeroed", i);
        return;
    }
    if (memcmp(&p.base, &base, sizeof base) != 0) fail("plan_ex: the base plan is not plan()'s", i);
    if (p.mode != (wd == 0.0 ? 0 : decoupled ? 2 : 1)) fail("plan_ex: mode", i);
    if (fbits(p.wd32) != fbits((float)wd)) fail("plan_ex: wd32", i);
    const long double exact = 1.0L - (long double)lr * (long double)wd;
    if (fabsl(exact) < 3e38L && !(fabsl((long double)p.decay - exact) <= ldexpl(fabsl(exact), -24) + ldexpl(1.0L, -52))) fail("plan_ex: decay", i);
    if (wd == 0.0 && p.decay != 1.0f) fail("plan_ex: decay without decay", i);
    mix(p.mode); mixf(p.wd32); mixf(p.decay);
}

}  // namespace

int main() {
    long cases = 0;
    static const int64_t sizes[] = {1, 2, 3, 4, 5, 100, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 65536, 1 << 22, (1 << 22) + 1};
    const int nsz = (int)(sizeof(sizes) / sizeof(sizes[0]));
    // ordinary segment lists, now and then one bad argument
    for (long i = 0; i < 40000; ++i, ++cases) {
        Args a = ordinary(1 + (int)(rnd() % BBB_MAX_SEGMENTS));
        for (int s = 0; s < a.nseg; ++s) {
            a.n[s] = rnd() % 4 ? sizes[rnd() % nsz] : 1 + (int64_t)(rnd() % 20000);
            a.grad[s] += 4 * (rnd() % 3 ? 0 : rnd() % 4);
            if (rnd() % 5 == 0) a.other[s] = rnd() % 2 ? 0 : 0x10001 + rnd() % 3;        // never looked at
            if (rnd() % 400 == 0) a.n[s] = (int64_t)(rnd() % 3) - 2;
            if (rnd() % 400 == 0) a.grad[s] = 0;
            if (rnd() % 400 == 0) a.grad[s] += 1 + rnd() % 3;
        }
        a.first = rnd() % 3 ? 0 : (int64_t)(rnd() % 100000);
        if (rnd() % 200 == 0) a.first = -(int64_t)(1 + rnd() % 5);
        if (rnd() % 200 == 0) a.first = INT32_MAX - (int64_t)(rnd() % 40);
        if (rnd() % 200 == 0) a.partials = rnd() % 2 ? 0 : a.partials + 1 + rnd() % 7;
        if (rnd() % 100 == 0) a.nseg = rnd() % 2 ? 0 : BBB_MAX_SEGMENTS + 1;
        walk(a, i);
    }
    // every refusal by name
    {
        Args a = ordinary(3); expect(a, 0, "an ordinary launch", cases++);
        a = ordinary(3); a.null_segs = true; expect(a, BBB_EINVAL, "null segs", cases++);
        a = ordinary(0); expect(a, BBB_EINVAL, "nseg 0", cases++);
        a = ordinary(-1); expect(a, BBB_EINVAL, "nseg -1", cases++);
        a = ordinary(16); expect(a, 0, "nseg 16", cases++);
        a = ordinary(17); expect(a, BBB_EINVAL, "nseg 17", cases++);
        a = ordinary(3); a.partials = 0; expect(a, BBB_EINVAL, "null partials", cases++);
        for (int off = 1; off < 8; ++off) { a = ordinary(3); a.partials += off; expect(a, BBB_EALIGN, "partials not 8-byte aligned", cases++); }
        a = ordinary(3); a.first = -1; expect(a, BBB_EINVAL, "first -1", cases++);
        a = ordinary(3); a.first = INT64_MIN; expect(a, BBB_EINVAL, "first INT64_MIN", cases++);
        for (int s = 0; s < 3; ++s) {
            a = ordinary(3); a.grad[s] = 0; expect(a, BBB_EINVAL, "null grad", cases++);
            for (int off = 1; off < 4; ++off) { a = ordinary(3); a.grad[s] += off; expect(a, BBB_EALIGN, "grad not 4-byte aligned", cases++); }
            a = ordinary(3); a.grad[s] += 4; expect(a, 0, "grad 4-byte aligned only", cases++);
            a = ordinary(3); a.other[s] = 0; expect(a, 0, "the other pointers are not looked at (null)", cases++);
            a = ordinary(3); a.other[s] += 1; expect(a, 0, "the other pointers are not looked at (misaligned)", cases++);
            a = ordinary(3); a.n[s] = 0; expect(a, BBB_EINVAL, "n 0", cases++);
            a = ordinary(3); a.n[s] = -1; expect(a, BBB_EINVAL, "n -1", cases++);
            a = ordinary(3); a.n[s] = INT64_MIN; expect(a, BBB_EINVAL, "n INT64_MIN", cases++);
        }
        a = ordinary(3); a.grad[0] += 2; a.n[1] = 0; expect(a, BBB_EALIGN, "segment 0 before segment 1", cases++);
        a = ordinary(3); a.n[0] = INT64_MAX; a.n[1] = 0; expect(a, BBB_ESHAPE, "shape of segment 0 before segment 1", cases++);
        a = ordinary(3); a.partials += 4; a.n[0] = 0; expect(a, BBB_EALIGN, "partials before the segments", cases++);
    }
    // the limits: one segment around 2^31 * 4096, the sum and `first` at INT32_MAX, n next to INT64_MAX
    {
        const int64_t k = 4096, top = (int64_t)INT32_MAX * k;
        static const int64_t ones[] = {1, 4095, 4096, 4097};
        for (int j = 0; j < 4; ++j) { Args a = ordinary(1); a.n[0] = ones[j]; expect(a, 0, "small n", cases++); }
        Args a = ordinary(1);
        a.n[0] = top; expect(a, 0, "(2^31 - 1) * 4096", cases++);
        a.n[0] = top - 1; expect(a, 0, "(2^31 - 1) * 4096 - 1", cases++);
        a.n[0] = top + 1; expect(a, BBB_ESHAPE, "(2^31 - 1) * 4096 + 1", cases++);
        a.n[0] = top; a.first = 1; expect(a, BBB_ESHAPE, "(2^31 - 1) chunks behind one partial", cases++);
        a.first = 0;
        a.n[0] = (1ll << 31) * k; expect(a, BBB_ESHAPE, "2^31 * 4096", cases++);
        a.n[0] = INT64_MAX; expect(a, BBB_ESHAPE, "INT64_MAX", cases++);
        a.n[0] = INT64_MAX - 4094; expect(a, BBB_ESHAPE, "INT64_MAX - 4094", cases++);
        a.n[0] = INT64_MAX - 4095; expect(a, BBB_ESHAPE, "INT64_MAX - 4095", cases++);
        a.n[0] = INT64_MAX; a.first = INT64_MAX; expect(a, BBB_ESHAPE, "INT64_MAX twice", cases++);
        a = ordinary(16);
        for (int s = 0; s < 16; ++s) a.n[s] = INT64_MAX;
        expect(a, BBB_ESHAPE, "16 x INT64_MAX", cases++);
        a = ordinary(3); a.first = INT32_MAX - 3; expect(a, 0, "first + chunks = INT32_MAX", cases++);
        a.first = INT32_MAX - 2; expect(a, BBB_ESHAPE, "first + chunks = INT32_MAX + 1", cases++);
        a.first = INT32_MAX; expect(a, BBB_ESHAPE, "first = INT32_MAX", cases++);
        a.first = INT64_MAX; expect(a, BBB_ESHAPE, "first = INT64_MAX", cases++);
        a = ordinary(3); a.n[0] = 1; a.n[1] = top - 2 * k; a.n[2] = 1; expect(a, 0, "sum of chunks INT32_MAX", cases++);
        a.n[2] = 4097; expect(a, BBB_ESHAPE, "sum of chunks INT32_MAX + 1", cases++);
    }
    // the finish launch's checks, in their order
    {
        using grad_norm_plan::finish_check;
        const float* P = at(0x70000);
        const float *N = at(0x80000), *C = at(0x80004), *O = at(0x80008), *S = at(0x8000c);
        expect_finish(finish_check(P, 7, 1.0, N, C, O, S), 0, "an ordinary finish", cases++);
        expect_finish(finish_check(P, 1, INFINITY, N, nullptr, nullptr, nullptr), 0, "norm only", cases++);
        expect_finish(finish_check(P, INT32_MAX, 1e-300, N, C, O, S), 0, "npartials INT32_MAX, tiny max_norm", cases++);
        expect_finish(finish_check(nullptr, 7, 1.0, N, C, O, S), BBB_EINVAL, "null partials", cases++);
        expect_finish(finish_check(P, 7, 1.0, nullptr, C, O, S), BBB_EINVAL, "null norm_out", cases++);
        expect_finish(finish_check(P, 0, 1.0, N, C, O, S), BBB_EINVAL, "npartials 0", cases++);
        expect_finish(finish_check(P, -1, 1.0, N, C, O, S), BBB_EINVAL, "npartials -1", cases++);
        expect_finish(finish_check(P, INT64_MIN, 1.0, N, C, O, S), BBB_EINVAL, "npartials INT64_MIN", cases++);
        expect_finish(finish_check(at(0x70004), 7, 1.0, N, C, O, S), BBB_EALIGN, "partials 4-byte aligned only", cases++);
        for (uint64_t off = 1; off < 4; ++off) {
            expect_finish(finish_check(P, 7, 1.0, at(0x80000 + off), C, O, S), BBB_EALIGN, "norm_out misaligned", cases++);
            expect_finish(finish_check(P, 7, 1.0, N, at(0x80004 + off), O, S), BBB_EALIGN, "coef_out misaligned", cases++);
            expect_finish(finish_check(P, 7, 1.0, N, C, at(0x80008 + off), S), BBB_EALIGN, "ok_out misaligned", cases++);
            expect_finish(finish_check(P, 7, 1.0, N, C, O, at(0x8000c + off)), BBB_EALIGN, "skipped_out misaligned", cases++);
        }
        expect_finish(finish_check(P, 7, 0.0, N, C, O, S), BBB_EINVAL, "max_norm 0", cases++);
        expect_finish(finish_check(P, 7, -0.0, N, C, O, S), BBB_EINVAL, "max_norm -0", cases++);
        expect_finish(finish_check(P, 7, -1.0, N, C, O, S), BBB_EINVAL, "max_norm < 0", cases++);
        expect_finish(finish_check(P, 7, NAN, N, C, O, S), BBB_EINVAL, "max_norm NaN", cases++);
        expect_finish(finish_check(P, 7, -INFINITY, N, C, O, S), BBB_EINVAL, "max_norm -inf", cases++);
        expect_finish(finish_check(P, (int64_t)INT32_MAX + 1, 1.0, N, C, O, S), BBB_ESHAPE, "npartials 2^31", cases++);
        expect_finish(finish_check(P, INT64_MAX, 1.0, N, C, O, S), BBB_ESHAPE, "npartials INT64_MAX", cases++);
        expect_finish(finish_check(at(0x70001), 7, NAN, N, C, O, S), BBB_EALIGN, "alignment before max_norm", cases++);
    }
    // the coefficient
    {
        using grad_norm_plan::coefficient;
        if (!isnan(coefficient(NAN, 1.0)) || !isnan(coefficient(NAN, INFINITY)) || !isnan(coefficient(-NAN, 1e-3))) fail("NaN norm", cases);
        if (coefficient(INFINITY, 1.0) != 0.0f || coefficient(INFINITY, 1e300) != 0.0f) fail("Inf norm", cases);
        if (coefficient(INFINITY, INFINITY) != 1.0f || coefficient(0.0f, INFINITY) != 1.0f) fail("norm only", cases);
        if (coefficient(0.0f, 1.0) != 1.0f || coefficient(1.0f, 1.0) != (float)(1.0 / (1.0 + 1e-6))) fail("norm at max_norm", cases);
        if (coefficient(0.5f, 1.0) != 1.0f || coefficient(3.0e38f, 1.0) <= 0.0f) fail("unclipped / huge norm", cases);
        static const float norms[] = {0.0f, 1e-30f, 1e-6f, 0.999999f, 1.0f, 1.000001f, 2.0f, 37.5f, 1e6f, 1e30f, 3.4e38f};
        static const double maxes[] = {1e-300, 1e-6, 0.1, 1.0, 5.0, 1e6, 1e300, INFINITY};
        for (float nm : norms)
            for (double mx : maxes) {
                const float c = coefficient(nm, mx);
                const double q = mx / ((double)nm + 1e-6);
                if (!(c >= 0.0f && c <= 1.0f)) fail("coefficient outside [0, 1]", cases);
                if (fbits(c) != fbits(q < 1.0 ? (float)q : 1.0f)) fail("coefficient is not the double formula rounded once", cases);
                mixf(c);
                ++cases;
            }
    }
    // plan_ex: a seeded sweep and its refusals
    {
        static const double wds[] = {0.0, 1e-2, 0.3, 1.0, 1e3, 1e300, INFINITY, -1e-300, -1.0, NAN};
        static const double lrs[] = {0.0, 1e-3, 3e-3, 0.1, 1e10, -1e-3, NAN};
        for (long i = 0; i < 20000; ++i, ++cases) {
            const double wd = rnd() % 4 ? wds[rnd() % 4] : wds[rnd() % 10], lr = rnd() % 8 ? lrs[1 + rnd() % 3] : lrs[rnd() % 7];
            const uint64_t step_dev = rnd() % 2 ? 0x50000 : 0, lr_dev = step_dev && rnd() % 2 ? 0x60000 : (rnd() % 50 ? 0 : 0x60000);
            uint64_t coef_dev = rnd() % 2 ? 0x90000 : 0, ok_dev = rnd() % 2 ? 0x90008 : 0;
            if (rnd() % 50 == 0) coef_dev += 1 + rnd() % 3;
            if (rnd() % 50 == 0) ok_dev += 1 + rnd() % 3;
            const int64_t step = rnd() % 20 ? 1 + (int64_t)(rnd() % 1000) : (int64_t)(rnd() % 3) - 1;
            const int nseg = rnd() % 50 ? 1 + (int)(rnd() % BBB_MAX_SEGMENTS) : (rnd() % 2 ? 0 : 17);
            const int64_t n0 = rnd() % 50 ? 1 + (int64_t)(rnd() % 5000) : (rnd() % 2 ? INT64_MAX : 0);
            walk_ex(lr, wd, (int)(rnd() % 2), step, step_dev, lr_dev, coef_dev, ok_dev, nseg, n0, cases);
        }
        walk_ex(1e-3, -1.0, 0, 1, 0, 0, 0x90002, 0, 3, 100, cases++);          // alignment before weight_decay
        walk_ex(-1e-3, 1e-2, 0, 1, 0, 0, 0x90002, 0, 3, 100, cases++);         // plan()'s checks before both
        walk_ex(1e-3, 1e-2, 1, 1, 0, 0, 0, 0, 1, INT64_MAX, cases++);
        walk_ex(1e-3, 1e-2, 1, 1, 0, 0, 0, 0, 1, (int64_t)INT32_MAX * 1024, cases++);
    }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld checksum %016llx\n", cases, counts[0], counts[1], counts[2], counts[3],
           (unsigned long long)sum);
    return 0;
}
