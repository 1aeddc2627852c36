// Host-only walk of the multi-tensor Adam step's launch plan (csrc/adam_plan.h) for tests/test_adam_sweep_cpu.py, which builds this
// file with -fsanitize=address,undefined: a seeded sweep of ordinary segment lists, every refusal (and that it leaves the plan
// zeroed), then the limits -- n at 1, 1023, 1024, 1025 and around 2^31 * 1024 and INT64_MAX, the sum of chunks at INT32_MAX and one
// above, nseg at 16 and 17, step at 1, 2^24 and INT64_MAX, beta at 0 and at the largest double below 1.  Checks the plan's own
// invariants against a 64-bit restatement of the checks bbb_adam_step made inline before the plan existed, and prints the case counts
// per return code and a checksum of everything the plan returns.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bbb_hip.h"
#include "../../pytorch-bayesiancnn_amd/csrc/adam_plan.h"

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

struct Seg {
    uint64_t p, g, m, v;     // addresses are only looked at, never read
    int64_t n;
};

struct Args {
    Seg seg[BBB_MAX_SEGMENTS + 1];
    int nseg;
    bool null_segs;
    double lr, beta1, beta2, eps;
    int64_t step;
    uint64_t step_dev, lr_dev;
};

// What bbb_adam_step checked inline before the plan existed, in the same order, in arithmetic that cannot overflow.
int old_code(const Args& a) {
    if (a.null_segs || a.nseg <= 0 || a.nseg > BBB_MAX_SEGMENTS || (a.step <= 0 && a.step_dev == 0)) return BBB_EINVAL;
    if (a.lr_dev != 0 && a.step_dev == 0) return BBB_EINVAL;
    if (((a.step_dev | a.lr_dev) & 3u) != 0) return BBB_EALIGN;
    if (!(a.lr >= 0.0) || !(a.beta1 >= 0.0 && a.beta1 < 1.0) || !(a.beta2 >= 0.0 && a.beta2 < 1.0) || !(a.eps >= 0.0)) return BBB_EINVAL;
    unsigned __int128 chunks = 0;
    for (int s = 0; s < a.nseg; ++s) {
        const Seg& g = a.seg[s];
        if (g.p == 0 || g.g == 0 || g.m == 0 || g.v == 0 || g.n <= 0) return BBB_EINVAL;
        if (((g.p | g.g | g.m | g.v) & 3u) != 0) return BBB_EALIGN;
        chunks += ((unsigned __int128)g.n + 1023) / 1024;
        if (chunks > 0x7fffffffu) return BBB_ESHAPE;
    }
    return 0;
}

float* at(uint64_t a) { return reinterpret_cast<float*>(a); }

bool zeroed(const adam_plan::Plan& p) {
    static const adam_plan::Plan zero = {};
    return memcmp(&p, &zero, sizeof p) == 0;
}

int walk(const Args& a, long i) {
    bbb_adam_segment_t segs[BBB_MAX_SEGMENTS + 1];
    for (int s = 0; s <= BBB_MAX_SEGMENTS; ++s) {
        segs[s].param = at(a.seg[s].p); segs[s].grad = at(a.seg[s].g);
        segs[s].exp_avg = at(a.seg[s].m); segs[s].exp_avg_sq = at(a.seg[s].v);
        segs[s].n = a.seg[s].n;
    }
    adam_plan::Plan p;
    memset(&p, 0x5a, sizeof p);
    const int rc = adam_plan::plan(a.null_segs ? nullptr : segs, a.nseg, a.lr, a.beta1, a.beta2, a.eps, a.step, at(a.step_dev), at(a.lr_dev), &p);
    mix(rc);
    if (rc != 0 && rc != BBB_EINVAL && rc != BBB_EALIGN && rc != BBB_ESHAPE) fail("return code", i);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
    if (rc != old_code(a)) fail("not the code of the inline checks", i);
    if (rc != 0) {
        if (!zeroed(p)) fail("a refused plan is not zeroed", i);
        return rc;
    }
    int64_t chunks = 0;
    for (int s = 0; s < a.nseg; ++s) {
        if (p.chunk_begin[s] != chunks) fail("chunk_begin", i);
        if (s > 0 && p.chunk_begin[s] <= p.chunk_begin[s - 1]) fail("chunk_begin is not strictly monotone over the segments", i);
        const int64_t c = a.seg[s].n / 1024 + (a.seg[s].n % 1024 != 0);
        if (c < 1 || (c - 1) * 1024 >= a.seg[s].n || c * 1024 < a.seg[s].n) fail("chunks of a segment", i);
        chunks += c;
        const bool vec = ((a.seg[s].p | a.seg[s].g | a.seg[s].m | a.seg[s].v) & 15u) == 0 && a.seg[s].n >= 4;
        if (p.vec[s] != (vec ? 1 : 0)) fail("vec", i);
        mix(p.chunk_begin[s]); mix(p.vec[s]);
    }
    if (chunks > INT32_MAX || p.chunks != chunks || p.chunks < a.nseg) fail("chunks", i);
    for (int s = a.nseg; s <= BBB_MAX_SEGMENTS; ++s)
        if (p.chunk_begin[s] != p.chunks) fail("chunk_begin behind the last segment", i);
    for (int s = a.nseg; s < BBB_MAX_SEGMENTS; ++s)
        if (p.vec[s] != 0) fail("vec behind the last segment", i);
    if (p.step != (a.step > 0 ? a.step : 1)) fail("step", i);
    // the scalars: each the fp32 nearest to the double value, never formed from fp32 pieces
    const double t = (double)p.step;
    if (p.beta1 != (float)a.beta1 || p.beta2 != (float)a.beta2 || p.eps != (float)a.eps) fail("beta1 / beta2 / eps", i);
    if (p.omb1 != (float)(1.0 - a.beta1) || p.omb2 != (float)(1.0 - a.beta2)) fail("1 - beta", i);
    // step_size and sqrt_bc2 against the bias corrections formed ANOTHER way, 1 - beta^t = -expm1(t log beta) (a few double ulps from
    // the header's 1 - pow(beta, t), so the two may round to neighbouring floats: held to one fp32 ulp).  This catches a wrong
    // formula -- t - 1, a missing root, the betas swapped; that each scalar is the double value rounded ONCE is held bit for bit by
    // tests/test_adam_sweep_cpu.py against Python's own doubles (adam_contract.check_scalars).
    const double bc1 = -expm1(t * log(a.beta1)), bc2 = -expm1(t * log(a.beta2));
    const double ss = a.lr / bc1, sb = sqrt(bc2);
    if (!(fabs((double)p.step_size - ss) <= ldexp(ss, -23)) && !(ss > 3e38 && p.step_size > 3e38f)) fail("step_size", i);
    if (!(fabs((double)p.sqrt_bc2 - sb) <= ldexp(sb, -23))) fail("sqrt_bc2", i);
    if (!(p.sqrt_bc2 > 0.0f && p.sqrt_bc2 <= 1.0f)) fail("sqrt_bc2 outside (0, 1]", i);
    if (!(p.step_size >= (float)a.lr) && a.lr <= 3e38) fail("step_size below lr", i);
    if (!(p.omb1 > 0.0f && p.omb1 <= 1.0f && p.omb2 > 0.0f && p.omb2 <= 1.0f)) fail("1 - beta outside (0, 1]", i);
    mix(p.chunks); mix(p.step);
    // (step_size and sqrt_bc2 are held to the recomputation above and kept out of the checksum: pow is the host library's)
    mixf(p.beta1); mixf(p.beta2); mixf(p.omb1); mixf(p.omb2); mixf(p.eps);
    return 0;
}

Args ordinary(int nseg) {
    Args a = {};
    a.nseg = nseg;
    for (int s = 0; s <= BBB_MAX_SEGMENTS; ++s) a.seg[s] = Seg{0x10000, 0x20000, 0x30000, 0x40000, 100};
    a.lr = 1e-3; a.beta1 = 0.9; a.beta2 = 0.999; a.eps = 1e-8; a.step = 1;
    return a;
}

void expect(const Args& a, int want, const char* what, long i) {
    if (walk(a, i) != want) fail(what, i);
}

}  // namespace

int main() {
    long cases = 0;
    static const int64_t sizes[] = {1, 2, 3, 4, 5, 100, 1023, 1024, 1025, 2047, 2048, 2049, 4099, 65536, 1 << 20, (1 << 20) + 1};
    const int nsz = (int)(sizeof(sizes) / sizeof(sizes[0]));
    static const double betas[] = {0.0, 0.5, 0.9, 0.99, 0.999, 0.9999999, 0.99999999999999988897769753748 /* 1 - 2^-53 */};
    static const int64_t steps[] = {1, 2, 7, 1000, 100000, (1 << 24) - 1, 1 << 24, (1ll << 53) + 1, INT64_MAX};
    // ordinary segment lists, now and then one bad argument
    for (long i = 0; i < 60000; ++i, ++cases) {
        Args a = ordinary(1 + (int)(rnd() % BBB_MAX_SEGMENTS));
        for (int s = 0; s < a.nseg; ++s) {
            Seg& g = a.seg[s];
            g.n = rnd() % 4 ? sizes[rnd() % nsz] : 1 + (int64_t)(rnd() % 5000);
            g.p += 4 * (rnd() % 3 ? 0 : rnd() % 4); g.g += 4 * (rnd() % 5 ? 0 : rnd() % 4);
            g.m += 4 * (rnd() % 7 ? 0 : rnd() % 4); g.v += 4 * (rnd() % 7 ? 0 : rnd() % 4);
            if (rnd() % 400 == 0) g.n = (int64_t)(rnd() % 3) - 2;
            if (rnd() % 400 == 0) (rnd() % 2 ? g.p : g.v) = 0;
            if (rnd() % 400 == 0) (rnd() % 2 ? g.g : g.m) += 1 + rnd() % 3;
        }
        a.beta1 = betas[rnd() % 7]; a.beta2 = betas[rnd() % 7];
        a.step = steps[rnd() % 9];
        a.lr = rnd() % 8 ? 1e-3 * (1 + rnd() % 100) : 0.0;
        a.eps = rnd() % 8 ? 1e-8 : (rnd() % 2 ? 0.0 : 1e-3);
        if (rnd() % 3 == 0) { a.step_dev = 0x50000; a.step = rnd() % 2 ? a.step : (int64_t)(rnd() % 3) - 2; }
        if (rnd() % 4 == 0) a.lr_dev = 0x60000;
        if (rnd() % 100 == 0) a.step_dev += 1 + rnd() % 3;
        if (rnd() % 100 == 0 && a.lr_dev) a.lr_dev += 2;
        if (rnd() % 100 == 0) a.step = -(int64_t)(rnd() % 2);
        if (rnd() % 100 == 0) a.nseg = rnd() % 2 ? 0 : BBB_MAX_SEGMENTS + 1;
        if (rnd() % 200 == 0) a.lr = rnd() % 2 ? -1e-3 : NAN;
        if (rnd() % 200 == 0) (rnd() % 2 ? a.beta1 : a.beta2) = rnd() % 3 == 0 ? 1.0 : (rnd() % 2 ? -0.1 : NAN);
        if (rnd() % 200 == 0) a.eps = rnd() % 2 ? -1e-8 : NAN;
        walk(a, i);
    }
    // every refusal by name, one wrong argument at a time
    {
        Args a = ordinary(3);
        expect(a, 0, "an ordinary launch", cases++);
        a = ordinary(3); a.null_segs = true; expect(a, BBB_EINVAL, "null segs", cases++);
        a = ordinary(0); expect(a, BBB_EINVAL, "nseg 0", cases++);
        a = ordinary(-1); expect(a, BBB_EINVAL, "nseg -1", cases++);
        a = ordinary(16); expect(a, 0, "nseg 16", cases++);
        a = ordinary(17); expect(a, BBB_EINVAL, "nseg 17", cases++);
        a = ordinary(3); a.step = 0; expect(a, BBB_EINVAL, "step 0 without step_dev", cases++);
        a = ordinary(3); a.step = -5; expect(a, BBB_EINVAL, "step < 0 without step_dev", cases++);
        a = ordinary(3); a.step = 0; a.step_dev = 0x50000; expect(a, 0, "step 0 with step_dev", cases++);
        a = ordinary(3); a.lr_dev = 0x60000; expect(a, BBB_EINVAL, "lr_dev without step_dev", cases++);
        a = ordinary(3); a.step_dev = 0x50002; expect(a, BBB_EALIGN, "step_dev misaligned", cases++);
        a = ordinary(3); a.step_dev = 0x50000; a.lr_dev = 0x60001; expect(a, BBB_EALIGN, "lr_dev misaligned", cases++);
        a = ordinary(3); a.lr = -1e-300; expect(a, BBB_EINVAL, "lr < 0", cases++);
        a = ordinary(3); a.lr = NAN; expect(a, BBB_EINVAL, "lr NaN", cases++);
        a = ordinary(3); a.lr = 0.0; expect(a, 0, "lr 0", cases++);
        a = ordinary(3); a.eps = -1e-300; expect(a, BBB_EINVAL, "eps < 0", cases++);
        a = ordinary(3); a.eps = NAN; expect(a, BBB_EINVAL, "eps NaN", cases++);
        for (int which = 0; which < 2; ++which) {
            double Args::*b = which ? &Args::beta2 : &Args::beta1;
            a = ordinary(3); a.*b = 1.0; expect(a, BBB_EINVAL, "beta 1", cases++);
            a = ordinary(3); a.*b = -1e-300; expect(a, BBB_EINVAL, "beta < 0", cases++);
            a = ordinary(3); a.*b = NAN; expect(a, BBB_EINVAL, "beta NaN", cases++);
            a = ordinary(3); a.*b = 0.0; expect(a, 0, "beta 0", cases++);
            a = ordinary(3); a.*b = betas[6]; expect(a, 0, "largest beta below 1", cases++);
        }
        for (int s = 0; s < 3; ++s)
            for (int k = 0; k < 4; ++k) {
                uint64_t Seg::*f = k == 0 ? &Seg::p : k == 1 ? &Seg::g : k == 2 ? &Seg::m : &Seg::v;
                a = ordinary(3); a.seg[s].*f = 0; expect(a, BBB_EINVAL, "null array", cases++);
                for (int off = 1; off < 4; ++off) {
                    a = ordinary(3); a.seg[s].*f += off; expect(a, BBB_EALIGN, "array not 4-byte aligned", cases++);
                }
                a = ordinary(3); a.seg[s].*f += 4; expect(a, 0, "array 4-byte aligned only", cases++);
            }
        a = ordinary(3); a.seg[2].n = 0; expect(a, BBB_EINVAL, "n 0", cases++);
        a = ordinary(3); a.seg[1].n = -1; expect(a, BBB_EINVAL, "n -1", cases++);
        a = ordinary(3); a.seg[0].n = INT64_MIN; expect(a, BBB_EINVAL, "n INT64_MIN", cases++);
        // the order of the checks: the first failing one names the code
        a = ordinary(3); a.seg[0].p += 2; a.seg[1].n = 0; expect(a, BBB_EALIGN, "segment 0 before segment 1", cases++);
        a = ordinary(3); a.seg[0].n = INT64_MAX; a.seg[1].n = 0; expect(a, BBB_ESHAPE, "shape of segment 0 before segment 1", cases++);
        a = ordinary(3); a.lr = -1.0; a.step_dev = 0x50001; expect(a, BBB_EALIGN, "scalar pointers before hyper-parameters", cases++);
    }
    // the chunk limit: one segment around 2^31 * 1024, the sum at INT32_MAX and one above, n next to INT64_MAX
    {
        const int64_t k = 1024, top = (int64_t)INT32_MAX * k;           // the most elements a launch takes
        static const int64_t ones[] = {1, 1023, 1024, 1025};
        for (int j = 0; j < 4; ++j) { Args a = ordinary(1); a.seg[0].n = ones[j]; expect(a, 0, "small n", cases++); }
        Args a = ordinary(1);
        a.seg[0].n = top; expect(a, 0, "(2^31 - 1) * 1024", cases++);
        a.seg[0].n = top - 1; expect(a, 0, "(2^31 - 1) * 1024 - 1", cases++);
        a.seg[0].n = top + 1; expect(a, BBB_ESHAPE, "(2^31 - 1) * 1024 + 1", cases++);
        a.seg[0].n = (1ll << 31) * k - 1; expect(a, BBB_ESHAPE, "2^31 * 1024 - 1", cases++);
        a.seg[0].n = (1ll << 31) * k; expect(a, BBB_ESHAPE, "2^31 * 1024", cases++);
        a.seg[0].n = (1ll << 31) * k + 1; expect(a, BBB_ESHAPE, "2^31 * 1024 + 1", cases++);
        a.seg[0].n = INT64_MAX; expect(a, BBB_ESHAPE, "INT64_MAX", cases++);
        a.seg[0].n = INT64_MAX - 1022; expect(a, BBB_ESHAPE, "INT64_MAX - 1022", cases++);
        a.seg[0].n = INT64_MAX - 1023; expect(a, BBB_ESHAPE, "INT64_MAX - 1023", cases++);
        a = ordinary(16);
        for (int s = 0; s < 16; ++s) a.seg[s].n = INT64_MAX;
        expect(a, BBB_ESHAPE, "16 x INT64_MAX", cases++);
        a = ordinary(3);                                                 // chunks 1 + (INT32_MAX - 2) + 1
        a.seg[0].n = 1; a.seg[1].n = top - 2 * k; a.seg[2].n = 1025 - 1024;
        expect(a, 0, "sum of chunks INT32_MAX", cases++);
        a.seg[2].n = 1025; expect(a, BBB_ESHAPE, "sum of chunks INT32_MAX + 1", cases++);
        a.seg[2].n = 1024; a.seg[1].n += 1; expect(a, BBB_ESHAPE, "sum of chunks INT32_MAX + 1, by one element", cases++);
        a = ordinary(16);
        for (int s = 0; s < 16; ++s) a.seg[s].n = top / 16;            // 16 x 134217727 chunks and 960 elements
        expect(a, BBB_ESHAPE, "16 even shares of the limit, each with a ragged chunk", cases++);
        for (int s = 0; s < 16; ++s) a.seg[s].n = (int64_t)(INT32_MAX / 16) * k;
        expect(a, 0, "16 shares below the limit", cases++);
    }
    // steps and betas at their ends, crossed
    for (int bi = 0; bi < 7; ++bi)
        for (int bj = 0; bj < 7; ++bj)
            for (int si = 0; si < 9; ++si, ++cases) {
                Args a = ordinary(2);
                a.beta1 = betas[bi]; a.beta2 = betas[bj]; a.step = steps[si];
                a.lr = (bi + bj) % 3 ? 1e-3 : 0.1;
                expect(a, 0, "step x beta", cases);
            }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld checksum %016llx\n", cases, counts[0], counts[1], counts[2], counts[3],
           (unsigned long long)sum);
    return 0;
}
