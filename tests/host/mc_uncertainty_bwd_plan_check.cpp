// Host-only walk of the launch plan of the uncertainty reduction's backward (plan_bwd in csrc/mc_uncertainty_plan.h) for
// tests/test_uncertainty_grad_cpu.py, which builds this file with -fsanitize=address,undefined: a seeded sweep of ordinary arguments
// (draws around the limit, any subset of the seven upstream gradients, misaligned and missing pointers), then arguments at the 32-bit
// limits.  Checks the plan's own invariants and the order of its refusals against the rule written out here in 64-bit arithmetic, and
// prints the case counts per return code and a checksum of everything the plan returns.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/bbb_hip.h"
#include "../../pytorch-bayesiancnn_amd/csrc/mc_uncertainty_plan.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull, sum = 0xcbf29ce484222325ull;
uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
void mix(int64_t v) { sum = (sum ^ (uint64_t)v) * 0x100000001b3ull; }

long counts[4];   // ok / EINVAL / EALIGN / ESHAPE

void fail(const char* what, long i) {
    printf("invariant broken: %s (case %ld)\n", what, i);
    exit(1);
}

struct Args {
    uint64_t logits, p_mean, out, ups[7];     // addresses are only looked at, never read
    int draws, batch, classes;
};

const void* at(uint64_t a) { return reinterpret_cast<const void*>(a); }

// The documented rule (include/bbb_hip.h), in 64-bit arithmetic.
int expected(const Args& a) {
    uint64_t any = 0;
    for (int k = 0; k < 7; ++k) any |= a.ups[k];
    if (a.logits == 0 || a.p_mean == 0 || a.out == 0 || a.draws <= 0 || a.batch <= 0 || a.classes <= 0 || any == 0) return BBB_EINVAL;
    if (((a.logits | a.p_mean | a.out | any) & 3u) != 0) return BBB_EALIGN;
    if ((int64_t)a.batch + 63 > INT32_MAX || a.draws > 202) return BBB_ESHAPE;
    return 0;
}

void walk(const Args& a, long i) {
    mc_uncertainty_plan::Plan p;
    const void* ups[7];
    for (int k = 0; k < 7; ++k) ups[k] = at(a.ups[k]);
    const int rc = mc_uncertainty_plan::plan_bwd(at(a.logits), at(a.p_mean), a.draws, a.batch, a.classes, ups, at(a.out), &p);
    mix(rc);
    if (rc != expected(a)) fail("return code", i);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
    if (rc != 0) {
        if (p.rows != 0 || p.blocks != 0 || p.lds_bytes != 0) fail("a refused plan is not empty", i);
        return;
    }
    mix(p.rows); mix(p.blocks); mix(p.lds_bytes);
    if (p.rows != 1) fail("one draw per block", i);
    if (p.blocks < 1 || (int64_t)p.blocks * 64 < a.batch || ((int64_t)p.blocks - 1) * 64 >= a.batch) fail("blocks", i);
    if ((int64_t)p.blocks * 64 - 1 > INT32_MAX) fail("image index of the last lane", i);
    if (a.draws > 65535) fail("gridDim.y", i);
    if (p.lds_bytes != 0) fail("lds", i);
}

uint64_t ptr(uint64_t base) { return rnd() % 64 == 0 ? 0 : base + (rnd() % 32 == 0 ? 1 + rnd() % 3 : 0); }

}  // namespace

int main() {
    long cases = 0;
    static const int smalls[] = {1, 2, 3, 7, 10, 15, 16, 17, 63, 64, 65, 74, 75, 100, 130, 201, 202, 203, 213, 512, 1000, 1024};
    const int ns = (int)(sizeof(smalls) / sizeof(smalls[0]));
    for (long i = 0; i < 60000; ++i, ++cases) {
        Args a = {};
        a.logits = ptr(0x1000);
        a.p_mean = ptr(0xA000);
        a.out = ptr(0xB000);
        const uint32_t mask = rnd() % 16 == 0 ? 0 : (rnd() % 4 == 0 ? 1u << (rnd() % 7) : rnd() % 128);
        for (int k = 0; k < 7; ++k)
            if (mask >> k & 1) a.ups[k] = 0x2000 + 0x1000 * (uint64_t)k + (rnd() % 64 == 0 ? 1 + rnd() % 3 : 0);
        a.draws = rnd() % 50 == 0 ? (int)(rnd() % 3) - 1 : (rnd() % 2 ? 1 + (int)(rnd() % 30) : smalls[rnd() % ns]);
        a.batch = rnd() % 50 == 0 ? (int)(rnd() % 3) - 1 : smalls[rnd() % ns];
        a.classes = rnd() % 50 == 0 ? (int)(rnd() % 3) - 1 : smalls[rnd() % ns];
        walk(a, i);
    }
    // the 32-bit limits
    static const int big[] = {1, 2, 64, 202, 203, 4096, 0x10000, 0x3FFFFFF, 0x4000000, 0x3FFFFFFF, 0x40000000, 0x7FFFFFC0, 0x7FFFFFC1,
                              0x7FFFFFFE, 0x7FFFFFFF, 0, -1, INT32_MIN};
    const int nb = (int)(sizeof(big) / sizeof(big[0]));
    for (long i = 0; i < 60000; ++i, ++cases) {
        Args a = {};
        a.logits = 0x1000;
        a.p_mean = 0xA000;
        a.out = 0xB000;
        a.ups[rnd() % 7] = 0x2000;
        a.draws = rnd() % 2 ? smalls[rnd() % ns] : big[rnd() % nb];
        a.batch = rnd() % 4 ? big[rnd() % nb] : smalls[rnd() % ns];
        a.classes = rnd() % 2 ? big[rnd() % nb] : smalls[rnd() % ns];
        walk(a, i);
    }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld checksum %016llx\n", cases, counts[0], counts[1], counts[2], counts[3],
           (unsigned long long)sum);
    return 0;
}
