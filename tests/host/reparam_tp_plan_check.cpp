// Host-only walk of the tensor-prior checks of the parameter pass (reparam_plan::priors in csrc/reparam_kl_plan.h) for
// tests/test_prior_cpu.py, which builds this file with -fsanitize=address,undefined: seeded PriorSegment arrays of exactly nseg
// entries (heap-allocated at that size, so a read past nseg is an error of the address sanitizer) for nseg from 1 to
// BBB_MAX_SEGMENTS and beyond both limits, pointers NULL / aligned / misaligned, pri == NULL.  Checks the returned count or code
// against a restatement of the rule.  (That the plan does not depend on the priors holds by signature: reparam_plan::forward never
// takes them.)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/bbb_hip.h"
#include "../../pytorch-bayesiancnn_amd/csrc/reparam_kl_plan.h"

namespace {

uint64_t state = 0x9E3779B97F4A7C15ull, sum = 0xcbf29ce484222325ull;
uint32_t rnd() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}
void mix(int64_t v) { sum = (sum ^ (uint64_t)v) * 0x100000001b3ull; }

void fail(const char* what, long i) {
    printf("invariant broken: %s (case %ld)\n", what, i);
    exit(1);
}

const float* at(uint64_t a) { return reinterpret_cast<const float*>(a); }     // addresses are only looked at, never read

}  // namespace

int main() {
    long cases = 0, counts[4] = {0, 0, 0, 0};    // scalar (0 pointers) / tensor (> 0) / EINVAL / EALIGN
    for (long i = 0; i < 200000; ++i) {
        const int pick = (int)(rnd() % 40);
        const int nseg = pick == 0 ? 0 : pick == 1 ? -1 : pick == 2 ? BBB_MAX_SEGMENTS + 1 : pick == 3 ? INT32_MAX : 1 + (int)(rnd() % BBB_MAX_SEGMENTS);
        const int alloc = nseg >= 1 && nseg <= BBB_MAX_SEGMENTS ? nseg : 1;
        bbb_segment_t* segs = (bbb_segment_t*)calloc((size_t)alloc, sizeof(bbb_segment_t));
        bbb_prior_segment_t* pri = (rnd() % 8 == 0) ? nullptr : (bbb_prior_segment_t*)calloc((size_t)alloc, sizeof(bbb_prior_segment_t));
        int want = 0;
        bool misaligned = false;
        for (int s = 0; s < alloc; ++s) {
            segs[s].mu = at(0x1000 + 64 * s);
            segs[s].rho = at(0x2000 + 64 * s);
            segs[s].n = 1 + rnd() % 5000;
            segs[s].draw_stride = segs[s].n;
            if (pri == nullptr) continue;
            for (int q = 0; q < 2; ++q) {
                const uint32_t kind = rnd() % 16;         // NULL, 16-byte aligned, 4-byte aligned, misaligned by 1..3 bytes
                uint64_t a = kind < 5 ? 0 : 0x100000 + 4096 * (uint64_t)(2 * s + q) + (kind < 10 ? 0 : kind < 15 ? 4 * (1 + rnd() % 3) : 1 + rnd() % 3);
                if (q == 0) pri[s].mu0 = at(a);
                else pri[s].sigma0 = at(a);
                want += a != 0;
                misaligned |= (a & 3) != 0;
            }
        }
        const bool bad_n = nseg <= 0 || nseg > BBB_MAX_SEGMENTS;
        const int rc = reparam_plan::priors(rnd() % 64 == 0 ? nullptr : segs, pri, nseg);
        // (segs == NULL is EINVAL too; re-ask with segs to compare the rest)
        const int rc2 = reparam_plan::priors(segs, pri, nseg);
        mix(rc); mix(rc2);
        const int expect = bad_n ? BBB_EINVAL : pri == nullptr ? 0 : misaligned ? BBB_EALIGN : want;
        if (rc2 != expect) fail("priors() differs from the rule", i);
        if (rc != rc2 && rc != BBB_EINVAL) fail("segs == NULL", i);
        counts[rc2 == BBB_EINVAL ? 2 : rc2 == BBB_EALIGN ? 3 : rc2 == 0 ? 0 : 1] += 1;
        free(segs);
        free(pri);
        ++cases;
    }
    printf("cases %ld scalar %ld tensor %ld einval %ld ealign %ld checksum %016llx\n", cases, counts[0], counts[1], counts[2], counts[3],
           (unsigned long long)sum);
    return 0;
}
