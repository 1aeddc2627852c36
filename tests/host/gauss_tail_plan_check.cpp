// Host-only walk of the launch plan of the Gaussian-likelihood tail (csrc/gauss_tail_plan.h) for tests/test_gauss_tail_cpu.py, which
// builds this file with -fsanitize=address,undefined: a seeded sweep of ordinary arguments (both forms, missing and misaligned pointers,
// clamp edges in either order, noise_sigma of every kind, draws and channels around their limits), then arguments at the 32-bit limits.
// Checks the plan's own invariants and the order of its refusals against the rule written out here in 64-bit arithmetic, and prints the
// case counts per return code and a checksum of everything the plan returns.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/bbb_hip.h"
#include "../../pytorch-bayesiancnn_amd/csrc/gauss_tail_plan.h"

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
    int entry;                    // 0 forward, 1 backward, 2 moments
    uint64_t p[7];                // addresses are only looked at, never read
                                  // forward: logits, y, kl, beta_dev, ll_out, loss_out; backward: logits, y, g_loss, beta_dev, g_logits,
                                  // g_kl; moments: logits, y, mean, epistemic, aleatoric, total, log_density
    gauss_tail_plan::Shape s;
};

const void* at(uint64_t a) { return reinterpret_cast<const void*>(a); }

// The documented rule (include/bbb_hip.h), in 64-bit arithmetic.
int expected(const Args& a) {
    const gauss_tail_plan::Shape& s = a.s;
    uint64_t all = 0;
    bool missing;
    if (a.entry == 0) {
        missing = !a.p[0] || !a.p[1] || !a.p[2] || !a.p[4] || !a.p[5];
        for (int k = 0; k < 6; ++k) all |= a.p[k];
    } else if (a.entry == 1) {
        missing = !a.p[0] || !a.p[1] || !a.p[2] || !a.p[4];
        for (int k = 0; k < 6; ++k) all |= a.p[k];
    } else {
        uint64_t any = 0;
        for (int k = 2; k < 7; ++k) any |= a.p[k];
        missing = !a.p[0] || any == 0 || (a.p[6] && !a.p[1]);
        all = a.p[0] | a.p[1] | any;
    }
    if (missing) return BBB_EINVAL;
    if (s.draws <= 0 || s.batch <= 0 || s.channels <= 0 || s.dims <= 0) return BBB_EINVAL;
    const bool hetero = (int64_t)s.channels == 2 * (int64_t)s.dims;
    if (!hetero && s.channels != s.dims) return BBB_EINVAL;
    if (isnan(s.log_var_min) || isnan(s.log_var_max) || s.log_var_min > s.log_var_max) return BBB_EINVAL;
    if (!hetero && (isnan(s.noise_sigma) || isinf(s.noise_sigma) || s.noise_sigma <= 0.0)) return BBB_EINVAL;
    if (s.mc < 0 || s.mc > 1 || s.mean_over < 0) return BBB_EINVAL;
    if ((all & 3u) != 0) return BBB_EALIGN;
    if (s.draws > 512 || s.channels > 1024 || (int64_t)s.batch + 63 > INT32_MAX) return BBB_ESHAPE;
    return 0;
}

void walk(const Args& a, long i) {
    gauss_tail_plan::Plan p;
    int rc;
    if (a.entry == 0) {
        rc = gauss_tail_plan::plan_fwd(at(a.p[0]), at(a.p[1]), at(a.p[2]), at(a.p[3]), at(a.p[4]), at(a.p[5]), a.s, &p);
    } else if (a.entry == 1) {
        rc = gauss_tail_plan::plan_bwd(at(a.p[0]), at(a.p[1]), at(a.p[2]), at(a.p[3]), at(a.p[4]), at(a.p[5]), a.s, &p);
    } else {
        const void* outs[gauss_tail_plan::kMoments];
        for (int k = 0; k < gauss_tail_plan::kMoments; ++k) outs[k] = at(a.p[2 + k]);
        rc = gauss_tail_plan::plan_moments(at(a.p[0]), at(a.p[1]), outs, a.s, &p);
    }
    mix(rc);
    if (rc != expected(a)) fail("return code", i);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
    if (rc != 0) {
        if (p.threads != 0 || p.blocks != 0 || p.lds_bytes != 0 || p.hetero != 0) fail("a refused plan is not empty", i);
        return;
    }
    mix(p.threads); mix(p.blocks); mix(p.lds_bytes); mix(p.hetero);
    if (p.threads != 64) fail("threads", i);
    if (p.blocks < 1 || (int64_t)p.blocks * 64 < a.s.batch || ((int64_t)p.blocks - 1) * 64 >= a.s.batch) fail("blocks", i);
    if ((int64_t)p.blocks * 64 - 1 > INT32_MAX) fail("image index of the last lane", i);
    if (p.hetero != (a.s.channels == 2 * a.s.dims ? 1 : 0)) fail("form", i);
    // the kernel's last LDS index: image 63, dimension 15 of a tile, pitch 17
    if (p.lds_bytes != 64 * 17 * 4 || (63 * gauss_tail_plan::kPitch + gauss_tail_plan::kTile) * 4 > p.lds_bytes) fail("lds", i);
    // the last logit a launch reads, in elements: below 2^63 by far, and the kernels index with int64
    if ((int64_t)a.s.draws * a.s.channels > 512 * 1024) fail("slab count", i);
}

double sigma_of(uint32_t r) {
    static const double v[] = {0.1, 1.0, 30.0, 1e-300, 1e300, 0.0, -1.0, INFINITY, -INFINITY, NAN};
    return v[r % 16 < 10 ? r % 16 : r % 3];
}

float edge_of(uint32_t r) {
    static const float v[] = {-20.0f, 20.0f, 0.0f, -3.0f, 2.0f, NAN, INFINITY, -INFINITY};
    return v[r % 32 < 8 ? r % 32 : r % 5];
}

}  // namespace

int main() {
    long cases = 0;
    static const int smalls[] = {1, 2, 3, 7, 8, 10, 15, 16, 17, 32, 33, 34, 63, 64, 65, 130, 511, 512, 513, 1000, 1023, 1024, 1025, 2048};
    const int ns = (int)(sizeof(smalls) / sizeof(smalls[0]));
    for (long i = 0; i < 60000; ++i, ++cases) {
        Args a = {};
        a.entry = (int)(rnd() % 3);
        const int np = a.entry == 2 ? 7 : 6;
        const uint32_t drop = rnd() % 8 == 0 ? 1u << (rnd() % np) : 0;
        const uint32_t mask = a.entry == 2 ? (rnd() % 4 == 0 ? (3u | ((rnd() % 32) << 2)) : (3u | (1u << (2 + rnd() % 5)))) : 0x3Fu;
        for (int k = 0; k < np; ++k)
            if ((mask & ~drop) >> k & 1) a.p[k] = 0x1000 * (uint64_t)(k + 1) + (rnd() % 64 == 0 ? 1 + rnd() % 3 : 0);
        if (a.entry != 2 && rnd() % 2) a.p[3] = 0;                       // beta_dev is optional
        if (a.entry == 1 && rnd() % 4 == 0) a.p[5] = 0;                  // g_kl too
        a.s.draws = rnd() % 50 == 0 ? (int)(rnd() % 3) - 1 : smalls[rnd() % ns];
        a.s.batch = rnd() % 50 == 0 ? (int)(rnd() % 3) - 1 : smalls[rnd() % ns];
        a.s.dims = rnd() % 50 == 0 ? (int)(rnd() % 3) - 1 : smalls[rnd() % ns];
        const uint32_t form = rnd() % 16;
        a.s.channels = form == 0 ? smalls[rnd() % ns] : (form % 2 ? 2 * a.s.dims : a.s.dims);
        a.s.noise_sigma = sigma_of(rnd());
        a.s.log_var_min = rnd() % 8 ? -20.0f : edge_of(rnd());
        a.s.log_var_max = rnd() % 8 ? 20.0f : edge_of(rnd());
        a.s.mc = a.entry == 2 ? 0 : (rnd() % 16 == 0 ? (int)(rnd() % 5) - 2 : (int)(rnd() % 2));
        a.s.mean_over = a.entry == 2 ? 0 : (rnd() % 16 == 0 ? -(int)(rnd() % 3) : (int)(rnd() % 3) * 20);
        walk(a, i);
    }
    // the 32-bit limits
    static const int big[] = {1, 2, 64, 512, 513, 1024, 1025, 4096, 0x10000, 0x3FFFFFF, 0x3FFFFFFF, 0x40000000, 0x7FFFFFC0, 0x7FFFFFC1,
                              0x7FFFFFFE, 0x7FFFFFFF, 0, -1, INT32_MIN};
    const int nb = (int)(sizeof(big) / sizeof(big[0]));
    for (long i = 0; i < 60000; ++i, ++cases) {
        Args a = {};
        a.entry = (int)(rnd() % 3);
        for (int k = 0; k < (a.entry == 2 ? 7 : 6); ++k) a.p[k] = 0x1000 * (uint64_t)(k + 1);
        a.s.draws = rnd() % 2 ? smalls[rnd() % ns] : big[rnd() % nb];
        a.s.batch = rnd() % 4 ? big[rnd() % nb] : smalls[rnd() % ns];
        a.s.dims = rnd() % 2 ? big[rnd() % nb] : smalls[rnd() % ns];
        a.s.channels = rnd() % 8 == 0 ? big[rnd() % nb] : (rnd() % 2 ? (int)((uint32_t)a.s.dims * 2u) : a.s.dims);
        a.s.noise_sigma = 1.0;
        a.s.log_var_min = -20.0f;
        a.s.log_var_max = 20.0f;
        a.s.mc = a.entry == 2 ? 0 : (int)(rnd() % 2);
        a.s.mean_over = a.entry == 2 ? 0 : (rnd() % 2 ? big[rnd() % nb] : 0);
        walk(a, i);
    }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld checksum %016llx\n", cases, counts[0], counts[1], counts[2], counts[3],
           (unsigned long long)sum);
    return 0;
}
