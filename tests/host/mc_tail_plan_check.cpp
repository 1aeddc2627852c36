// Host-only walk of the batch-innermost Monte-Carlo tail's launch plan (csrc/mc_tail_plan.h) for tests/test_tail_sweep_cpu.py, which
// builds this file with -fsanitize=address,undefined: a seeded sweep of ordinary arguments (units, groups and shares of a group of
// steps), then arguments at the 32-bit limits (batch_slice x slices, units, grp x slices: every count inside the plan must be guarded,
// not overflow).  Checks the plan's own invariants, that it admits nothing the checks it replaced refused, and prints the case counts
// per return code and a checksum of everything it returns.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/bbb_hip.h"
#include "../../pytorch-bayesiancnn_amd/csrc/mc_tail_plan.h"

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
    uint64_t logits, lse, kl_in, kl_out, counter;     // addresses are only looked at, never read
    int units, slices, unit_off, batch_slice, classes, mean_over, grp, goff;
};

const void* at(uint64_t a) { return reinterpret_cast<const void*>(a); }

// The checks mc_tail_launch made inline before the plan existed, in 64-bit arithmetic: true = refused.
bool old_refuses(const Args& a) {
    if ((a.kl_out != 0 && a.kl_in == 0) || ((a.kl_in | a.kl_out | a.counter) & 3u) != 0) return true;
    if (a.logits == 0 || a.lse == 0 || a.units <= 0 || a.slices <= 0 || a.unit_off < 0 || a.batch_slice <= 0 || a.classes <= 0 ||
        a.mean_over < 0 || a.units > 4096 || a.grp < 0 || a.goff < 0 ||
        (a.grp > 0 && (a.goff >= a.grp || (int64_t)a.grp * a.slices < (int64_t)a.units + a.goff)))
        return true;
    if (((a.logits | a.lse) & 3u) != 0) return true;
    return (int64_t)a.batch_slice * a.slices > 0x7fffffffLL;
}

void walk(const Args& a, long i) {
    mc_tail_plan::Plan p;
    const int rc = mc_tail_plan::plan(at(a.logits), at(a.lse), at(a.kl_in), at(a.kl_out), at(a.counter), a.units, a.slices, a.unit_off,
                                      a.batch_slice, a.classes, a.mean_over, a.grp, a.goff, &p);
    mix(rc);
    if (rc != 0 && rc != BBB_EINVAL && rc != BBB_EALIGN && rc != BBB_ESHAPE) fail("return code", i);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
    if (rc != 0) {
        if (p.per_slice != 0 || p.ny != 0 || p.blocks != 0 || p.lds_bytes != 0 || p.keep_max != 0) fail("a refused plan is not empty", i);
        return;
    }
    mix(p.per_slice); mix(p.ny); mix(p.blocks); mix(p.lds_bytes); mix(p.keep_max);
    if (old_refuses(a)) fail("admits what the inline checks refused", i);
    const int64_t batch = (int64_t)a.batch_slice * a.slices;
    if (p.ny < 1 || p.ny > 16) fail("ny", i);
    if (p.ny != (p.per_slice > a.classes ? p.per_slice : a.classes) && p.ny != 16) fail("ny is min(max(per_slice, classes), 16)", i);
    if (p.blocks < 1 || (int64_t)p.blocks * 64 < batch || ((int64_t)p.blocks - 1) * 64 >= batch) fail("blocks", i);
    if ((int64_t)p.blocks * 64 - 1 > INT32_MAX) fail("image index of the last lane", i);
    if ((int64_t)a.units + a.slices - 1 > INT32_MAX) fail("units - e0 + slices - 1 of the kernel", i);
    if (p.per_slice < 1 || p.per_slice > 640) fail("per_slice", i);
    // the log sum-exps take per_slice * 256 bytes; up to 320 draws the row maxima take as much again
    if (p.keep_max != (p.per_slice <= 320 ? 1 : 0)) fail("keep_max", i);
    if (p.lds_bytes != p.per_slice * 256 * (p.keep_max ? 2 : 1) || p.lds_bytes > 160 * 1024) fail("lds", i);
    // every image's local draws fit the LDS rows: units u = off + e of slice s are e0, e0 + S, ... < units; a step holds grp slabs
    if (a.grp == 0 && ((int64_t)a.units + a.slices - 1) / a.slices != p.per_slice) fail("per_slice of units", i);
    if (a.grp > 0 && (p.per_slice != a.grp || (int64_t)a.slices * a.grp > INT32_MAX)) fail("per_slice of groups", i);
}

}  // namespace

int main() {
    long cases = 0;
    static const int smalls[] = {1, 2, 3, 7, 10, 16, 17, 63, 64, 65, 100, 130, 512, 640, 641, 1000, 1024, 4096, 4097};
    const int ns = (int)(sizeof(smalls) / sizeof(smalls[0]));
    // ordinary arguments: units, groups and shares
    for (long i = 0; i < 120000; ++i, ++cases) {
        Args a = {};
        a.logits = 0x1000 + (rnd() % 32 == 0 ? 1 + rnd() % 3 : 0);
        a.lse = rnd() % 64 == 0 ? 0 : 0x2000 + (rnd() % 32 == 0 ? 2 : 0);
        if (rnd() % 2) {
            a.kl_in = rnd() % 16 == 0 ? 0 : 0x3000 + (rnd() % 32 == 0 ? 1 : 0);
            a.kl_out = 0x4000 + (rnd() % 32 == 0 ? 2 : 0);
            a.counter = rnd() % 2 ? 0x5000 + (rnd() % 32 == 0 ? 3 : 0) : 0;
        }
        a.batch_slice = rnd() % 50 == 0 ? (int)(rnd() % 3) - 1 : smalls[rnd() % 13];
        a.classes = rnd() % 50 == 0 ? (int)(rnd() % 3) - 1 : smalls[rnd() % 17];
        a.mean_over = rnd() % 3 ? 0 : (int)(rnd() % 30) - 1;
        const int form = (int)(rnd() % 3);
        if (form == 0) {                 // work units
            a.units = rnd() % 3 ? 1 + (int)(rnd() % 80) : smalls[rnd() % ns];
            a.slices = rnd() % 40 == 0 ? (int)(rnd() % 3) - 1 : 1 + (int)(rnd() % 9);
            a.unit_off = (int)(rnd() % 12) - (rnd() % 40 == 0);
        } else if (form == 1) {          // whole steps
            a.slices = 1 + (int)(rnd() % 20);
            a.grp = rnd() % 4 ? 1 + (int)(rnd() % 30) : smalls[rnd() % ns];
            a.units = a.slices * a.grp > 5000 ? 5000 : a.slices * a.grp;
        } else {                         // a share of a group of steps, sometimes off the grid
            a.slices = 1 + (int)(rnd() % 6);
            a.grp = rnd() % 4 ? 1 + (int)(rnd() % 30) : smalls[rnd() % ns];
            a.goff = (int)(rnd() % (uint32_t)(a.grp + 1)) - (rnd() % 40 == 0);
            const int64_t room = (int64_t)a.slices * a.grp - a.goff;
            a.units = (int)(1 + rnd() % (uint32_t)(room > 0 ? (room > 4100 ? 4100 : room) : 1)) + (rnd() % 20 == 0 ? 3 : 0);
        }
        walk(a, i);
    }
    // the 32-bit limits: batch_slice x slices, units, grp x slices
    static const int big[] = {1, 2, 64, 640, 641, 4096, 4097, 0x8000, 0x10000, 0x333333, 0x3FFFFFF, 0x4000000, 0x3FFFFFFF, 0x40000000,
                              0x7FFFFFC0, 0x7FFFFFC1, 0x7FFFFFFE, 0x7FFFFFFF, 0, -1, INT32_MIN};
    const int nb = (int)(sizeof(big) / sizeof(big[0]));
    for (long i = 0; i < 120000; ++i, ++cases) {
        Args a = {};
        a.logits = 0x1000; a.lse = 0x2000;
        a.units = rnd() % 2 ? smalls[rnd() % ns] : big[rnd() % nb];
        a.slices = rnd() % 3 ? big[rnd() % nb] : smalls[rnd() % ns];
        a.batch_slice = rnd() % 3 ? big[rnd() % nb] : smalls[rnd() % ns];
        a.classes = rnd() % 4 ? smalls[rnd() % ns] : big[rnd() % nb];
        a.unit_off = rnd() % 4 ? 0 : big[rnd() % nb];
        a.mean_over = rnd() % 4 ? 0 : big[rnd() % nb];
        if (rnd() % 2) {
            a.grp = rnd() % 2 ? big[rnd() % nb] : smalls[rnd() % ns];
            a.goff = rnd() % 2 ? 0 : (rnd() % 2 ? big[rnd() % nb] : (a.grp > 0 ? (int)(rnd() % (uint32_t)a.grp) : 0));
        }
        walk(a, i);
    }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld checksum %016llx\n", cases, counts[0], counts[1], counts[2], counts[3],
           (unsigned long long)sum);
    return 0;
}
