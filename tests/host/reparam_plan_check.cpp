// Host-only walk of the parameter pass's launch plan (csrc/reparam_kl_plan.h) for tests/test_reparam_sweep_cpu.py, which builds
// this file with -fsanitize=address,undefined: the forward plan and the backward's segment walk over a seeded sweep of ordinary
// segment lists and over descriptors whose sizes, draws and slots sit near the 32- and 64-bit limits (every count inside the plan
// must be guarded, not overflow).  Checks the plan's own invariants and prints a checksum of everything it returns.
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

long counts[4];   // ok / EINVAL / EALIGN / ESHAPE over all plan calls

void tally(int rc) {
    mix(rc);
    counts[rc == 0 ? 0 : rc == BBB_EINVAL ? 1 : rc == BBB_EALIGN ? 2 : 3] += 1;
}

void fail(const char* what, long i) {
    printf("invariant broken: %s (case %ld)\n", what, i);
    exit(1);
}

void walk(const bbb_segment_t* segs, int nseg, int draws, int slots, long i) {
    reparam_plan::Plan p;
    const int rc = reparam_plan::forward(segs, nseg, draws, slots, (i & 1) != 0, &p);
    tally(rc);
    if (rc == 0) {
        mix(p.kernel); mix(p.gpt); mix(p.nt); mix(p.chunks); mix(p.n_small); mix(p.small_chunk0); mix(p.tm_blocks); mix(p.grid);
        for (int s = 0; s <= BBB_MAX_SEGMENTS; ++s) { mix(p.chunk_begin[s]); mix(p.tm_begin[s]); }
        for (int s = 0; s < BBB_MAX_SEGMENTS; ++s) mix(p.tm_cg[s]);
        if (p.chunks <= 0 || p.chunk_begin[0] != 0 || p.chunk_begin[BBB_MAX_SEGMENTS] != p.chunks) fail("chunk walk", i);
        if (p.n_small < 0 || p.small_chunk0 < 0 || p.small_chunk0 > p.chunks || p.n_small != (int64_t)(p.chunks - p.small_chunk0) * draws)
            fail("per-draw split", i);
        if (p.grid != (int64_t)p.tm_blocks + p.n_small + p.small_chunk0 + (i & 1)) fail("grid", i);
        if (p.n_small != 0 && (p.kernel != 0 || p.gpt != 1 || p.tm_blocks != 0 || draws < 2)) fail("split outside its rule", i);
        if (p.kernel == 1 && (p.tm_blocks != 0 || p.nt != 0)) fail("generic kernel with fast-kernel fields", i);
        for (int s = 0; s < nseg; ++s)
            if (segs[s].w_tm_cin != 0 && (p.tm_cg[s] <= 0 || p.tm_cg[s] * (int64_t)segs[s].w_taps > reparam_plan::kChunk)) fail("tm_cg", i);
    }
    int32_t cb[BBB_MAX_SEGMENTS + 1];
    const int rb = reparam_plan::segments(segs, nseg, draws, true, 1, cb);
    tally(rb < 0 ? rb : 0);
    if (rb >= 0) mix(rb);
}

float* at(uint64_t a) { return reinterpret_cast<float*>(a); }     // addresses are only looked at, never read

}  // namespace

int main() {
    long cases = 0;
    static const int64_t sizes[] = {1, 3, 4, 5, 10, 1023, 1024, 1025, 2049, 4099, 34848, 1 << 20, (1 << 24) + 4099};
    static const uint32_t taps[] = {0, 1, 2, 9, 25, 121, 128, 129}, cins[] = {8, 16, 40, 64, 12};
    static const int drawset[] = {1, 2, 3, 10, 16, 17, 25};
    for (long i = 0; i < 60000; ++i, ++cases) {
        bbb_segment_t segs[BBB_MAX_SEGMENTS + 1] = {};
        const int nseg = i % 50 == 0 ? (int)(rnd() % 19) - 1 : 1 + (int)(rnd() % BBB_MAX_SEGMENTS);
        const int kind = (int)(rnd() % 4);            // 0, 1: dense fp32; 2: some external eps; 3: some bf16 rows
        for (int s = 0; s < nseg && s <= BBB_MAX_SEGMENTS; ++s) {
            bbb_segment_t& g = segs[s];
            const uint64_t mis = rnd() % 16 == 0 ? 4 * (rnd() % 4) + (rnd() % 64 == 0) : 0;
            g.mu = at(0x1000 + mis); g.rho = at(0x2000); g.w = rnd() % 8 ? at(0x3000 + (rnd() % 16 == 0 ? 4 : 0)) : nullptr;
            g.sigma = rnd() % 2 ? at(0x4000) : nullptr;
            g.n = rnd() % 3 ? sizes[rnd() % 13] : 1 + (int64_t)(rnd() % 3000000);
            g.draw_stride = g.n + (rnd() % 4 == 0 ? (int64_t)(rnd() % 9) - 1 : 0);
            g.stream_id = rnd();
            if (kind == 2 && rnd() % 2) g.eps = at(0x5000);
            if (kind == 3 && rnd() % 2) {
                g.w_row_len = rnd() % 2 ? 1 + rnd() % 1100 : 72;
                if (rnd() % 2) g.n = (int64_t)g.w_row_len * (1 + rnd() % 12);
                g.w_taps = rnd() % 3 == 0 ? taps[rnd() % 8] : 0;
            } else if (rnd() % 6 == 0) {
                g.w_tm_cin = cins[rnd() % 5];
                g.w_taps = taps[rnd() % 8];
                if (rnd() % 8) g.n = (int64_t)g.w_tm_cin * (g.w_taps ? g.w_taps : 1) * (1 + rnd() % 70);
                g.draw_stride = g.n + 4 * (rnd() % 3);
            }
        }
        const int slots = rnd() % 2 ? 2048 : 8 * (1 + (int)(rnd() % 400));
        walk(nseg < 0 ? nullptr : segs, nseg, rnd() % 100 == 0 ? (int)(rnd() % 3) - 1 : drawset[rnd() % 7], slots, i);
    }
    // launches next to the per-draw split's rule, in both directions
    for (long i = 0; i < 20000; ++i, ++cases) {
        bbb_segment_t segs[3] = {};
        const int slots = 8 * (1 + (int)(rnd() % 320));
        const int64_t chunks = (int64_t)slots * (1 + rnd() % 3) + (int64_t)(rnd() % 5) - 2 + (rnd() % 2 ? rnd() % (uint32_t)slots : 0);
        int64_t left = chunks * 1024 - (int64_t)(rnd() % 1024);
        for (int s = 0; s < 3; ++s) {
            segs[s].mu = at(0x1000); segs[s].rho = at(0x2000); segs[s].w = at(0x3000);
            segs[s].n = s == 2 ? left : 1 + (int64_t)(rnd() % (uint32_t)(left / 2 > 0 ? left / 2 : 1));
            if (segs[s].n > left - (2 - s)) segs[s].n = left - (2 - s);
            segs[s].draw_stride = segs[s].n;
            left -= segs[s].n;
        }
        walk(segs, 3, drawset[rnd() % 7], slots, i);
    }
    // the extremes: sizes, draws and slots from {small, near 2^31, near 2^41, near 2^63}
    static const int64_t big[] = {1, 1024, (int64_t)1 << 24, ((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 41) - 1025,
                                  ((int64_t)1 << 41) - 1024, (int64_t)1 << 41, INT64_MAX - 1023, INT64_MAX, -1, 0};
    static const int ints[] = {1, 2, 17, 2048, 1 << 20, 0x3FFFFFFF, 0x40000000, 0x7FFFFFFF, 0, -1};
    for (long i = 0; i < 40000; ++i, ++cases) {
        bbb_segment_t segs[BBB_MAX_SEGMENTS] = {};
        const int nseg = 1 + (int)(rnd() % BBB_MAX_SEGMENTS);
        for (int s = 0; s < nseg; ++s) {
            bbb_segment_t& g = segs[s];
            g.mu = at(0x1000); g.rho = at(0x2000); g.w = at(0x3000);
            g.n = rnd() % 3 ? big[rnd() % 3] : big[rnd() % 12];
            g.draw_stride = rnd() % 2 ? g.n : big[rnd() % 12];
            if (rnd() % 8 == 0) { g.w_tm_cin = 8u << (rnd() % 28); g.w_taps = taps[rnd() % 8]; }
            else if (rnd() % 8 == 0) { g.w_row_len = rnd() % 2 ? 0xFFFFFFFFu : 1u << (rnd() % 32); g.w_taps = rnd() % 2 ? 0xFFFFFFFFu : taps[rnd() % 8]; }
        }
        walk(segs, nseg, ints[rnd() % 10], ints[rnd() % 10], i);
    }
    printf("cases %ld ok %ld einval %ld ealign %ld eshape %ld checksum %016llx\n", cases, counts[0], counts[1], counts[2], counts[3],
           (unsigned long long)sum);
    return 0;
}
