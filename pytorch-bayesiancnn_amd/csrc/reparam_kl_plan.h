// Host-side launch plan of the fused reparameterisation + KL pass (csrc/reparam_kl.hip): the argument checks, the chunk walk,
// the choice between the fast and the generic kernel, groups per thread, store flavour, the tap-major blocks at the front of the
// grid and the one-block-per-draw split of the last chunks.  Plain C++17, no HIP headers: bbb_reparam_kl_fwd takes its launch
// shape from here, bbb_reparam_kl_plan reports it, and tests/host/reparam_plan_check.cpp walks it under the sanitizers.
#ifndef BBB_REPARAM_KL_PLAN_H
#define BBB_REPARAM_KL_PLAN_H

#include <stdint.h>

#include "../../include/bbb_hip.h"

namespace reparam_plan {

constexpr int kThreads = 256;
constexpr int kChunk = kThreads * 4;                         // elements per (block, group slot): 4 per thread
constexpr int64_t kBigTotal = (int64_t)kChunk * 16384;       // more elements than this: 4 groups per thread, streaming stores
constexpr int64_t kMaxN = (int64_t)INT32_MAX * kChunk;       // a longer tensor has more chunks than a grid has blocks

struct Plan {
    int32_t kernel;        // 0 = reparam_kl_fast_kernel, 1 = reparam_kl_fwd_kernel (external eps or bf16 rows)
    int32_t gpt;           // 16-byte groups per thread: 1 | 4
    int32_t nt;            // fast kernel: non-temporal stores of w
    int32_t chunks;        // publishers of a KL partial = blocks of a launch that is not split
    int32_t n_small;       // leading blocks that own ONE draw of one of the last chunks
    int32_t small_chunk0;  // first chunk handled by them
    int32_t tm_blocks;     // tap-major blocks at the front of the grid
    int32_t grid;          // blocks of the launch, the summing block included when the KL is wanted
    int32_t chunk_begin[BBB_MAX_SEGMENTS + 1];
    int32_t tm_begin[BBB_MAX_SEGMENTS + 1];
    int32_t tm_cg[BBB_MAX_SEGMENTS];
};

// The per-segment checks of both entries and the chunk walk: chunk_begin[0 .. BBB_MAX_SEGMENTS]; returns the chunk count or an error.
inline int segments(const bbb_segment_t* segs, int nseg, int draws, bool bwd, int gpt, int32_t* chunk_begin) {
    if (segs == nullptr || nseg <= 0 || nseg > BBB_MAX_SEGMENTS || draws <= 0) return BBB_EINVAL;
    int64_t chunks = 0;
    const int64_t per = (int64_t)kChunk * gpt;
    for (int s = 0; s < nseg; ++s) {
        const bbb_segment_t& g = segs[s];
        if (g.mu == nullptr || g.rho == nullptr || g.n <= 0) return BBB_EINVAL;
        if (g.draw_stride < g.n && draws > 1 && (g.w || g.eps)) return BBB_EINVAL;
        if ((((uintptr_t)g.mu | (uintptr_t)g.rho | (g.w_row_len ? 0 : (uintptr_t)g.w) | (uintptr_t)g.sigma | (uintptr_t)g.eps) & 3u) != 0)
            return BBB_EALIGN;
        if (g.w_row_len != 0 && (bwd || g.w == nullptr || g.n % g.w_row_len != 0 || ((uintptr_t)g.w & 1u))) return BBB_EINVAL;
        if (g.w_tm_cin != 0) {      // fp32 tap-major output: dense Philox-sampled fp32 segment, [rows][C][T] with C % 8 == 0, 16-byte aligned
            if (bwd || g.w_row_len != 0 || g.w_taps < 2 || g.w_taps > 128 || g.w_tm_cin % 8 != 0 || g.w == nullptr || g.eps != nullptr ||
                g.n % ((int64_t)g.w_tm_cin * g.w_taps) != 0)
                return BBB_EINVAL;
            if ((((uintptr_t)g.mu | (uintptr_t)g.rho | (uintptr_t)g.w) & 15u) != 0 || (g.draw_stride & 3) != 0) return BBB_EALIGN;
        } else if (g.w_taps > 1 && (g.w_row_len == 0 || g.w_row_len % g.w_taps != 0)) return BBB_EINVAL;
        if (g.n > kMaxN) return BBB_ESHAPE;
        chunk_begin[s] = (int32_t)chunks;
        chunks += (g.n + per - 1) / per;
        if (chunks > INT32_MAX) return BBB_ESHAPE;
    }
    for (int s = nseg; s <= BBB_MAX_SEGMENTS; ++s) chunk_begin[s] = (int32_t)chunks;
    return (int)chunks;
}

// Tensor priors (bbb_reparam_kl_tp_*): pri[s].mu0 / .sigma0 are [segs[s].n] fp32 or NULL (= the launch-wide scalar).  Returns how many
// pointers are set -- 0, also for pri == NULL, means the scalar kernels run -- or an error.  The prior never enters the plan.
inline int priors(const bbb_segment_t* segs, const bbb_prior_segment_t* pri, int nseg) {
    if (segs == nullptr || nseg <= 0 || nseg > BBB_MAX_SEGMENTS) return BBB_EINVAL;
    if (pri == nullptr) return 0;
    int set = 0;
    for (int s = 0; s < nseg; ++s) {
        if ((((uintptr_t)pri[s].mu0 | (uintptr_t)pri[s].sigma0) & 3u) != 0) return BBB_EALIGN;
        set += (pri[s].mu0 != nullptr) + (pri[s].sigma0 != nullptr);
    }
    return set;
}

// Everything of the forward's plan that does not depend on the device: kernel, gpt, chunks, the tap-major blocks.
inline int forward_shape(const bbb_segment_t* segs, int nseg, int draws, Plan* p) {
    *p = Plan{};
    int64_t total = 0;
    if (segs != nullptr && nseg > 0 && nseg <= BBB_MAX_SEGMENTS)
        for (int s = 0; s < nseg; ++s) {
            if (segs[s].n <= 0 || segs[s].n > kMaxN) { total = 0; break; }     // refused below, whatever gpt is
            total += segs[s].n;
        }
    const bool big = total > kBigTotal;                         // > 16M elements: longer blocks, streaming stores
    p->gpt = big ? 4 : 1;
    const int chunks = segments(segs, nseg, draws, false, p->gpt, p->chunk_begin);
    if (chunks < 0) return chunks;
    p->chunks = chunks;
    // The fast kernel applies when every segment is a dense fp32, Philox-sampled tensor (alignment is handled per segment).
    bool fast = true;
    for (int s = 0; s < nseg; ++s)
        if (segs[s].eps != nullptr || segs[s].w_row_len != 0) fast = false;
#ifdef BBB_FORCE_GENERIC_REPARAM     // timing experiments: the general kernel on inputs the fast one would take
    fast = false;
#endif
    p->kernel = fast ? 0 : 1;
    if (fast) {
        // tap-major segments: their draws come from extra blocks at the front of the grid (tm_block)
        int64_t tmb = 0;
        for (int s = 0; s < nseg; ++s) {
            p->tm_begin[s] = (int32_t)tmb;
            p->tm_cg[s] = 0;
            if (segs[s].w_tm_cin != 0) {
                const int64_t rc_total = segs[s].n / segs[s].w_taps;
                int64_t cg = (kChunk / (int)segs[s].w_taps) & ~7;
                if (cg > rc_total) cg = rc_total;
                p->tm_cg[s] = (int)cg;
                const int64_t nb = (rc_total + cg - 1) / cg;
                if (tmb + nb > 0x3fffffffLL) return BBB_ESHAPE;
                tmb += nb;
            }
        }
        for (int s = nseg; s <= BBB_MAX_SEGMENTS; ++s) p->tm_begin[s] = (int32_t)tmb;
        p->tm_blocks = (int32_t)tmb;
    } else {
        for (int s = 0; s < nseg; ++s)
            if (segs[s].w_tm_cin != 0) return BBB_EINVAL;                 // tap-major outputs: Philox-sampled dense launches only
    }
    return 0;
}

// The rest: `slots` = 256-thread blocks the device keeps resident at once.
// A launch a little larger than one round of resident blocks (the model-sized case: 2137 chunks on 2048 slots) would
// run its excess blocks alone at the end, one wave per SIMD, for a whole 10-draw block time.  Instead the LAST
// `excess` chunks are cut into one block per draw and put FIRST in the grid: they finish early, the whole-chunk
// blocks behind them fill the freed slots, and the launch ends with every SIMD still sharing work.  (The block of
// draw 0 owns the chunk's KL partial and sigma output; partial indices = chunk indices, so the KL sum is unchanged.)
inline int forward_grid(Plan* p, int draws, int slots, bool want_kl) {
    const int chunks = p->chunks;
    int excess = 0;
    if (p->kernel == 0 && p->gpt == 1 && draws > 1 && slots > 0 && chunks > slots && chunks <= 3 * (int64_t)slots && p->tm_blocks == 0)
        excess = chunks % slots;
    const int64_t n_small = (int64_t)excess * draws;
    const int64_t grid = (int64_t)p->tm_blocks + n_small + (chunks - excess) + (want_kl ? 1 : 0);
    if (n_small > INT32_MAX || grid > INT32_MAX) return BBB_ESHAPE;
    p->n_small = (int32_t)n_small;
    p->small_chunk0 = chunks - excess;
    p->grid = (int32_t)grid;
    // Store flavour of w (measured, AlexNet's 12 tensors, us per launch, plain / non-temporal): E=4 14.6 / 12.2, E=10
    // 21.7 / 19.2, E=25 40.0 / 42.5 -- with plain stores the launch ends with up to 32 MB of dirty L2 lines to write back
    // at the kernel boundary; streaming them out as they are produced wins until the launch is long enough to hide that.
    p->nt = (p->kernel == 0 && (p->gpt == 4 || draws <= 16)) ? 1 : 0;
    return 0;
}

inline int forward(const bbb_segment_t* segs, int nseg, int draws, int slots, bool want_kl, Plan* p) {
    const int rc = forward_shape(segs, nseg, draws, p);
    return rc != 0 ? rc : forward_grid(p, draws, slots, want_kl);
}

}  // namespace reparam_plan

#endif
