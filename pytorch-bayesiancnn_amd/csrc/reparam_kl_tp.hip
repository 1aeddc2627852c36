// Per-weight Gaussian priors for the fused reparameterisation + KL pass: bbb_reparam_kl_tp_fwd / _tp_bwd / _tp_plan (include/bbb_hip.h)
// over the TP = true instantiations of the kernels of reparam_kl_kernels.cuh.  A translation unit of its own: in one unit the compiler
// schedules reparam_kl_fast_kernel<1, false> differently once its tensor-prior sibling is instantiated next to it.
#include "reparam_kl_kernels.cuh"

// The checks of the scalar entry's segments first, then those of the prior pointers; with no pointer set (or no KL wanted: nothing
// else reads a prior) the launch is the scalar entry's own.
extern "C" int bbb_reparam_kl_tp_fwd(const bbb_segment_t* segs, const bbb_prior_segment_t* pri, int nseg, int draws, float prior_mu,
                                     float prior_sigma, uint64_t seed, uint32_t call0, uint32_t flags, double* kl_partials,
                                     float* kl_out, double* kl_out64, const uint32_t* call_dev, void* stream) {
    reparam_plan::Plan p;
    const int rc = reparam_plan::forward_shape(segs, nseg, draws, &p);
    if (rc != 0) return rc;
    const int tp = reparam_plan::priors(segs, pri, nseg);
    if (tp < 0) return tp;
    if (tp == 0 || (kl_out == nullptr && kl_out64 == nullptr))
        return bbb_reparam_kl_fwd(segs, nseg, draws, prior_mu, prior_sigma, seed, call0, flags, kl_partials, kl_out, kl_out64, call_dev,
                                  stream);
    return forward_launch<true>(segs, pri, nseg, draws, prior_mu, prior_sigma, seed, call0, flags, kl_partials, kl_out, kl_out64,
                                call_dev, stream);
}

// The prior never enters the plan: the same eight fields, after the same checks plus those of the prior pointers.
extern "C" int bbb_reparam_kl_tp_plan(const bbb_segment_t* segs, const bbb_prior_segment_t* pri, int nseg, int draws, int slots,
                                      int32_t* kernel, int32_t* gpt, int32_t* nt, int32_t* chunks, int32_t* n_small,
                                      int32_t* small_chunk0, int32_t* tm_blocks, int32_t* grid) {
    reparam_plan::Plan p;
    const int rc = reparam_plan::forward_shape(segs, nseg, draws, &p);
    if (rc != 0) return rc;
    const int tp = reparam_plan::priors(segs, pri, nseg);
    if (tp < 0) return tp;
    return bbb_reparam_kl_plan(segs, nseg, draws, slots, kernel, gpt, nt, chunks, n_small, small_chunk0, tm_blocks, grid);
}

extern "C" int bbb_reparam_kl_tp_bwd(const bbb_segment_t* segs, const bbb_prior_segment_t* pri, int nseg, int draws, float prior_mu,
                                     float prior_sigma, uint64_t seed, uint32_t call0, uint32_t flags, const float* gkl,
                                     float* const* grad_mu, float* const* grad_rho, const uint32_t* call_dev, void* stream) {
    int32_t chunk_begin[BBB_MAX_SEGMENTS + 1];
    const int chunks = reparam_plan::segments(segs, nseg, draws, true, 1, chunk_begin);
    if (chunks < 0) return chunks;
    const int tp = reparam_plan::priors(segs, pri, nseg);
    if (tp < 0) return tp;
    if (tp == 0)
        return bbb_reparam_kl_bwd(segs, nseg, draws, prior_mu, prior_sigma, seed, call0, flags, gkl, grad_mu, grad_rho, call_dev, stream);
    return backward_launch<true>(segs, pri, nseg, draws, prior_mu, prior_sigma, seed, call0, flags, gkl, grad_mu, grad_rho, call_dev,
                                 stream);
}
