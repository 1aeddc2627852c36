// The scalar-prior entries of the fused reparameterisation + KL pass (bbb_reparam_kl_fwd / _bwd / _plan, bbb_reparam_partials,
// bbb_eps_dump) over the kernels of reparam_kl_kernels.cuh, TP = false.
#include "reparam_kl_kernels.cuh"

namespace {

__global__ __launch_bounds__(kThreads) void eps_dump_kernel(float* out, int64_t n, int64_t start, uint32_t k0, uint32_t k1,
                                                            uint32_t call, uint32_t stream_id) {
    const int64_t g0 = start >> 2;
    const int64_t g = g0 + (int64_t)blockIdx.x * kThreads + threadIdx.x;
    float z[4];
    bbb::normal4((uint64_t)g, stream_id, call, k0, k1, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = g * 4 + j - start;
        if (i >= 0 && i < n) out[i] = z[j];
    }
}

}  // namespace

// 256-thread blocks the current device keeps resident at once: 8 per CU (<= 64 VGPRs, 2 KB LDS; 32 waves per CU).
int bbb_reparam_resident_blocks() {
    static int cached[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 2048;
    if (cached[dev] == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        cached[dev] = cus * 8;
    }
    return cached[dev];
}

extern "C" int64_t bbb_reparam_partials(const bbb_segment_t* segs, int nseg) {
    if (segs == nullptr || nseg <= 0 || nseg > BBB_MAX_SEGMENTS) return BBB_EINVAL;
    int64_t chunks = 0;
    for (int s = 0; s < nseg; ++s) chunks += (segs[s].n + kChunk - 1) / kChunk;
    return chunks;
}

extern "C" int bbb_reparam_kl_fwd(const bbb_segment_t* segs, int nseg, int draws, float prior_mu, float prior_sigma,
                                  uint64_t seed, uint32_t call0, uint32_t flags, double* kl_partials, float* kl_out,
                                  double* kl_out64, const uint32_t* call_dev, void* stream) {
    return forward_launch<false>(segs, nullptr, nseg, draws, prior_mu, prior_sigma, seed, call0, flags, kl_partials, kl_out, kl_out64,
                                 call_dev, stream);
}

// What bbb_reparam_kl_fwd launches for these segments: the same plan, no launch.  Out-pointers may be NULL.
extern "C" int bbb_reparam_kl_plan(const bbb_segment_t* segs, int nseg, int draws, int slots, int32_t* kernel, int32_t* gpt,
                                   int32_t* nt, int32_t* chunks, int32_t* n_small, int32_t* small_chunk0, int32_t* tm_blocks,
                                   int32_t* grid) {
    reparam_plan::Plan p;
    int rc = reparam_plan::forward_shape(segs, nseg, draws, &p);
    if (rc != 0) return rc;
    rc = reparam_plan::forward_grid(&p, draws, slots > 0 ? slots : (p.kernel == 0 ? bbb_reparam_resident_blocks() : 0), true);
    if (rc != 0) return rc;
    if (kernel) *kernel = p.kernel;
    if (gpt) *gpt = p.gpt;
    if (nt) *nt = p.nt;
    if (chunks) *chunks = p.chunks;
    if (n_small) *n_small = p.n_small;
    if (small_chunk0) *small_chunk0 = p.small_chunk0;
    if (tm_blocks) *tm_blocks = p.tm_blocks;
    if (grid) *grid = p.grid;
    return 0;
}

extern "C" int bbb_reparam_kl_bwd(const bbb_segment_t* segs, int nseg, int draws, float prior_mu, float prior_sigma,
                                  uint64_t seed, uint32_t call0, uint32_t flags, const float* gkl,
                                  float* const* grad_mu, float* const* grad_rho, const uint32_t* call_dev, void* stream) {
    return backward_launch<false>(segs, nullptr, nseg, draws, prior_mu, prior_sigma, seed, call0, flags, gkl, grad_mu, grad_rho,
                                  call_dev, stream);
}

extern "C" int bbb_eps_dump(float* out, int64_t n, int64_t start, uint64_t seed, uint32_t call, uint32_t stream_id, void* stream) {
    if (out == nullptr || n <= 0 || start < 0) return BBB_EINVAL;
    const int64_t groups = ((start + n + 3) >> 2) - (start >> 2);
    const int blocks = (int)((groups + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(eps_dump_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, out, n, start,
                       (uint32_t)seed, (uint32_t)(seed >> 32), call, stream_id);
    return (int)hipGetLastError();
}
