// Global L2 norm of up to 16 gradient tensors per launch, for FusedAdam's clipping and its non-finite guard (training extension):
//     norm = fp32( sqrt( sum_i double(g_i)^2 ) ),   coef = fp32( min(1, max_norm / (double(norm) + 1e-6)) )
// Every square and every partial sum is float64, so the norm has no range of its own: gradients of 1e30 or of 1e-30 give their norm,
// where an fp32 accumulation gives inf or 0.  Two kinds of launch, and the reduction across workgroups happens at the launch boundary
// between them -- no ticket, no counter, no spin, no float atomic, nothing that can wait on another workgroup:
//   grad_sumsq_kernel     one block per 4096-element chunk of one segment -> ONE float64 at partials[first + chunk];
//   grad_norm_finish_kernel   one block sums the partials in index order and writes norm, coef, ok and the skipped-step counter.
// Every sum is a FIXED tree: thread t of a chunk always owns elements {1024 q + 4 t + j : q, j = 0..3} and adds them in that order,
// lanes fold by halves, the four waves add as (0 + 1) + (2 + 3).  The 16-byte and the scalar load paths differ in the loads only, so a
// partial does not depend on alignment, and the norm depends on the ORDER of the tensors only, not on how they are dealt to launches.
// HBM traffic: 4 B read per element.  The checks and the chunk walk live in csrc/grad_norm_plan.h (host only).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "grad_norm_plan.h"

namespace {

constexpr int kThreads = grad_norm_plan::kThreads;
constexpr int kChunk = grad_norm_plan::kChunk;
constexpr int kWaves = kThreads / 64;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct SumsqArgs {
    const float* grad[BBB_MAX_SEGMENTS];
    int64_t n[BBB_MAX_SEGMENTS];
    int32_t chunk_begin[BBB_MAX_SEGMENTS + 1];
    int32_t nseg;
    double* partials;          // already offset by `first`
};

// The block's sum in thread 0 (other threads: unspecified).  Lanes fold by halves (32, 16, .. 1), then (w0 + w1) + (w2 + w3).
__device__ inline double block_sum(double acc, double* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const SumsqArgs a) {
    __shared__ double lds[kWaves];
    const int chunk = blockIdx.x;
    int s = 0;
    while (s + 1 < a.nseg && chunk >= a.chunk_begin[s + 1]) ++s;
    const float* g = a.grad[s];
    const int64_t n = a.n[s];
    const int64_t base = (int64_t)(chunk - a.chunk_begin[s]) * kChunk + (int64_t)threadIdx.x * 4;
    const bool aligned = ((uintptr_t)g & 15u) == 0;
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i0 = base + (int64_t)q * (kThreads * 4);
        float x[4];
        if (aligned && i0 + 4 <= n) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(g + i0);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = g4[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = i0 + j < n ? g[i0 + j] : 0.0f;      // behind n: + 0.0, which changes no sum of squares
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)x[j] * (double)x[j];             // (the product of two floats is exact in double)
    }
    const double sum = block_sum(acc, lds);
    if (threadIdx.x == 0) a.partials[chunk] = sum;
}

__global__ __launch_bounds__(kThreads) void grad_norm_finish_kernel(const double* partials, int npartials, double max_norm, int skip,
                                                                    float* norm_out, float* coef_out, float* ok_out, int32_t* skipped_out) {
    __shared__ double lds[kWaves];
    double acc = 0.0;
    for (int i = threadIdx.x; i < npartials; i += kThreads) acc += partials[i];
    const double sum = block_sum(acc, lds);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(sum);             // NaN if any partial is NaN, else +Inf if any is Inf
    const bool finite = norm - norm == 0.0f;
    *norm_out = norm;
    if (coef_out != nullptr) *coef_out = grad_norm_plan::coefficient(norm, max_norm);
    if (ok_out != nullptr) *ok_out = (skip != 0 && !finite) ? 0.0f : 1.0f;
    if (skipped_out != nullptr && skip != 0 && !finite) *skipped_out = *skipped_out + 1;
}

}  // namespace

extern "C" int bbb_grad_sumsq(const bbb_adam_segment_t* segs, int nseg, double* partials, int64_t first, void* stream) {
    grad_norm_plan::Plan p;
    const int rc = grad_norm_plan::plan(segs, nseg, partials, first, &p);
    if (rc != 0) return rc;
    SumsqArgs a = {};
    for (int s = 0; s < nseg; ++s) { a.grad[s] = segs[s].grad; a.n[s] = segs[s].n; }
    for (int s = 0; s <= BBB_MAX_SEGMENTS; ++s) a.chunk_begin[s] = p.chunk_begin[s];
    a.nseg = nseg;
    a.partials = partials + first;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(p.chunks), dim3(kThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// What bbb_grad_sumsq launches for these arguments: the same plan, no launch, no device.  Out-pointers may be NULL; a refusal writes zeros.
extern "C" int bbb_grad_sumsq_plan(const bbb_adam_segment_t* segs, int nseg, const double* partials, int64_t first, int32_t* chunks,
                                   int32_t* chunk_begin, int32_t* vec) {
    grad_norm_plan::Plan p;
    const int rc = grad_norm_plan::plan(segs, nseg, partials, first, &p);
    if (chunks) *chunks = p.chunks;
    if (chunk_begin) for (int s = 0; s <= BBB_MAX_SEGMENTS; ++s) chunk_begin[s] = p.chunk_begin[s];
    if (vec) for (int s = 0; s < BBB_MAX_SEGMENTS; ++s) vec[s] = p.vec[s];
    return rc;
}

extern "C" int bbb_grad_norm_finish(const double* partials, int64_t npartials, double max_norm, int skip, float* norm_out, float* coef_out,
                                    float* ok_out, int32_t* skipped_out, void* stream) {
    const int rc = grad_norm_plan::finish_check(partials, npartials, max_norm, norm_out, coef_out, ok_out, skipped_out);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, partials, (int)npartials, max_norm, skip,
                       norm_out, coef_out, ok_out, skipped_out);
    return (int)hipGetLastError();
}

// The finish launch's checks and, for a given fp32 norm, the coefficient it would write (host only; *coef may be NULL).
extern "C" int bbb_grad_norm_finish_plan(const double* partials, int64_t npartials, double max_norm, const float* norm_out,
                                         const float* coef_out, const float* ok_out, const int32_t* skipped_out, float norm, float* coef) {
    const int rc = grad_norm_plan::finish_check(partials, npartials, max_norm, norm_out, coef_out, ok_out, skipped_out);
    if (coef) *coef = rc == 0 ? grad_norm_plan::coefficient(norm, max_norm) : 0.0f;
    return rc;
}
