// Uncertainty scores of T Monte-Carlo forwards on batch-innermost logits, [T][C][B], in one launch on gfx950: the mean logit, the mean
// probability, the epistemic / aleatoric split of bbb_uncertainty, and the three entropy scores (predictive entropy, expected entropy,
// mutual information).  No transpose, no atomics; a result never depends on which workgroup ran first.
//
// blockDim = (64 images, ny <= 16), lanes = consecutive images so every read is coalesced (as mc_tail_cb_kernel).
//   Phase 1, rows over draws: per (draw, image) the row's maximum, its log partition logf(sum exp(v - mx)) and the entropy H[p_t] go
//   into LDS (normalized: the softplus sum, its logarithm, H[p_t]).  ONE thread adds the C terms of a row: compensated sums.
//   Phase 2, rows over classes: per (image, class) a first sweep over the draws for sum v, sum p, sum p^2, then -- p_bar known -- a
//   second sweep for sum (p - p_bar)^2 and the KL sum p (log p - log p_bar).  A thread's shares of sum_c p_bar log p_bar and of the KL
//   sum (compensated over its classes) go into LDS; row 0 adds the rows in ascending order and writes the three per-image scores.
// log p_t = (v - mx) - log partition, the max-first order of the tail kernels (mc_tail.hip), and p_t = expf(log p_t); normalized:
// p_t = q / z, log p_t = logf(q) - logf(z) with q = softplus(v).  A term with p = 0 contributes exactly 0 (0 * -inf never forms);
// the tests `p == 0.0f` are false for NaN, so a NaN stays a NaN.
// The backward (mc_uncertainty_cb_bwd_kernel, further down) is one launch too: one thread per (draw, image), no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "mc_uncertainty_plan.h"
#include "smem_attr.h"

namespace {

using mc_uncertainty_plan::kThreads;
using mc_uncertainty_plan::kRows;

struct UncOut {
    float *pred, *p_mean, *epi, *ale, *ent, *exp_ent, *mi;
};

// Compensated running sum (as row_log_sum_exp in mc_tail.hip: a plain sum of 1024 terms was 125 ulp off).
struct Comp {
    float s = 0.0f, c = 0.0f;
    __device__ __forceinline__ void add(float x) {
        const float y = x - c;
        const float t = s + y;
        c = (t - s) - y;
        s = t;
    }
};

__device__ __forceinline__ float softplus20(float v) { return v > 20.0f ? v : log1pf(expf(v)); }      // as uncertainty_kernel

// (log p, p) of one logit; a = the row's maximum (NORM: its softplus sum), lz = the row's log partition.
template <bool NORM>
__device__ __forceinline__ void prob(float v, float a, float lz, float* ls, float* p) {
    if (NORM) {
        const float q = softplus20(v);
        *ls = logf(q) - lz;
        *p = q / a;
    } else {
        *ls = (v - a) - lz;
        *p = expf(*ls);
    }
}

// f(i, p[i * stride]) for i = 0 .. n - 1 in ascending order, four loads in flight: every loop of the kernel is a chain of dependent
// adds behind a strided read, and one read per trip leaves the kernel waiting on memory (the order of the arithmetic is untouched).
template <class F>
__device__ __forceinline__ void strided(const float* __restrict__ p, int64_t stride, int n, F f) {
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[(i + j) * stride];
#pragma unroll
        for (int j = 0; j < 4; ++j) f(i + j, v[j]);
    }
    for (; i < n; ++i) f(i, p[i * stride]);
}

template <bool NORM>
__global__ __launch_bounds__(kThreads * kRows) void mc_uncertainty_cb_kernel(const float* __restrict__ logits, int T, int C, int B,
                                                                             const UncOut o) {
    extern __shared__ float lds[];
    const int tx = threadIdx.x, ty = threadIdx.y, ny = blockDim.y;
    float* s_a = lds;                           // [T][64] row maximum (NORM: softplus sum)
    float* s_l = lds + T * kThreads;            // [T][64] log partition
    float* s_h = lds + 2 * T * kThreads;        // [T][64] H[p_t]
    float* red = lds + 3 * T * kThreads;        // [2][ny][64] the rows' shares of sum_c p_bar log p_bar and of the KL sum
    const int b = blockIdx.x * kThreads + tx;
    const bool ok = b < B;
    const int bb = ok ? b : B - 1;
    const int64_t slab = (int64_t)C * B;
    for (int t = ty; t < T; t += ny) {
        const float* p = logits + t * slab + bb;
        float a;
        Comp z;
        if (NORM) {
            strided(p, B, C, [&](int, float v) { z.add(softplus20(v)); });
            a = z.s;
        } else {
            float mx = -INFINITY;
            strided(p, B, C, [&](int, float v) { mx = fmaxf(mx, v); });
            strided(p, B, C, [&](int, float v) { z.add(expf(v - mx)); });
            a = mx;
        }
        const float lz = logf(z.s);
        Comp h;
        strided(p, B, C, [&](int, float v) {
            float ls, pr;
            prob<NORM>(v, a, lz, &ls, &pr);
            h.add(pr == 0.0f ? 0.0f : pr * ls);
        });
        s_a[t * kThreads + tx] = a;
        s_l[t * kThreads + tx] = lz;
        s_h[t * kThreads + tx] = -h.s;
    }
    __syncthreads();
    const float fT = (float)T;
    Comp ent, kl;
    for (int c = ty; c < C; c += ny) {
        const float* p = logits + (int64_t)c * B + bb;
        float s_v = 0.0f, s_p = 0.0f, s_p2 = 0.0f;
        strided(p, slab, T, [&](int t, float v) {
            float ls, pr;
            prob<NORM>(v, s_a[t * kThreads + tx], s_l[t * kThreads + tx], &ls, &pr);
            s_v += v;
            s_p += pr;
            s_p2 += pr * pr;
        });
        const float pbar = s_p / fT;
        const float lpbar = logf(pbar);
        float s_d2 = 0.0f, s_kl = 0.0f;
        strided(p, slab, T, [&](int t, float v) {
            float ls, pr;
            prob<NORM>(v, s_a[t * kThreads + tx], s_l[t * kThreads + tx], &ls, &pr);
            const float d = pr - pbar;
            s_d2 += d * d;
            const float lpb = T == 1 ? ls : lpbar;          // one draw: log p_bar IS log p_t (logf(expf(ls)) is not ls in every bit)
            s_kl += (pr == 0.0f || pbar == 0.0f) ? 0.0f : pr * (ls - lpb);
        });
        ent.add(pbar == 0.0f ? 0.0f : pbar * lpbar);
        kl.add(s_kl);
        if (ok) {
            const int64_t i = (int64_t)b * C + c;
            if (o.pred != nullptr) o.pred[i] = s_v / fT;
            if (o.p_mean != nullptr) o.p_mean[i] = pbar;
            if (o.epi != nullptr) o.epi[i] = s_d2 / fT;
            if (o.ale != nullptr) o.ale[i] = pbar - s_p2 / fT;
        }
    }
    red[ty * kThreads + tx] = ent.s;
    red[(ny + ty) * kThreads + tx] = kl.s;
    __syncthreads();
    if (ty == 0 && ok) {
        float e = 0.0f, m = 0.0f, h = 0.0f;
        for (int r = 0; r < ny; ++r) {
            e += red[r * kThreads + tx];
            m += red[(ny + r) * kThreads + tx];
        }
        for (int t = 0; t < T; ++t) h += s_h[t * kThreads + tx];
        m /= fT;
        if (o.ent != nullptr) o.ent[b] = -e;
        if (o.exp_ent != nullptr) o.exp_ent[b] = h / fT;
        if (o.mi != nullptr) o.mi[b] = m < 0.0f ? 0.0f : m;        // (not fmaxf: a NaN stays)
    }
}

template <bool NORM>
int launch(const float* logits, int draws, int batch, int classes, const UncOut& o, const mc_uncertainty_plan::Plan& p, hipStream_t stream) {
    if (p.lds_bytes > mc_uncertainty_plan::kDefaultLdsBytes) {      // (more than 74 draws: beyond what a kernel gets unasked)
        static SmemAttrState attr_state;
        if (const int rc = ensure_dynamic_smem(reinterpret_cast<const void*>(mc_uncertainty_cb_kernel<NORM>), p.lds_bytes, attr_state))
            return rc;
    }
    hipLaunchKernelGGL(mc_uncertainty_cb_kernel<NORM>, dim3(p.blocks), dim3(kThreads, p.rows), (size_t)p.lds_bytes, stream, logits, draws,
                       classes, batch, o);
    return (int)hipGetLastError();
}

// ---- backward: d (sum of upstream x outputs) / d logits, [T][C][B], in one launch ------------------------------------------------------
// Upstream gradients of the seven outputs; a NULL pointer is a zero, in the SAME arithmetic (0 * NaN stays NaN, as the reference's).
struct UncUp {
    const float *pred, *p_mean, *epi, *ale, *ent, *exp_ent, *mi;
};

__device__ __forceinline__ float up(const float* w, int64_t i) { return w != nullptr ? w[i] : 0.0f; }

// One thread = one (draw t, image b): with p_bar read back from the forward nothing else of the image is needed.  Sweeps over the C
// classes as phase 1 of the forward (maximum, log partition), then D = sum_k p G (compensated), then the C results:
//   G[k] = (-(w_ent + w_mi) log p_bar[k] - (w_ee - w_mi) log p[k] + w_pm[k] + 2 w_epi[k] (p[k] - p_bar[k]) + w_ale[k] (1 - 2 p[k])) / T
//   d logits[c] = J[c] (G[c] - D) + w_pred[c] / T,     J = p (softmax),  sigmoid(v) / z (normalized; 1 / z for v > 20)
// A class with p == 0 adds exactly 0 to D and gets w_pred / T alone (its log p may be -inf: neither 0 * -inf nor log 0 is formed); the
// log p_bar term is 0 where p_bar == 0 (p_bar >= p / T: only beside a p in the subnormals).  The tests are false for NaN.  T == 1:
// log p_bar IS log p.  blockDim = (64, 1), grid = (ceil(B / 64), T): lanes = consecutive images, every [.][.][B] access coalesced.
template <bool NORM>
__global__ __launch_bounds__(kThreads) void mc_uncertainty_cb_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ p_mean,
                                                                         int T, int C, int B, const UncUp w, float* __restrict__ out) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const int64_t off = (int64_t)blockIdx.y * C * B + b;
    const float* p = logits + off;
    float a;
    Comp z;
    if (NORM) {
        strided(p, B, C, [&](int, float v) { z.add(softplus20(v)); });
        a = z.s;
    } else {
        float mx = -INFINITY;
        strided(p, B, C, [&](int, float v) { mx = fmaxf(mx, v); });
        strided(p, B, C, [&](int, float v) { z.add(expf(v - mx)); });
        a = mx;
    }
    const float lz = logf(z.s);
    const float fT = (float)T;
    const float c_bar = -(up(w.ent, b) + up(w.mi, b)), c_t = -(up(w.exp_ent, b) - up(w.mi, b));
    const int64_t row = (int64_t)b * C;
    // (G, p) of class k; G is only used where p != 0
    auto grad = [&](int k, float v, float* pr) {
        float ls;
        prob<NORM>(v, a, lz, &ls, pr);
        const float pb = p_mean[row + k];
        const float lpb = T == 1 ? ls : logf(pb);
        const float t_bar = pb == 0.0f ? 0.0f : c_bar * lpb;
        const float t_epi = 2.0f * up(w.epi, row + k) * (*pr - pb);
        const float t_ale = up(w.ale, row + k) * (1.0f - 2.0f * *pr);
        return ((((t_bar + c_t * ls) + up(w.p_mean, row + k)) + t_epi) + t_ale) / fT;
    };
    Comp d;
    strided(p, B, C, [&](int k, float v) {
        float pr;
        const float g = grad(k, v, &pr);
        d.add(pr == 0.0f ? 0.0f : pr * g);
    });
    float* o = out + off;
    strided(p, B, C, [&](int k, float v) {
        float pr;
        const float g = grad(k, v, &pr);
        float j = pr;
        if (NORM) j = (v > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-v))) / a;
        o[(int64_t)k * B] = (pr == 0.0f ? 0.0f : j * (g - d.s)) + up(w.pred, row + k) / fT;
    });
}

template <bool NORM>
int launch_bwd(const float* logits, const float* p_mean, int draws, int batch, int classes, const UncUp& w, float* out,
               const mc_uncertainty_plan::Plan& p, hipStream_t stream) {
    hipLaunchKernelGGL(mc_uncertainty_cb_bwd_kernel<NORM>, dim3(p.blocks, draws), dim3(kThreads, p.rows), 0, stream, logits, p_mean, draws,
                       classes, batch, w, out);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int bbb_mc_uncertainty_cb_bwd_plan(const float* logits, const float* p_mean, int draws, int batch, int classes, const float* w_pred,
                                              const float* w_p_mean, const float* w_epistemic, const float* w_aleatoric,
                                              const float* w_entropy, const float* w_expected_entropy, const float* w_mutual_info,
                                              const float* d_logits, int32_t* rows, int32_t* blocks, int32_t* lds_bytes) {
    const void* const ups[mc_uncertainty_plan::kUpstreams] = {w_pred, w_p_mean, w_epistemic, w_aleatoric, w_entropy, w_expected_entropy,
                                                              w_mutual_info};
    mc_uncertainty_plan::Plan p;
    const int rc = mc_uncertainty_plan::plan_bwd(logits, p_mean, draws, batch, classes, ups, d_logits, &p);
    if (rows != nullptr) *rows = p.rows;
    if (blocks != nullptr) *blocks = p.blocks;
    if (lds_bytes != nullptr) *lds_bytes = p.lds_bytes;
    return rc;
}

extern "C" int bbb_mc_uncertainty_cb_bwd(const float* logits, const float* p_mean, int draws, int batch, int classes, int normalized,
                                         const float* w_pred, const float* w_p_mean, const float* w_epistemic, const float* w_aleatoric,
                                         const float* w_entropy, const float* w_expected_entropy, const float* w_mutual_info,
                                         float* d_logits, void* stream) {
    const void* const ups[mc_uncertainty_plan::kUpstreams] = {w_pred, w_p_mean, w_epistemic, w_aleatoric, w_entropy, w_expected_entropy,
                                                              w_mutual_info};
    mc_uncertainty_plan::Plan p;
    if (const int rc = mc_uncertainty_plan::plan_bwd(logits, p_mean, draws, batch, classes, ups, d_logits, &p)) return rc;
    const UncUp w{w_pred, w_p_mean, w_epistemic, w_aleatoric, w_entropy, w_expected_entropy, w_mutual_info};
    return normalized ? launch_bwd<true>(logits, p_mean, draws, batch, classes, w, d_logits, p, (hipStream_t)stream)
                      : launch_bwd<false>(logits, p_mean, draws, batch, classes, w, d_logits, p, (hipStream_t)stream);
}

extern "C" int bbb_mc_uncertainty_cb_plan(const float* logits, int draws, int batch, int classes, const float* pred, const float* p_mean,
                                          const float* epistemic, const float* aleatoric, const float* entropy,
                                          const float* expected_entropy, const float* mutual_info, int32_t* rows, int32_t* blocks,
                                          int32_t* lds_bytes) {
    const void* const outs[mc_uncertainty_plan::kOutputs] = {pred, p_mean, epistemic, aleatoric, entropy, expected_entropy, mutual_info};
    mc_uncertainty_plan::Plan p;
    const int rc = mc_uncertainty_plan::plan(logits, draws, batch, classes, outs, &p);
    if (rows != nullptr) *rows = p.rows;
    if (blocks != nullptr) *blocks = p.blocks;
    if (lds_bytes != nullptr) *lds_bytes = p.lds_bytes;
    return rc;
}

extern "C" int bbb_mc_uncertainty_cb(const float* logits, int draws, int batch, int classes, int normalized, float* pred, float* p_mean,
                                     float* epistemic, float* aleatoric, float* entropy, float* expected_entropy, float* mutual_info,
                                     void* stream) {
    const void* const outs[mc_uncertainty_plan::kOutputs] = {pred, p_mean, epistemic, aleatoric, entropy, expected_entropy, mutual_info};
    mc_uncertainty_plan::Plan p;
    if (const int rc = mc_uncertainty_plan::plan(logits, draws, batch, classes, outs, &p)) return rc;
    const UncOut o{pred, p_mean, epistemic, aleatoric, entropy, expected_entropy, mutual_info};
    return normalized ? launch<true>(logits, draws, batch, classes, o, p, (hipStream_t)stream)
                      : launch<false>(logits, draws, batch, classes, o, p, (hipStream_t)stream);
}
