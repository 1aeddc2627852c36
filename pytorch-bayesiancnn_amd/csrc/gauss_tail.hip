// Gaussian-likelihood tail of a Monte-Carlo step on batch-innermost logits [E][C][B] for gfx950: the ELBO of a regression model
// (forward: LL [B] in one launch, the loss in a one-block launch behind it; backward: ONE launch) and the predictive moments (ONE launch).
// The regression twin of the categorical tail (mc_tail.hip) and of mc_uncertainty.hip; plain HIP, no atomics, no inline assembly.
//
// Targets y [B][D] fp32.  Heteroscedastic (C == 2 D): channel d is the mean mu, channel D + d the log-variance s.  Homoscedastic
// (C == D): s = 2 log(noise_sigma), a constant rounded to fp32 once on the host.  With s_c = clamp(s, lo, hi), r = y - mu:
//   ll[e][d][b] = -0.5 * ((log 2 pi + s_c) + (r * r) * expf(-s_c))         (this order, no contraction: see the pragma below)
//   L[e][b]     = sum_d ll, d ascending, a plain fp32 sum
//   LL[b]       = logmeanexp: m + logf(z) - log n, with (m, z) the ONLINE log-sum-exp over e ascending (draw 0: m = L, z = 1; then
//                 L > m ? (z = z * expf(m - L) + 1, m = L) : (z += expf(L - m))); n = mean_over > 0 ? mean_over : E, log n rounded on the host
//                 mean: (sum_e L, e ascending) / E
//   loss        = -((train_size / B) * sum_b LL[b]) + beta * kl; sum_b: thread t of ONE 256-thread block adds b = t, t + 256, ... in
//                 ascending order, then a fixed tree (128, 64, ..., 1) -- the value does not depend on how many blocks wrote LL.
// blockDim = 64 lanes = 64 consecutive images, so every logit read is a coalesced row of 64 images per (e, channel), as in
// mc_tail_cb_kernel and mc_uncertainty_cb_kernel.  y is row-major: the block's images x 16 dimensions are staged through LDS with
// consecutive lanes on consecutive addresses (D <= 16: the block's whole slab of y is one contiguous run, staged once; D > 16: a tile
// per 16 dimensions, staged again for every draw -- y stays in L2), pitch 17 floats, so a lane reads its row without bank conflicts.
//
// The forward's two launches meet at the launch boundary (as bbb_elbo_cb_fwd's tail + loss pair and bbb_grad_norm_finish do): no
// workgroup waits for another.  The backward RECOMPUTES L[e][b] from the logits (nothing but LL is kept from the forward, and the
// backward does not read it): one walk for (m, z) -- the same function the forward runs, hence the same bits -- and one for the
// weights w[e][b] = expf(L - (m + logf(z))) (mean: 1 / E) and the gradients
//   g_mu = c * w * (r * expf(-s_c)),   g_s = c * w * (0.5 * ((r * r) * expf(-s_c) - 1)) inside [lo, hi], exactly 0 outside,
//   c = -(train_size / B) * g_loss;   g_kl = beta * g_loss.
// A draw 1e4 below the best one has expf(...) == 0: weight exactly 0 in both directions.  The clamp is written with comparisons, not
// fminf / fmaxf, so a NaN stays a NaN: image b's LL, the loss, and image b's gradient columns become NaN, no other image's.
// The moments walk d outermost: mean = (sum_e mu) / E, epistemic = (sum_e (mu - mean)^2) / E in a second pass over the draws (never
// E[mu^2] - mean^2), aleatoric = (sum_e expf(s_c)) / E, total = epistemic + aleatoric; log_density (with y) = LL in the logmeanexp
// form with n = E, by the forward's own function.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "gauss_tail_plan.h"

// L must have the same bits wherever it is recomputed: no fused multiply-add that one inlining context forms and another does not.
#pragma clang fp contract(off)

namespace {

using gauss_tail_plan::kLossThreads;
using gauss_tail_plan::kPitch;
using gauss_tail_plan::kThreads;
using gauss_tail_plan::kTile;

constexpr float kLog2Pi = 1.8378770664093453f;

struct Geo {
    const float* logits;      // [E][C][B]
    const float* y;           // [B][D] (moments: may be null)
    int E, C, D, B;
    int hetero;
    float s_const;            // homoscedastic: 2 log(noise_sigma)
    float lo, hi;             // clamp of the log-variance
};

__device__ __forceinline__ float clamp_keep_nan(float s, float lo, float hi) { return s < lo ? lo : (s > hi ? hi : s); }

// y[b0 .. b0 + nb)[d0 .. d0 + nd) -> tile[image][j]: consecutive lanes read consecutive addresses of each image's nd-float run (nd == D:
// of the whole slab).
__device__ __forceinline__ void stage_y(const Geo& g, int d0, int nd, float* tile) {
    const int b0 = blockIdx.x * kThreads;
    const int nb = g.B - b0 < kThreads ? g.B - b0 : kThreads;
    for (int i = threadIdx.x; i < nb * nd; i += kThreads) {
        const int r = i / nd, j = i - r * nd;
        tile[r * kPitch + j] = g.y[(int64_t)(b0 + r) * g.D + d0 + j];
    }
}

// f(d, mu, s, y) for d = 0 .. D - 1 ascending, draw e of image bb (the lane's image, clamped into the batch).  Every lane of the
// block calls it with the same e: it holds barriers when D > kTile.
template <class F>
__device__ __forceinline__ void walk_draw(const Geo& g, int e, int bb, float* tile, F f) {
    const float* p = g.logits + (int64_t)e * g.C * g.B + bb;
    const bool single = g.D <= kTile;                       // staged once by the kernel
    for (int d0 = 0; d0 < g.D; d0 += kTile) {
        const int nd = g.D - d0 < kTile ? g.D - d0 : kTile;
        if (!single) {
            __syncthreads();
            stage_y(g, d0, nd, tile);
            __syncthreads();
        }
        for (int j = 0; j < nd; ++j) {
            const int d = d0 + j;
            const float mu = p[(int64_t)d * g.B];
            const float s = g.hetero ? p[(int64_t)(g.D + d) * g.B] : g.s_const;
            f(d, mu, s, tile[threadIdx.x * kPitch + j]);
        }
    }
}

// L[e][bb]
__device__ __forceinline__ float draw_ll(const Geo& g, int e, int bb, float* tile) {
    float L = 0.0f;
    walk_draw(g, e, bb, tile, [&](int, float mu, float s, float yv) {
        const float sc = clamp_keep_nan(s, g.lo, g.hi);
        const float r = yv - mu;
        L += -0.5f * ((kLog2Pi + sc) + (r * r) * expf(-sc));
    });
    return L;
}

// (m, z) of the online log-sum-exp over the draws (mc == 0), or (sum_e L, unused) (mc == 1)
__device__ __forceinline__ void reduce_draws(const Geo& g, int mc, int bb, float* tile, float* m_out, float* z_out) {
    float m = draw_ll(g, 0, bb, tile), z = 1.0f;
    for (int e = 1; e < g.E; ++e) {
        const float L = draw_ll(g, e, bb, tile);
        if (mc != 0) {
            m += L;
        } else if (L > m) {
            z = z * expf(m - L) + 1.0f;
            m = L;
        } else {
            z += expf(L - m);
        }
    }
    *m_out = m;
    *z_out = z;
}

__device__ __forceinline__ float image_ll(const Geo& g, int mc, float log_n, int bb, float* tile) {
    float m, z;
    reduce_draws(g, mc, bb, tile, &m, &z);
    return mc != 0 ? m / (float)g.E : (m + logf(z)) - log_n;
}

__global__ __launch_bounds__(kThreads) void gauss_ll_kernel(const Geo g, int mc, float log_n, float* __restrict__ ll_out) {
    __shared__ float tile[kThreads * kPitch];
    const int b = blockIdx.x * kThreads + threadIdx.x;
    const int bb = b < g.B ? b : g.B - 1;
    if (g.D <= kTile) {
        stage_y(g, 0, g.D, tile);
        __syncthreads();
    }
    const float ll = image_ll(g, mc, log_n, bb, tile);
    if (b < g.B) ll_out[b] = ll;
}

__global__ __launch_bounds__(kLossThreads) void gauss_loss_kernel(const float* __restrict__ ll, const float* __restrict__ kl, float beta,
                                                                  const float* __restrict__ beta_dev, float gscale, int B,
                                                                  float* __restrict__ loss) {
    __shared__ float part[kLossThreads];
    float acc = 0.0f;
    for (int b = threadIdx.x; b < B; b += kLossThreads) acc += ll[b];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kLossThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = -(gscale * part[0]) + (beta_dev ? *beta_dev : beta) * (*kl);
}

__global__ __launch_bounds__(kThreads) void gauss_bwd_kernel(const Geo g, int mc, const float* __restrict__ g_loss, float gscale,
                                                             float beta, const float* __restrict__ beta_dev,
                                                             float* __restrict__ g_logits, float* __restrict__ g_kl) {
    __shared__ float tile[kThreads * kPitch];
    const int b = blockIdx.x * kThreads + threadIdx.x;
    const bool ok = b < g.B;
    const int bb = ok ? b : g.B - 1;
    const float gl = *g_loss;
    if (blockIdx.x == 0 && threadIdx.x == 0 && g_kl != nullptr) *g_kl = (beta_dev ? *beta_dev : beta) * gl;
    if (g.D <= kTile) {
        stage_y(g, 0, g.D, tile);
        __syncthreads();
    }
    float m = 0.0f, z = 1.0f;
    if (mc == 0) reduce_draws(g, 0, bb, tile, &m, &z);
    const float lse = m + logf(z);
    const float c = -gscale * gl;
    for (int e = 0; e < g.E; ++e) {
        const float w = mc != 0 ? 1.0f / (float)g.E : expf(draw_ll(g, e, bb, tile) - lse);
        const float cw = c * w;
        float* o = g_logits + (int64_t)e * g.C * g.B + bb;
        walk_draw(g, e, bb, tile, [&](int d, float mu, float s, float yv) {
            const float sc = clamp_keep_nan(s, g.lo, g.hi);
            const float r = yv - mu;
            const float ei = expf(-sc);
            if (!ok) return;
            o[(int64_t)d * g.B] = cw * (r * ei);
            if (g.hetero) o[(int64_t)(g.D + d) * g.B] = (s >= g.lo && s <= g.hi) ? cw * (0.5f * ((r * r) * ei - 1.0f)) : 0.0f;
        });
    }
}

struct MomOut {
    float *mean, *epi, *ale, *total, *logd;
};

__global__ __launch_bounds__(kThreads) void gauss_moments_kernel(const Geo g, float log_n, const MomOut o) {
    __shared__ float tile[kThreads * kPitch];
    const int b = blockIdx.x * kThreads + threadIdx.x;
    const bool ok = b < g.B;
    const int bb = ok ? b : g.B - 1;
    const float fE = (float)g.E;
    const int64_t slab = (int64_t)g.C * g.B;
    for (int d = 0; d < g.D; ++d) {
        const float* p = g.logits + (int64_t)d * g.B + bb;
        float s_mu = 0.0f, s_ale = 0.0f;
        for (int e = 0; e < g.E; ++e) {
            s_mu += p[e * slab];
            const float s = g.hetero ? p[e * slab + (int64_t)g.D * g.B] : g.s_const;
            s_ale += expf(clamp_keep_nan(s, g.lo, g.hi));
        }
        const float mean = s_mu / fE;
        float s_d2 = 0.0f;
        for (int e = 0; e < g.E; ++e) {
            const float dv = p[e * slab] - mean;
            s_d2 += dv * dv;
        }
        if (ok) {
            const int64_t i = (int64_t)b * g.D + d;
            const float epi = s_d2 / fE, ale = s_ale / fE;
            if (o.mean != nullptr) o.mean[i] = mean;
            if (o.epi != nullptr) o.epi[i] = epi;
            if (o.ale != nullptr) o.ale[i] = ale;
            if (o.total != nullptr) o.total[i] = epi + ale;
        }
    }
    if (o.logd == nullptr) return;                          // (the same for every lane of the launch)
    if (g.D <= kTile) {
        stage_y(g, 0, g.D, tile);
        __syncthreads();
    }
    const float ll = image_ll(g, 0, log_n, bb, tile);
    if (ok) o.logd[b] = ll;
}

Geo geo_of(const float* logits, const float* y, const gauss_tail_plan::Shape& s, const gauss_tail_plan::Plan& p) {
    Geo g;
    g.logits = logits;
    g.y = y;
    g.E = s.draws;
    g.C = s.channels;
    g.D = s.dims;
    g.B = s.batch;
    g.hetero = p.hetero;
    g.s_const = p.hetero ? 0.0f : (float)(2.0 * log(s.noise_sigma));
    g.lo = s.log_var_min;
    g.hi = s.log_var_max;
    return g;
}

float log_n_of(const gauss_tail_plan::Shape& s) { return (float)log((double)(s.mean_over > 0 ? s.mean_over : s.draws)); }

void write_plan(const gauss_tail_plan::Plan& p, int32_t* threads, int32_t* blocks, int32_t* lds_bytes) {
    if (threads != nullptr) *threads = p.threads;
    if (blocks != nullptr) *blocks = p.blocks;
    if (lds_bytes != nullptr) *lds_bytes = p.lds_bytes;
}

}  // namespace

extern "C" int bbb_gauss_elbo_cb_fwd_plan(const float* logits, const float* y, const float* kl, const float* beta_dev, int draws, int batch,
                                          int channels, int dims, double noise_sigma, float log_var_min, float log_var_max, int mc,
                                          int mean_over, const float* ll_out, const float* loss_out, int32_t* threads, int32_t* blocks,
                                          int32_t* lds_bytes) {
    const gauss_tail_plan::Shape s{draws, batch, channels, dims, noise_sigma, log_var_min, log_var_max, mc, mean_over};
    gauss_tail_plan::Plan p;
    const int rc = gauss_tail_plan::plan_fwd(logits, y, kl, beta_dev, ll_out, loss_out, s, &p);
    write_plan(p, threads, blocks, lds_bytes);
    return rc;
}

extern "C" int bbb_gauss_elbo_cb_fwd(const float* logits, const float* y, const float* kl, float beta, const float* beta_dev,
                                     float train_size, int draws, int batch, int channels, int dims, double noise_sigma,
                                     float log_var_min, float log_var_max, int mc, int mean_over, float* ll_out, float* loss_out,
                                     void* stream) {
    const gauss_tail_plan::Shape s{draws, batch, channels, dims, noise_sigma, log_var_min, log_var_max, mc, mean_over};
    gauss_tail_plan::Plan p;
    if (const int rc = gauss_tail_plan::plan_fwd(logits, y, kl, beta_dev, ll_out, loss_out, s, &p)) return rc;
    hipLaunchKernelGGL(gauss_ll_kernel, dim3(p.blocks), dim3(p.threads), 0, (hipStream_t)stream, geo_of(logits, y, s, p), mc, log_n_of(s),
                       ll_out);
    if (const int rc = (int)hipGetLastError()) return rc;
    hipLaunchKernelGGL(gauss_loss_kernel, dim3(1), dim3(kLossThreads), 0, (hipStream_t)stream, ll_out, kl, beta, beta_dev,
                       train_size / (float)batch, batch, loss_out);
    return (int)hipGetLastError();
}

extern "C" int bbb_gauss_elbo_cb_bwd_plan(const float* logits, const float* y, const float* g_loss, const float* beta_dev, int draws,
                                          int batch, int channels, int dims, double noise_sigma, float log_var_min, float log_var_max,
                                          int mc, int mean_over, const float* g_logits, const float* g_kl, int32_t* threads,
                                          int32_t* blocks, int32_t* lds_bytes) {
    const gauss_tail_plan::Shape s{draws, batch, channels, dims, noise_sigma, log_var_min, log_var_max, mc, mean_over};
    gauss_tail_plan::Plan p;
    const int rc = gauss_tail_plan::plan_bwd(logits, y, g_loss, beta_dev, g_logits, g_kl, s, &p);
    write_plan(p, threads, blocks, lds_bytes);
    return rc;
}

extern "C" int bbb_gauss_elbo_cb_bwd(const float* logits, const float* y, const float* g_loss, float beta, const float* beta_dev,
                                     float train_size, int draws, int batch, int channels, int dims, double noise_sigma,
                                     float log_var_min, float log_var_max, int mc, int mean_over, float* g_logits, float* g_kl,
                                     void* stream) {
    const gauss_tail_plan::Shape s{draws, batch, channels, dims, noise_sigma, log_var_min, log_var_max, mc, mean_over};
    gauss_tail_plan::Plan p;
    if (const int rc = gauss_tail_plan::plan_bwd(logits, y, g_loss, beta_dev, g_logits, g_kl, s, &p)) return rc;
    hipLaunchKernelGGL(gauss_bwd_kernel, dim3(p.blocks), dim3(p.threads), 0, (hipStream_t)stream, geo_of(logits, y, s, p), mc, g_loss,
                       train_size / (float)batch, beta, beta_dev, g_logits, g_kl);
    return (int)hipGetLastError();
}

extern "C" int bbb_gauss_moments_cb_plan(const float* logits, const float* y, int draws, int batch, int channels, int dims,
                                         double noise_sigma, float log_var_min, float log_var_max, const float* mean,
                                         const float* epistemic, const float* aleatoric, const float* total, const float* log_density,
                                         int32_t* threads, int32_t* blocks, int32_t* lds_bytes) {
    const gauss_tail_plan::Shape s{draws, batch, channels, dims, noise_sigma, log_var_min, log_var_max, 0, 0};
    const void* const outs[gauss_tail_plan::kMoments] = {mean, epistemic, aleatoric, total, log_density};
    gauss_tail_plan::Plan p;
    const int rc = gauss_tail_plan::plan_moments(logits, y, outs, s, &p);
    write_plan(p, threads, blocks, lds_bytes);
    return rc;
}

extern "C" int bbb_gauss_moments_cb(const float* logits, const float* y, int draws, int batch, int channels, int dims, double noise_sigma,
                                    float log_var_min, float log_var_max, float* mean, float* epistemic, float* aleatoric, float* total,
                                    float* log_density, void* stream) {
    const gauss_tail_plan::Shape s{draws, batch, channels, dims, noise_sigma, log_var_min, log_var_max, 0, 0};
    const void* const outs[gauss_tail_plan::kMoments] = {mean, epistemic, aleatoric, total, log_density};
    gauss_tail_plan::Plan p;
    if (const int rc = gauss_tail_plan::plan_moments(logits, y, outs, s, &p)) return rc;
    const MomOut o{mean, epistemic, aleatoric, total, log_density};
    hipLaunchKernelGGL(gauss_moments_kernel, dim3(p.blocks), dim3(p.threads), 0, (hipStream_t)stream, geo_of(logits, y, s, p), log_n_of(s),
                       o);
    return (int)hipGetLastError();
}
