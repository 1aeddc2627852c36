/*
 * bbb_hip.h -- C ABI of libbbb_hip.so, the MI355X (gfx950) Bayes-by-Backprop hot path.
 *
 * The upstream project (kumar-shridhar/PyTorch-BayesianCNN) is pure Python and has no FFI; this
 * header is the native boundary its `layers` package would bind.  Each entry point names the
 * upstream lines it replaces.  Conventions:
 *   - every pointer is a DEVICE pointer to fp32 data unless it says "host";
 *   - nothing is allocated, freed or retained; outputs are caller-owned buffers;
 *   - `stream` is a hipStream_t (0 = the null stream); every call only enqueues work on it;
 *   - return value: 0 on success, a negative BBB_E* code for argument errors, or the positive
 *     hipError_t of a failed launch.  No call aborts or throws.
 *   - tensors are contiguous: activations NCHW, conv weights [Cout, Cin, kh, kw], linear weights
 *     [out, in], all row-major (the reference's own layouts).
 *
 * Noise contract (replaces torch.empty(shape).normal_(0,1) on the CPU generator,
 * layers/BBB/BBBConv.py:63,68; layers/BBB_LRT/BBBConv.py:78): element i of noise stream
 * (seed, call, stream_id) is output (i & 3) of
 *     Philox4x32-7(counter = {lo32(i >> 2), i >> 34, stream_id, call}, key = {lo32(seed), hi32(seed)})
 * (Random123; 7 rounds = its published BigCrush-passing minimum) pushed through Box-Muller pairs
 * (x0,x1)->(z0,z1), (x2,x3)->(z2,z3) with 23-bit mantissas
 *     u1 = 1 - (xa >> 9) * 2^-23 in (0,1],  u2 = (xb >> 9) * 2^-23 in [0,1),  z = sqrt(-2 ln u1) * {cos,sin}(2 pi u2).
 * (ABI <= 3 used Philox4x32-10 and 24-bit uniforms; the stream definition is part of the ABI version.)
 * Monte-Carlo draw j of an ensemble uses call = call0 + j, so a batched E-draw launch and E
 * single-draw launches produce the same numbers, and any GPU can materialise any draw.
 */
#ifndef BBB_HIP_H
#define BBB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBB_ABI_VERSION 13
#define BBB_MAX_SEGMENTS 16

#define BBB_EINVAL (-1)   /* bad argument (null pointer, non-positive size, too many segments) */
#define BBB_EALIGN (-2)   /* pointer not 4-byte aligned */
#define BBB_ESHAPE (-3)   /* inconsistent convolution geometry */

/* One parameter tensor pair (mu, rho) of a Bayesian layer: W or bias. */
typedef struct bbb_segment {
    const float* mu;      /* [n]  W_mu / bias_mu */
    const float* rho;     /* [n]  W_rho / bias_rho */
    float* w;             /* out [draws][n] at w + e*draw_stride: mu + softplus(rho)*eps; NULL = no sampling */
    float* sigma;         /* out [n]: softplus(rho), or its square when BBB_SIGMA_SQUARED; NULL = skip */
    const float* eps;     /* test entry: external noise [draws][n] (same stride as w); NULL = on-chip Philox */
    int64_t n;            /* elements */
    int64_t draw_stride;  /* elements between consecutive draws of w / eps (>= n) */
    uint32_t stream_id;   /* noise stream of this tensor */
    uint32_t w_row_len;   /* 0: w is fp32, dense.  > 0: w is BF16 (round-to-nearest-even), a matrix with rows of
                             w_row_len elements stored at a pitch of w_row_len rounded up to 8 elements -- the operand
                             layout of bbb_conv2d_chwn_bf16_fwd; draw_stride then counts bf16 elements, the pad columns
                             are written as zeros, and `eps` (fp32) keeps the dense [draws][n] layout with stride n */
    uint32_t w_taps;      /* bf16 rows only.  0 / 1: row elements keep the tensor's own order ([cin][kh][kw]).  T > 1: the
                             row is a [cin][T] matrix (T = kh*kw) and is written TRANSPOSED, [T][cin] ("tap-major":
                             element (ci, t) lands at column t*cin + ci), the BBB_BF16_W_TAP_MAJOR operand layout */
    uint32_t w_tm_cin;    /* fp32 w only (w_row_len == 0; ABI 11).  C > 0: the tensor is [rows][C][T] with T = w_taps (2..128), C % 8 == 0,
                             and w is written TAP-MAJOR, fp32 [draws][rows][T][C] -- the weight operand of bbb_conv2d_c8x3_fwd.  Noise
                             elements, sigma and KL are those of the dense launch (the noise of a weight is keyed by its index in
                             the tensor's own order); mu, rho and w 16-byte aligned, draw_stride % 4 == 0, on-chip noise only. */
} bbb_segment_t;

#define BBB_SIGMA_SQUARED 1u   /* flags: write sigma^2 (the LRT variance operand) instead of sigma */
#define BBB_KL_TEXTBOOK   2u   /* flags: KL(q||p) instead of the reference's swapped-argument form */
#define BBB_GW_MEAN_ONLY  4u   /* bbb_reparam_kl_bwd flags: the `w` gradients reach mu only (no eps term into rho): an LRT layer's
                                * d loss / d W_mu folded into the KL backward instead of a separate accumulation per tensor */

/*
 * Fused reparameterisation + KL over up to BBB_MAX_SEGMENTS tensors and `draws` Monte-Carlo draws in
 * ONE pass over (mu, rho).  Replaces, per layer and per draw: the CPU normal_ + H2D copy, log1p(exp(rho)),
 * mu + eps*sigma (layers/BBB/BBBConv.py:63-70, BBBLinear.py:56-63), the sigma / sigma**2 of the LRT
 * layers (layers/BBB_LRT/BBBConv.py:64-69, BBBLinear.py:58-63) and metrics.calculate_kl as called by
 * kl_loss() (metrics.py:27-29 via layers/BBB/BBBConv.py:79-83), plus the Python sum over layers
 * (layers/misc.py:20-23).
 *   segs        host array of nseg descriptors (copied into the kernel arguments)
 *   kl_partials device scratch, at least bbb_reparam_partials(segs, nseg) doubles, 8-byte aligned, FILLED WITH 0xFF
 *               BYTES before the first launch that uses it ("not published yet"); every launch leaves the slots it
 *               used in that state again.  One scratch buffer per stream (launches that may overlap must not share one).
 *   kl_out      device float: sum over all segments of the KL term (NULL = no KL)
 *   kl_out64    optional device double with the same sum (NULL = skip)
 *   call_dev    optional DEVICE uint32 added to call0 when the kernel runs (NULL = 0).  This is what lets a
 *               captured hipGraph draw fresh noise on every replay: the graph also contains the increment.
 * KL does not depend on eps; the sum is reduced in a fixed order in fp64 (bitwise reproducible): every 1024-element
 * chunk publishes an fp64 partial before its draws start and one extra block of the same launch adds them up in index
 * order -- one launch, no separate finish kernel, the reduction hidden behind the sampling work.
 */
int bbb_reparam_kl_fwd(const bbb_segment_t* segs, int nseg, int draws,
                       float prior_mu, float prior_sigma,
                       uint64_t seed, uint32_t call0, uint32_t flags,
                       double* kl_partials, float* kl_out, double* kl_out64,
                       const uint32_t* call_dev, void* stream);

/* Number of doubles of scratch bbb_reparam_kl_fwd needs for these segments, host-only helper. */
int64_t bbb_reparam_partials(const bbb_segment_t* segs, int nseg);

/* What bbb_reparam_kl_fwd launches for these segments (additive to ABI 13; host only, needs no device: tests, profiling): the entry's
 * own plan, without the launch.  slots: 256-thread blocks resident at once (8 per compute unit); <= 0 = ask the current device as
 * the launcher does.  *kernel: 0 = the fast kernel (every segment dense fp32 with on-chip noise), 1 = the generic one (external eps
 * or bf16 rows).  *gpt: 16-byte groups per thread, 4 when the segments total more than 1024 * 16384 elements, else 1.  *nt: the
 * fast kernel stores w non-temporally (gpt 4 or draws <= 16).  *chunks: (1024 * gpt)-element chunks = KL partials.  *n_small,
 * *small_chunk0: when slots < chunks <= 3 * slots, draws > 1, gpt 1 and no tap-major segment, the last chunks % slots chunks (from
 * *small_chunk0 on) run as one block per draw at the front of the grid, *n_small blocks in all; else 0 and *chunks.  *tm_blocks:
 * blocks that write the fp32 tap-major segments (w_tm_cin), ahead of everything else.  *grid: blocks of a launch that wants the
 * KL (the summing block included; one fewer without).  Returns what the launch entry returns for the same segments: 0, BBB_EINVAL,
 * BBB_EALIGN, or BBB_ESHAPE when a count does not fit 32 bits.  Out-pointers may be NULL. */
int bbb_reparam_kl_plan(const bbb_segment_t* segs, int nseg, int draws, int slots, int32_t* kernel, int32_t* gpt, int32_t* nt,
                        int32_t* chunks, int32_t* n_small, int32_t* small_chunk0, int32_t* tm_blocks, int32_t* grid);

/*
 * Backward of bbb_reparam_kl_fwd (what autograd derives for the reference):
 *   grad_mu  = sum_e gw[e] + gkl * (mu - mu0) / sigma^2
 *   grad_rho = (sum_e gw[e]*eps[e] + gkl * (1/sigma - sigma0^2/sigma^3 - (mu-mu0)^2/sigma^3)) * sigmoid(rho)
 * eps is regenerated from (seed, call0 + e, stream_id), never stored.  In each segment `w` holds the
 * incoming gradient gw [draws][n] (may be NULL = 0), `eps` optional external noise, and `sigma` (may be NULL = 0) the
 * incoming gradient gs [n] w.r.t. the forward's sigma output -- sigma^2 with BBB_SIGMA_SQUARED in flags, the LRT layers'
 * variance operand (layers/BBB_LRT/BBBConv.py:64-69) -- which adds gs * sigmoid(rho), resp. gs * 2 sigma * sigmoid(rho), to
 * grad_rho.
 * grad_mu / grad_rho are arrays of nseg device pointers given on the host.  gkl: device float
 * (d loss / d kl), NULL = 0.  call_dev: as in bbb_reparam_kl_fwd (a captured training step regenerates the forward's noise).
 */
int bbb_reparam_kl_bwd(const bbb_segment_t* segs, int nseg, int draws,
                       float prior_mu, float prior_sigma,
                       uint64_t seed, uint32_t call0, uint32_t flags,
                       const float* gkl, float* const* grad_mu, float* const* grad_rho,
                       const uint32_t* call_dev, void* stream);

/*
 * Per-weight Gaussian priors (additive to ABI 13): the same pass against N(mu0_i, sigma0_i^2) per element instead of one scalar
 * pair for the whole launch -- the posterior of an earlier task as the prior of the next (variational continual learning), or an
 * empirical-Bayes prior centred on pretrained weights (MOPED).  pri: host array of nseg entries, pri[s] for segs[s]; both pointers
 * are DEVICE fp32 [segs[s].n] in the tensor's own order, 4-byte aligned (else BBB_EALIGN), and either may be NULL independently:
 * that quantity of that segment is then the launch-wide scalar (prior_mu / prior_sigma).  pri == NULL, or no pointer set: the
 * launch IS bbb_reparam_kl_fwd / _bwd's, same kernels, same bits.
 *   KL term, reference form (metrics.py:28 in the call-site argument order; a_i = sigma0_i / sigma_i, b_i = (mu_i - mu0_i) / sigma_i):
 *       0.5 * (2 ln(sigma_i / sigma0_i) - 1 + a_i^2 + b_i^2)
 *   BBB_KL_TEXTBOOK (a_i = sigma_i / sigma0_i, b_i = (mu0_i - mu_i) / sigma0_i):
 *       0.5 * (-2 ln(sigma_i / sigma0_i) - 1 + a_i^2 + b_i^2)
 *   backward, reference form:  grad_mu  += gkl * (mu_i - mu0_i) / sigma_i^2
 *                              grad_rho += gkl * (1/sigma_i - (sigma0_i^2 + (mu_i - mu0_i)^2) / sigma_i^3) * sigmoid(rho_i)
 *             textbook form:   grad_mu  += gkl * (mu_i - mu0_i) / sigma0_i^2
 *                              grad_rho += gkl * (sigma_i / sigma0_i^2 - 1/sigma_i) * sigmoid(rho_i)
 *   Nothing flows to the prior.  With mu0 = mu and sigma0 = softplus(rho) the true KL is 0 and the fp32 sum may come out slightly
 *   negative.
 * The prior reaches the KL only: w, sigma / sigma^2, the noise, tap-major and bf16 outputs are the scalar launch's, bit for bit, and
 * the launch shape (kernel, grid, chunks, split, summing block: bbb_reparam_kl_tp_plan) does not depend on the prior.  HBM traffic
 * per element: (8 + 4 per prior tensor + 4 E) B for E draws.
 * prior_sigma > 0 is checked on the host whether or not a segment falls back to it.  Tensor ELEMENTS are not checked: a
 * sigma0_i <= 0 or a non-finite element follows IEEE and stays in the sum, so the KL is NaN or Inf; no other output changes.
 * Every other argument is bbb_reparam_kl_fwd's / _bwd's / _plan's.  bbb_reparam_kl_tp_plan returns what bbb_reparam_kl_tp_fwd returns
 * for the same segments and priors, and reports the same eight fields as bbb_reparam_kl_plan.
 */
typedef struct bbb_prior_segment {
    const float* mu0;      /* [n] prior means, NULL = prior_mu */
    const float* sigma0;   /* [n] prior standard deviations (> 0), NULL = prior_sigma */
} bbb_prior_segment_t;

int bbb_reparam_kl_tp_fwd(const bbb_segment_t* segs, const bbb_prior_segment_t* pri, int nseg, int draws,
                          float prior_mu, float prior_sigma,
                          uint64_t seed, uint32_t call0, uint32_t flags,
                          double* kl_partials, float* kl_out, double* kl_out64,
                          const uint32_t* call_dev, void* stream);
int bbb_reparam_kl_tp_bwd(const bbb_segment_t* segs, const bbb_prior_segment_t* pri, int nseg, int draws,
                          float prior_mu, float prior_sigma,
                          uint64_t seed, uint32_t call0, uint32_t flags,
                          const float* gkl, float* const* grad_mu, float* const* grad_rho,
                          const uint32_t* call_dev, void* stream);
int bbb_reparam_kl_tp_plan(const bbb_segment_t* segs, const bbb_prior_segment_t* pri, int nseg, int draws, int slots,
                           int32_t* kernel, int32_t* gpt, int32_t* nt, int32_t* chunks, int32_t* n_small, int32_t* small_chunk0,
                           int32_t* tm_blocks, int32_t* grid);

/* One parameter tensor of an Adam step: all four arrays hold n fp32 elements on the device. */
typedef struct bbb_adam_segment {
    float* param;        /* updated in place */
    const float* grad;
    float* exp_avg;      /* first moment, updated in place */
    float* exp_avg_sq;   /* second moment, updated in place */
    int64_t n;
} bbb_adam_segment_t;

/*
 * Multi-tensor Adam (training extension): the optimizer.step() of main_bayesian.py:58 for up to BBB_MAX_SEGMENTS
 * tensors in one launch, torch.optim.Adam semantics (amsgrad off, no weight decay), operation order as torch's:
 *   m += (g - m)(1 - beta1);  v = v*beta2 + (1 - beta2) g^2;  p -= lr/(1 - beta1^step) * m / (sqrt(v)/sqrt(1 - beta2^step) + eps)
 * `step` is the 1-based count of this update.  Hyper-parameters are doubles: derived scalars (1 - beta, the bias
 * corrections) are formed in double and rounded to fp32 once, as torch does.  step_dev (optional): DEVICE float holding the
 * step count (torch's capturable-Adam convention); when given it overrides `step` and the bias corrections are computed on
 * the device, so a captured hipGraph advances correctly on every replay.  lr_dev (optional, only with step_dev): DEVICE
 * float holding the learning rate, read at run time instead of `lr` -- a scheduler (the reference uses ReduceLROnPlateau,
 * main_bayesian.py:118) can then change the rate of an already captured step.
 */
int bbb_adam_step(const bbb_adam_segment_t* segs, int nseg, double lr, double beta1, double beta2, double eps,
                  int64_t step, const float* step_dev, const float* lr_dev, void* stream);
/* What bbb_adam_step launches for these arguments (additive to ABI 13; host only, needs no device: tests): the entry's own plan
 * (csrc/adam_plan.h), without the launch.  Addresses are only looked at.  *chunks: blocks of 1024 elements, at most 2^31 - 1 (more:
 * BBB_ESHAPE); chunk_begin[17]: first block of segment s, [nseg .. 16] = *chunks; scalars[7]: the host path's fp32 step_size =
 * lr / (1 - beta1^step), sqrt(1 - beta2^step), beta1, beta2, 1 - beta1, 1 - beta2, eps, each formed in double and rounded once (with
 * step_dev the kernel forms the first two itself; they are then those of max(step, 1)); vec[16]: 1 where a segment's four pointers
 * are jointly 16-byte aligned and n >= 4, so that some thread moves 16 bytes at a time.  Returns what the launch entry returns before
 * its launch; a refusal writes zeros.  Out-pointers may be NULL. */
int bbb_adam_step_plan(const bbb_adam_segment_t* segs, int nseg, double lr, double beta1, double beta2, double eps,
                       int64_t step, const float* step_dev, const float* lr_dev, int32_t* chunks, int32_t* chunk_begin,
                       float* scalars, int32_t* vec);

/*
 * Global gradient norm for clipping and for the non-finite guard (training extension, additive to ABI 13; csrc/grad_norm.hip).
 *   norm = fp32(sqrt(sum over every element of every tensor of double(g)^2)): every square and every partial sum is float64, the
 *   root is float64, ONE rounding to fp32.  Range-free: 1537 gradients of 1e30 give 3.9e31, of 1e-30 give 3.9e-29.  Any NaN gives
 *   NaN; +-Inf without a NaN gives +Inf.
 * bbb_grad_sumsq: up to BBB_MAX_SEGMENTS segments, of which ONLY grad and n are read (the other pointers may be anything).  One
 *   256-thread block per 4096-element chunk of a segment writes that chunk's sum of squares to partials[first + chunk] (device
 *   float64, 8-byte aligned).  A tensor list longer than 16 takes several launches with `first` advanced by the chunks before it.
 *   A chunk's partial is a fixed tree over its elements and does not depend on the alignment of grad (the 16-byte path differs in
 *   the loads only).  Nothing else is written.  Checks: BBB_EINVAL (null segs / partials / grad, nseg outside 1..16, n <= 0,
 *   first < 0), BBB_EALIGN (partials not 8-byte, grad not 4-byte aligned), BBB_ESHAPE (first + chunks above 2^31 - 1).
 * bbb_grad_norm_finish: ONE block sums partials[0 .. npartials) in index order as a fixed tree in float64 and writes
 *   *norm_out = the fp32 norm;
 *   *coef_out = fp32(min(1, max_norm / (double(norm) + 1e-6))) -- torch.nn.utils.clip_grad_norm_'s coefficient, evaluated in double on
 *               the fp32 norm and rounded once; the comparison is written out, so a NaN norm gives NaN (not 1), an Inf norm 0, and
 *               the value is exactly 1.0f when nothing is clipped.  max_norm = +inf is "norm only": 1 unless the norm is NaN;
 *   *ok_out   = 0.0f when skip != 0 and the norm is not finite, else 1.0f;
 *   *skipped_out += 1 (device int32) when skip != 0 and the norm is not finite.
 *   coef_out, ok_out and skipped_out may be NULL.  Checks: BBB_EINVAL (null partials / norm_out, npartials <= 0), BBB_EALIGN
 *   (partials not 8-byte, an output not 4-byte aligned), BBB_EINVAL (max_norm <= 0 or NaN), BBB_ESHAPE (npartials above 2^31 - 1).
 * The reduction across workgroups happens at the launch boundary between the two: no ticket, counter, spin or atomic, so neither
 * launch can wait on anything, and the result is bitwise reproducible -- it depends on the values and the ORDER of the tensors only,
 * not on how they are dealt to launches.  Both launches are legal inside a stream capture.
 * The _plan entries are host only and need no device: the sumsq plan reports *chunks, chunk_begin[17] and vec[16] (1: grad 16-byte
 * aligned and n >= 4) and writes zeros on a refusal; the finish plan returns the finish launch's code and, when `coef` is not NULL,
 * the coefficient it would write for the fp32 norm `norm` (0 on a refusal).
 */
int bbb_grad_sumsq(const bbb_adam_segment_t* segs, int nseg, double* partials, int64_t first, void* stream);
int bbb_grad_sumsq_plan(const bbb_adam_segment_t* segs, int nseg, const double* partials, int64_t first, int32_t* chunks,
                        int32_t* chunk_begin, int32_t* vec);
int bbb_grad_norm_finish(const double* partials, int64_t npartials, double max_norm, int skip, float* norm_out, float* coef_out,
                         float* ok_out, int32_t* skipped_out, void* stream);
int bbb_grad_norm_finish_plan(const double* partials, int64_t npartials, double max_norm, const float* norm_out, const float* coef_out,
                              const float* ok_out, const int32_t* skipped_out, float norm, float* coef);

/*
 * bbb_adam_step with weight decay, a clip coefficient and a skip flag (additive to ABI 13).  Per element, each line of bbb_adam_step
 * in its own operation order, preceded by
 *   g1 = coef * g                        one fp32 rounding; only with coef_dev (DEVICE float, e.g. bbb_grad_norm_finish's coef_out)
 *   decoupled != 0:  p0 = p * decay      decay = fp32(1 - lr * weight_decay) formed in double (torch: param.mul_(1 - lr * wd));
 *                                        with lr_dev the kernel forms it from the device rate, as it does step_size
 *   decoupled == 0:  g1 = g1 + wd32 * p  wd32 = fp32(weight_decay), two roundings (torch: grad.add(param, alpha = wd))
 * and then m' = m + (g1 - m)(1 - beta1), v' = v beta2 + (1 - beta2) g1 g1, p' = p0 - step_size (m' / (sqrt(v') / sqrt_bc2 + eps)).
 * weight_decay == 0 applies neither form.  ok_dev (DEVICE float, optional): when it holds 0 the launch stores NOTHING -- parameters
 * and both moments stay bit for bit (a skipped step; the caller keeps the step count).  grad is never written: unlike
 * torch.nn.utils.clip_grad_norm_, clipping scales the gradient on its way into the update and leaves the tensor as it is.
 * With weight_decay = 0, coef_dev = NULL and ok_dev = NULL -- or with both pointing at 1.0f -- the results are bbb_adam_step's bits
 * (one kernel body, compile-time switches).  Checks: all of bbb_adam_step's in its order, then coef_dev / ok_dev 4-byte aligned
 * (BBB_EALIGN), then weight_decay >= 0 and not NaN (BBB_EINVAL).
 * bbb_adam_step_ex_plan: as bbb_adam_step_plan; scalars[9] = its seven, then wd32 and decay; *mode = 0 (no decay), 1 (L2), 2 (decoupled).
 */
int bbb_adam_step_ex(const bbb_adam_segment_t* segs, int nseg, double lr, double beta1, double beta2, double eps,
                     double weight_decay, int decoupled, int64_t step, const float* step_dev, const float* lr_dev,
                     const float* coef_dev, const float* ok_dev, void* stream);
int bbb_adam_step_ex_plan(const bbb_adam_segment_t* segs, int nseg, double lr, double beta1, double beta2, double eps,
                          double weight_decay, int decoupled, int64_t step, const float* step_dev, const float* lr_dev,
                          const float* coef_dev, const float* ok_dev, int32_t* chunks, int32_t* chunk_begin, float* scalars,
                          int32_t* vec, int32_t* mode);

/* Test entry: materialise n elements of a noise stream starting at element `start`. */
int bbb_eps_dump(float* out, int64_t n, int64_t start, uint64_t seed, uint32_t call, uint32_t stream_id, void* stream);

/* Geometry of one conv2d / linear contraction, batched over Monte-Carlo draws.
 * Every entry that takes one makes the same checks on it first (csrc/conv_desc_check.h): sizes, strides and dilations are positive
 * and paddings non-negative (BBB_EINVAL); the output map ho = (h + 2 pad_h - dil_h (kh - 1) - 1) / stride_h + 1 (wo alike) exists and
 * fits an int (BBB_ESHAPE).  A kernel that reaches past the padded input -- h + 2 pad_h - dil_h (kh - 1) - 1 < 0 on either axis --
 * has no output pixel and is BBB_ESHAPE in EVERY entry, whatever the stride (before this rule only bbb_conv2d_chwn_fwd and its
 * split / LRT forms refused it; the others let C's division round the negative numerator towards zero and computed one row). */
typedef struct bbb_conv_desc {
    int32_t batch;        /* B images per draw */
    int32_t cin, h, w;    /* input  [draws|1][B][cin][h][w]  (linear: h = w = 1) */
    int32_t cout, kh, kw; /* weight [draws|1][cout][cin][kh][kw] */
    int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int32_t draws;        /* E: independent weight sets / output slabs */
    int64_t x_draw_stride; /* elements between draws of x (0 = every draw reads the same x) */
    int64_t w_draw_stride; /* elements between draws of w (0 = shared weights) */
    int64_t b_draw_stride; /* elements between draws of bias (0 = shared) */
    int32_t act;          /* fused epilogue: 0 none, 1 ReLU, 2 Softplus(beta=1, threshold=20).  A NaN pre-activation gives a NaN, as
                             torch.relu / F.softplus do (never 0 or 20); +Inf stays +Inf, -Inf becomes 0. */
    /* Work units for ensemble sharding (batch-innermost entry points only; all zero = every slab is a whole draw).
     * With unit_div = S > 1 the `draws` slabs of a launch are UNITS u = unit_off + e of the draw-major grid
     * (Monte-Carlo draw, batch slice): draw = u / S, slice = u % S, `batch` = images per slice.  Slab e then reads
     * weight / bias set (u / S) - (unit_off / S) ... i.e. (unit_off % S + e) / S relative to the first set passed in,
     * writes output slab e, and reads input slab e -- or, with x_unit_mod = S (a layer whose input is the same for every
     * draw), input slab u % S of an [S][cin][h][w][batch] tensor.  unit_off is passed already reduced modulo S. */
    int32_t unit_div;
    int32_t unit_off;
    int32_t x_unit_mod;
    int32_t w_row_pitch;  /* fp32 batch-innermost entry only: elements between consecutive output-channel rows of w (0 = dense,
                             cin*kh*kw).  Lets a launch contract over a K-slice of a wider matrix in place (split-K over draws). */
    int32_t b_offset;     /* LRT noise only: global index of local image 0 (batch-parallel shards), added to the image index
                             that keys the activation noise; a unit's slice adds slice * batch on top */
    int32_t x_unit_div;   /* batch-innermost entry points (ABI 8).  D > 1: output slab e reads INPUT slab e / D (x holds draws / D
                             slabs at x_draw_stride) -- several Monte-Carlo steps in one launch: slab e = step e / D, draw e % D,
                             the first layer's input being the same for all D draws of a step.  Weight / bias set: e, as usual.
                             0 / 1: input slab e.  Not combined with work units (unit_div > 1). */
    int32_t x_unit_off;   /* with x_unit_div = D > 1: output slab e reads input slab (e + x_unit_off) / D, 0 <= x_unit_off < D -- a
                             rank's share of a GROUP of steps starts in the middle of a step (draws x_unit_off .. D-1 of its first
                             step); x then holds ceil((draws + x_unit_off) / D) slabs and draws need not be a multiple of D. */
    int32_t pool;         /* 1 (bbb_conv2d_chwn_fwd only): the layer is followed by [activation ->] MaxPool2d(kernel 2, stride 2)
                             and the launch writes the POOLED map y[draws][cout][ho/2][wo/2][batch] -- one workgroup walks the four
                             conv pixels of a pooling window and keeps the running maximum of act(conv + bias) in registers; bit
                             for bit bbb_maxpool_chwn(bbb_conv2d_chwn_fwd(...), 2, 2).  Needs even ho and wo and a layer without a
                             split contraction (bbb_conv2d_chwn_splitk_scratch reports k_split 1), else BBB_EINVAL; items are four
                             times fewer and four times longer, so it pays for launches that still spread evenly over the chip
                             (the callers decide: bbb_hip/ops.py pool_fusion_ok).  0: none.
                             bbb_conv2d_chwn_bf16_fwd (ABI 9): 1 = MaxPool2d(2, 2), (k << 8) | s = MaxPool2d(k, s); admitted: 2 / 2
                             and 3 / 2, for first layers with a row pitch <= 128 (weights in registers: 3Conv3FC conv1, LeNet
                             conv1) -> y [draws][cout][hp][wp][B]; the maximum is taken over the fp32 contraction results, then
                             bias, activation and the bf16 rounding once per pooled pixel (non-decreasing: the same values as
                             bbb_maxpool_chwn_bf16 of the unfused launch). */
    int32_t w_tap_major;  /* fp32 batch-innermost entries (bbb_conv2d_chwn_fwd, _splitk_fwd, the LRT forms; ABI 13): 1 = w rows are
                             [kh][kw][cin] instead of [cin][kh][kw] AND the contraction runs tap-major (in-bounds taps outermost, cin
                             innermost) -- the same products, summed in another order.  Training extension: the role-swapped weight
                             gradient reads the output gradient [cout][ho][wo][batch] in place as such a weight operand (no
                             transposed copy).  Elsewhere it must be 0. */
} bbb_conv_desc_t;

/*
 * y[e] = conv2d(x[e], w[e], bias[e]) on the fp32 matrix cores (implicit im2col GEMM, groups = 1).
 * Replaces F.conv2d / F.linear in layers/BBB/BBBConv.py:77 and layers/BBB/BBBLinear.py:70.
 * y: [draws][B][cout][ho][wo], contiguous.  bias may be NULL.
 */
int bbb_conv2d_fwd(const bbb_conv_desc_t* d, const float* x, const float* w, const float* bias,
                   float* y, void* stream);

/*
 * Local-reparameterisation layer in one launch (layers/BBB_LRT/BBBConv.py:71-81, BBBLinear.py:65-73):
 *   act_mu  = conv(x, w_mu, b_mu);  act_var = 1e-16 + conv(x*x, w_var, b_var)
 *   y       = act_mu + sqrt(act_var) * eps          (sample != 0)   |   act_mu   (sample == 0)
 * Both contractions share one staged x tile (squared in registers); eps is generated in the epilogue,
 * element index ((b*cout + c)*ho + oh)*wo + ow of stream (seed, call0 + e, stream_id).  Here d->draws
 * slabs of x are independent samples sharing w_mu / w_var (w_draw_stride must be 0).
 *   eps_ext   test entry: external noise with y's layout (NULL = Philox)
 *   act_mu_out / act_var_out: optional copies of the two moments (NULL = skip)
 */
int bbb_lrt_conv2d_fwd(const bbb_conv_desc_t* d, const float* x, const float* w_mu, const float* w_var,
                       const float* b_mu, const float* b_var, float* y,
                       float* act_mu_out, float* act_var_out, const float* eps_ext,
                       uint64_t seed, uint32_t call0, uint32_t stream_id, int sample,
                       const uint32_t* call_dev, void* stream);

/* What bbb_conv2d_fwd (lrt == 0) or bbb_lrt_conv2d_fwd (lrt != 0) launches for d (additive to ABI 13; host only, needs no device:
 * tests, profiling): the entries' own plan (csrc/conv_gemm_plan.h).  *bm: output pixels per workgroup, 128 when
 * ceil(batch ho wo / 128) * ceil(cout / 64) * draws >= 768, else 64; *linear: 1 for 1 x 1 taps on a 1 x 1 map without padding (x is
 * read as the row-major [batch][cin] matrix it is); *bk: k per staged tile, 32 | 16 (LRT); *k_tiles = ceil(cin kh kw / bk);
 * grid = (ceil(batch ho wo / bm), ceil(cout / 64), draws).  Returns the code the launch entry returns for d and valid, 4-byte
 * aligned operands: 0, BBB_EINVAL or BBB_ESHAPE (LRT: a weight or bias draw stride is BBB_EINVAL); a refusal writes nothing.  Any
 * out-pointer may be NULL. */
int bbb_conv2d_fwd_plan(const bbb_conv_desc_t* d, int lrt, int32_t* bm, int32_t* linear, int32_t* bk, int32_t* k_tiles,
                        int32_t grid[3]);

/*
 * Batch-innermost ("CHWN") variants used by the batched Monte-Carlo ensemble path.
 *   x: [draws|1][cin][h][w][B]   y: [draws][cout][ho][wo][B]   (B = d->batch, B % 4 == 0, 16-byte aligned)
 * Same contraction and same results as bbb_conv2d_fwd / bbb_lrt_conv2d_fwd (weights keep the reference's
 * [cout][cin][kh][kw] layout); one workgroup per (output pixel, 64 channels, 64|128 images) and kernel taps
 * that fall into the zero padding are skipped instead of multiplied.  LRT eps is indexed by the canonical
 * NCHW element index, so both layouts consume the identical noise stream.
 */
int bbb_conv2d_chwn_fwd(const bbb_conv_desc_t* d, const float* x, const float* w, const float* bias,
                        float* y, void* stream);
/* The same launch with the contraction on the 16-bit matrix pipe at fp32 accuracy, RANGE-FREE ("split bf16", ABI 8): every fp32
 * operand element is cut into hi = bf16(a), mid = bf16(a - hi), lo = bf16(a - hi - mid) (a = hi + mid + lo exactly; bf16 has
 * fp32's exponent range: no operand scales, windows or saturation) and every product is
 * lo*hi + hi*lo + mid*mid + mid*hi + hi*mid + hi*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- the dropped terms are
 * < 2^-23 |a b|.  Same descriptor as bbb_conv2d_chwn_fwd (work units, x_unit_div, w_row_pitch included); not bit-identical to it.
 * Opt-in (ops.gemm_mode = "bf16x3").  Operands must be finite.
 * flags = 0: x and y are the fp32 tensors of bbb_conv2d_chwn_fwd (operands are cut while their tiles are staged).
 * BBB_S3_IN / BBB_S3_OUT: x / y travel in the split ACTIVATION format "S3" -- three bf16 planes per slab,
 * [draws|1][3][C][H][W][B] (batch % 8 == 0, 16-byte aligned; d->x_draw_stride then counts bf16 elements, 3*C*H*W*B per slab or
 * 0 = shared) -- the exact fp32 values stored as their three pieces, written once by the producing launch and staged by the
 * consumer without arithmetic (the kernel is bound by the VALU work of the split otherwise).  bbb_maxpool_chwn_s3 pools S3
 * tensors; bbb_s3_convert converts fp32 <-> S3 (both exact). */
#define BBB_S3_IN  1u
#define BBB_S3_OUT 2u
int bbb_conv2d_chwn_bf16x3_fwd(const bbb_conv_desc_t* d, const void* x, const float* w, const float* bias, void* y, uint32_t flags,
                               void* stream);
/* nn.MaxPool2d(k, s) on an S3 tensor [slabs][3][channels][h][w][batch] -> [slabs][3][channels][ho][wo][batch]: the S3 form of what
 * bbb_maxpool_chwn computes on the fp32 values. */
int bbb_maxpool_chwn_s3(const void* x, void* y, int64_t slabs, int channels, int h, int w, int batch, int k, int s, void* stream);
/* fp32 [slabs][n] -> S3 [slabs][3][n] (to_s3 != 0) or back (to_s3 == 0); n % 8 == 0; exact in both directions. */
int bbb_s3_convert(const void* src, void* dst, int64_t slabs, int64_t n, int to_s3, void* stream);
/*
 * The split-bf16 contraction over MFMA-READY operands (ABI 11): same arithmetic as bbb_conv2d_chwn_bf16x3_fwd (three bf16 pieces per
 * fp32 element, six products per fp32 product, fp32 accumulation, in-bounds taps only), with both operands laid out the way
 * v_mfma_f32_32x32x16_bf16 wants them, so that the k loop holds no operand arithmetic, no transposing LDS reads and no LDS traffic
 * on the image side:
 *   x: "c8 S3" activations, bf16 [draws|1][3][cin / 8][h][w][B][8] -- the hi / mid / lo pieces (exact: hi + mid + lo is the fp32
 *      value) of the 8 channels 8g .. 8g + 7 of an image are 16 adjacent bytes of a plane = one lane's B operand.  cin % 16 == 0,
 *      B % 4 == 0, 16-byte aligned; d->x_draw_stride counts bf16 elements (3 * cin * h * w * B per slab, or 0 = shared).
 *   w: fp32, TAP-MAJOR rows [draws|1][cout][kh * kw][cin] -- what bbb_reparam_kl_fwd writes for a segment with w_tm_cin = cin,
 *      w_taps = kh * kw (bbb_w_tap_major converts a dense tensor); 16-byte aligned, draw strides multiples of 4 elements.
 *   y: c8 S3 [draws][3][cout / 8][ho][wo][B][8] (cout % 8 == 0), or with BBB_C8X3_OUT_F32 the fp32 batch-innermost tensor
 *      [draws][cout][ho][wo][B] of bbb_conv2d_chwn_fwd (the logits layer).
 * Work units / x_unit_div as in bbb_conv2d_chwn_fwd; d->pool and d->w_row_pitch must be 0.  bbb_maxpool_chwn_s3 pools c8 S3 tensors
 * (channels = cin / 8, batch = 8 * B: the window maximum is element-wise on 16-byte vectors); bbb_c8s3_convert converts
 * fp32 batch-innermost [slabs][channels][positions][batch] <-> c8 S3 (exact both ways).  Replaces F.conv2d / F.linear of
 * layers/BBB/BBBConv.py:77, layers/BBB/BBBLinear.py:70; every slab (three planes) must stay below 1 GiB.
 * BBB_C8X3_TILE128 / _TILE256 force the images per workgroup and the BBB_C8X3_NT bits the channels per workgroup (default: by layer
 * and launch size); the MFMA sequence per output element, hence every output bit, is the same for all of them.
 */
#define BBB_C8X3_OUT_F32 1u
#define BBB_C8X3_TILE128 2u
#define BBB_C8X3_TILE256 4u
#define BBB_C8X3_POOL 8u          /* the launch also applies MaxPool2d(2, 2) to the activated output ("parallel window": the four waves of a
                                     workgroup own the four pixels of a window).  pad == 0, even ho and wo, c8 S3 output
                                     [draws][3][cout / 8][ho / 2][wo / 2][B][8]; bit for bit the plain launch + bbb_maxpool_chwn_s3(2, 2).
                                     TILE128 / TILE256 then mean 32 / 64 images per workgroup. */
#define BBB_C8X3_NT_SHIFT 4       /* bits 4..6: force the channels per workgroup, 32 * NT with NT = 2, 3 or 4 (0: by layer and launch size) */
#define BBB_C8X3_NT_MASK 0x70u
/* bits 8..23: four nibbles = leading rows, leading columns, trailing rows, trailing columns of the INPUT map that are all zero (the
 * materialised padding of a bbb_s2d_c8s3 block image): their products are exact zeros and are not computed -- same result as
 * computing them, less work.  A promise of the caller: non-zero data there is silently ignored. */
#define BBB_C8X3_ZERO_LEAD_H(n) (((uint32_t)(n) & 15u) << 8)
#define BBB_C8X3_ZERO_LEAD_W(n) (((uint32_t)(n) & 15u) << 12)
#define BBB_C8X3_ZERO_TRAIL_H(n) (((uint32_t)(n) & 15u) << 16)
#define BBB_C8X3_ZERO_TRAIL_W(n) (((uint32_t)(n) & 15u) << 20)
#define BBB_C8X3_ZERO_MASK 0x00FFFF00u
int bbb_conv2d_c8x3_fwd(const bbb_conv_desc_t* d, const void* x, const float* w, const float* bias, void* y, uint32_t flags,
                        void* stream);
/* to_c8s3: 1 = fp32 -> c8 S3, 0 = back; 2 = fp32 -> six planes (values + squares), 3 = six planes -> fp32 (the LRT chain's slabs) */
int bbb_c8s3_convert(const void* src, void* dst, int64_t slabs, int channels, int64_t positions, int batch, int to_c8s3, void* stream);
/*
 * The LRT form of the same contraction (ABI 12; layers/BBB_LRT/BBBConv.py:62-87, BBBLinear.py:56-79 in the split-bf16 mode):
 *   act_mu = conv(x, w_mu) + b_mu,  act_var = 1e-16 + conv(x^2, w_var) + b_var,  y = act(act_mu + sqrt(act_var) * eps)
 * with both contractions on v_mfma_f32_32x32x16_bf16 (two weight tiles, two sets of image fragments and accumulators per
 * workgroup) and eps drawn in the epilogue exactly as bbb_lrt_conv2d_chwn_fwd draws it (element index of the output's canonical
 * [B][cout][ho][wo] slab, stream (seed, call0 + draw, stream_id); d->b_offset and work units key the GLOBAL image index).
 *   x, y: SIX-plane c8 S3 slabs [draws|1][6][c / 8][h][w][B][8] -- the three pieces of the values, then the three pieces of their
 *      squares (squared in fp32 by whoever writes the slab: this launch's epilogue, bbb_maxpool_chwn_s3sq, bbb_s2d_c8s3sq,
 *      bbb_c8s3_convert mode 2); d->x_draw_stride counts bf16 elements (6 * cin * h * w * B per slab, or 0 = shared).
 *      With BBB_C8X3_OUT_F32, y is the fp32 tensor [draws][cout][ho][wo][B] (the logits layer).
 *   w_mu, w_var: fp32 tap-major [cout][kh * kw][cin], shared by the slabs (d->w_draw_stride == d->b_draw_stride == 0).
 * flags: BBB_C8X3_OUT_F32, BBB_C8X3_TILE128 / _TILE256, BBB_C8X3_ZERO_*; no pooled form.  sample == 0: y = act(act_mu).
 * bbb_maxpool_chwn_s3sq pools six-plane slabs (maximum over the values; the squares are those of the pooled values);
 * bbb_s2d_c8s3sq is bbb_s2d_c8s3 with the squares' planes behind; bbb_c8s3_convert modes 2 / 3 convert fp32 <-> six planes.
 */
int bbb_lrt_conv2d_c8x3_fwd(const bbb_conv_desc_t* d, const void* x, const float* w_mu, const float* w_var, const float* b_mu,
                            const float* b_var, void* y, uint64_t seed, uint32_t call0, uint32_t stream_id, int sample,
                            const uint32_t* call_dev, uint32_t flags, void* stream);
/*
 * bbb_conv2d_c8x3_plan: which of its 20 kernel instantiations bbb_conv2d_c8x3_fwd (lrt == 0) or bbb_lrt_conv2d_c8x3_fwd (lrt != 0)
 * starts for this descriptor and flags word.  Host only: launches nothing, needs no device.  *form: BBB_C8X3_FORM_*; *nt: 32-channel
 * tiles per workgroup (2 | 3 | 4); *images_per_wg: 128 | 256 (pooled: 32 | 64); *items: work items; *blocks: workgroups (items rounded
 * up to 8).  Out-pointers may be NULL.  Returns 0 or what the launch entry returns for every check that does not involve an operand
 * pointer; the two call the same plan (csrc/pconv_c8x3_plan.h).
 * Forms: ((NT - 2) * 2 + (MT - 1)) * 3 + output, MT = 32-image fragments per wave, output 0 = c8 S3, 1 = fp32, 2 = pooled c8 S3;
 * then the two LRT instantiations (NT 2, MT 1).
 */
#define BBB_C8X3_FORM_NT2_MT1_S3 0
#define BBB_C8X3_FORM_NT2_MT1_F32 1
#define BBB_C8X3_FORM_NT2_MT1_POOL 2
#define BBB_C8X3_FORM_NT2_MT2_S3 3
#define BBB_C8X3_FORM_NT2_MT2_F32 4
#define BBB_C8X3_FORM_NT2_MT2_POOL 5
#define BBB_C8X3_FORM_NT3_MT1_S3 6
#define BBB_C8X3_FORM_NT3_MT1_F32 7
#define BBB_C8X3_FORM_NT3_MT1_POOL 8
#define BBB_C8X3_FORM_NT3_MT2_S3 9
#define BBB_C8X3_FORM_NT3_MT2_F32 10
#define BBB_C8X3_FORM_NT3_MT2_POOL 11
#define BBB_C8X3_FORM_NT4_MT1_S3 12
#define BBB_C8X3_FORM_NT4_MT1_F32 13
#define BBB_C8X3_FORM_NT4_MT1_POOL 14
#define BBB_C8X3_FORM_NT4_MT2_S3 15
#define BBB_C8X3_FORM_NT4_MT2_F32 16
#define BBB_C8X3_FORM_NT4_MT2_POOL 17
#define BBB_C8X3_FORM_LRT_S3 18
#define BBB_C8X3_FORM_LRT_F32 19
int bbb_conv2d_c8x3_plan(const bbb_conv_desc_t* d, uint32_t flags, int lrt, int32_t* form, int32_t* nt, int32_t* images_per_wg,
                         int64_t* items, int64_t* blocks);
int bbb_maxpool_chwn_s3sq(const void* x, void* y, int64_t slabs, int channels, int h, int w, int batch, int k, int s, void* stream);
int bbb_s2d_c8s3sq(const float* x, void* y, int64_t blocks, int batch, int channels, int h, int w, int k, int stride, int pad, void* stream);
/*
 * Space-to-depth operands (ABI 12): a strided layer with few input channels (AlexNet conv1: 3 channels, 11 x 11, stride 4, padding 5 --
 * models/BayesianModels/BayesianAlexNet.py:33) as a layer bbb_conv2d_c8x3_fwd can take.  With m = ceil(k / stride) it is the m x m
 * convolution, stride 1, no padding, of the block image x'[(c s + dy) s + dx][bh][bw] = xpad[c][s bh + dy][s bw + dx] with weights
 * w'[(mr, mq)][(c s + dy) s + dx] = w[c][s mr + dy][s mq + dx] (zero outside the k x k taps); C' = channels * stride^2 rounded up to a
 * multiple of 16.  Same products as F.conv2d(x, w, stride, padding) of layers/BBB/BBBConv.py:77 plus exact zeros.
 * bbb_s2d_c8s3: the caller's NCHW fp32 batch [blocks * batch][channels][h][w] -> c8 S3 [blocks][3][C' / 8][ho + m - 1][wo + m - 1][batch][8]
 * (one block per batch slice / per step of a launch); bbb_w_s2d_tap_major: w [rows][channels][k][k] -> [rows][m * m][C'].
 */
int bbb_s2d_c8s3(const float* x, void* y, int64_t blocks, int batch, int channels, int h, int w, int k, int stride, int pad, void* stream);
int bbb_w_s2d_tap_major(const float* w, float* out, int64_t rows, int channels, int k, int stride, void* stream);
/* w [rows][cin][taps] -> out [rows][taps][cin] (rows = draws * cout): the tap-major weight layout from the reference's. */
int bbb_w_tap_major(const float* w, float* out, int64_t rows, int cin, int taps, void* stream);
int bbb_lrt_conv2d_chwn_fwd(const bbb_conv_desc_t* d, const float* x, const float* w_mu, const float* w_var,
                            const float* b_mu, const float* b_var, float* y,
                            float* act_mu_out, float* act_var_out, const float* eps_ext,
                            uint64_t seed, uint32_t call0, uint32_t stream_id, int sample,
                            const uint32_t* call_dev, void* stream);

/*
 * Split-contraction forms of the two batch-innermost entry points above (ABI 6; a property of the LAYER since ABI 8).
 * A draw of a late AlexNet layer is a few dozen workgroups, each bounded by its serial k loop (conv4: 48 tiles of 32 k on 128 of
 * the 256 CUs).  For such layers -- at most 16 (output pixel, 64-channel tile) groups and at least 16 k tiles; the plan depends on
 * the layer's GEOMETRY only, never on batch, draws or work units -- the contraction of every output tile is cut into k_split = 2..4
 * consecutive k ranges whose partial sums are added in range order: ((p0 + p1) + p2) + p3.  Two executions of that one
 * definition, chosen by launch size, same bits:
 *   - across workgroups (launches of <= 384 items of 64 images, when scratch is given): each range is its own workgroup, partial
 *     accumulator tiles go to `scratch`, the last arriver adds them in range order, applies bias / activation / the LRT sampling
 *     step and stores y;
 *   - inside one workgroup (any other launch; no scratch needed): the k loop restarts its accumulator at every range boundary.
 * So one draw computed alone, the same draw inside a 10-draw launch, as a work unit of a sharded step or as one of several steps
 * per launch is the same number, bit for bit.  Against the UNSPLIT chain of bbb_conv2d_chwn_fwd the partial sums round
 * separately: ~1e-7 relative, 1-2e-6 of max|logit| through a model.
 *   bbb_conv2d_chwn_splitk_scratch: the layer's plan -> *k_split (1 = no split: same as the plain entry point) and the scratch
 *     bytes THIS launch (d->draws, d->batch) needs for the cross-workgroup form (0: it runs the in-workgroup form).
 *     lrt != 0: sizes for the LRT entry point (two accumulator sets).
 *   scratch: device memory, 256-byte aligned, ZERO-FILLED before its first use (arrival tickets live at its start and every
 *     launch leaves them zero again); one scratch buffer per stream in flight; NULL = always the in-workgroup form.
 * k_split must be the planned value (BBB_EINVAL otherwise); k_split <= 1 behaves exactly like the plain entry point.
 */
int64_t bbb_conv2d_chwn_splitk_scratch(const bbb_conv_desc_t* d, int lrt, int32_t* k_split);
int bbb_conv2d_chwn_splitk_fwd(const bbb_conv_desc_t* d, const float* x, const float* w, const float* bias, float* y,
                               int k_split, void* scratch, int64_t scratch_bytes, void* stream);
int bbb_lrt_conv2d_chwn_splitk_fwd(const bbb_conv_desc_t* d, const float* x, const float* w_mu, const float* w_var,
                                   const float* b_mu, const float* b_var, float* y,
                                   float* act_mu_out, float* act_var_out, const float* eps_ext,
                                   uint64_t seed, uint32_t call0, uint32_t stream_id, int sample,
                                   const uint32_t* call_dev, int k_split, void* scratch, int64_t scratch_bytes, void* stream);
/*
 * bbb_conv2d_chwn_plan: which launch form bbb_conv2d_chwn_fwd / _splitk_fwd (lrt == 0) or bbb_lrt_conv2d_chwn_fwd / _splitk_fwd
 * (lrt != 0) takes for this descriptor, k_split as the launch would be given it and has_scratch != 0 when the launch would be
 * given enough scratch for the cross-workgroup form.  Host only: launches nothing, needs no device.  *form: BBB_FP32_FORM_*;
 * *bm: images per work item (64 | 128); *ilv: staging loads interleaved with the MFMAs; *items: work items; *blocks: workgroups
 * (the cross-workgroup split: items * k_split, rounded up to 8).  Out-pointers may be NULL.  Returns 0 or what the launch entry
 * returns for every check that does not involve an operand pointer; the two call the same plan (csrc/pconv_plan.h).
 */
#define BBB_FP32_FORM_64_ILV 0         /* pconv_gemm_kernel<64, false, ILV> */
#define BBB_FP32_FORM_64 1
#define BBB_FP32_FORM_128_ILV 2        /* 128-image tiles */
#define BBB_FP32_FORM_128 3
#define BBB_FP32_FORM_SEQ64_ILV 4      /* the layer's split inside one workgroup per item */
#define BBB_FP32_FORM_SEQ64 5
#define BBB_FP32_FORM_SEQ128_ILV 6
#define BBB_FP32_FORM_SEQ128 7
#define BBB_FP32_FORM_CROSS 8          /* ... across workgroups, through scratch */
#define BBB_FP32_FORM_POOL 9           /* d->pool: MaxPool2d(2, 2) inside the launch */
#define BBB_FP32_FORM_LRT64_ILV 10     /* the LRT kernel: 64-image tiles only */
#define BBB_FP32_FORM_LRT64 11
#define BBB_FP32_FORM_LRT_SEQ64 12
#define BBB_FP32_FORM_LRT_CROSS 13
#define BBB_FP32_FORM_LRT_POOL 14
int bbb_conv2d_chwn_plan(const bbb_conv_desc_t* d, int lrt, int k_split, int has_scratch, int32_t* form, int32_t* bm, int32_t* ilv,
                         int64_t* items, int64_t* blocks);

/*
 * Pooling on batch-innermost planes x [planes][h][w][B] -> y [planes][ho][wo][B] (csrc/pool2d.hip; bf16 planes: csrc/pool2d_bf16.hip),
 * one descriptor and one plan (csrc/pool_plan.h) for both kinds.  The output map is floor mode's, ho = (h + 2 pad_h - kh) / stride_h + 1.
 *   BBB_POOL_MAX  nn.MaxPool2d(kernel_size=k, stride=s) (no padding, floor mode; models/BayesianModels/BayesianAlexNet.py:37): a square
 *                 window, one stride, no padding, count_include_pad 0 -- what the maximum kernels implement.  Every maximum of the
 *                 forward (these entries, the S3 / c8 S3 pools and the pooled conv forms) keeps a NaN wherever it sits in the
 *                 window, as F.max_pool2d does.  Its launch entries take
 *                 scalars (bbb_maxpool_chwn, bbb_pool_act_bwd_chwn, bbb_lrt_pool_act_bwd_chwn, and on bf16 planes bbb_maxpool_chwn_bf16,
 *                 bbb_pool_act_bwd_chwn_bf16) and build this descriptor themselves; a backward's k = 0 (the activation alone) is
 *                 planned as the 1 x 1 window at stride 1.
 *   BBB_POOL_AVG  (additive to ABI 13) nn.AvgPool2d(kernel_size, stride, padding, ceil_mode=False, count_include_pad,
 *                 divisor_override=None) -- and nn.AdaptiveAvgPool2d on a map its output size divides, which is the window
 *                 (h / oh, w / ow) at the same stride without padding -- for models built from the layers package beyond the three
 *                 of the zoo (LeNet-style stacks, global-average-pool heads).  Its launch entries take the descriptor
 *                 (bbb_avgpool_*) and refuse any other kind as an unknown one (BBB_EINVAL).
 * What an entry checks, in order, by family (the plan: in the order bbb_avgpool_plan documents):
 *   forwards (bbb_maxpool_chwn, bbb_avgpool_chwn, and their _bf16 twins): null x / y (BBB_EINVAL); the plan; 16-byte alignment (BBB_EALIGN).
 *   fp32 backwards (bbb_pool_act_bwd_chwn, bbb_avgpool_act_bwd_chwn): null g_out / y / g_pre or an activation outside 0..2
 *     (BBB_EINVAL); the plan; alignment of the three (BBB_EALIGN).
 *   LRT backwards (bbb_lrt_pool_act_bwd_chwn, bbb_lrt_avgpool_act_bwd_chwn): FIRST null act_mu / act_var / g_var, then moment_planes
 *     (positive, dividing planes; both BBB_EINVAL), then the alignment of those three (BBB_EALIGN); then everything of the fp32
 *     backwards; last the g_out2 / x_out pair: both or neither, x_planes positive and dividing planes (BBB_EINVAL), their alignment.
 *   bf16 backwards (bbb_pool_act_bwd_chwn_bf16, bbb_avgpool_act_bwd_chwn_bf16): null g_out / g_pre, null y (the max entry: unless k = 0
 *     and act = 0) (BBB_EINVAL); the plan; alignment (BBB_EALIGN); then an activation outside 0..2 or unknown flag bits (BBB_EINVAL).
 * For the scalar entries every single violation is the code it always was, with one exception no memory reaches: the plan bounds the
 * forward AND the backward grid, so a max forward whose own grid fits an int while planes * h * w * B / group threads do not (over 8 TB
 * of input) is BBB_ESHAPE where it used to launch.  Where two violations coincide, the order above decides.
 */
#define BBB_POOL_AVG 1        /* bbb_pool_desc_t::kind (0 is not a kind) */
#define BBB_POOL_MAX 2
typedef struct bbb_pool_desc {
    int32_t kind;              /* BBB_POOL_AVG | BBB_POOL_MAX */
    int32_t h, w, batch;       /* the input map and the images per plane (batch % 4 == 0; % 8 on bf16 planes) */
    int32_t kh, kw;            /* window (BBB_POOL_MAX: kh == kw) */
    int32_t stride_h, stride_w;   /* (BBB_POOL_MAX: equal) */
    int32_t pad_h, pad_w;      /* zero padding, 2 * pad <= k on each axis (torch's rule: every window then holds a valid tap); BBB_POOL_MAX: 0 */
    int32_t count_include_pad; /* 1: the divisor is kh * kw; 0: the number of taps inside the map (BBB_POOL_MAX: 0) */
} bbb_pool_desc_t;

/* What the launches of this section do for a descriptor of either kind (host only, needs no device; the name dates from the average
 * pool, which it answered for first): the output map and the workgroups (256 threads, one per 16-byte group of 4 images) of the
 * forward and of the backward, or the code all of them refuse it with BEFORE anything is launched: BBB_EINVAL for a null descriptor,
 * an unknown kind, a non-positive size, a negative padding, a count_include_pad other than 0 / 1, or a BBB_POOL_MAX descriptor with
 * a rectangular window, two strides, a padding or count_include_pad 1; BBB_ESHAPE for batch % 4 != 0, 2 * pad > k on an axis, a
 * window larger than the padded map, or a grid that does not fit an int; BBB_EINVAL for an out_plane_pitch (the backward's, 0 =
 * dense) that is below h * w * batch or not a multiple of 4.  Out-pointers may be NULL. */
int bbb_avgpool_plan(const bbb_pool_desc_t* d, int64_t planes, int64_t out_plane_pitch, int32_t* ho, int32_t* wo, int64_t* fwd_blocks,
                     int64_t* bwd_blocks);

/* BBB_POOL_MAX forward: y [planes][(h-k)/s+1][(w-k)/s+1][B]. */
int bbb_maxpool_chwn(const float* x, float* y, int64_t planes, int h, int w, int batch, int k, int s, void* stream);

/*
 * Training extension: backward of [fused activation -> nn.MaxPool2d(k, s)] on batch-innermost planes (k = 0: activation only).
 *   y      [planes][h][w][B]   the layer's ACTIVATED output (what the forward GEMM stored)
 *   g_out  [planes][hp][wp][B] gradient w.r.t. the pooled output (k = 0: same shape as y)
 *   g_pre  [planes][h][w][B]   gradient w.r.t. the pre-activation: the first maximum of every window receives that window's
 *                              gradient (torch's max_pool2d backward), times act'(.) recovered from y (Softplus: 1 - exp(-y)).
 * Gather formulation: deterministic, handles overlapping windows (k > s).  out_plane_pitch (elements, multiple of 4; 0 = dense
 * h*w*B): pitch between the planes of g_pre -- the first layer's gradient is written straight into the padded-row matrix its
 * weight-gradient GEMM reads (rows of exactly 2^n bytes would all fall into one memory channel).
 */
int bbb_pool_act_bwd_chwn(const float* g_out, const float* y, float* g_pre, int64_t planes, int h, int w, int batch,
                          int k, int s, int act, int64_t out_plane_pitch, void* stream);

/*
 * The same pass for a local-reparameterisation layer (layers/BBB_LRT/BBBConv.py:71-81: out = act_mu + sqrt(act_var) * eps, then
 * the activation, then the pool): besides g_mu = the gradient w.r.t. act_mu (what bbb_pool_act_bwd_chwn calls g_pre) it writes
 *   g_var = g_mu * (v - act_mu) / (2 * act_var),   v = the pre-activation recovered from y (Softplus: y + log(1 - exp(-y)) below
 *           the threshold of 20; ReLU: y, and no gradient where y == 0; act = 0: y itself)
 * -- the gradient w.r.t. act_var, since sqrt(act_var) * eps = v - act_mu.  act_mu / act_var: [moment_planes][h][w][B] with
 * moment_planes == planes, or a divisor of it when consecutive groups of moment_planes planes (the draws of a first layer whose
 * input and weights every draw shares) were sampled from ONE pair of moments.  g_mu and g_var share out_plane_pitch.
 * g_out2 / x_out (both or neither; ABI 13): the incoming gradient is g_out + 2 * x_out * g_out2 -- the two input gradients of the
 * LRT layer above (through its mean and its variance weights) and this layer's output x_out [x_planes][hp][wp][B] (x_planes divides
 * planes), combined on the fly with bbb_lrt_glue mode 1's arithmetic instead of by a launch of its own.
 */
int bbb_lrt_pool_act_bwd_chwn(const float* g_out, const float* y, const float* act_mu, const float* act_var, float* g_mu,
                              float* g_var, int64_t planes, int64_t moment_planes, int h, int w, int batch, int k, int s, int act,
                              int64_t out_plane_pitch, const float* g_out2, const float* x_out, int64_t x_planes, void* stream);

/* x [planes][h][w][B] -> y [planes][ho][wo][B]: the taps of a window that lie inside the map are added in scan order (rows, then
 * columns) by plain fp32 adds, then divided ONCE (IEEE division) by the divisor.  The order depends on the window alone, so a
 * plane computed alone or among others is the same bits.  x, y 16-byte aligned. */
int bbb_avgpool_chwn(const bbb_pool_desc_t* d, const float* x, float* y, int64_t planes, void* stream);

/* Training extension: bbb_pool_act_bwd_chwn with the average pool's routing.  y [planes][h][w][B] the layer's ACTIVATED output,
 * g_out [planes][ho][wo][B]; g_pre(h, w) = act'(.) * sum of g_out(oh, ow) / divisor(oh, ow) over the windows that contain (h, w), in
 * ascending (oh, ow) order; elements no window covers receive 0.  Gather form: no atomics, deterministic.  act, out_plane_pitch and
 * the activation arithmetic as there. */
int bbb_avgpool_act_bwd_chwn(const bbb_pool_desc_t* d, const float* g_out, const float* y, float* g_pre, int64_t planes, int act,
                             int64_t out_plane_pitch, void* stream);

/* ... and bbb_lrt_pool_act_bwd_chwn with it, argument for argument: act_mu / act_var over moment_planes planes, g_var = g_mu *
 * (v - act_mu) / (2 act_var), the g_out2 / x_out combine of the incoming gradient. */
int bbb_lrt_avgpool_act_bwd_chwn(const bbb_pool_desc_t* d, const float* g_out, const float* y, const float* act_mu, const float* act_var,
                                 float* g_mu, float* g_var, int64_t planes, int64_t moment_planes, int act, int64_t out_plane_pitch,
                                 const float* g_out2, const float* x_out, int64_t x_planes, void* stream);

/*
 * Average pooling on bf16 planes (csrc/pool2d_bf16.hip, beside the maximum pool of that mode: bbb_maxpool_chwn_bf16,
 * bbb_pool_act_bwd_chwn_bf16; additive to ABI 13): the average pool of the bf16 storage mode, opt-in from Python
 * (LaunchConfig.bf16_avgpool).  The descriptor is the one above with batch % 8 == 0: a thread moves a 16-byte group of 8 images.
 *
 * bbb_avgpool_bf16_plan: bbb_avgpool_plan at that group width, for both kinds like it -- the same checks in the same order, BBB_ESHAPE for batch % 8 != 0,
 *   BBB_EINVAL for an out_plane_pitch that is not a multiple of 8 (csrc/pool_plan.h: plan_bf16).
 * bbb_avgpool_chwn_bf16: x [planes][h][w][B] bf16 -> y [planes][ho][wo][B] bf16.  The valid taps of a window are converted to fp32
 *   (exact), added in scan order (rows, then columns) by plain fp32 adds, divided ONCE (IEEE division) by bbb_avgpool_chwn's divisor,
 *   and the quotient is rounded ONCE to bf16, nearest-even.  The order depends on the window alone: a plane computed alone or among
 *   others is the same bits.
 * bbb_avgpool_act_bwd_chwn_bf16: bbb_avgpool_act_bwd_chwn's routing on bbb_pool_act_bwd_chwn_bf16's storage rules.  y
 *   [planes][h][w][B] the stored bf16 ACTIVATED output, g_out [planes][ho][wo][B] bf16 or, with BBB_BF16_BWD_G_F32, fp32;
 *   g_act(h, w) = the fp32 sum of g_out(oh, ow) / divisor(oh, ow) (each an IEEE division) over the windows that contain (h, w), in
 *   ascending (oh, ow); elements no window covers receive 0.  g_pre = g_act * act'(y) (ReLU [y > 0]; Softplus 1 - exp(-y), 1 above
 *   20), rounded once to bf16; with BBB_BF16_BWD_OUT_F32 written as the fp32 values of that rounding.  out_plane_pitch: 0 = dense,
 *   else elements (% 8 == 0).  Gather form: no atomics, deterministic.  There is no LRT form.
 * Both launches check, in this order: null pointers (BBB_EINVAL), the plan, 16-byte alignment of every pointer (BBB_EALIGN), then
 * act outside 0..2 or unknown flag bits (BBB_EINVAL).
 */
int bbb_avgpool_bf16_plan(const bbb_pool_desc_t* d, int64_t planes, int64_t out_plane_pitch, int32_t* ho, int32_t* wo,
                          int64_t* fwd_blocks, int64_t* bwd_blocks);
int bbb_avgpool_chwn_bf16(const bbb_pool_desc_t* d, const void* x, void* y, int64_t planes, void* stream);
int bbb_avgpool_act_bwd_chwn_bf16(const bbb_pool_desc_t* d, const void* g_out, const void* y, void* g_pre, int64_t planes, int act,
                                  int64_t out_plane_pitch, uint32_t flags, void* stream);

/*
 * E noise draws from ONE pair of LRT moments, batch-innermost: y[e] = act(act_mu + sqrt(act_var) * eps[e]) with eps exactly
 * as bbb_lrt_conv2d_chwn_fwd would have drawn it for draw e (layers/BBB_LRT/BBBConv.py:78-81).  For an LRT layer whose input
 * is the same for every draw (the first layer of a model) this replaces E identical pairs of contractions by one.
 *   act_mu, act_var: [channels][pixels][batch] (the act_mu_out / act_var_out of a draws = 1, sample = 0 launch)
 *   y: [draws][channels][pixels][batch]
 *   b_offset: global index of local image 0 (batch-parallel shards; bbb_conv_desc_t::b_offset of the GEMM form), ABI 6
 */
int bbb_lrt_sample_chwn(const float* act_mu, const float* act_var, float* y, int draws, int channels, int pixels, int batch,
                        int b_offset, int act, uint64_t seed, uint32_t call0, uint32_t stream_id, const uint32_t* call_dev,
                        void* stream);

/*
 * The LRT sampling step alone, reference layout: y = act_mu + sqrt(act_var) * eps over `draws` contiguous slabs of n
 * elements (layers/BBB_LRT/BBBConv.py:78-81), eps = element i of noise stream (seed, call0 + e, stream_id) -- the same
 * numbers bbb_lrt_conv2d_fwd draws.  Used by the training path, which computes the two moments with split-K launches.
 */
int bbb_lrt_sample_nchw(const float* act_mu, const float* act_var, float* y, int64_t n, int draws, uint64_t seed,
                        uint32_t call0, uint32_t stream_id, const uint32_t* call_dev, void* stream);

/*
 * BF16 storage variants of the batch-innermost path (BASELINE.json configs[1]: "BBB layers, bf16"); fp32 accumulation,
 * fp32 bias and fp32 epilogue (bias + activation), one rounding (nearest-even) when a value is stored as bf16.
 *   x: [draws|1][cin][h][w][B] bf16   (B % 8 == 0, 16-byte aligned, draw strides multiples of 8 elements)
 *   w: [draws|1][cout][Kp] bf16       K = cin*kh*kw, Kp = K rounded up to 8, pad columns zero -- what bbb_reparam_kl_fwd
 *                                     writes for a segment with w_row_len = K.  Column order inside a row: the reference's
 *                                     (ci, r, q), or with BBB_BF16_W_TAP_MAJOR (needs cin % 8 == 0) (r, q, ci) = a segment
 *                                     written with w_taps = kh*kw.  Tap-major rows let the kernel skip the kernel taps
 *                                     that fall into the zero padding (as the fp32 kernel does) and still move weights as
 *                                     16-byte vectors; with the reference order those taps are multiplied by zeros.
 *   y: [draws][cout][ho][wo][B]       bf16, or fp32 with BBB_BF16_OUT_F32 (the logits layer feeding bbb_mc_tail)
 * d->w_draw_stride counts bf16 elements (cout*Kp per draw when dense).  Same contraction as bbb_conv2d_chwn_fwd
 * (layers/BBB/BBBConv.py:77, BBBLinear.py:70) on v_mfma_f32_32x32x16_bf16.  BBB layers only (no LRT variant).
 * Channel-interleaved activations (ABI 10): [draws][C / 8][h][w][B][8] -- the 8 channels 8g .. 8g + 7 of an image are 16 adjacent
 * bytes, so a lane's MFMA operand (8 consecutive channels of one image) is ONE 16-byte load and a conv layer needs neither LDS
 * staging nor transposing reads for its images.  Same element count and draw strides as the batch-innermost tensor; same values.
 *   BBB_BF16_X_C8    x is in that layout.  Accepted where the library has a kernel that reads it: tap-major rows of 32 input
 *                    channels, 5 x 5 taps, stride 1, dilation 1, padding < 5, bf16 output (3Conv3FC conv2: a strip of three output
 *                    pixels per workgroup, every input position fetched once for all the pixels it is a tap of); BBB_EINVAL else.
 *   BBB_BF16_OUT_C8  y is written in that layout (cout % 8 == 0).  Accepted by the pooled first-layer forms (d->pool != 0) and
 *                    together with BBB_BF16_X_C8; BBB_EINVAL else.
 * Bit for bit the results of the batch-innermost forms (the same MFMA sequence per output element).
 */
#define BBB_BF16_OUT_F32      1u
#define BBB_BF16_W_TAP_MAJOR  2u
#define BBB_BF16_X_C8         4u   /* x is channel-interleaved: [draws|1][cin / 8][h][w][B][8] (ABI 10) */
#define BBB_BF16_OUT_C8       8u   /* y is written channel-interleaved: [draws][cout / 8][ho][wo][B][8] (ABI 10) */
int bbb_conv2d_chwn_bf16_fwd(const bbb_conv_desc_t* d, const void* x, const void* w, const float* bias, void* y,
                             uint32_t flags, void* stream);
/* What bbb_conv2d_chwn_bf16_fwd picks for (d, flags) (additive to ABI 13; host only, needs no device: tests, profiling).  *form: the
 * kernel; for BBB_BF16_FORM_GENERAL *shape = 22 (128 channels x 128 images per workgroup), 14 (64 x 256) or 12 (64 x 128),
 * *k_groups = 1 | 2 | 4, *wave_specialised = 0 | 1 (all three 0 for the other forms).  Out-pointers may be NULL.  Returns what the
 * launch entry returns for every check that does not involve an operand pointer; the two call the same plan (csrc/pconv_bf16_plan.h). */
#define BBB_BF16_FORM_GENERAL 0        /* pconv_bf16_kernel */
#define BBB_BF16_FORM_SMALLK 1         /* short contraction (row pitch <= 128), weights in registers */
#define BBB_BF16_FORM_SMALLK_POOL 2    /* ... with the pooling in the launch, strip form */
#define BBB_BF16_FORM_SMALLK_POOLWIN 3 /* ... window-resident form (small launches) */
#define BBB_BF16_FORM_STRIP8 4         /* BBB_BF16_X_C8 */
#define BBB_BF16_FORM_FEWOUT 5         /* classifiers: <= 16 outputs, a row of >= 512 */
int bbb_conv2d_chwn_bf16_plan(const bbb_conv_desc_t* d, uint32_t flags, int32_t* form, int32_t* shape, int32_t* k_groups,
                              int32_t* wave_specialised);
/* nn.MaxPool2d(k, s) on [planes][h][w][B] bf16 (B % 8 == 0); exact (max commutes with the rounding). */
int bbb_maxpool_chwn_bf16(const void* x, void* y, int64_t planes, int h, int w, int batch, int k, int s, void* stream);
/* fp32 [batch][plane] (an NCHW tensor, plane = C*H*W) -> bf16 [plane][batch] (batch-innermost), nearest-even. */
int bbb_nchw_to_chwn_bf16(const float* x, void* y, int batch, int64_t plane, void* stream);
/* The same for `slices` batches stored back to back (ABI 7): x [slices][batch][plane] -> y [slices][plane][batch], one launch
 * (a rank's batch slices; the batches of several one-draw steps that share a launch). */
int bbb_nchw_to_chwn_bf16_slices(const float* x, void* y, int batch, int64_t plane, int slices, void* stream);

/*
 * The local-reparameterisation layer on bf16 storage (additive to ABI 13; layers/BBB_LRT/BBBConv.py:71-81, BBBLinear.py:65-73):
 *   act_mu  = sum x * bf16(W_mu) + b_mu
 *   act_var = 1e-16 + sum bf16(x^2) * bf16(sigma^2) + sigma_b^2
 *   y       = act(act_mu + sqrt(act_var) * eps)        (sample != 0)   |   act(act_mu)   (sample == 0)
 * x is the STORED bf16 value; x^2 is its exact fp32 square rounded once to bf16 (nearest even), formed inside the kernel; both
 * contractions run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation from one staged x tile; biases, the sampling step and the
 * activation are fp32; y is rounded once when stored as bf16.  eps is the element bbb_lrt_conv2d_chwn_fwd draws: canonical index
 * ((b + d->b_offset) * cout + c) * ho * wo + pixel of stream (seed, call0 + slab, stream_id).
 *   x:           [draws|1][cin][h][w][B] bf16 (B % 8 == 0, 16-byte aligned); d->x_unit_div / x_unit_off as in bbb_conv2d_chwn_fwd
 *   w_mu, w_var: [cout][Kp] bf16 rows as bbb_lrt_weights_bf16 writes them (Kp = cin*kh*kw rounded up to 8, zero pad; column order
 *                (ci, r, q), or (r, q, ci) with BBB_BF16_W_TAP_MAJOR, cin % 8 == 0), SHARED by every slab of the launch:
 *                d->w_draw_stride == d->b_draw_stride == 0.  b_mu / b_var: fp32 [cout], both or neither.
 *   y:           [draws][cout][ho][wo][B] bf16, or fp32 with BBB_BF16_OUT_F32 (the logits layer).  May be NULL when sample == 0 and
 *                the moment outputs are given (a moments-only launch).
 *   act_mu_out / act_var_out: optional fp32 [draws][cout][ho][wo][B] copies of the two moments (both or neither).
 * No work units, no pooled form (BBB_EINVAL).  Every sum has a fixed order that depends on the layer's geometry only, so a slab
 * computed alone or inside a larger launch is the same bits.
 * bbb_lrt_conv2d_chwn_bf16_plan reports what the launcher picks for a descriptor: *shape = 22 (128 channels x 128 images per
 * workgroup), 14 (64 x 256) or 12 (64 x 128), *k_groups = 1 | 2, *wave_specialised = 0 | 1.  Host only (tests, profiling).
 */
int bbb_lrt_conv2d_chwn_bf16_fwd(const bbb_conv_desc_t* d, const void* x, const void* w_mu, const void* w_var, const float* b_mu,
                                 const float* b_var, void* y, float* act_mu_out, float* act_var_out, uint64_t seed, uint32_t call0,
                                 uint32_t stream_id, int sample, const uint32_t* call_dev, uint32_t flags, void* stream);
int bbb_lrt_conv2d_chwn_bf16_plan(const bbb_conv_desc_t* d, uint32_t flags, int32_t* shape, int32_t* k_groups,
                                  int32_t* wave_specialised);
/* bbb_lrt_sample_chwn with bf16 output: y[e] = bf16(act(act_mu + sqrt(act_var) * eps[e])), [draws][channels][pixels][batch], from one
 * pair of fp32 moments (a moments-only bbb_lrt_conv2d_chwn_bf16_fwd launch); bit for bit what `draws` sampling launches of that
 * entry point store.  batch % 8 == 0. */
int bbb_lrt_sample_chwn_bf16(const float* act_mu, const float* act_var, void* y, int draws, int channels, int pixels, int batch,
                             int b_offset, int act, uint64_t seed, uint32_t call0, uint32_t stream_id, const uint32_t* call_dev,
                             void* stream);
/* fp32 matrices [rows][row_len] -> bf16 [rows][Kp] in the bf16 GEMMs' row layout (Kp = row_len rounded up to 8, zero pad), up to
 * BBB_BF16_ROWS_MAX_SEGMENTS of them in ONE launch: the W_mu and sigma^2 operands of every LRT layer of a model.  taps > 0: the
 * source row is [cin][taps] and the output row tap-major, column t * cin + ci (cin = row_len / taps, cin % 8 == 0); 0: as it is. */
#define BBB_BF16_ROWS_MAX_SEGMENTS 32
typedef struct bbb_bf16_rows_segment {
    const float* src;
    void* dst;            /* 16-byte aligned */
    int64_t rows;
    int32_t row_len;
    int32_t taps;
} bbb_bf16_rows_segment_t;
int bbb_lrt_weights_bf16(const bbb_bf16_rows_segment_t* segs, int nseg, void* stream);

/*
 * Monte-Carlo tail (main_bayesian.py:49,53 / :78,80 + utils.py:14-22): per draw log_softmax over
 * classes, then log-sum-exp over the local draws.
 *   logits [draws][B][C]  ->  lse [B][C] = log sum_e exp(log_softmax(logits[e])[b][c])
 * log_outputs = lse - log(E_total) (applied when mean_over > 0: lse - log(mean_over)).
 * Ranks of an ensemble-sharded job combine their lse blocks with one more log-sum-exp.
 * Every entry below subtracts a row's maximum before its log partition, ls = (v - max) - log sum exp(v - max), forward and
 * backward alike: adding a constant to a row of logits changes no rounding.  classes <= 1024 here and in bbb_uncertainty.
 */
int bbb_mc_tail(const float* logits, int draws, int batch, int classes, int mean_over,
                float* lse_out, void* stream);

/* bbb_mc_tail for logits stored batch-innermost, [draws][C][B] (output of the batched ensemble path); lse_out is [B][C].
 * draws <= 512.  This and the four entries after the ELBO pair are one kernel launched from one plan (csrc/mc_tail_plan.h): one float
 * of LDS per image and draw the image reduces over, so at most 640 such draws (160 KB; more: BBB_ESHAPE), at most 4096 slabs in a
 * launch, slices * batch_slice <= 2^31 - 64 images. */
int bbb_mc_tail_cb(const float* logits, int draws, int batch, int classes, int mean_over,
                   float* lse_out, void* stream);
/* Backward of bbb_mc_tail_cb (training extension, ABI 12; loss.backward() of main_bayesian.py:57 through log_softmax + logmeanexp):
 * g_logits [draws][classes][batch] from g_lse [batch][classes] and the forward's lse [batch][classes]. */
int bbb_mc_tail_cb_bwd(const float* logits, const float* lse, const float* g_lse, float* g_logits, int draws, int batch, int classes,
                       int mean_over, void* stream);

/* Training extension: the ELBO of one Monte-Carlo step on the device (metrics.py:7-14: nll_loss(log_outputs, target, mean) *
 * train_size + beta * kl; main_bayesian.py:55-56).  lse [batch][classes] = bbb_mc_tail_cb's output, target [batch] int64 (entries
 * outside [0, classes) contribute nothing), kl / loss_out device scalars; beta_dev != NULL: the KL weight is read from the device
 * (a captured step's run-time value) instead of `beta`.  One block, fixed summation order. */
int bbb_elbo_cb_fwd(const float* lse, const int64_t* target, const float* kl, float beta, const float* beta_dev, float train_size,
                    int batch, int classes, float* loss_out, void* stream);
/* Its backward in one launch: g_logits [draws][classes][batch] = d loss / d logits through log_softmax + logmeanexp (as
 * bbb_mc_tail_cb_bwd with g_lse = -(train_size / batch) * g_loss at the target class), g_kl (device scalar, may be NULL) =
 * beta * g_loss. */
int bbb_elbo_cb_bwd(const float* logits, const float* lse, const int64_t* target, const float* g_loss, float beta,
                    const float* beta_dev, float train_size, float* g_logits, float* g_kl, int draws, int batch, int classes,
                    int mean_over, void* stream);

/* The same for a rank's WORK UNITS (bbb_conv_desc_t: unit u = unit_off + e is draw u / slices, batch slice u % slices):
 * logits [units][C][batch_slice] -> lse_out [slices * batch_slice][C]; image b of slice s gets the log-sum-exp over the local
 * units of that slice, -inf where the rank holds none (the ranks' blocks are then combined by one more log-sum-exp).
 * units <= 4096, ceil(units / slices) <= 640; unit_off of any size (taken modulo slices). */
int bbb_mc_tail_units(const float* logits, int units, int slices, int unit_off, int batch_slice, int classes, int mean_over,
                      float* lse_out, void* stream);

/* bbb_mc_tail_units + the end of a captured Monte-Carlo step in the same launch (ABI 6): kl_out = kl_in * kl_scale (kl_in: the KL
 * of ONE forward from bbb_reparam_kl_fwd; the reference sums it once per forward, main_bayesian.py:76-77; kl_out NULL = skip) and
 * *counter += counter_add (the device-side call counter that bbb_reparam_kl_fwd / the LRT entry points read through `call_dev`:
 * all of a step's readers run before its tail, so the next replay of the graph draws fresh noise; counter NULL = skip). */
int bbb_mc_tail_units_step(const float* logits, int units, int slices, int unit_off, int batch_slice, int classes, int mean_over,
                           float* lse_out, const float* kl_in, float kl_scale, float* kl_out, uint32_t* counter,
                           uint32_t counter_add, void* stream);

/* Several Monte-Carlo steps in one set of launches (ABI 8): logits [groups * draws][C][batch] hold `groups` consecutive steps of
 * `draws` forwards each, step g on its own batch (slab g * draws + j = draw j of step g; main_bayesian.py:73-80 run `groups`
 * times) -> lse_out [groups * batch][C], block g = the log-sum-exp over step g's draws (minus log(mean_over) when > 0).
 * kl_in / kl_scale / kl_out / counter / counter_add as in bbb_mc_tail_units_step (all NULL / 0 = plain tail).
 * groups * draws <= 4096, draws <= 640. */
int bbb_mc_tail_groups_step(const float* logits, int groups, int draws, int batch, int classes, int mean_over,
                            float* lse_out, const float* kl_in, float kl_scale, float* kl_out, uint32_t* counter,
                            uint32_t counter_add, void* stream);

/* A RANK'S SHARE of a group of steps (ABI 8): the `slabs` local draws are draws first_off, first_off + 1, ... of the draw-major
 * enumeration (step g, draw j) -> g * draws + j of `steps` consecutive local steps (the share may start and end in the middle of a
 * step): lse_out [steps * batch][C], block k = the log-sum-exp over the LOCAL draws of local step k (no mean; -inf where it holds none);
 * the ranks' blocks are combined by one more log-sum-exp.  kl / counter arguments as in bbb_mc_tail_units_step.
 * slabs <= 4096, 0 <= first_off < draws <= 640, first_off + slabs <= steps * draws. */
int bbb_mc_tail_share_step(const float* logits, int slabs, int steps, int draws, int first_off, int batch, int classes,
                           float* lse_out, const float* kl_in, float kl_scale, float* kl_out, uint32_t* counter,
                           uint32_t counter_add, void* stream);

/*
 * Uncertainty decomposition over `draws` stochastic forwards (uncertainty_estimation.py:37-58 per image, :61-102 per
 * batch): logits [draws][B][C] -> pred = mean logits, epistemic = mean (p_hat - p_bar)^2, aleatoric = p_bar - mean p_hat^2,
 * each [B][C]; p_hat = softmax(logits), or softplus(logits)/sum when `normalized`.
 */
int bbb_uncertainty(const float* logits, int draws, int batch, int classes, int normalized,
                    float* pred, float* epistemic, float* aleatoric, void* stream);

/*
 * Uncertainty scores of batch-innermost logits in ONE launch (additive to ABI 13): logits [draws][C][B] fp32, as the batched
 * ensemble path leaves them -- no transpose, no atomics, lanes = 64 consecutive images.  With p_t = softmax(logits[t]) over the
 * classes (normalized != 0: softplus(v) / sum softplus(v), softplus(v) = v for v > 20) and p_bar = (1/draws) sum_t p_t:
 *   pred, p_mean, epistemic, aleatoric [B][C]: mean logit, p_bar, (1/draws) sum_t (p_t - p_bar)^2 (second pass over the draws,
 *                                              no cancellation), p_bar - (1/draws) sum_t p_t^2
 *   entropy, expected_entropy, mutual_info [B]: H[p_bar] = -sum_c p_bar log p_bar, (1/draws) sum_t H[p_t], and
 *                                              (1/draws) sum_t sum_c p_t (log p_t - log p_bar) -- the KL form, clamped below at 0,
 *                                              not the difference of the two entropies (which loses the small values)
 * log p_t is the log-softmax in the order of the tail entries, (v - max) - log sum exp(v - max); normalized: log softplus(v) -
 * log sum softplus.  A term with p = 0 contributes exactly 0 (a class at -inf does not make an entropy NaN); with draws = 1
 * log p_bar IS log p_t, so epistemic and mutual_info are exactly 0.  Image b's results depend on its own draws x C logits only.
 * Any output pointer may be NULL: that output is not written, the others keep their bits.
 * Limits (csrc/mc_uncertainty_plan.h): draws <= 202 -- a workgroup keeps three floats per (draw, image) and 8 KB of row partials
 * in its 160 KB of LDS; batch <= INT32_MAX - 63; any classes.  Checks in this order: BBB_EINVAL (NULL logits, a size that is not
 * positive, all seven outputs NULL), BBB_EALIGN (a pointer that is not 4-byte aligned), BBB_ESHAPE (batch or draws beyond the
 * limits).
 */
int bbb_mc_uncertainty_cb(const float* logits, int draws, int batch, int classes, int normalized, float* pred, float* p_mean,
                          float* epistemic, float* aleatoric, float* entropy, float* expected_entropy, float* mutual_info,
                          void* stream);

/* What bbb_mc_uncertainty_cb launches for these arguments, without the launch (host only, needs no device): the same checks and
 * return codes; *rows: rows of the 64-lane block, min(16, max(draws, classes)); *blocks: ceil(batch / 64); *lds_bytes: the dynamic
 * LDS of the launch, draws * 768 + 8192.  Each of the three may be NULL. */
int bbb_mc_uncertainty_cb_plan(const float* logits, int draws, int batch, int classes, const float* pred, const float* p_mean,
                               const float* epistemic, const float* aleatoric, const float* entropy,
                               const float* expected_entropy, const float* mutual_info, int32_t* rows, int32_t* blocks,
                               int32_t* lds_bytes);

/*
 * Backward of bbb_mc_uncertainty_cb in ONE launch (additive to ABI 13): d_logits [draws][C][B] = d L / d logits for
 * L = sum of (upstream gradient x output) over the seven outputs; every element is written.  logits and normalized as in the forward;
 * p_mean [B][C] is the forward's p_mean output of the same logits (required: with it a (draw, image) pair needs no other pair).
 * Upstream gradients: w_pred, w_p_mean, w_epistemic, w_aleatoric [B][C]; w_entropy, w_expected_entropy, w_mutual_info [B]; a NULL
 * pointer is a zero in the same arithmetic.  Per image, with p, log p, p_bar as the forward defines them:
 *   G[t][k] = (-(w_ent + w_mi) log p_bar[k] - (w_ee - w_mi) log p[t][k] + w_pm[k] + 2 w_epi[k] (p[t][k] - p_bar[k])
 *              + w_ale[k] (1 - 2 p[t][k])) / draws,          D[t] = sum_k p[t][k] G[t][k]   (compensated, one thread),
 *   d_logits[t][c] = J[t][c] (G[t][c] - D[t]) + w_pred[c] / draws,   J = p (softmax); sigmoid(v) / sum softplus (normalized; the
 *   derivative of softplus(v) is 1 for v > 20).
 * A class with p = 0 contributes exactly 0 to D and receives w_pred / draws alone (neither 0 * -inf nor log 0 is formed), the
 * log p_bar term is 0 where p_bar = 0, and a NaN stays a NaN inside its image; with draws = 1 log p_bar IS log p.  The forward's clamp of
 * mutual_info at 0 is not differentiated: the gradient is that of the KL form.  No atomics; image b's gradient depends on its own
 * draws x C logits only, not on the batch or the launch shape.
 * Limits (csrc/mc_uncertainty_plan.h): draws <= 202 (the forward's), batch <= INT32_MAX - 63; any classes.  Checks in this order:
 * BBB_EINVAL (NULL logits, p_mean or d_logits, a size that is not positive, all seven upstream gradients NULL), BBB_EALIGN (a
 * pointer that is not 4-byte aligned), BBB_ESHAPE (batch or draws beyond the limits).
 */
int bbb_mc_uncertainty_cb_bwd(const float* logits, const float* p_mean, int draws, int batch, int classes, int normalized,
                              const float* w_pred, const float* w_p_mean, const float* w_epistemic, const float* w_aleatoric,
                              const float* w_entropy, const float* w_expected_entropy, const float* w_mutual_info, float* d_logits,
                              void* stream);

/* What bbb_mc_uncertainty_cb_bwd launches for these arguments, without the launch (host only): the same checks and return codes;
 * *rows: draws of a 64-lane block, 1; *blocks: gridDim.x = ceil(batch / 64) (gridDim.y = draws); *lds_bytes: 0.  Each may be NULL. */
int bbb_mc_uncertainty_cb_bwd_plan(const float* logits, const float* p_mean, int draws, int batch, int classes, const float* w_pred,
                                   const float* w_p_mean, const float* w_epistemic, const float* w_aleatoric, const float* w_entropy,
                                   const float* w_expected_entropy, const float* w_mutual_info, const float* d_logits, int32_t* rows,
                                   int32_t* blocks, int32_t* lds_bytes);

/*
 * Regression with a Gaussian likelihood on batch-innermost logits (additive to ABI 13; csrc/gauss_tail.hip): logits [draws][C][B] fp32
 * as the batched ensemble path and the training nodes leave them, targets y [B][dims] fp32.  channels == 2 * dims (heteroscedastic):
 * channel d is the mean mu, channel dims + d the log-variance s; channels == dims (homoscedastic): s = 2 log(noise_sigma), rounded to
 * fp32 once (noise_sigma is not read in the heteroscedastic form).  With s_c = clamp(s, log_var_min, log_var_max) and r = y - mu:
 *   ll[e][d][b] = -0.5 (log 2 pi + s_c + r^2 exp(-s_c)),   L[e][b] = sum_d ll (d ascending),
 *   LL[b] = logsumexp_e L[e][b] - log(mean_over > 0 ? mean_over : draws)   (mc = 0: the log of the mixture predictive density; the
 *           log-sum-exp is an online one over e ascending and subtracts the running maximum first, so a draw 1e4 below the best one
 *           weighs exactly 0)   or   (1 / draws) sum_e L[e][b]   (mc = 1: the ELBO's expected log-likelihood),
 *   loss = -(train_size / B) sum_b LL[b] + beta * kl   (beta_dev != NULL: the KL weight is read from the device, as bbb_elbo_cb_fwd).
 * bbb_gauss_elbo_cb_fwd: two launches that meet at the launch boundary -- LL [B] by 64-image blocks (ll_out), then ONE 256-thread block
 * adds LL in a fixed order (thread t: b = t, t + 256, ...; then a fixed tree) into loss_out: the loss does not depend on the number of
 * workgroups, every sum has a fixed order, there are no atomics.  y is staged through LDS (coalesced reads of the row-major targets).
 * A NaN in a logit or target of image b makes LL[b] and the loss NaN (the clamp keeps a NaN).
 * Limits (csrc/gauss_tail_plan.h): draws <= 512, channels <= 1024, batch <= INT32_MAX - 63.  Checks of all three entries, in this order:
 * BBB_EINVAL (a required pointer that is NULL; a size that is not positive; channels neither dims nor 2 * dims; log_var_min >
 * log_var_max; homoscedastic with a noise_sigma that is not finite and positive; mc outside {0, 1}; mean_over < 0), BBB_EALIGN (a
 * pointer, optional ones included, that is not 4-byte aligned), BBB_ESHAPE (the limits).
 */
int bbb_gauss_elbo_cb_fwd(const float* logits, const float* y, const float* kl, float beta, const float* beta_dev, float train_size,
                          int draws, int batch, int channels, int dims, double noise_sigma, float log_var_min, float log_var_max,
                          int mc, int mean_over, float* ll_out, float* loss_out, void* stream);

/* What bbb_gauss_elbo_cb_fwd launches first for these arguments, without the launch (host only, needs no device): the same checks and
 * return codes; *threads: lanes of a block, 64 (one image each); *blocks: ceil(batch / 64); *lds_bytes: the staged tile of y,
 * 64 x 17 floats = 4352.  The second launch is always one block of 256 threads.  Each of the three may be NULL. */
int bbb_gauss_elbo_cb_fwd_plan(const float* logits, const float* y, const float* kl, const float* beta_dev, int draws, int batch,
                               int channels, int dims, double noise_sigma, float log_var_min, float log_var_max, int mc, int mean_over,
                               const float* ll_out, const float* loss_out, int32_t* threads, int32_t* blocks, int32_t* lds_bytes);

/* Its backward in ONE launch: g_logits [draws][C][B] (every element written) and g_kl (device scalar, may be NULL) = beta * g_loss.
 * L[e][b] is RECOMPUTED from the logits by the forward's own code (nothing is kept from the forward), then per (e, b):
 *   w = exp(L[e][b] - logsumexp_e L[.][b])  (mc = 0)  or  1 / draws  (mc = 1),      c = -(train_size / B) * g_loss,
 *   g_mu = c w r exp(-s_c),   g_s = c w 0.5 (r^2 exp(-s_c) - 1) for log_var_min <= s <= log_var_max, exactly 0 outside
 * (torch.clamp's gradient).  A NaN of image b makes image b's columns NaN and no other's.  Same limits, same order of the checks;
 * required: logits, y, g_loss, g_logits. */
int bbb_gauss_elbo_cb_bwd(const float* logits, const float* y, const float* g_loss, float beta, const float* beta_dev, float train_size,
                          int draws, int batch, int channels, int dims, double noise_sigma, float log_var_min, float log_var_max,
                          int mc, int mean_over, float* g_logits, float* g_kl, void* stream);

/* What bbb_gauss_elbo_cb_bwd launches, without the launch (host only): outputs as bbb_gauss_elbo_cb_fwd_plan's. */
int bbb_gauss_elbo_cb_bwd_plan(const float* logits, const float* y, const float* g_loss, const float* beta_dev, int draws, int batch,
                               int channels, int dims, double noise_sigma, float log_var_min, float log_var_max, int mc, int mean_over,
                               const float* g_logits, const float* g_kl, int32_t* threads, int32_t* blocks, int32_t* lds_bytes);

/* Predictive moments of a regression model in ONE launch: mean [B][dims] = (1 / draws) sum_e mu, epistemic = (1 / draws) sum_e
 * (mu - mean)^2 (a second pass over the draws, never E[mu^2] - mean^2), aleatoric = (1 / draws) sum_e exp(s_c), total = epistemic +
 * aleatoric, and log_density [B] = LL[b] in the mc = 0 form with mean_over = draws (needs y; y may be NULL otherwise).  Any output
 * pointer may be NULL: that output is not written, the others keep their bits.  Checks as above: BBB_EINVAL also for all five outputs
 * NULL and for log_density without y. */
int bbb_gauss_moments_cb(const float* logits, const float* y, int draws, int batch, int channels, int dims, double noise_sigma,
                         float log_var_min, float log_var_max, float* mean, float* epistemic, float* aleatoric, float* total,
                         float* log_density, void* stream);

/* What bbb_gauss_moments_cb launches, without the launch (host only): outputs as bbb_gauss_elbo_cb_fwd_plan's. */
int bbb_gauss_moments_cb_plan(const float* logits, const float* y, int draws, int batch, int channels, int dims, double noise_sigma,
                              float log_var_min, float log_var_max, const float* mean, const float* epistemic, const float* aleatoric,
                              const float* total, const float* log_density, int32_t* threads, int32_t* blocks, int32_t* lds_bytes);

/* [rows][cols] -> [cols][rows] (e.g. an NCHW batch [B][C*H*W] into the batch-innermost [C*H*W][B] layout). */
int bbb_transpose2d(const float* in, float* out, int64_t rows, int64_t cols, void* stream);

/* Batched strided transpose: out[i1*out_b1 + i2*out_b2 + c*out_col + r] = in[i1*in_b1 + i2*in_b2 + r*in_row + c] for r < rows,
 * c < cols, i1 < nb1, i2 < nb2 (nb1*nb2 <= 65535).  Training extension: operand layouts of the role-swapped weight gradient. */
int bbb_transpose_batched(const float* in, float* out, int rows, int cols, int nb1, int nb2, int64_t in_b1, int64_t in_b2,
                          int64_t in_row, int64_t out_b1, int64_t out_b2, int64_t out_col, void* stream);

/* The same with three batch dimensions nb[3] (product <= 65535; strides in_b[3] / out_b[3]) and a summed one:
 * out[i1*out_b[0] + i2*out_b[1] + i3*out_b[2] + c*out_col + r] = sum_{s < nsum, ascending} in[i1*in_b[0] + i2*in_b[1] + i3*in_b[2]
 * + s*in_sum + r*in_row + c].  Training extension: the batch chunks of a role-swapped weight gradient summed in a fixed order
 * while the taps move innermost; an output gradient written straight into the chunked weight-operand layout.  square_off != 0: every
 * output's square is written too, square_off elements behind it (x and x^2 of an LRT layer's weight gradients in one pass). */
int bbb_transpose_sum_batched(const float* in, float* out, int rows, int cols, const int32_t* nb, const int64_t* in_b,
                              const int64_t* out_b, int64_t in_row, int64_t out_col, int nsum, int64_t in_sum, int64_t square_off,
                              void* stream);

/* Training extension: out [draws][cin][cout][kh*kw] = w [draws][cout][cin][kh*kw] with the taps reversed (spatial flip +
 * channel transpose: the weights of the stride-1 input-gradient convolution). */
int bbb_flip_transpose_w(const float* w, float* out, int64_t draws, int cout, int cin, int khkw, void* stream);
/* The same over two sources: out's draws [0, draws_each) from w0, [draws_each, 2*draws_each) from w1 (the mean and variance
 * weights of a local-reparameterisation layer as one operand: both input gradients in one launch of the forward kernel). */
int bbb_flip_transpose_w_pair(const float* w0, const float* w1, float* out, int64_t draws_each, int cout, int cin, int khkw,
                              void* stream);
/* ... and for up to 16 weight sets in ONE launch (every layer's input-gradient weights of a training step): segment i flips
 * `draws` sets [cout][cin][khkw] from w0 -- or, with w1 != NULL, draws / 2 from w0 then draws / 2 from w1 -- into out. */
typedef struct {
    const float* w0;
    const float* w1;      /* NULL, or the second source (draws must then be even) */
    float* out;           /* [draws][cin][cout][khkw] */
    int64_t draws;
    int32_t cout, cin, khkw, reserved;
} bbb_flip_seg_t;
int bbb_flip_transpose_w_multi(const bbb_flip_seg_t* segs, int n_segs, void* stream);

/* Training extension: im2col of an NCHW batch x [batch][cin][h][w] (geometry from d; draws / strides / act ignored) into
 * out [ho*wo][batch][Jp], Jp = cin*kh*kw rounded up to 4 (pad columns zero): the K-major operand of the first layer's
 * weight-gradient GEMM (see bbb_hip/ops.py: conv2d_chwn_weight_grad_shared_input). */
int bbb_im2col_pbj(const float* x, float* out, const bbb_conv_desc_t* d, void* stream);

/* Training extension, additive in ABI 13: the gather half of a FIRST layer's input gradient (d loss / d x of the caller's batch,
 * which every draw shares).  The contraction D[(ci, r, q)][ho][wo][b] = sum_(e, co) w[e][co][ci][r][q] * g_pre[e][co][ho][wo][b] runs
 * on bbb_conv2d_chwn_fwd as a 1x1 convolution (bbb_hip/ops.py: first_layer_input_grad); this folds D onto the input pixels:
 *   dx[b][ci][h][w] = sum over the taps (r, q) with h = ho*sh - ph + r*dh, w = wo*sw - pw + q*dw of D[(ci, r, q)][ho][wo][b]
 * (geometry from d: batch, cin, h, w, kh, kw, stride, padding, dilation; the other fields are ignored).  D's rows are row_pitch
 * (>= ho*wo*batch) elements apart.  x == NULL: dx = that sum.  x != NULL (a local-reparameterisation first layer): D holds two sets,
 * the second set_stride (>= cin*kh*kw*row_pitch) elements behind the first, and dx = sum(set 0) + 2 * x * sum(set 1) with x the NCHW
 * input.  dx, x: NCHW [batch][cin][h][w]; pixels no tap reaches get 0.  Taps are added in ascending (r, q) order, no atomics. */
int bbb_input_grad_col2im(const float* dcol, int64_t row_pitch, int64_t set_stride, const float* x, float* dx,
                          const bbb_conv_desc_t* d, void* stream);

/* Training extension, additive in ABI 13: the input gradient of a STRIDED layer y = conv(x, w) in the batch-innermost layout, as
 * the transposed ("fractionally strided") form of bbb_conv2d_chwn_fwd's launch (csrc/pconv_dgrad.hip):
 *   dx[e][ci][ih][iw][b] = sum over co and the taps (r', q') of g_pre[e][co][oh][ow][b] * w_flipped[e][ci][co][r'][q']
 * where tap r' takes part iff t = ih - pad_h + r' * dil_h satisfies t >= 0, t % up_h == 0 and oh = t / up_h < h (columns alike).
 * d is the descriptor of the launch a stride-1 layer's gradient takes on bbb_conv2d_chwn_fwd -- batch; cin, h, w = channels and
 * map of g_pre (the layer's cout, ho, wo); cout = channels of dx (the layer's cin); kh, kw, dil = the layer's; stride 1;
 * pad = dil * (k - 1) - the layer's padding (>= 0); draws, x_draw_stride (g_pre) and w_draw_stride (0: every draw shares one
 * weight set) as usual; every other field 0 -- and the layer's stride travels as the upsampling factors (up_h, up_w), the map of
 * dx as (out_h, out_w): it must be one whose forward gives g_pre's map, (out + 2 p - dil (k - 1) - 1) / up + 1 == h | w, else
 * BBB_ESHAPE.  g_pre [draws|1][cin][h][w][B], w_flipped [draws|1][cout][cin][kh][kw] (bbb_flip_transpose_w*), dx
 * [draws][cout][out_h][out_w][B].  No inserted zero and no padding tap is multiplied: the (pixel, tap) pairs visited are the
 * forward launch's in-bounds pairs.  A pixel no tap reaches (up > dil (k - 1) + 1, rows the forward's floor dropped) is written
 * as zeros.  One fmaf chain per element in a fixed order (channel-major, then taps ascending), no atomics, no scratch, never
 * split: a draw's slab does not depend on what shares the launch.  up_h == up_w == 1 is BBB_EINVAL (that gradient is
 * bbb_conv2d_chwn_fwd on the flipped weights: there is one way to compute it). */
int bbb_conv2d_chwn_dgrad(const bbb_conv_desc_t* d, const float* g_pre, const float* w_flipped, float* dx, int up_h, int up_w,
                          int out_h, int out_w, void* stream);
/* What that launch takes (host only, no device): *bm images per item (64 | 128), *ilv staging loads interleaved, *items, *blocks --
 * the tile and interleave choice bbb_conv2d_chwn_fwd makes for a plain launch of the same pixels, channels, images and draws (one
 * rule, csrc/pconv_plan.h).  Returns 0 or what the launch entry returns for every check that does not involve an operand pointer.
 * Out-pointers may be NULL.  The sibling of bbb_conv2d_chwn_bf16_dgrad_plan. */
int bbb_conv2d_chwn_dgrad_plan(const bbb_conv_desc_t* d, int up_h, int up_w, int out_h, int out_w, int32_t* bm, int32_t* ilv,
                               int64_t* items, int64_t* blocks);

/* Training extension, the small steps between the gradient GEMMs (ABI 8; deterministic, no atomics):
 * bbb_plane_sum: out[r] = sum over o < outer, j < cols of x[o*outer_stride + r*row_pitch + j] -- bias gradients (the gradient w.r.t.
 *   a layer's pre-activation summed over pixels and images per (draw, channel) plane; outer > 1 also sums over draws: LRT biases).
 * bbb_sum_leading: out[i] = sum over o < outer of x[o*n + i], added in index order -- the draws of a first LRT layer share
 *   one pair of moments, and shared-weight gradients are summed over draws.
 * bbb_lrt_glue: mode 0: out = x*x (the variance contraction's operand, layers/BBB_LRT/BBBConv.py:73); mode 1: out[i] = a[i] +
 *   2*x[i % x_n]*b[i] -- the LRT input gradient dgrad(g_mu, mu) + 2 x dgrad(g_var, sigma^2) with x one slab or one per draw. */
int bbb_plane_sum(const float* x, float* out, int64_t outer, int64_t rows, int64_t cols, int64_t row_pitch, int64_t outer_stride,
                  void* stream);
int bbb_sum_leading(const float* x, float* out, int64_t outer, int64_t n, void* stream);
int bbb_lrt_glue(const float* a, const float* x, const float* b, float* out, int64_t n, int64_t x_n, int mode, void* stream);

/*
 * bf16 training backward (the bf16 storage mode of the training step; additive entry points, ABI 13).  The gradient contractions
 * run on bbb_conv2d_chwn_bf16_fwd (dgrad: the forward on flipped, channel-transposed weight rows; wgrad: the forward with batch and
 * channel roles swapped); these are the steps around them.  Deterministic, no atomics, 16-byte vector stores.
 * bbb_pool_act_bwd_chwn_bf16: bbb_pool_act_bwd_chwn on bf16 storage.  y [planes][h][w][B] bf16 (the stored activated output),
 *   g_out [planes][hp][wp][B] bf16, or fp32 with BBB_BF16_BWD_G_F32; g_pre = act'(y) * route(g_out) in fp32 (routing to the first
 *   maximum among the stored bf16 values, act' from the bf16 y), rounded once to bf16 (nearest-even) -- written as bf16, or with
 *   BBB_BF16_BWD_OUT_F32 as the fp32 values of that rounding.  B % 8 == 0; out_plane_pitch: 0 = dense, else elements (% 8 == 0).
 * bbb_plane_sum_bf16: out[r] = sum over j < cols of x[r*row_pitch + j], bf16 in, fp32 accumulation in a fixed order (bias
 *   gradients); cols and row_pitch multiples of 8.
 * bbb_flip_transpose_w_bf16: w [draws][cout][Kpi] bf16 rows (Kp = row length rounded up to 8) -> out [draws][cin][Kpo] with the
 *   taps reversed and the channels transposed, pad columns zero: the weight operand of the input gradient.  Row orders: (ci, tap)
 *   or, with BBB_BF16_FLIP_IN_TAP_MAJOR, (tap, ci); out (co, tap) or, with BBB_BF16_FLIP_OUT_TAP_MAJOR (cout % 8 == 0), (tap, co).
 * bbb_chwn_to_bhwc_bf16: [draws][c][hw][B] -> [draws][B][hw][c_pad] bf16, channels c .. c_pad-1 zero (B, c_pad multiples of 8).
 * bbb_batch_chunks_bf16: [outer][rows][B] -> [outer][chunks][rows][B / chunks] bf16 (B % (8 * chunks) == 0).
 */
#define BBB_BF16_BWD_G_F32          1u
#define BBB_BF16_BWD_OUT_F32        2u
#define BBB_BF16_FLIP_IN_TAP_MAJOR  1u
#define BBB_BF16_FLIP_OUT_TAP_MAJOR 2u
int bbb_pool_act_bwd_chwn_bf16(const void* g_out, const void* y, void* g_pre, int64_t planes, int h, int w, int batch, int k, int s,
                               int act, int64_t out_plane_pitch, uint32_t flags, void* stream);
int bbb_plane_sum_bf16(const void* x, float* out, int64_t rows, int64_t cols, int64_t row_pitch, void* stream);
int bbb_flip_transpose_w_bf16(const void* w, void* out, int64_t draws, int cout, int cin, int khkw, uint32_t flags, void* stream);
int bbb_chwn_to_bhwc_bf16(const void* x, void* out, int64_t draws, int c, int64_t hw, int batch, int c_pad, void* stream);
int bbb_batch_chunks_bf16(const void* x, void* out, int64_t outer, int64_t rows, int batch, int chunks, void* stream);

/* bf16 training backward, additive in ABI 13: the input gradient of a STRIDED layer on bf16 storage -- bbb_conv2d_chwn_dgrad's
 * transposed launch on the general bf16 GEMM (csrc/pconv_bf16.hip, pconv_bf16_kernel TR).  The argument contract is
 * bbb_conv2d_chwn_dgrad's: d describes the stride-1 launch on the flipped rows (batch; cin, h, w = channels and map of g_pre;
 * cout = channels of dx; kh, kw, dil = the layer's; stride 1; pad = dil * (k - 1) - the layer's padding; draws, x_draw_stride,
 * w_draw_stride; every other field 0), (up_h, up_w) = the layer's stride ((1, 1) is BBB_EINVAL: that gradient is
 * bbb_conv2d_chwn_bf16_fwd on the flipped rows), (out_h, out_w) = the map of dx, which must be one whose forward gives g_pre's map
 * (else BBB_ESHAPE).  Operands as bbb_conv2d_chwn_bf16_fwd's: g_pre [draws|1][cin][h][w][B] bf16, B % 8 == 0; w_flipped
 * [draws|1][cout][Kp] bf16 rows as bbb_flip_transpose_w_bf16 writes them, Kp = cin*kh*kw rounded up to 8, in (ci, r, q) order or,
 * with flags = BBB_BF16_W_TAP_MAJOR (cin % 8 == 0), (r, q, ci) order (no other flag is accepted); dx [draws][cout][out_h][out_w][B]
 * bf16; all three 16-byte aligned, draw strides multiples of 8 elements (else BBB_EALIGN); the forward's 32-bit offset limits and
 * cin*kh*kw < 2^24 (else BBB_ESHAPE).  fp32 accumulation in a fixed order, one rounding to nearest-even, no bias / activation /
 * pooling, no atomics, no scratch.  Tap-major rows: only the taps that take part are contracted (no inserted zero, no padding
 * tap).  Reference-order rows: the full row is contracted with the other taps' image rows read as zero (about up_h * up_w times
 * the useful matrix work).  A pixel no tap reaches is written as +0.  Every check happens before any launch. */
int bbb_conv2d_chwn_bf16_dgrad(const bbb_conv_desc_t* d, const void* g_pre, const void* w_flipped, void* dx, int up_h, int up_w,
                               int out_h, int out_w, uint32_t flags, void* stream);
/* What that launch picks (additive to ABI 13; host only): *shape = 22 | 14 | 12, *k_groups = 1 | 2, *wave_specialised = 0 | 1, as
 * for bbb_conv2d_chwn_bf16_plan -- always the general kernel.  Out-pointers may be NULL; the launch entry's codes for every check
 * that does not involve an operand pointer. */
int bbb_conv2d_chwn_bf16_dgrad_plan(const bbb_conv_desc_t* d, int up_h, int up_w, int out_h, int out_w, uint32_t flags,
                                    int32_t* shape, int32_t* k_groups, int32_t* wave_specialised);

/* bf16 training backward, additive in ABI 13: the contraction half of a FIRST layer's input gradient on bf16 operands -- what
 * bbb_hip/ops.py: first_layer_input_grad runs as a transpose + bbb_conv2d_chwn_fwd for the fp32 node (csrc/input_grad_bf16.hip):
 *   D[(ci, r, q)][ho][wo][b] = sum over (e, co) of w[e][co][ci][r][q] * g_pre[e][co][ho][wo][b]
 * followed, unchanged, by bbb_input_grad_col2im(D, d_row_pitch, 0, NULL, dx, d, stream).
 * d is the LAYER: batch, cin, h, w, cout, kh, kw, stride, pad, dil, draws = E, w_draw_stride = cout * Kp with Kp = cin*kh*kw rounded
 * up to 8; every other field 0.  g_pre: the E*cout rows (e, co), g_row_pitch (>= ho*wo*batch, % 8 == 0) elements apart, bf16 or,
 * with BBB_BF16_BWD_G_F32, fp32 values that are exactly bf16-representable (what bbb_pool_act_bwd_chwn_bf16 writes with
 * BBB_BF16_BWD_OUT_F32, at the padded plane pitch: taken by their high halves while staging, no bf16 copy).  w: the rows
 * [E][cout][Kp] of the parameter pass, read IN PLACE (no transposed copy), in (ci, r, q) order or, with BBB_BF16_W_TAP_MAJOR
 * (cin % 8 == 0), (r, q, ci) order; D's rows are in (ci, r, q) order either way, cin*kh*kw of them d_row_pitch (>= ho*wo*batch,
 * % 4 == 0) fp32 elements apart.  Any other flag bit is BBB_EINVAL.  g_pre, w and D 16-byte aligned (else BBB_EALIGN), B % 8 == 0,
 * E*cout*g_row_pitch, E*cout*Kp and cin*kh*kw*d_row_pitch below 2^31 (else BBB_ESHAPE).
 * v_mfma_f32_32x32x16_bf16, fp32 accumulation over (e, co) in ascending order, never split and never rounded: an element of D does
 * not depend on what else is in the launch, a column not on the other columns.  E*cout, cin*kh*kw and ho*wo*batch need not be
 * multiples of anything but B's 8: tails are masked on both operands -- nothing outside the E*cout rows' first ho*wo*batch columns
 * and the weight rows' first cin*kh*kw columns is read, nothing outside D's cin*kh*kw x ho*wo*batch is written (the pad columns of
 * either pitch are left alone).  No atomics, no scratch.  Every check happens before any launch, in this order: BBB_EINVAL (nulls,
 * flags, the descriptor), BBB_EALIGN (pointers, pitches), BBB_ESHAPE (the map, B % 8, pitches below a row, the 32-bit limits, the
 * grid); csrc/input_grad_bf16_plan.h states them one by one. */
int bbb_first_layer_dgrad_bf16(const bbb_conv_desc_t* d, const void* g_pre, int64_t g_row_pitch, const void* w, float* dcol,
                               int64_t d_row_pitch, uint32_t flags, void* stream);
/* What that launch takes (host only): *tile_j rows of D (32 when cin*kh*kw <= 32, else 64: a function of the layer alone) and
 * *tile_n = 128 columns per workgroup, *k_chunks = ceil(E*cout / 32) steps of the contraction every workgroup walks, *blocks
 * workgroups: the (row tile, column tile) pairs rounded up to a multiple of 8 (dealt to the 8 XCDs in runs, so that the row tiles
 * that read one tile of g_pre share an L2).  Out-pointers may be NULL; the launch entry's codes for every check that does not involve an operand pointer. */
int bbb_first_layer_dgrad_bf16_plan(const bbb_conv_desc_t* d, int64_t g_row_pitch, int64_t d_row_pitch, uint32_t flags,
                                    int32_t* tile_j, int32_t* tile_n, int32_t* k_chunks, int64_t* blocks);

/* bf16 input gradients of LRT models, additive in ABI 13 (opt-in from Python: LaunchConfig.bf16_lrt_input_grad; csrc/pool2d_bf16.hip):
 * the activation side of a local-reparameterisation layer's backward on bf16 planes -- bbb_lrt_pool_act_bwd_chwn on
 * bbb_pool_act_bwd_chwn_bf16's storage rules, for frozen parameters (there is no weight side, and no average-pool form).
 *   y [planes][h][w][B] bf16, the stored activated output bf16(act(act_mu + sqrt(act_var) * eps)) (NULL only with k = 0 and act = 0:
 *   the logits layer, whose output is fp32 and enters nothing); act_var fp32 [moment_planes][h][w][B]
 *   (moment_planes = planes, or one draw's worth when every draw shares one pair of moments; a multiple of `channels` that divides
 *   planes); g_out [planes][hp][wp][B] bf16 or, with BBB_BF16_BWD_G_F32, fp32; or, g_out2 != NULL (never with BBB_BF16_BWD_G_F32), the
 *   incoming gradient is fmaf(2 * x_out, g_out2, g_out) in fp32: the two bf16 input gradients of the layer above and this layer's
 *   (pooled) bf16 output x_out [x_planes][hp][wp][B], x_planes dividing planes.  k, s: MaxPool2d(k, s), k = 0 the activation alone.
 *     g_act = the routing of bbb_pool_act_bwd_chwn_bf16 (first maximum in scan order among the stored bf16 values)
 *     g_mu  = g_act * act'(y)                      -> bf16, one rounding
 *     g_var = g_mu * eps / (2 sqrt(act_var))       -> bf16, one rounding (from the fp32 g_mu)
 *   with eps REGENERATED from the counter: the forward's element of the pre-pool output -- canonical index
 *   ((b + b_offset) * channels + n) * h * w + pixel, n = plane % channels, call call0 + *call_dev + plane / channels, stream_id, as
 *   bbb_lrt_sample_chwn_bf16 / bbb_lrt_conv2d_chwn_bf16_fwd draw it.  Everything else fp32 in registers.  g_mu / g_var dense, or planes
 *   at out_plane_pitch elements (% 8 == 0).  16-byte vector loads and stores only, no atomics, no scratch, the same bits on every run.
 *   Checks, before any launch: BBB_EINVAL (a null operand, act, a flag other than BBB_BF16_BWD_G_F32, b_offset < 0, non-positive or
 *   non-dividing plane / channel counts, half a combine or one with fp32 g_out, then the pooling plan's: non-positive sizes),
 *   BBB_ESHAPE (B % 8 != 0, a window larger than the map, index ranges), BBB_EALIGN (an operand that is not 16-byte aligned). */
int bbb_lrt_pool_act_bwd_chwn_bf16(const void* g_out, const void* y, const float* act_var, void* g_mu, void* g_var, int64_t planes,
                                   int64_t moment_planes, int channels, int h, int w, int batch, int k, int s, int act,
                                   int64_t out_plane_pitch, const void* g_out2, const void* x_out, int64_t x_planes, uint64_t seed,
                                   uint32_t call0, const uint32_t* call_dev, uint32_t stream_id, int b_offset, uint32_t flags,
                                   void* stream);

/* Library / device introspection (host-only). */
int bbb_abi_version(void);
const char* bbb_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* BBB_HIP_H */
