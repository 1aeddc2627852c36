// The local-reparameterisation (LRT) form of the bf16 pixel-major implicit GEMM of pconv_bf16.hip
// (layers/BBB_LRT/BBBConv.py:71-81, BBBLinear.py:65-73 on bf16 storage):
//   act_mu  = sum x * bf16(W_mu) + b_mu
//   act_var = 1e-16 + sum bf16(x^2) * bf16(sigma^2) + sigma_b^2
//   y       = act(act_mu + sqrt(act_var) * eps)
// Same decomposition as pconv_bf16_kernel -- one workgroup = (output pixel, 64 | 128 channels, 128 | 256 images), weights as the
// MFMA "A" operand, [k][b] image rows in LDS, the k-contiguous image operand from the LDS transpose read, tap-major rows skip the
// taps that fall into the padding -- with TWO accumulator sets per wave fed from ONE staged image tile: the weight tile holds the
// W_mu rows of the workgroup's channels and, behind them, their sigma^2 rows; the image operand of the variance contraction is the
// square of the staged bf16 value, formed in fp32 (exact: 8 x 8 significant bits) and rounded once to bf16 (nearest even).
// Where x^2 is formed: in registers, right after the transpose read (16 multiplies + 8 packed conversions per 16-k step and wave,
// beside 8 MFMAs) -- no second image tile in LDS, no second set of transpose reads on the LDS pipe, which is what the parent
// kernel saturates first.  (Squaring once per workgroup while staging, into a second LDS tile, gave the same bits and measured
// slower on every AlexNet layer: profiles/bf16_lrt_notes.md section 3.)
// LRT weights do not depend on the draw: every slab of a launch reads the same two weight matrices (bbb_lrt_weights_bf16 writes
// them, once per step), so there is no per-draw weight tensor and no parameter pass per draw.
// eps is the element the fp32 kernel draws (pconv_body.cuh, LRT epilogue): canonical NCHW index of the draw's [B][Cout][Ho][Wo]
// slab keyed by the global image index, stream (seed, call0 + slab, stream_id).
// Summation order: a k-group adds its 64-k tiles in order and the groups are added in group order, so the bits of an output
// depend on the number of k-groups only -- which the launcher derives from the LAYER's geometry, never from the launch size: a
// draw computed alone, inside a 10-draw launch or as one of several steps per launch is the same number.  Tile shape and wave
// specialisation follow the launch size; they do not change a bit.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/bbb_hip.h"
#include "bbb_common.cuh"
#include "pconv_args.h"
#include "pconv_bf16_plan.h"
#include "smem_attr.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

using bf16_plan::BK;                     // (k per tile, weight row pitch, k per decode chunk and k-group: pconv_bf16_plan.h)
using bf16_plan::LDWB;
using bf16_plan::KCH;
constexpr int TPC = KCH / BK;

__device__ __forceinline__ uint16_t f2bf(float v) {              // round to nearest even (v_cvt_pk_bf16_f32)
    return __builtin_bit_cast(uint16_t, (__bf16)v);
}

// bf16(x * x) of eight stored bf16 values: widened exactly, squared exactly in fp32, rounded once
__device__ __forceinline__ bf16x8 square8(bf16x8 b) {
    const u32x4 w = __builtin_bit_cast(u32x4, b);
    u32x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float lo = __builtin_bit_cast(float, w[u] << 16);
        const float hi = __builtin_bit_cast(float, w[u] & 0xFFFF0000u);
        const bf16x2 q = {(__bf16)bbb::mul_rn(lo, lo), (__bf16)bbb::mul_rn(hi, hi)};
        o[u] = __builtin_bit_cast(uint32_t, q);
    }
    return __builtin_bit_cast(bf16x8, o);
}

// Workgroup = KG k-groups x (WN x WM) waves, every wave a 64-channel x 64-image block of BOTH moments (2 x 2 MFMA tiles each:
// 128 accumulator registers per lane; at most 512 threads per workgroup, so every wave has 256 registers).  WS: 4 extra staging
// waves, two LDS stages, as in pconv_bf16_kernel.
template <bool OUT_F32, int WN, int WM, int KG, bool WS>
__global__ __launch_bounds__(64 * WN * WM * KG + (WS ? 256 : 0)) void pconv_bf16_lrt_kernel(const PConvArgs p) {
    static_assert(!WS || KG == 1, "wave specialisation replaces the k-groups");
    constexpr int GT = 64 * WN * WM;                              // MFMA threads per k-group
    constexpr int LT = WS ? 256 : GT;                             // threads that stage one tile
    constexpr int NSTG = WS ? 2 : 1;                              // LDS stages per k-group
    constexpr int BN = 64 * WN, BM = 64 * WM;
    constexpr int LDXB = BM + 32;                                 // image row pitch: = 64 B mod 256 for BM = 128, 256
    constexpr int WROWS = LT / 8, PPS = BN / WROWS, WPASS = 2 * PPS;   // weight tile: [2 * BN] rows (W_mu, then sigma^2), PPS passes per set
    static_assert(PPS * WROWS == BN, "a staging pass must not straddle the two weight sets");
    constexpr int XL = BM / 8, XROWS = LT / XL, XPASS = BK / XROWS;   // image tile: XL lanes x 16 B per row
    constexpr int KCHG = KCH * KG;
    constexpr int kStage = BK * LDXB + 2 * BN * LDWB;             // elements per stage
    extern __shared__ __attribute__((aligned(16))) uint16_t smem[];
    const bool producer = WS && __builtin_amdgcn_readfirstlane((int)threadIdx.x >= GT ? 1 : 0) != 0;
    const int kg = WS ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x / GT);
    uint16_t* Xs = smem + kg * kStage;                            // stage 0 of this group (stage s: + s * kStage)
    uint16_t* Ws = Xs + BK * LDXB;
    int32_t* kt_all = reinterpret_cast<int32_t*>(smem + KG * NSTG * kStage);   // [2][KCHG] image-row offsets per k
    int32_t* kw_all = kt_all + 2 * KCHG;                                   // [2][KCHG] weight-column offsets per k

    const int bid = blockIdx.x;
    const int xcd = bid & 7;
    const int64_t item = (int64_t)xcd * p.per_xcd + (bid >> 3);
    const int64_t item_end = (int64_t)(xcd + 1) * p.per_xcd;
    if (item >= item_end || item >= (int64_t)p.G * p.Mtiles) return;
    const int g = (int)(item / p.Mtiles);
    const int j = (int)(item - (int64_t)g * p.Mtiles);
    const int e = g / p.Ntiles;
    const int ex = p.x_div > 1 ? (e + p.x_off) / p.x_div : e;     // several steps per launch: slab e reads its step's batch
    const int n0 = (g - e * p.Ntiles) * BN;
    const int pix = j / p.nbt;
    const int b0 = (j - pix * p.nbt) * BM;
    const int oh = pix / p.Wo, ow = pix - oh * p.Wo;
    const int ihb = oh * p.sh - p.ph, iwb = ow * p.sw - p.pw;
    const int Kp = p.Kp;
    // in-bounds tap rectangle of this pixel (tap-major rows only; otherwise every tap is enumerated)
    int r_lo = 0, q_lo = 0, nr = p.kh, nq = p.kw;
    if (p.wtap) {
        r_lo = ihb < 0 ? (-ihb + p.dh - 1) / p.dh : 0;
        q_lo = iwb < 0 ? (-iwb + p.dw - 1) / p.dw : 0;
        int r_hi = (p.H - 1 - ihb) >= 0 ? (p.H - 1 - ihb) / p.dh + 1 : 0;
        int q_hi = (p.W - 1 - iwb) >= 0 ? (p.W - 1 - iwb) / p.dw + 1 : 0;
        r_hi = r_hi < p.kh ? r_hi : p.kh;
        q_hi = q_hi < p.kw ? q_hi : p.kw;
        nr = r_hi > r_lo ? r_hi - r_lo : 0;
        nq = q_hi > q_lo ? q_hi - q_lo : 0;
    }
    const int K = p.wtap ? p.Cin * nr * nq : p.K;                 // contraction length of this pixel
    const int niter = (K + BK * KG - 1) / (BK * KG);              // every group runs the same number of iterations

    const int tid = (int)threadIdx.x - kg * GT;                   // thread within its k-group (MFMA role)
    const int ltid = WS ? (int)threadIdx.x - GT : tid;            // thread within the staging team
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = (wave / WM) * 64, wm = (wave % WM) * 64;

    constexpr uint32_t kOOB = 0xFFFFFFF0u;
    constexpr uint32_t kWInv = 0x7FFFFFF0u;                       // + a row offset (< 2^31): out of range, no wrap
    const uint32_t kXInv = p.x_inv;
    const uint16_t* xb = reinterpret_cast<const uint16_t*>(p.x) + (int64_t)ex * p.x_ds;
    const int64_t x_bytes = (int64_t)p.Cin * p.H * p.W * p.B * 2;
    const int64_t w_bytes = (int64_t)p.Cout * Kp * 2;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(xb), 0, (int)x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, (int)w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t w2rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w2), 0, (int)w_bytes, 0x00020000);

    const int wr = ltid >> 3, wseg = (ltid & 7) * 8;
    const uint32_t wbase = (uint32_t)(n0 + wr) * (uint32_t)Kp * 2u;
    const uint32_t wstep = (uint32_t)WROWS * (uint32_t)Kp * 2u;
    const int xkr = ltid / XL, xb8 = (ltid % XL) * 8;
    const uint32_t xcol = (uint32_t)(b0 + xb8) * 2u;

    // k -> (weight column offset, image row offset), float-reciprocal division + fix-up (exact below 2^24)
    const float inv_khkw = 1.0f / (float)p.khkw, inv_kw = 1.0f / (float)p.kw;
    const float inv_cin = 1.0f / (float)p.Cin, inv_nq = nq > 0 ? 1.0f / (float)nq : 0.0f;
    auto fill_chunk = [&](int chunk) {
        for (int i = WS ? ltid : (int)threadIdx.x; i < KCHG; i += WS ? LT : GT * KG) {
            const int k = chunk * KCHG + i;
            uint32_t xo = kXInv, wo = kWInv;
            if (p.wtap) {
                if (k < K) {
                    int t = (int)((float)k * inv_cin);
                    int ci = k - t * p.Cin;
                    if (ci < 0) { --t; ci += p.Cin; } else if (ci >= p.Cin) { ++t; ci -= p.Cin; }
                    int rr = (int)((float)t * inv_nq);
                    int qq = t - rr * nq;
                    if (qq < 0) { --rr; qq += nq; } else if (qq >= nq) { ++rr; qq -= nq; }
                    const int r = r_lo + rr, q = q_lo + qq;
                    wo = (uint32_t)((r * p.kw + q) * p.Cin + ci) * 2u;
                    xo = (uint32_t)((ci * p.H + ihb + r * p.dh) * p.W + iwb + q * p.dw) * (uint32_t)p.B * 2u;
                }
            } else {
                if (k < Kp) wo = (uint32_t)k * 2u;                 // the zero pad columns K..Kp-1 are part of the row
                if (k < K) {
                    int ci = (int)((float)k * inv_khkw);
                    int rq = k - ci * p.khkw;
                    if (rq < 0) { --ci; rq += p.khkw; } else if (rq >= p.khkw) { ++ci; rq -= p.khkw; }
                    int r = (int)((float)rq * inv_kw);
                    int q = rq - r * p.kw;
                    if (q < 0) { --r; q += p.kw; } else if (q >= p.kw) { ++r; q -= p.kw; }
                    const int ih = ihb + r * p.dh, iw = iwb + q * p.dw;
                    if (ih >= 0 && ih < p.H && iw >= 0 && iw < p.W)
                        xo = (uint32_t)((ci * p.H + ih) * p.W + iw) * (uint32_t)p.B * 2u;
                }
            }
            kt_all[(chunk & 1) * KCHG + i] = (int32_t)xo;
            kw_all[(chunk & 1) * KCHG + i] = (int32_t)wo;
        }
    };

    u32x4 wreg[WPASS], xreg[XPASS];
    auto load_tile = [&](int it) {                       // iteration `it`: this group's 64-k tile is it*KG + kg
        const int buf = (it / TPC) & 1;
        const int kb = ((it % TPC) * KG + kg) * BK;
        const uint32_t wo = wbase + (uint32_t)kw_all[buf * KCHG + kb + wseg];   // 8 consecutive k of one tap / one row
        uint32_t xo[XPASS];
#pragma unroll
        for (int ps = 0; ps < XPASS; ++ps) xo[ps] = (uint32_t)kt_all[buf * KCHG + kb + xkr + ps * XROWS] + xcol;
#pragma unroll
        for (int ps = 0; ps < XPASS; ++ps) xreg[ps] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xo[ps], 0, 0));
#pragma unroll
        for (int ps = 0; ps < PPS; ++ps) {               // the same rows and columns of both matrices
            wreg[ps] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wo + (uint32_t)ps * wstep, 0, 0));
            wreg[PPS + ps] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(w2rs, wo + (uint32_t)ps * wstep, 0, 0));
        }
    };
    auto store_tile = [&](int stage) {
        uint16_t* Xd = Xs + stage * kStage;
        uint16_t* Wd = Ws + stage * kStage;
#pragma unroll
        for (int ps = 0; ps < WPASS; ++ps) *reinterpret_cast<u32x4*>(&Wd[(wr + ps * WROWS) * LDWB + wseg]) = wreg[ps];   // row BN + n: sigma^2 of channel n
#pragma unroll
        for (int ps = 0; ps < XPASS; ++ps) *reinterpret_cast<u32x4*>(&Xd[(xkr + ps * XROWS) * LDXB + xb8]) = xreg[ps];
    };

    f32x16 acc[2][2], accv[2][2];                        // act_mu and act_var contractions
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[t][u][r] = 0.0f; accv[t][u][r] = 0.0f; }

    const int lrow = lane & 31, lk = lane >> 5;
    // transpose-read address of this lane inside a 16-k step (see pconv_bf16_kernel)
    const int tg = lane >> 4, tt = lane & 15;
    const int tr_off = ((8 * (tg >> 1) + (tt >> 2)) * LDXB + wm + 16 * (tg & 1) + 4 * (tt & 3));
    typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

    auto mma_tile = [&](int stage) {
        const uint16_t* Xs = smem + (kg * NSTG + stage) * kStage;
        const uint16_t* Ws = Xs + BK * LDXB;
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
            bf16x8 b[2], b2[2], a[2], a2[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const s16x4 blo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(&Xs[tr_off + mt * 32 + kk * 16 * LDXB]));
                const s16x4 bhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(&Xs[tr_off + mt * 32 + (kk * 16 + 4) * LDXB]));
                b[mt] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(blo, bhi, 0, 1, 2, 3, 4, 5, 6, 7));
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                a[nt] = *reinterpret_cast<const bf16x8*>(&Ws[(wn + nt * 32 + lrow) * LDWB + kk * 16 + lk * 8]);
                a2[nt] = *reinterpret_cast<const bf16x8*>(&Ws[(BN + wn + nt * 32 + lrow) * LDWB + kk * 16 + lk * 8]);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[nt], b[mt], acc[nt][mt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) b2[mt] = square8(b[mt]);        // VALU work that overlaps the MFMAs above
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) accv[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[nt], b2[mt], accv[nt][mt], 0, 0, 0);
        }
    };

    if constexpr (WS) {
        if (producer) {
            // ---- staging waves: tile t+1 -> stage (t+1)&1 while the MFMA waves are on stage t&1; tile t+2 in flight ----
            if (niter > 0) fill_chunk(0);
            __syncthreads();                                       // P0: table chunk 0 visible to all staging waves
            if (niter > 0) {
                load_tile(0);
                if (KCHG < K) fill_chunk(1);
                store_tile(0);
            }
            __syncthreads();                                       // P1: stage 0 = tile 0, table chunk 1 visible
            if (niter > 1) load_tile(1);
            for (int t = 0; t < niter; ++t) {
                if (t + 1 < niter) {
                    store_tile((t + 1) & 1);                       // registers hold tile t+1, issued one iteration ago
                    if (t + 2 < niter) load_tile(t + 2);
                }
                // decode chunk c+1 during the first tile of chunk c (c >= 1): same schedule as pconv_bf16_kernel
                if ((t % TPC) == 0 && t / TPC >= 1 && (t / TPC + 1) * KCHG < K) fill_chunk(t / TPC + 1);
                __syncthreads();
            }
            return;
        }
        __syncthreads();                                           // P0
        __syncthreads();                                           // P1
        for (int t = 0; t < niter; ++t) {
            mma_tile(t & 1);
            __syncthreads();
        }
    } else {
        fill_chunk(0);
        __syncthreads();
        load_tile(0);
        if (KCHG < K) fill_chunk(1);
        store_tile(0);
        __syncthreads();
        for (int t = 0; t < niter; ++t) {
            const bool more = (t + 1) < niter;
            if (more) load_tile(t + 1);
            if ((t % TPC) == 1 && t / TPC >= 1 && (t / TPC + 1) * KCHG < K) fill_chunk(t / TPC + 1);
            mma_tile(0);
            __syncthreads();
            if (more) store_tile(0);
            __syncthreads();
        }
    }

    // ---- cross-group reduction (fixed order: group 0 + 1 + ...), one moment after the other through the idle stage memory ----
    if (KG > 1) {
        float* red = reinterpret_cast<float*>(smem);               // [KG-1][64][GT] floats
        auto reduce = [&](f32x16 (&src)[2][2]) {
            if (kg > 0) {
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) red[((kg - 1) * 64 + (nt * 2 + mt) * 16 + r) * GT + tid] = src[nt][mt][r];
            }
            __syncthreads();
            if (kg == 0) {
#pragma unroll
                for (int g2 = 1; g2 < KG; ++g2)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                            for (int r = 0; r < 16; ++r) src[nt][mt][r] += red[((g2 - 1) * 64 + (nt * 2 + mt) * 16 + r) * GT + tid];
            }
            __syncthreads();                                       // the buffer is free for the next moment / the epilogue
        };
        reduce(acc);
        reduce(accv);
        if (kg > 0) return;
    }

    // ---- epilogue: moments, noise, sampling step, activation ----
    const int HoWo = p.Ho * p.Wo;
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.bias ? p.bias : p.w), 0, p.bias ? p.Cout * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t b2rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.bias2 ? p.bias2 : p.w), 0, p.bias2 ? p.Cout * 4 : 0, 0x00020000);
    constexpr int OSZ = OUT_F32 ? 4 : 2;
    const int slab_f32 = (int)((int64_t)p.Cout * HoWo * p.B * 4);
    char* yb = reinterpret_cast<char*>(p.y) + (int64_t)e * p.y_ds * OSZ;
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(yb, 0, p.y ? (int)((int64_t)p.Cout * HoWo * p.B * OSZ) : 0, 0x00020000);
    const bool moments = p.y_mu != nullptr;                       // (the launcher passes both moment outputs or neither)
    const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc(
        moments ? reinterpret_cast<char*>(p.y_mu + (int64_t)e * p.y_ds) : yb, 0, moments ? slab_f32 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(
        moments ? reinterpret_cast<char*>(p.y_var + (int64_t)e * p.y_ds) : yb, 0, moments ? slab_f32 : 0, 0x00020000);
    const uint32_t call = p.call0 + (p.call_dev ? *p.call_dev : 0u) + (uint32_t)e;
    const bool want_y = p.y != nullptr;
    constexpr int TP = 64 + 8;                                    // staging row pitch (elements): 144 B
    uint16_t* T = smem + wave * (64 * TP);
    if constexpr (!OUT_F32) __syncthreads();                      // stage / reduction memory is free from here on
    // (one channel tile per call: a loop over both is too large for the unroller, and the accumulators need static indices)
    auto finish_tile = [&](auto nt_c) {
        constexpr int nt = decltype(nt_c)::value;
        {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int nl = nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                const int n = n0 + wn + nl;
                const float bm = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(brs, (uint32_t)n * 4u, 0, 0));
                const float bv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(b2rs, (uint32_t)n * 4u, 0, 0));
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const int b = b0 + wm + mt * 32 + lrow;
                    const bool ok = (b < p.B) & (n < p.Cout);
                    const uint32_t o = (uint32_t)(((int64_t)n * HoWo + pix) * p.B + b);
                    const float mu = acc[nt][mt][r] + bm;
                    const float var = 1e-16f + (accv[nt][mt][r] + bv);
                    if (moments) {
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, mu), mrs, ok ? o * 4u : kOOB, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, var), vrs, ok ? o * 4u : kOOB, 0, 0);
                    }
                    if (want_y) {
                        float v = mu;
                        if (p.sample && ok) {      // canonical NCHW element index of this draw's [B][Cout][Ho][Wo] slab
                            const uint64_t idx = (uint64_t)(((int64_t)(b + p.b_off) * p.Cout + n) * HoWo + pix);
                            float z4[4];
                            bbb::normal4(idx >> 2, p.stream_id, call, p.k0, p.k1, z4);
                            const int c = (int)(idx & 3);
                            const float z = c == 0 ? z4[0] : c == 1 ? z4[1] : c == 2 ? z4[2] : z4[3];
                            v = __builtin_fmaf(__builtin_amdgcn_sqrtf(var), z, mu);
                        }
                        v = bbb::apply_act(v, p.act);
                        if constexpr (OUT_F32) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), yrs, ok ? o * 4u : kOOB, 0, 0);
                        else T[nl * TP + mt * 32 + lrow] = f2bf(v);
                    }
                }
            }
        }
    };
    if (want_y || moments) {
        finish_tile(std::integral_constant<int, 0>{});
        finish_tile(std::integral_constant<int, 1>{});
    }
    if constexpr (!OUT_F32) {
        // hidden layers: the wave's 64 x 64 block through its private LDS image, 16-byte stores of 8 images (pconv_bf16_kernel)
        if (!want_y) return;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int ps = 0; ps < 8; ++ps) {
            const int v = ps * 64 + lane;
            const int row = v >> 3, grp = v & 7;
            const u32x4 q = *reinterpret_cast<const u32x4*>(&T[row * TP + grp * 8]);
            const int n = n0 + wn + row, b = b0 + wm + grp * 8;
            const uint32_t off = ((b < p.B) & (n < p.Cout)) ? (uint32_t)(((int64_t)n * HoWo + pix) * p.B + b) * 2u : kOOB;
            __builtin_amdgcn_raw_buffer_store_b128(q, yrs, off, 0, 0);
        }
    }
}

// (two weight tiles per stage, W_mu and sigma^2: launch_cfg, smem_attr.h)
template <bool OUT_F32, int WN, int WM, int KG, bool WS>
int launch_lrt(const PConvArgs& a, int64_t blocks, hipStream_t st) {
    return launch_cfg<&pconv_bf16_lrt_kernel<OUT_F32, WN, WM, KG, WS>, WN, WM, KG, WS, 2>(a, blocks, st);
}

template <bool OUT_F32>
int launch_shape(const PConvArgs& a, int shape, int kgs, bool ws, int64_t blocks, hipStream_t st) {
    if (shape == 22) {
        if (ws) return launch_lrt<OUT_F32, 2, 2, 1, true>(a, blocks, st);
        return kgs == 2 ? launch_lrt<OUT_F32, 2, 2, 2, false>(a, blocks, st) : launch_lrt<OUT_F32, 2, 2, 1, false>(a, blocks, st);
    }
    if (shape == 14) return kgs == 2 ? launch_lrt<OUT_F32, 1, 4, 2, false>(a, blocks, st) : launch_lrt<OUT_F32, 1, 4, 1, false>(a, blocks, st);
    return kgs == 2 ? launch_lrt<OUT_F32, 1, 2, 2, false>(a, blocks, st) : launch_lrt<OUT_F32, 1, 2, 1, false>(a, blocks, st);
}

// y[e] = bf16(act(act_mu + sqrt(act_var) * eps[e])) for E draws of ONE pair of fp32 moments: the bf16-output form of
// lrt_sample_chwn_kernel (mc_tail.hip) with the sampling step written exactly as the GEMM epilogue above writes it, so that a
// moments-only launch + this equals E sampling launches bit for bit.  One thread = 2 images x PPT consecutive pixels.
template <int PPT>
__global__ __launch_bounds__(256) void lrt_sample_chwn_bf16_kernel(const float* __restrict__ mu, const float* __restrict__ var,
                                                                   uint32_t* __restrict__ y, int E, int C, int HW, int B2, int act,
                                                                   uint32_t k0, uint32_t k1, uint32_t call0, uint32_t stream_id,
                                                                   const uint32_t* __restrict__ call_dev, int b_off) {
    const int64_t HWq = HW / PPT;
    const int64_t total = (int64_t)E * C * HWq * B2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int bp = (int)(i % B2);
    int64_t t = i / B2;
    const int q = (int)(t % HWq);
    t /= HWq;
    const int n = (int)(t % C);
    const int e = (int)(t / C);
    const uint32_t call = call0 + (call_dev ? *call_dev : 0u) + (uint32_t)e;
    float z[2][4];
    uint64_t idx0[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        idx0[h] = (uint64_t)(((int64_t)(2 * bp + h + b_off) * C + n) * HW + (int64_t)q * PPT);   // keyed by the GLOBAL image index
        bbb::normal4(idx0[h] >> 2, stream_id, call, k0, k1, z[h]);
    }
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int64_t o2 = ((int64_t)n * HW + (int64_t)q * PPT + j) * B2 + bp;          // pair offset inside one draw's slab
        uint32_t packed = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = PPT == 4 ? j : (int)(idx0[h] & 3);
            const float zz = c == 0 ? z[h][0] : c == 1 ? z[h][1] : c == 2 ? z[h][2] : z[h][3];
            const float v = __builtin_fmaf(__builtin_amdgcn_sqrtf(var[2 * o2 + h]), zz, mu[2 * o2 + h]);
            packed |= (uint32_t)f2bf(bbb::apply_act(v, act)) << (16 * h);
        }
        y[(int64_t)e * C * HW * B2 + o2] = packed;
    }
}

// fp32 [rows][cin][taps] -> bf16 [rows][Kp] in the GEMM's row layout (pitch K rounded up to 8, zero pad; taps > 0: tap-major
// columns t * cin + ci), every segment of the table in one launch: blockIdx.y = segment, one thread = 8 output columns.
struct RowSegs { bbb_bf16_rows_segment_t s[BBB_BF16_ROWS_MAX_SEGMENTS]; };
__global__ __launch_bounds__(256) void rows_to_bf16_kernel(const RowSegs segs) {
    const bbb_bf16_rows_segment_t& s = segs.s[blockIdx.y];
    const int K = s.row_len, Kp8 = (K + 7) >> 3;
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= s.rows * Kp8) return;
    const int64_t row = v / Kp8;
    const int k0 = (int)(v - row * Kp8) * 8;
    const float* src = s.src + row * K;
    const int cin = s.taps > 0 ? K / s.taps : K;
    u32x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float f[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = k0 + 2 * u + h;
            f[h] = 0.0f;
            if (k < K) {
                if (s.taps > 0) { const int t = k / cin, ci = k - t * cin; f[h] = src[ci * s.taps + t]; }
                else f[h] = src[k];
            }
        }
        o[u] = (uint32_t)f2bf(f[0]) | ((uint32_t)f2bf(f[1]) << 16);
    }
    reinterpret_cast<u32x4*>(s.dst)[v] = o;
}

}  // namespace

extern "C" int bbb_lrt_weights_bf16(const bbb_bf16_rows_segment_t* segs, int nseg, void* stream) {
    if (segs == nullptr || nseg <= 0 || nseg > BBB_BF16_ROWS_MAX_SEGMENTS) return BBB_EINVAL;
    RowSegs a = {};
    int64_t most = 0;
    for (int i = 0; i < nseg; ++i) {
        const bbb_bf16_rows_segment_t& s = segs[i];
        if (s.src == nullptr || s.dst == nullptr || s.rows <= 0 || s.row_len <= 0 || s.taps < 0) return BBB_EINVAL;
        if (s.taps > 0 && (s.row_len % s.taps != 0 || (s.row_len / s.taps) % 8 != 0)) return BBB_ESHAPE;   // a 16-byte vector must not straddle two taps
        if (((uintptr_t)s.src & 3u) != 0 || ((uintptr_t)s.dst & 15u) != 0) return BBB_EALIGN;
        const int64_t vecs = s.rows * ((s.row_len + 7) >> 3);
        most = vecs > most ? vecs : most;
        a.s[i] = s;
    }
    const int64_t blocks = (most + 255) / 256;
    if (blocks > 0x7fffffffLL) return BBB_ESHAPE;
    hipLaunchKernelGGL(rows_to_bf16_kernel, dim3((unsigned)blocks, (unsigned)nseg), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int bbb_lrt_sample_chwn_bf16(const float* act_mu, const float* act_var, void* y, int draws, int channels, int pixels,
                                        int batch, int b_offset, int act, uint64_t seed, uint32_t call0, uint32_t stream_id,
                                        const uint32_t* call_dev, void* stream) {
    if (act_mu == nullptr || act_var == nullptr || y == nullptr || draws <= 0 || channels <= 0 || pixels <= 0 || batch <= 0 ||
        act < 0 || act > 2 || b_offset < 0)
        return BBB_EINVAL;
    if (batch % 8 != 0) return BBB_ESHAPE;
    if ((((uintptr_t)act_mu | (uintptr_t)act_var) & 7u) != 0 || ((uintptr_t)y & 3u) != 0) return BBB_EALIGN;
    const int ppt = pixels % 4 == 0 ? 4 : 1;
    const int64_t total = (int64_t)draws * channels * (pixels / ppt) * (batch / 2);
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return BBB_ESHAPE;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (ppt == 4)
        hipLaunchKernelGGL(lrt_sample_chwn_bf16_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, act_mu, act_var,
                           reinterpret_cast<uint32_t*>(y), draws, channels, pixels, batch / 2, act, k0, k1, call0, stream_id, call_dev, b_offset);
    else
        hipLaunchKernelGGL(lrt_sample_chwn_bf16_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, act_mu, act_var,
                           reinterpret_cast<uint32_t*>(y), draws, channels, pixels, batch / 2, act, k0, k1, call0, stream_id, call_dev, b_offset);
    return (int)hipGetLastError();
}

extern "C" int bbb_lrt_conv2d_chwn_bf16_plan(const bbb_conv_desc_t* d, uint32_t flags, int32_t* shape, int32_t* k_groups,
                                             int32_t* wave_specialised) {
    (void)flags;
    bf16_plan::LrtPlan p;
    if (const int rc = bf16_plan::lrt_plan(d, &p)) return rc;
    if (shape) *shape = p.tile.shape;
    if (k_groups) *k_groups = p.tile.kgs;
    if (wave_specialised) *wave_specialised = p.tile.ws ? 1 : 0;
    return 0;
}

extern "C" int bbb_lrt_conv2d_chwn_bf16_fwd(const bbb_conv_desc_t* d, const void* x, const void* w_mu, const void* w_var,
                                            const float* b_mu, const float* b_var, void* y, float* act_mu_out, float* act_var_out,
                                            uint64_t seed, uint32_t call0, uint32_t stream_id, int sample, const uint32_t* call_dev,
                                            uint32_t flags, void* stream) {
    const bool out_f32 = (flags & BBB_BF16_OUT_F32) != 0, tap_major = (flags & BBB_BF16_W_TAP_MAJOR) != 0;
    bf16_plan::LrtPlan p;
    if (const int rc = bf16_plan::lrt_plan(d, &p)) return rc;
    if (x == nullptr || w_mu == nullptr || w_var == nullptr) return BBB_EINVAL;
    if ((flags & ~(BBB_BF16_OUT_F32 | BBB_BF16_W_TAP_MAJOR)) != 0 || d->act < 0 || d->act > 2) return BBB_EINVAL;
    if ((b_mu == nullptr) != (b_var == nullptr) || (act_mu_out == nullptr) != (act_var_out == nullptr)) return BBB_EINVAL;
    if (y == nullptr && (act_mu_out == nullptr || sample)) return BBB_EINVAL;        // y may be left out of a moments-only launch
    if (d->w_draw_stride != 0 || d->b_draw_stride != 0) return BBB_EINVAL;           // LRT weights are shared by the slabs
    if (conv_desc_check::unit_fields(d, conv_desc_check::kSteps) != 0 || d->w_row_pitch != 0 || d->w_tap_major != 0 || d->pool != 0 ||
        d->b_offset < 0)
        return BBB_EINVAL;                                                           // steps per launch, no work units, no pooled form
    if (const int rc = bf16_plan::vector_rows(d, tap_major)) return rc;
    bf16_plan::Geom g;
    if (const int rc = bf16_plan::slab_limits(d, p.ho, p.wo, bf16_plan::kLrtLimits, &g)) return rc;
    if ((((uintptr_t)x | (uintptr_t)w_mu | (uintptr_t)w_var) & 15u) != 0 || ((uintptr_t)y & (out_f32 ? 3u : 15u)) != 0 ||
        (((uintptr_t)b_mu | (uintptr_t)b_var | (uintptr_t)act_mu_out | (uintptr_t)act_var_out) & 3u) != 0)
        return BBB_EALIGN;
    if ((d->x_draw_stride & 7) != 0) return BBB_EALIGN;
    bf16_plan::TileGrid t = {};
    if (const int rc = bf16_plan::tile_grid(p.tile.shape, p.work, &t)) return rc;
    PConvArgs a = {};
    bf16_plan::fill_geometry(a, d, g, tap_major);
    a.x = reinterpret_cast<const float*>(x);
    a.w = reinterpret_cast<const float*>(w_mu); a.w2 = reinterpret_cast<const float*>(w_var);
    a.bias = b_mu; a.bias2 = b_var;
    a.y = reinterpret_cast<float*>(y); a.y_mu = act_mu_out; a.y_var = act_var_out;
    a.x_div = d->x_unit_div; a.x_off = d->x_unit_off;
    a.b_off = d->b_offset;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.call0 = call0; a.stream_id = stream_id;
    a.sample = sample ? 1 : 0;
    a.call_dev = call_dev;
    a.Ntiles = t.Ntiles; a.G = t.G; a.nbt = t.nbt; a.Mtiles = t.Mtiles; a.per_xcd = t.per_xcd;
    hipStream_t st = (hipStream_t)stream;
    return out_f32 ? launch_shape<true>(a, p.tile.shape, p.tile.kgs, p.tile.ws, t.blocks, st)
                   : launch_shape<false>(a, p.tile.shape, p.tile.kgs, p.tile.ws, t.blocks, st);
}
