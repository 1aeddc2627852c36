// Kernel-argument block shared by the five pixel-major GEMM families (pconv_gemm.hip, pconv_dgrad.hip, pconv_bf16.hip,
// pconv_bf16_lrt.hip, pconv_c8x3.hip), and the tap enumeration of the transposed forms (tr_axis: pconv_dgrad.hip, pconv_bf16.hip).
#pragma once
#include <stdint.h>

struct PConvArgs {
    const float* x;
    const float* w;
    const float* w2;
    const float* bias;
    const float* bias2;
    float* y;
    float* y_mu;
    float* y_var;
    const float* eps_ext;
    int64_t x_ds, w_ds, b_ds, y_ds;
    int32_t B, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo;
    int32_t K, Kp, khkw, act, sample;   // Kp: bf16 weight row pitch (pconv_bf16.hip)
    int32_t Mtiles, nbt, Ntiles, G, per_xcd;
    uint32_t k0, k1, call0, stream_id;
    int32_t wtap;        // bf16: weight rows are tap-major ((r, q, ci) order)
    uint32_t x_inv;      // byte offset that marks an invalid image row: x_inv + any column offset is out of range and does not wrap
    const uint32_t* call_dev;
    int32_t unit_div, unit_off, x_mod, b_off;   // work units (include/bbb_hip.h, bbb_conv_desc_t); unit_div <= 1: slab = draw
    int32_t ksplit;      // split contraction (pconv_body.cuh, SPLIT): k ranges per item, 0 / 1 = none
    int32_t* tickets;    // [items] arrival counters, zero between launches
    float* part;         // [items][ksplit][sets][64][BM] partial accumulator tiles
    int32_t px_run;      // pconv_bf16_smallk_kernel: consecutive output pixels per workgroup
    int64_t x_ps, y_ps;  // pconv_bf16x3 S3 operands: elements between the hi / mid / lo planes of an activation slab
    int32_t pool;        // bbb_conv_desc_t::pool: the launch also applies MaxPool2d(2, 2) to the activated output (pconv_body.cuh, POOL)
    int32_t x_div, x_off; // bbb_conv_desc_t::x_unit_div / x_unit_off: output slab e reads input slab (e + x_off) / x_div (x_div <= 1: slab e)
    int32_t y_f32;       // pconv_bf16_fewout_kernel: y is fp32 (the logits layer) instead of bf16
    int32_t vh0, vh1, vw0, vw1;   // pconv_c8x3: input rows [vh0, vh1) x columns [vw0, vw1) may hold non-zero data (the rest is declared zero)
    int32_t y_c8;        // pconv_bf16.hip: y is written channel-interleaved, [cout / 8][ho][wo][B][8] (BBB_BF16_OUT_C8)
    int32_t up_h, up_w, tstep_h, tstep_w;   // pconv_body.cuh, TR (the strided input gradient): the layer's stride and the step between taps that take part
};

// TR, one axis of the transposed ("fractionally strided") item (pconv_body.cuh, pconv_bf16.hip): the taps r = lo + i * step, i < cnt,
// are those with t = base + r * d >= 0, t % up == 0 and t / up < n -- an arithmetic progression with step = up / gcd(up, d) whose
// first member is among the first `step` taps (bbb_hip/ops.py: dgrad_tap_plan restates it on the host)
__device__ __forceinline__ void tr_axis(int base, int d, int up, int step, int k, int n, int& lo, int& cnt) {
    lo = 0; cnt = 0;
    int first = -1;
    for (int r = 0; r < step && r < k; ++r)
        if ((base + r * d) % up == 0) { first = r; break; }
    if (first < 0) return;
    const int t0 = base + first * d, sd = step * d;                  // (sd is a multiple of up: members stay divisible)
    const int r0 = first + (t0 < 0 ? (-t0 + sd - 1) / sd : 0) * step;
    const int lim = (n - 1) * up - base;                              // r * d <= lim  <=>  t / up <= n - 1
    if (lim < 0) return;
    int r1 = lim / d;
    r1 = r1 < k - 1 ? r1 : k - 1;
    if (r1 < r0) return;
    lo = r0; cnt = (r1 - r0) / step + 1;
}
