// Input gradient of a STRIDED convolution in the batch-innermost layout: the transposed ("fractionally strided") form of the
// fp32 pixel-major GEMM (pconv_body.cuh, TR).
//
// For y = conv(x, w) with stride (sh, sw), padding (ph, pw), dilation (dh, dw):
//     dx[e][ci][ih][iw][b] = sum over co and the taps (r', q') of g[e][co][oh][ow][b] * wf[e][ci][co][r'][q']
// with wf the flipped, channel-transposed weights (bbb_flip_transpose_w*), qh = dh * (kh - 1) - ph, t = ih - qh + r' * dh, and
// tap r' taking part iff t >= 0, t % sh == 0 and oh = t / sh < Ho (columns alike).  One workgroup owns one pixel (ih, iw) of dx,
// 64 of its channels and 64 | 128 images, as in the forward; the taps that take part form an arithmetic progression per axis
// (step s / gcd(s, d)), so the in-bounds taps are still a rectangle nr x nq and only the per-pixel tap ranges and the
// k_eff -> (weight offset, g row) table differ from the forward's item: the k loop, the staging, the MFMA schedule and the
// epilogue are the forward's.  No product with an inserted zero and no padding tap is computed -- the (pixel, tap) pairs visited
// are exactly the forward launch's in-bounds pairs -- and a pixel no tap reaches (s > d * (k - 1) + 1, rows the forward's floor
// dropped) has an empty contraction and is stored as zeros.  One fmaf chain per output element in a fixed order, no atomics, no
// scratch; the contraction is never split, so a draw's gradient is the same number whatever else shares the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "bbb_common.cuh"
#include "pconv_args.h"
#include "pconv_body.cuh"
#include "pconv_plan.h"

namespace {

using namespace pconv;

template <int BM, bool ILV>
__global__ __launch_bounds__(kThreads) void pconv_dgrad_kernel(const PConvArgs p) {
    // block -> work item as in pconv_gemm_kernel: weight-tile sharers on one XCD
    const int bid = blockIdx.x;
    const int xcd = bid & 7;
    const int64_t item = (int64_t)xcd * p.per_xcd + (bid >> 3);
    const int64_t item_end = (int64_t)(xcd + 1) * p.per_xcd;
    if (item >= item_end || item >= (int64_t)p.G * p.Mtiles) return;
    pconv_item<BM, false, ILV, kPlain, true>(p, item);
}

int gcd(int a, int b) {
    while (b != 0) { const int t = a % b; a = b; b = t; }
    return a;
}

}  // namespace

extern "C" int bbb_conv2d_chwn_dgrad_plan(const bbb_conv_desc_t* d, int up_h, int up_w, int out_h, int out_w, int32_t* bm, int32_t* ilv,
                                          int64_t* items, int64_t* blocks) {
    pconv_plan::Plan pl;
    uint32_t x_inv = 0;
    if (const int rc = pconv_plan::dgrad_plan(d, up_h, up_w, out_h, out_w, 0, &x_inv, &pl)) return rc;
    if (bm) *bm = pl.bm;
    if (ilv) *ilv = pl.ilv;
    if (items) *items = pl.items;
    if (blocks) *blocks = pl.blocks;
    return 0;
}

// The checks, the tile and the grid: pconv_plan.h (dgrad_plan: items and tile choice are the forward launcher's own rule).
extern "C" int bbb_conv2d_chwn_dgrad(const bbb_conv_desc_t* d, const float* g_pre, const float* w_flipped, float* dx, int up_h,
                                     int up_w, int out_h, int out_w, void* stream) {
    int ptr_rc = 0;
    if (g_pre == nullptr || w_flipped == nullptr || dx == nullptr) ptr_rc = BBB_EINVAL;
    else if ((((uintptr_t)g_pre | (uintptr_t)dx) & 15u) != 0 || (((uintptr_t)w_flipped) & 3u) != 0) ptr_rc = BBB_EALIGN;
    pconv_plan::Plan pl;
    PConvArgs a = {};
    if (const int rc = pconv_plan::dgrad_plan(d, up_h, up_w, out_h, out_w, ptr_rc, &a.x_inv, &pl)) return rc;
    a.x = g_pre; a.w = w_flipped; a.y = dx;
    a.B = d->batch; a.Cin = d->cin; a.H = d->h; a.W = d->w; a.Cout = d->cout; a.kh = d->kh; a.kw = d->kw;
    a.sh = 1; a.sw = 1; a.ph = d->pad_h; a.pw = d->pad_w; a.dh = d->dil_h; a.dw = d->dil_w;
    a.Ho = out_h; a.Wo = out_w; a.K = d->cin * d->kh * d->kw; a.Kp = a.K; a.khkw = d->kh * d->kw;
    a.x_ds = d->x_draw_stride; a.w_ds = d->w_draw_stride;
    a.y_ds = (int64_t)d->cout * out_h * out_w * d->batch;
    a.up_h = up_h; a.up_w = up_w;
    a.tstep_h = up_h / gcd(up_h, d->dil_h); a.tstep_w = up_w / gcd(up_w, d->dil_w);
    a.Ntiles = pl.Ntiles; a.G = pl.G; a.nbt = pl.nbt; a.Mtiles = pl.Mtiles; a.per_xcd = pl.per_xcd;
    const dim3 grid((unsigned)pl.blocks), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (pl.bm == 128) {
        if (pl.ilv) hipLaunchKernelGGL((pconv_dgrad_kernel<128, true>), grid, block, 0, st, a);
        else        hipLaunchKernelGGL((pconv_dgrad_kernel<128, false>), grid, block, 0, st, a);
    } else {
        if (pl.ilv) hipLaunchKernelGGL((pconv_dgrad_kernel<64, true>), grid, block, 0, st, a);
        else        hipLaunchKernelGGL((pconv_dgrad_kernel<64, false>), grid, block, 0, st, a);
    }
    return (int)hipGetLastError();
}
