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

extern "C" int bbb_conv2d_chwn_dgrad(const bbb_conv_desc_t* d, const float* g_pre, const float* w_flipped, float* dx, int up_h,
                                     int up_w, int out_h, int out_w, void* stream) {
    if (d == nullptr) return BBB_EINVAL;
    if (d->batch <= 0 || d->cin <= 0 || d->h <= 0 || d->w <= 0 || d->cout <= 0 || d->kh <= 0 || d->kw <= 0 || d->pad_h < 0 ||
        d->pad_w < 0 || d->dil_h <= 0 || d->dil_w <= 0 || d->draws <= 0 || up_h <= 0 || up_w <= 0 || out_h <= 0 || out_w <= 0)
        return BBB_EINVAL;
    // d describes the stride-1 launch on the flipped weights; the layer's stride travels as the upsampling factors
    if (d->stride_h != 1 || d->stride_w != 1) return BBB_EINVAL;
    if (up_h == 1 && up_w == 1) return BBB_EINVAL;          // a stride-1 layer's gradient is bbb_conv2d_chwn_fwd: one way to compute it
    if (d->act != 0 || d->pool != 0 || d->w_tap_major != 0 || d->w_row_pitch != 0 || d->unit_div != 0 || d->unit_off != 0 ||
        d->x_unit_mod != 0 || d->x_unit_div != 0 || d->x_unit_off != 0 || d->b_offset != 0)
        return BBB_EINVAL;
    if (d->x_draw_stride < 0 || d->w_draw_stride < 0) return BBB_EINVAL;
    if (d->batch % 4 != 0) return BBB_ESHAPE;
    // (out_h, out_w) must be a map whose forward (padding p = d (k - 1) - q >= 0, stride up) gives exactly the g map of d
    const int fph = d->dil_h * (d->kh - 1) - d->pad_h, fpw = d->dil_w * (d->kw - 1) - d->pad_w;
    if (fph < 0 || fpw < 0) return BBB_ESHAPE;
    const int64_t nh = (int64_t)out_h + 2 * fph - (int64_t)d->dil_h * (d->kh - 1) - 1;
    const int64_t nw = (int64_t)out_w + 2 * fpw - (int64_t)d->dil_w * (d->kw - 1) - 1;
    if (nh < 0 || nw < 0 || nh / up_h + 1 != d->h || nw / up_w + 1 != d->w) return BBB_ESHAPE;
    // per-draw slabs are addressed through 32-bit buffer offsets (as in the forward's checks)
    const int64_t g_bytes = (int64_t)d->cin * d->h * d->w * d->batch * 4, dx_bytes = (int64_t)d->cout * out_h * out_w * d->batch * 4;
    if ((int64_t)d->cin * d->h * d->w > 0x7fffffffLL || (int64_t)d->cin * d->kh * d->kw > 0x7fffffffLL) return BBB_ESHAPE;
    if (g_bytes > 0xFFFE0000LL || dx_bytes > 0xFFFE0000LL || ((int64_t)d->cout + 64) * d->cin * d->kh * d->kw * 4 > 0x3FFFFFFFLL ||
        (int64_t)d->batch * 4 > 0x0FFFFFFFLL)
        return BBB_ESHAPE;
    PConvArgs a = {};
    a.x_inv = (0xFFFFFFF0u - ((uint32_t)d->batch + 512u) * 4u) & ~15u;
    if (g_bytes > (int64_t)a.x_inv) return BBB_ESHAPE;
    if (g_pre == nullptr || w_flipped == nullptr || dx == nullptr) return BBB_EINVAL;
    if ((((uintptr_t)g_pre | (uintptr_t)dx) & 15u) != 0 || (((uintptr_t)w_flipped) & 3u) != 0) return BBB_EALIGN;
    a.x = g_pre; a.w = w_flipped; a.y = dx;
    a.B = d->batch; a.Cin = d->cin; a.H = d->h; a.W = d->w; a.Cout = d->cout; a.kh = d->kh; a.kw = d->kw;
    a.sh = 1; a.sw = 1; a.ph = d->pad_h; a.pw = d->pad_w; a.dh = d->dil_h; a.dw = d->dil_w;
    a.Ho = out_h; a.Wo = out_w; a.K = d->cin * d->kh * d->kw; a.Kp = a.K; a.khkw = d->kh * d->kw;
    a.x_ds = d->x_draw_stride; a.w_ds = d->w_draw_stride;
    a.y_ds = (int64_t)d->cout * out_h * out_w * d->batch;
    a.up_h = up_h; a.up_w = up_w;
    a.tstep_h = up_h / gcd(up_h, d->dil_h); a.tstep_w = up_w / gcd(up_w, d->dil_w);
    // items and tile choice as the forward launcher makes them (pconv_gemm.hip, launch()): 128-image tiles unless that leaves
    // fewer than 3 workgroups per CU or pads the image axis by a quarter; staging loads interleaved with the MFMAs for launches
    // of up to ~12k items
    a.Ntiles = (a.Cout + BN - 1) / BN;
    a.G = a.Ntiles * d->draws;
    const int64_t pixels = (int64_t)out_h * out_w;
    const int64_t nb128 = pixels * ((a.B + 127) / 128) * a.G;
    int bm = nb128 < 768 ? 64 : 128;
    if (bm == 128 && (a.B + 127) / 128 * 128 * 4 >= a.B * 5 && (a.B + 63) / 64 * 64 < (a.B + 127) / 128 * 128) bm = 64;
    a.nbt = (a.B + bm - 1) / bm;
    const int64_t mt = pixels * a.nbt;
    if (mt > 0x7fffffffLL) return BBB_ESHAPE;
    a.Mtiles = (int)mt;
    const int64_t items = (int64_t)a.G * mt;
    const int64_t per = (items + 7) / 8;
    if (8 * per > 0x7fffffffLL) return BBB_ESHAPE;
    a.per_xcd = (int32_t)per;
    const bool ilv = items <= 12000;
    const dim3 grid((unsigned)(8 * per)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (bm == 128) {
        if (ilv) hipLaunchKernelGGL((pconv_dgrad_kernel<128, true>), grid, block, 0, st, a);
        else     hipLaunchKernelGGL((pconv_dgrad_kernel<128, false>), grid, block, 0, st, a);
    } else {
        if (ilv) hipLaunchKernelGGL((pconv_dgrad_kernel<64, true>), grid, block, 0, st, a);
        else     hipLaunchKernelGGL((pconv_dgrad_kernel<64, false>), grid, block, 0, st, a);
    }
    return (int)hipGetLastError();
}
