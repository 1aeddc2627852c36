// First-layer input gradient of the batch-innermost training backward (bbb_hip/fast_train.py): d loss / d x for the caller's batch,
// which every Monte-Carlo draw shares -- saliency maps and adversarial steps through ensemble.mc_forward / train.forward_loss.
//   dx[b][ci][h][w] = sum_e sum_co sum_(r,q) g_pre[e][co][ho][wo][b] * w[e][co][ci][r][q],  h = ho*sh - ph + r*dh, w = wo*sw - pw + q*dw
// The contraction over (e, co) runs on the forward GEMM as a 1x1 "convolution" (bbb_hip/ops.py: first_layer_input_grad):
//   D[(ci, r, q)][ho][wo][b] = sum_(e,co) W[(e, co)][(ci, r, q)] * G[(e, co)][ho][wo][b]
// and this file holds the gather that folds D back onto the input pixels (col2im): every input pixel sums the taps that reach it in
// ascending (r, q) order, one thread per (pixel, image) -- no atomics, the same bits on every run -- and the result is written in the
// caller's NCHW layout through an LDS transpose (reads run along the images, writes along the pixels of an image).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "conv_desc_check.h"

namespace {

constexpr int kTileP = 32;      // NCHW positions (ci, h, w) per workgroup: 128 contiguous bytes of an image's gradient
constexpr int kTileB = 64;      // images per workgroup: one per lane of a wave

// LRT: dx = (sum over set 0) + 2 x * (sum over set 1), set 1 `set_stride` elements behind set 0 (bbb_lrt_glue mode 1's arithmetic)
template <bool LRT>
__global__ __launch_bounds__(256) void col2im_nchw_kernel(const float* __restrict__ dcol, int64_t row_pitch, int64_t set_stride,
                                                          const float* __restrict__ x, float* __restrict__ dx, int B, int H, int W,
                                                          int Ho, int Wo, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                                          int64_t chw, int64_t p_tiles) {
    // [image][position], rows padded by one: the phase-1 writes (lanes = images) and the phase-2 reads (lanes = positions) both hit
    // 32 distinct banks per half wave
    __shared__ float t0[kTileB][kTileP + 1];
    __shared__ float t1[LRT ? kTileB : 1][kTileP + 1];
    const int64_t tile = blockIdx.x;
    const int64_t p0 = (tile % p_tiles) * kTileP;
    const int b0 = (int)(tile / p_tiles) * kTileB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = b0 + lane;
    for (int i = wave; i < kTileP; i += 4) {
        const int64_t p = p0 + i;
        float a0 = 0.0f, a1 = 0.0f;
        if (p < chw && b < B) {
            const int w = (int)(p % W);
            const int64_t t = p / W;
            const int h = (int)(t % H);
            const int ci = (int)(t / H);
            // the taps that reach (h, w): h + ph = ho*sh + r*dh with 0 <= ho < Ho, 0 <= r < kh -- walked as output rows ho from the
            // highest down, i.e. r ascending (and q ascending inside), ~kh*dh/sh candidates instead of kh divisions
            const int hp = h + ph, wp = w + pw;
            const int ho_hi = min(hp / sh, Ho - 1), wo_hi = min(wp / sw, Wo - 1);
            for (int ho = ho_hi; ho >= 0; --ho) {
                const int rd = hp - ho * sh;             // = r * dh
                if (rd > (kh - 1) * dh) break;
                if (dh != 1 && rd % dh != 0) continue;
                const int r = dh == 1 ? rd : rd / dh;
                for (int wo = wo_hi; wo >= 0; --wo) {
                    const int qd = wp - wo * sw;
                    if (qd > (kw - 1) * dw) break;
                    if (dw != 1 && qd % dw != 0) continue;
                    const int q = dw == 1 ? qd : qd / dw;
                    const int64_t off = ((int64_t)(ci * kh + r) * kw + q) * row_pitch + ((int64_t)ho * Wo + wo) * B + b;
                    a0 += dcol[off];
                    if (LRT) a1 += dcol[set_stride + off];
                }
            }
        }
        t0[lane][i] = a0;
        if (LRT) t1[lane][i] = a1;
    }
    __syncthreads();
    const int pl = threadIdx.x % kTileP;
    const int64_t p = p0 + pl;
    if (p >= chw) return;
    for (int bl = threadIdx.x / kTileP; bl < kTileB; bl += 256 / kTileP) {
        const int bb = b0 + bl;
        if (bb >= B) break;
        const int64_t o = (int64_t)bb * chw + p;
        float v = t0[bl][pl];
        if (LRT) v = fmaf(2.0f * x[o], t1[bl][pl], v);
        dx[o] = v;
    }
}

}  // namespace

extern "C" int bbb_input_grad_col2im(const float* dcol, int64_t row_pitch, int64_t set_stride, const float* x, float* dx,
                                     const bbb_conv_desc_t* d, void* stream) {
    using conv_desc_check::mul_cap;
    if (dcol == nullptr || dx == nullptr || d == nullptr || !conv_desc_check::positive_map(d)) return BBB_EINVAL;
    if ((((uintptr_t)dcol | (uintptr_t)x | (uintptr_t)dx) & 3u) != 0) return BBB_EALIGN;
    int32_t ho = 0, wo = 0;
    if (const int rc = conv_desc_check::out_map(d, &ho, &wo)) return rc;
    const int64_t J = mul_cap(d->cin, d->kh, d->kw);
    if (J > 0x7fffffffLL || row_pitch < mul_cap(ho, wo, d->batch)) return BBB_ESHAPE;
    if (x != nullptr && set_stride < mul_cap(J, row_pitch)) return BBB_ESHAPE;   // the two sets of an LRT layer must not overlap
    const int64_t chw = mul_cap(d->cin, d->h, d->w);
    const int64_t p_tiles = (chw + kTileP - 1) / kTileP;
    const int64_t blocks = mul_cap(p_tiles, (d->batch + kTileB - 1) / kTileB);
    if (blocks > 0x7fffffffLL) return BBB_ESHAPE;
    if (x != nullptr)
        hipLaunchKernelGGL(col2im_nchw_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dcol, row_pitch, set_stride,
                           x, dx, d->batch, d->h, d->w, ho, wo, d->kh, d->kw, d->stride_h, d->stride_w, d->pad_h, d->pad_w, d->dil_h,
                           d->dil_w, chw, p_tiles);
    else
        hipLaunchKernelGGL(col2im_nchw_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dcol, row_pitch, (int64_t)0,
                           x, dx, d->batch, d->h, d->w, ho, wo, d->kh, d->kw, d->stride_h, d->stride_w, d->pad_h, d->pad_w, d->dil_h,
                           d->dil_w, chw, p_tiles);
    return (int)hipGetLastError();
}
