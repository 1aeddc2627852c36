// The bf16 training backward's glue (training extension, bf16 storage mode): everything around the
// gradient contractions, which themselves run on the bf16 forward GEMM (bbb_conv2d_chwn_bf16_fwd):
//   * per-plane sums of a bf16 tensor (bias gradients, fp32 accumulation),
//   * the flipped, channel-transposed bf16 weight rows of an input gradient (dgrad operand at the bf16 GEMM's row pitch),
//   * [E][C][P][B] -> [E][B][P][Cpad] (the input of a role-swapped weight gradient; pad channels zero),
//   * [E][R][B] -> [E][S][R][B/S] (the output gradient as S batch chunks of tap-major weight rows: a K split run as extra draws).
// All of them move 16-byte vectors of 8 bf16 where they store, deterministic (fixed reduction trees, no atomics).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bbb_hip.h"
#include "bf16_pack.cuh"

namespace {

using namespace bf16_pack;

// out[r] = sum over j < cols of x[r * row_pitch + j] (bf16 in, fp32 out).  One 256-thread block per row: every thread walks
// 16-byte vectors at a stride of 256 (pairwise within a vector, then in index order), then a fixed LDS tree.
__global__ __launch_bounds__(256) void plane_sum_bf16_kernel(const u32x4* __restrict__ x, float* __restrict__ out, int64_t cols8,
                                                             int64_t pitch8) {
    __shared__ float sm[256];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const u32x4* p = x + r * pitch8;
    float acc = 0.0f;
    for (int64_t j = tid; j < cols8; j += 256) {
        float v[8];
        unpack8(p[j], v);
        acc += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    sm[tid] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) sm[tid] += sm[tid + st];
        __syncthreads();
    }
    if (tid == 0) out[r] = sm[0];
}

// out [draws][cin][Kpo] = the rows of w [draws][cout][Kpi] with the taps reversed and the channels transposed.  Row orders:
// IN_TM (r, q, ci) else (ci, r, q); OUT_TM (r, q, co) else (co, r, q).  Kp = row length rounded up to 8; the pad is written zero.
// One thread per 8 consecutive output columns (one 16-byte store).
__global__ __launch_bounds__(256) void flip_transpose_bf16_kernel(const uint16_t* __restrict__ w, u32x4* __restrict__ out, int64_t total8,
                                                                  int cout, int cin, int T, int Kpi, int Kpo, int in_tm, int out_tm) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int kv = (int)(i % (Kpo / 8));
    const int64_t row = i / (Kpo / 8);
    const int ci = (int)(row % cin);
    const int64_t d = row / cin;
    const uint16_t* wd = w + d * cout * (int64_t)Kpi;
    const int Ko = cout * T;
    uint32_t r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = kv * 8 + j;
        uint32_t v = 0;
        if (c < Ko) {
            const int tp = out_tm ? c / cout : c % T;
            const int co = out_tm ? c % cout : c / T;
            const int tap = T - 1 - tp;
            v = wd[(int64_t)co * Kpi + (in_tm ? tap * cin + ci : ci * T + tap)];
        }
        r[j] = v;
    }
    out[i] = u32x4{r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16)};
}

// [E][C][P][B] -> [E][B][P][Cp] through a 64 x 64 LDS tile per (draw, pixel); channels C <= c < Cp are written zero.
// Grid: x = channel tiles x image tiles, y = pixels, z = draws.
__global__ __launch_bounds__(256) void chwn_to_bhwc_bf16_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ out, int C, int P, int B,
                                                                int Cp, int ctiles) {
    __shared__ uint16_t tile[64][72];                  // 144-byte rows: 16-byte aligned, rows four banks apart
    const int ct = blockIdx.x % ctiles, bt = blockIdx.x / ctiles;
    const int p = blockIdx.y;
    const int64_t e = blockIdx.z;
    const int c0 = ct * 64, b0 = bt * 64;
    const int B8 = B / 8, Cp8 = Cp / 8;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = threadIdx.x + 256 * it;
        const int cl = idx >> 3, bv = idx & 7;
        const int c = c0 + cl, b = b0 + bv * 8;
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (c < C && b < B) v = x[((e * C + c) * P + p) * B8 + b / 8];
        *reinterpret_cast<u32x4*>(&tile[cl][bv * 8]) = v;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = threadIdx.x + 256 * it;
        const int bl = idx >> 3, cv = idx & 7;
        const int b = b0 + bl, c = c0 + cv * 8;
        if (b < B && c < Cp) {
            uint32_t r[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = tile[cv * 8 + j][bl];
            out[((e * B + b) * P + p) * Cp8 + c / 8] = u32x4{r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16)};
        }
    }
}

// [E][R][B] -> [E][S][R][B/S]: chunk s of row r holds images s*B/S .. (s+1)*B/S - 1.  One 16-byte vector per thread.
__global__ __launch_bounds__(256) void batch_chunks_bf16_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ out, int64_t total8,
                                                                int64_t R, int B8, int S) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total8) return;
    const int Bs8 = B8 / S;
    const int v = (int)(i % Bs8);
    int64_t t = i / Bs8;
    const int64_t r = t % R;
    t /= R;
    const int s = (int)(t % S);
    const int64_t e = t / S;
    out[i] = x[(e * R + r) * B8 + (int64_t)s * Bs8 + v];
}

}  // namespace

extern "C" int bbb_plane_sum_bf16(const void* x, float* out, int64_t rows, int64_t cols, int64_t row_pitch, void* stream) {
    if (x == nullptr || out == nullptr || rows <= 0 || cols <= 0 || row_pitch < cols) return BBB_EINVAL;
    if (cols % 8 != 0 || row_pitch % 8 != 0) return BBB_ESHAPE;
    if ((((uintptr_t)x & 15u) | ((uintptr_t)out & 3u)) != 0) return BBB_EALIGN;
    if (rows > 0x7fffffffLL) return BBB_ESHAPE;
    hipLaunchKernelGGL(plane_sum_bf16_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const u32x4*>(x), out,
                       cols / 8, row_pitch / 8);
    return (int)hipGetLastError();
}

extern "C" int bbb_flip_transpose_w_bf16(const void* w, void* out, int64_t draws, int cout, int cin, int khkw, uint32_t flags, void* stream) {
    if (w == nullptr || out == nullptr || draws <= 0 || cout <= 0 || cin <= 0 || khkw <= 0) return BBB_EINVAL;
    if ((flags & ~(BBB_BF16_FLIP_IN_TAP_MAJOR | BBB_BF16_FLIP_OUT_TAP_MAJOR)) != 0) return BBB_EINVAL;
    const bool in_tm = (flags & BBB_BF16_FLIP_IN_TAP_MAJOR) != 0, out_tm = (flags & BBB_BF16_FLIP_OUT_TAP_MAJOR) != 0;
    if ((in_tm && cin % 8 != 0) || (out_tm && cout % 8 != 0)) return BBB_ESHAPE;
    const int64_t Ki = (int64_t)cin * khkw, Ko = (int64_t)cout * khkw;
    if (Ki >= (1LL << 30) || Ko >= (1LL << 30)) return BBB_ESHAPE;
    const int Kpi = (int)((Ki + 7) & ~7LL), Kpo = (int)((Ko + 7) & ~7LL);
    if ((((uintptr_t)w | (uintptr_t)out) & 15u) != 0) return BBB_EALIGN;
    const int64_t total8 = draws * cin * (Kpo / 8);
    const int64_t blocks = (total8 + 255) / 256;
    if (blocks > 0x7fffffffLL) return BBB_ESHAPE;
    hipLaunchKernelGGL(flip_transpose_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint16_t*>(w),
                       reinterpret_cast<u32x4*>(out), total8, cout, cin, khkw, Kpi, Kpo, in_tm ? 1 : 0, out_tm ? 1 : 0);
    return (int)hipGetLastError();
}

extern "C" int bbb_chwn_to_bhwc_bf16(const void* x, void* out, int64_t draws, int c, int64_t hw, int batch, int c_pad, void* stream) {
    if (x == nullptr || out == nullptr || draws <= 0 || c <= 0 || hw <= 0 || batch <= 0 || c_pad < c) return BBB_EINVAL;
    if (batch % 8 != 0 || c_pad % 8 != 0) return BBB_ESHAPE;
    if ((((uintptr_t)x | (uintptr_t)out) & 15u) != 0) return BBB_EALIGN;
    const int64_t ctiles = (c_pad + 63) / 64, btiles = (batch + 63) / 64;
    if (ctiles * btiles > 0x7fffffffLL || hw > 65535 || draws > 65535) return BBB_ESHAPE;
    hipLaunchKernelGGL(chwn_to_bhwc_bf16_kernel, dim3((unsigned)(ctiles * btiles), (unsigned)hw, (unsigned)draws), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const u32x4*>(x), reinterpret_cast<u32x4*>(out), c, (int)hw, batch, c_pad,
                       (int)ctiles);
    return (int)hipGetLastError();
}

extern "C" int bbb_batch_chunks_bf16(const void* x, void* out, int64_t outer, int64_t rows, int batch, int chunks, void* stream) {
    if (x == nullptr || out == nullptr || outer <= 0 || rows <= 0 || batch <= 0 || chunks <= 0) return BBB_EINVAL;
    if (batch % (8 * chunks) != 0) return BBB_ESHAPE;
    if ((((uintptr_t)x | (uintptr_t)out) & 15u) != 0) return BBB_EALIGN;
    const int64_t total8 = outer * rows * (batch / 8);
    const int64_t blocks = (total8 + 255) / 256;
    if (blocks > 0x7fffffffLL) return BBB_ESHAPE;
    hipLaunchKernelGGL(batch_chunks_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const u32x4*>(x),
                       reinterpret_cast<u32x4*>(out), total8, rows, batch / 8, chunks);
    return (int)hipGetLastError();
}
