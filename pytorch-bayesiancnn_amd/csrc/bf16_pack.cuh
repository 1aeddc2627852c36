// bf16 storage <-> fp32 registers, 8 values per 16-byte vector: what the kernels that move bf16 planes as whole vectors share
// (train_bf16.hip, pool2d_bf16.hip, the bf16 section of pool_act_bwd.cuh).  Element 2j of a vector is the low half of word j.
#ifndef BBB_BF16_PACK_CUH
#define BBB_BF16_PACK_CUH

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bf16_pack {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf2f(uint32_t bits16) { return __uint_as_float(bits16 << 16); }

__device__ __forceinline__ uint32_t f2bf(float v) {             // round to nearest even (v_cvt_pk_bf16_f32)
    return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v);
}

__device__ __forceinline__ void unpack8(const u32x4 v, float (&o)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[2 * j] = bf2f(v[j] & 0xFFFFu);
        o[2 * j + 1] = bf2f(v[j] >> 16);
    }
}

__device__ __forceinline__ u32x4 pack8(const uint32_t (&r)[8]) {
    return u32x4{r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16)};
}

}  // namespace bf16_pack

#endif
