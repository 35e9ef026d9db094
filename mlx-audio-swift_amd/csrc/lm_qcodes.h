// lm_qcodes.h - device helpers for MLX affine-quantised codes as the code-streaming kernels hold them (lm_qgemm.hip, token_engine_q.hip):
// one lane's 8 codes of a [NT][KT][64 lanes][8 codes] tile (8 bytes at 8 bit, 4 bytes at 4 bit) and the 16-bit scale / bias payloads.
#pragma once
#include "common.h"

typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
template <int BITS> struct QTile;
template <> struct QTile<8> { typedef u32x2_t type; };
template <> struct QTile<4> { typedef unsigned int type; };

// 8 codes -> 8 bf16 values (exact).  (float)(byte) is v_cvt_f32_ubyteN; the pair conversion is v_cvt_pk_bf16_f32.
// (Measured alternative: v_perm_b32 placing byte k under the exponent of 2^23, one v_pk_add_f32 per pair, then the same pack - 16
// instead of 12 instructions per fragment and no faster anywhere: profiles/r03/qgemm_loads_vs_math.jsonl.)
__device__ __forceinline__ bf16x8_t dq_codes(u32x2_t w) {
    bf16x8_t r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[e] = (short)f32_to_bf16((float)((w.x >> (8 * e)) & 0xffu));
        r[4 + e] = (short)f32_to_bf16((float)((w.y >> (8 * e)) & 0xffu));
    }
    return r;
}
__device__ __forceinline__ bf16x8_t dq_codes(unsigned int w) {
    bf16x8_t r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (short)f32_to_bf16((float)((w >> (4 * e)) & 0xfu));
    return r;
}
// one 16-bit scale / bias (low half of w) -> float32, exactly: SBT 0 = bf16, 1 = f16 (v_cvt_f32_f16)
template <int SBT>
__device__ __forceinline__ float sb_to_f32(uint32_t w) {
    if (SBT == 1) return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
    return __uint_as_float(w << 16);
}
