// bf16_tile.h - what the register-staged bf16 big GEMMs of the encoders share: k_gemm_big of whisper_kernels.hip (Whisper, Moonshine,
// Smart Turn) and k_lasr_gemm of lasr.hip.  Device code only.  C[m][n] = sum_k X[m][k] W[n][k] on v_mfma_f32_16x16x32_bf16 with W as
// the A operand, so a lane's four accumulator elements are four consecutive n of one row m.  Shared: the tile constants, the main
// loop of a 2 x 2 wave block (bf16_tile_contract) and the pack / unpack of four bf16 in a uint2 (also used by k_gemm_big2 / k_gemm_big3).
// An engine keeps what differs: its parameter struct, its LDS arrays, its epilogue with its rounding points, its launcher and tile
// rule.  The loops over a wave's C/D quads with their edge skips are written out in each kernel.  One form of a shared walk was
// measured, a helper taking the epilogue as a lambda that captures the parameter struct by reference: same bits, other code in every
// kernel, slower (profiles/bf16_tile/README.md).  That is that form's result; a walk that keeps the kernels' code is still open.
// Contract of a change here: every includer's outputs stay bit for bit (tests/test_gpu_bf16_gemm_bits.py, tests/test_gpu_front_bits.py),
// the k-slabs of 32 are accumulated in ascending order, one MFMA per slab, and the timings of profiles/bf16_tile/README.md hold.
#pragma once
#include "common.h"

constexpr int BF16_BK = 32, BF16_LD = 40;      // k per slab; padded LDS row (bf16 elements): 80 B rows keep 16-B fragments aligned

// four bf16 of consecutive columns in one 8-byte word: what an epilogue reads of a residual row and writes of C
__device__ __forceinline__ void bf16x4_unpack(uint2 q, float (&v)[4]) {
    v[0] = __uint_as_float(q.x << 16); v[1] = __uint_as_float(q.x & 0xffff0000u);
    v[2] = __uint_as_float(q.y << 16); v[3] = __uint_as_float(q.y & 0xffff0000u);
}
// (four values, not an array: behind a `const uint16_t (&)[4]` the compiler pairs the roundings that feed it differently, and every
// kernel's epilogue changes)
__device__ __forceinline__ uint2 bf16x4_pack(uint16_t r0, uint16_t r1, uint16_t r2, uint16_t r3) {
    uint2 v;
    v.x = (uint32_t)r0 | ((uint32_t)r1 << 16);
    v.y = (uint32_t)r2 | ((uint32_t)r3 << 16);
    return v;
}

// The contraction of a 256-thread block, 2 x 2 waves, a wave holding TI x TI MFMA tiles: block tile 32 TI squared at (n0, m0), Ws / Xs
// [32 TI][BF16_LD] in the caller's LDS.  Staging: 32 TI rows x 32 k = TI / 2 chunks of 16 B per operand and thread, the next k-slab held
// in registers across the barrier pair; rows past N / M are staged as zeros.  K % 32 == 0, ldx % 8 == 0.  Leaves acc[i][j]: the tile at
// n = n0 + (wave >> 1) 16 TI + 16 i, m = m0 + (wave & 1) 16 TI + 16 j; C/D lane l, element e: n + 4 (l >> 4) + e, m + (l & 15).
template <int TI>
__device__ __forceinline__ void bf16_tile_contract(const bf16_t* W, const bf16_t* X, int ldx, int M, int N, int K, int n0, int m0,
                                                   bf16_t (*Ws)[BF16_LD], bf16_t (*Xs)[BF16_LD], f32x4_t (&acc)[TI][TI]) {
    constexpr int NCH = TI / 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wm = wave & 1;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TI; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int r0 = tid >> 2, c0 = (tid & 3) * 8;
    uint4 wreg[NCH], xreg[NCH];
    auto load = [&](int k0) {
#pragma unroll
        for (int h = 0; h < NCH; ++h) {
            const int row = r0 + 64 * h, n = n0 + row, m = m0 + row;
            wreg[h] = (n < N) ? *reinterpret_cast<const uint4*>(W + (size_t)n * K + k0 + c0) : make_uint4(0, 0, 0, 0);
            xreg[h] = (m < M) ? *reinterpret_cast<const uint4*>(X + (size_t)m * ldx + k0 + c0) : make_uint4(0, 0, 0, 0);
        }
    };
    load(0);
    for (int k0 = 0; k0 < K; k0 += BF16_BK) {
        __syncthreads();
#pragma unroll
        for (int h = 0; h < NCH; ++h) {
            *reinterpret_cast<uint4*>(&Ws[r0 + 64 * h][c0]) = wreg[h];
            *reinterpret_cast<uint4*>(&Xs[r0 + 64 * h][c0]) = xreg[h];
        }
        __syncthreads();
        if (k0 + BF16_BK < K) load(k0 + BF16_BK);
        bf16x8_t a[TI], b[TI];
#pragma unroll
        for (int i = 0; i < TI; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(&Ws[wn * 16 * TI + i * 16 + (lane & 15)][(lane >> 4) * 8]);
#pragma unroll
        for (int j = 0; j < TI; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(&Xs[wm * 16 * TI + j * 16 + (lane & 15)][(lane >> 4) * 8]);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}
