// f32_tile.h - what the exact-f32 contractions of the f32 audio engines (ecapa_lid.hip, fsmn_vad.hip, sensevoice.hip, mossformer2.hip, sortformer.hip)
// share: device code only.  A block of 256 threads (four waves) forms a tile of C = A B^T on v_mfma_f32_32x32x2_f32, K staged F32_KC
// at a time through As[rows][F32_KC + 1] / Bs[cols][F32_KC + 1] in LDS.  An engine keeps what differs: its parameter struct, its
// staging loops with their operand loads, and its epilogue arithmetic.
// Contract of a change here: every engine's outputs stay bit for bit (tests/test_gpu_front_bits.py), and the kernels compile to the
// instructions they had (DESIGN.md says how that was checked); the K steps of a tile are accumulated in ascending order, two at a time.
#pragma once
#include "common.h"

constexpr int F32_KC = 32, F32_TILE = 64;      // K columns staged a step; edge of the 64 x 64 tile

// C/D map of the 32 x 32 MFMA: accumulator element r of a lane is column lane & 31, row f32_tile_row(r, lane >> 5)
__device__ __forceinline__ int f32_tile_row(int r, int kh) { return (r & 3) + 8 * (r >> 2) + 4 * kh; }

// the 16 MFMA steps of one staged K slab: the lane holds row `arow` of As and rows `brow + 32 ct` of Bs, kh = lane >> 5
template <int CT>
__device__ __forceinline__ void f32_tile_mfma(const float (*As)[F32_KC + 1], const float (*Bs)[F32_KC + 1], int arow, int brow, int kh,
                                              f32x16_t (&acc)[CT]) {
#pragma unroll
    for (int kk = 0; kk < F32_KC; kk += 2) {
        const float a = As[arow][kk + kh];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[brow + ct * 32][kk + kh], acc[ct], 0, 0, 0);
    }
}

// the tile holds none of the row's frames: Y[row0 + t][co] = 0 over the tile's part of [0, nr) x [0, N)
template <int TT, int TC>
__device__ __forceinline__ void f32_tile_zero(float* Y, int ldy, size_t row0, int t0, int c0, int nr, int N) {
    for (int i = threadIdx.x; i < TT * TC; i += 256) {
        const int t = t0 + i / TC, co = c0 + i % TC;
        if (t < nr && co < N) Y[(row0 + t) * ldy + co] = 0.0f;
    }
}
