// parakeet_encoder_bf16.h - the opt-in bf16 form of the Conformer-block chain of parakeet_encoder.h (pk_encoder), for parakeet.hip and
// canary.hip: include it behind parakeet_encoder.h.  Selected per handle before finalize (pk_set_encoder_dtype); the f32 chain, its bits and
// its launch counts are untouched, and the chain here keeps the same 1 + 15 L launches (k_sf_intake, k_sf_stats and k_sf_ln are reused: the
// residual stream is f32 in both modes).  Front end and stem stay f32.
//
// PRECISION CONTRACT of bf16 mode.
//   f32: the residual stream h, the LayerNorm statistics, biases, LayerNorm parameters, bias_u / bias_v, the folded depthwise taps; every
//        accumulation, the softmax and every epilogue computation.
//   bf16, round-to-nearest-even, once, at each of these points: the eight block matrices (ff1a, ff1b, qkv, o, pw1, pw2, ff2a, ff2b) and each
//        layer's projected distance table P (projected in f32 by the f32 GEMM, then rounded); the operand a contraction stages (LN(h) is
//        formed in f32 and rounded as it enters LDS); the activations written to the big, qkv and att buffers, which are bf16 buffers in
//        this mode; inside attention q qscale + u and q qscale + v (summed in f32, rounded once) and the probabilities in front of P V.
//        The row sum l adds the unrounded f32 probabilities.
//   Both modes: a row's encoder output is bit-identical whatever its batch, the padding behind lens[b] or what lies there (NaN included):
//        tile shapes depend on (N, K) only, never on M or the batch, partial sums are combined in one fixed order, no atomics on floats.
//
// Kernels:
//   k_pk_gemm_bf16        Y = epilogue(load(X) W^T) on v_mfma_f32_16x16x32_bf16, f32 accumulators, k-slabs of 32 in ascending order.  256
//                         threads, 2 x 2 waves, a wave TI x TI MFMA tiles: block tile 64 x 64 (TI 2) or 32 x 32 (TI 1), chosen per ROLE
//                         (PKB_ROLE, i.e. from N and K alone); the smaller tile exists for fill at short M and is kept measurable.
//                         Loads: f32 h through the LayerNorm prologue (two float4 of x, w, b a thread and slab; mean, rstd of
//                         k_sf_stats), or a bf16 activation in 16-byte chunks; the next slab is held in registers across the
//                         barrier pair.  Epilogues: bias + none / SiLU -> bf16, or bias + h = R + ra v -> f32.  Rows behind cnt[b]: zero.
//   k_pk_attn_bf16<NS>    relative-position flash attention, head sizes 1..128 zero-padded to NS slabs of 32.  A block is 32 queries x head
//                         x row, two waves; a wave owns 16 queries over ALL head dimensions: its (q + u) and (q + v) fragments are 2 x 4 NS
//                         VGPRs, so no wave ever exchanges partial scores.  32-key tiles ascending; K tile, V tile (transposed) and the
//                         block's 32 + 31 band rows of P are staged once per block.  Content scores S^T[key][query]: the A rows are read
//                         from LDS in the order 8 (r >> 2) + 4 t + (r & 3), so a lane ends up with the eight CONSECUTIVE keys 8 g .. 8 g + 7
//                         of its query - exactly the B fragment of P V, no shuffle.  Band product of the 16 + 32 - 1 table rows a wave's
//                         queries can see (three 16-row MFMA tiles) goes through a wave-private LDS patch [48][17] floats from which a lane
//                         takes the shifted diagonal (distance i - j, the literal rel-shift's entry; rows outside the table are zeros).
//                         Online softmax in f32 (the four lane groups of a query combine by xor 16, 32: one fixed order), P V with the
//                         rounded probabilities.  LDS at NS 4: 8704 + 10240 + 17408 + 6528 = 42880 bytes, three blocks a CU.
//   k_pk_glu_dwconv_bf16  k_sf_glu_dwconv's tile + halo in LDS with bf16 pw1 rows in and a bf16 att row out, arithmetic in f32.
#pragma once

#include "bf16_tile.h"

namespace {

enum { PKB_LOAD_BF16 = 0, PKB_LOAD_LN, PKB_LOAD_LN_SILU };         // LN_SILU: Nemotron's pointwise_conv2 (nemotron_encoder_bf16.h)
enum { PKB_EPI_NONE = 0, PKB_EPI_SILU, PKB_EPI_RES };               // bf16 store, bf16 store, f32 store of R + ra v
enum { PKB_TILE64 = 0, PKB_TILE32 };
enum { PKB_FF1A = 0, PKB_FF1B, PKB_QKV, PKB_O, PKB_PW1, PKB_PW2, PKB_FF2A, PKB_FF2B, PKB_ROLES };

// THE table of the launcher: what each role of the block loads, stores, and which tile rule it gets.  A role's (N, K) is fixed by the
// model, so the rule depends on (N, K) alone.  Both rules were measured for every role at 126 frames x batch 1 / 8 / 32 and at 751 frames
// (profiles/parakeet_bf16/README.md): 32 x 32 wins the K = d roles at batch 1 by 3 to 5 us a launch and loses every role at batch 32 by
// a factor of 1.5 to 1.8; summed over a block 64 x 64 everywhere is the faster table at both ends, so that is what stands here.
struct PkbRole { int load, epi, rule; };
static const PkbRole PKB_ROLE[PKB_ROLES] = {
    {PKB_LOAD_LN, PKB_EPI_SILU, PKB_TILE64},    // ff1a  [f][d]
    {PKB_LOAD_BF16, PKB_EPI_RES, PKB_TILE64},   // ff1b  [d][f]
    {PKB_LOAD_LN, PKB_EPI_NONE, PKB_TILE64},    // qkv   [3 d][d]
    {PKB_LOAD_BF16, PKB_EPI_RES, PKB_TILE64},   // o     [d][d]
    {PKB_LOAD_LN, PKB_EPI_NONE, PKB_TILE64},    // pw1   [2 d][d]
    {PKB_LOAD_BF16, PKB_EPI_RES, PKB_TILE64},   // pw2   [d][d]
    {PKB_LOAD_LN, PKB_EPI_SILU, PKB_TILE64},    // ff2a  [f][d]
    {PKB_LOAD_BF16, PKB_EPI_RES, PKB_TILE64},   // ff2b  [d][f]
};

// ============================================================================ the contraction
// Y[b][t][n] = epilogue(sum_k load(X)[b][t][k] W[n][k]); min(cnt[b], Tp) live rows a batch entry, the rows behind them are written as zero.
// K % 32 == 0, N % 8 == 0, ldx % 8 == 0, ldy % 4 == 0.
struct PkbGemm {
    const float* Xf; const bf16_t* Xb; int ldx;              // LN load: f32 rows; else bf16 rows (LN_SILU: bf16 rows, stats, lnw, lnb)
    const bf16_t* W; const float* bias;                      // [N][K]; bias null: none
    bf16_t* Yb; float* Yf; int ldy;                          // PKB_EPI_RES: Yf, else Yb
    const int* cnt; int Tp, K, N, epi;
    const float *stats, *lnw, *lnb;                          // LN load: stats [rows][2] = mean, rstd
    const float* R; int ldr; float ra;                       // PKB_EPI_RES: Yf = R + ra v
};

__device__ __forceinline__ uint32_t pkb_pack2(float a, float b) { return (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16); }

template <int LOAD, int TI>
__global__ void __launch_bounds__(256) k_pk_gemm_bf16(PkbGemm p) {
    constexpr int BT = 32 * TI;
    __shared__ __attribute__((aligned(16))) bf16_t Ws[BT][BF16_LD];
    __shared__ __attribute__((aligned(16))) bf16_t Xs[BT][BF16_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wn = wave >> 1, wm = wave & 1;
    const int b = blockIdx.z, m0 = blockIdx.x * BT, n0 = blockIdx.y * BT, T = min(p.cnt[b], p.Tp);
    const size_t row0 = (size_t)b * p.Tp;
    if (m0 >= T) {                                                  // (uniform over the block) nothing live: zeros
        for (int i = tid; i < BT * BT; i += 256) {
            const int m = m0 + i / BT, n = n0 + i % BT;
            if (m >= p.Tp || n >= p.N) continue;
            if (p.epi == PKB_EPI_RES) p.Yf[(row0 + m) * p.ldy + n] = 0.0f;
            else p.Yb[(row0 + m) * p.ldy + n] = 0;
        }
        return;
    }
    f32x4_t acc[TI][TI];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TI; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    // staging: BT rows x 32 k = 4 BT chunks of 16 B per operand; thread tid takes chunk tid (TI 1: the first 128 threads)
    const bool stager = tid < 4 * BT;
    const int r0 = tid >> 2, c0 = (tid & 3) * 8, ms = m0 + r0, ns = n0 + r0;
    const bool xlive = stager && ms < T, wlive = stager && ns < p.N;
    float mean = 0.0f, rstd = 0.0f;
    if ((LOAD == PKB_LOAD_LN || LOAD == PKB_LOAD_LN_SILU) && xlive) { mean = p.stats[2 * (row0 + ms)]; rstd = p.stats[2 * (row0 + ms) + 1]; }
    uint4 wreg = make_uint4(0, 0, 0, 0), xreg = make_uint4(0, 0, 0, 0);
    auto load = [&](int k0) {
        if (wlive) wreg = *reinterpret_cast<const uint4*>(p.W + (size_t)ns * p.K + k0 + c0);
        if (!xlive) return;
        if constexpr (LOAD == PKB_LOAD_LN_SILU) {                   // SiLU((x - mean) rstd w + b) in f32 from the widened bf16 x; rounded here, once
            const uint4 q = *reinterpret_cast<const uint4*>(p.Xb + (row0 + ms) * p.ldx + k0 + c0);
            const float4* w = reinterpret_cast<const float4*>(p.lnw + k0 + c0);
            const float4* bb = reinterpret_cast<const float4*>(p.lnb + k0 + c0);
            const float4 w0 = w[0], w1 = w[1], b0 = bb[0], b1 = bb[1];
            float lo[4], hi[4];
            bf16x4_unpack(make_uint2(q.x, q.y), lo);
            bf16x4_unpack(make_uint2(q.z, q.w), hi);
            auto act = [&](float x, float wv, float bv) { const float v = fmaf((x - mean) * rstd, wv, bv); return v / (1.0f + expf(-v)); };
            xreg.x = pkb_pack2(act(lo[0], w0.x, b0.x), act(lo[1], w0.y, b0.y));
            xreg.y = pkb_pack2(act(lo[2], w0.z, b0.z), act(lo[3], w0.w, b0.w));
            xreg.z = pkb_pack2(act(hi[0], w1.x, b1.x), act(hi[1], w1.y, b1.y));
            xreg.w = pkb_pack2(act(hi[2], w1.z, b1.z), act(hi[3], w1.w, b1.w));
        } else if (LOAD == PKB_LOAD_LN) {                                  // (x - mean) rstd w + b in f32, as k_sf_gemm's LN load; rounded here, once
            const float4* x = reinterpret_cast<const float4*>(p.Xf + (row0 + ms) * p.ldx + k0 + c0);
            const float4* w = reinterpret_cast<const float4*>(p.lnw + k0 + c0);
            const float4* bb = reinterpret_cast<const float4*>(p.lnb + k0 + c0);
            const float4 x0 = x[0], x1 = x[1], w0 = w[0], w1 = w[1], b0 = bb[0], b1 = bb[1];
            xreg.x = pkb_pack2(fmaf((x0.x - mean) * rstd, w0.x, b0.x), fmaf((x0.y - mean) * rstd, w0.y, b0.y));
            xreg.y = pkb_pack2(fmaf((x0.z - mean) * rstd, w0.z, b0.z), fmaf((x0.w - mean) * rstd, w0.w, b0.w));
            xreg.z = pkb_pack2(fmaf((x1.x - mean) * rstd, w1.x, b1.x), fmaf((x1.y - mean) * rstd, w1.y, b1.y));
            xreg.w = pkb_pack2(fmaf((x1.z - mean) * rstd, w1.z, b1.z), fmaf((x1.w - mean) * rstd, w1.w, b1.w));
        } else {
            xreg = *reinterpret_cast<const uint4*>(p.Xb + (row0 + ms) * p.ldx + k0 + c0);
        }
    };
    load(0);
    for (int k0 = 0; k0 < p.K; k0 += BF16_BK) {
        __syncthreads();
        if (stager) {
            *reinterpret_cast<uint4*>(&Ws[r0][c0]) = wreg;
            *reinterpret_cast<uint4*>(&Xs[r0][c0]) = xreg;
        }
        __syncthreads();
        if (k0 + BF16_BK < p.K) load(k0 + BF16_BK);
        bf16x8_t a[TI], x[TI];
#pragma unroll
        for (int i = 0; i < TI; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(&Ws[wn * 16 * TI + i * 16 + (lane & 15)][(lane >> 4) * 8]);
#pragma unroll
        for (int j = 0; j < TI; ++j) x[j] = *reinterpret_cast<const bf16x8_t*>(&Xs[wm * 16 * TI + j * 16 + (lane & 15)][(lane >> 4) * 8]);
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], x[j], acc[i][j], 0, 0, 0);
    }
    // C/D: lane l, element e = column n + 4 (l >> 4) + e of row m + (l & 15)
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TI; ++j) {
            const int m = m0 + wm * 16 * TI + j * 16 + (lane & 15), n = n0 + wn * 16 * TI + i * 16 + 4 * (lane >> 4);
            if (m >= p.Tp || n >= p.N) continue;
            const size_t row = row0 + m;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (m < T) {
                const float4 add = p.bias ? *reinterpret_cast<const float4*>(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
                v[0] = acc[i][j][0] + add.x; v[1] = acc[i][j][1] + add.y; v[2] = acc[i][j][2] + add.z; v[3] = acc[i][j][3] + add.w;
                if (p.epi == PKB_EPI_SILU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.0f + expf(-v[e]));
                } else if (p.epi == PKB_EPI_RES) {
                    const float4 r = *reinterpret_cast<const float4*>(p.R + row * p.ldr + n);
                    v[0] = fmaf(p.ra, v[0], r.x); v[1] = fmaf(p.ra, v[1], r.y); v[2] = fmaf(p.ra, v[2], r.z); v[3] = fmaf(p.ra, v[3], r.w);
                }
            }
            if (p.epi == PKB_EPI_RES) *reinterpret_cast<float4*>(p.Yf + row * p.ldy + n) = make_float4(v[0], v[1], v[2], v[3]);
            else *reinterpret_cast<uint2*>(p.Yb + row * p.ldy + n) = make_uint2(pkb_pack2(v[0], v[1]), pkb_pack2(v[2], v[3]));
        }
}

template <class Ctx>
static void pkb_gemm_launch(Ctx* c, const PkbGemm& p, int load, int rule, int B) {
    const int bt = rule == PKB_TILE32 ? 32 : 64;
    const dim3 grid(cdiv(p.Tp, bt), cdiv(p.N, bt), B);
    if (load == PKB_LOAD_LN) {
        if (rule == PKB_TILE32) MIS_LAUNCH(c, (k_pk_gemm_bf16<PKB_LOAD_LN, 1>), grid, dim3(256), p);
        else MIS_LAUNCH(c, (k_pk_gemm_bf16<PKB_LOAD_LN, 2>), grid, dim3(256), p);
    } else {
        if (rule == PKB_TILE32) MIS_LAUNCH(c, (k_pk_gemm_bf16<PKB_LOAD_BF16, 1>), grid, dim3(256), p);
        else MIS_LAUNCH(c, (k_pk_gemm_bf16<PKB_LOAD_BF16, 2>), grid, dim3(256), p);
    }
}

// ============================================================================ attention
struct PkbAttn {
    const bf16_t* qkv; int ld, koff, voff;                   // q at column h hd, k at koff + h hd, v at voff + h hd
    bf16_t* out; int ldo;
    const int* cnt; int Tp, hd;
    float qscale, sdk;                                       // q x qscale at staging; score / sdk
    const float *u, *v;                                      // [H][hd]
    const bf16_t* P; int ldp, Tcap;                          // projected table [2 Tcap - 1][ldp], row dist + Tcap - 1
};

constexpr int PKB_QW = 2;                                    // waves a block, 16 queries each
constexpr int PKB_QB = 16 * PKB_QW;

// 8 consecutive bf16 of a row of which the columns < lim are real (the rest zeros); vec: the 16-byte load is aligned
__device__ __forceinline__ uint4 pkb_chunk(const bf16_t* src, int col, int lim, bool vec) {
    if (vec && col + 8 <= lim) return *reinterpret_cast<const uint4*>(src + col);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (col + e < lim) w[e >> 1] |= (uint32_t)src[col + e] << (16 * (e & 1));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int NS>
__global__ void __launch_bounds__(64 * PKB_QW) k_pk_attn_bf16(PkbAttn p) {
    constexpr int HP = 32 * NS, LDK = HP + 8, CH = HP / 8, NT = 64 * PKB_QW, BR = PKB_QB + 32;
    __shared__ __attribute__((aligned(16))) bf16_t Ks[32][LDK];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[HP][BF16_LD];    // [dimension][key]
    __shared__ __attribute__((aligned(16))) bf16_t Pb[BR][LDK];        // band row r = table row q0 - kb - 31 + Tcap - 1 + r
    __shared__ float Gp[PKB_QW][48][17];                               // a wave's band products [band row][query]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * PKB_QB, n = min(p.cnt[b], p.Tp), hd = p.hd;
    const size_t rowbase = (size_t)b * p.Tp;
    if (q0 >= n) {                                                  // (uniform over the block)
        for (int i = tid; i < PKB_QB * hd; i += NT) {
            const int t = q0 + i / hd;
            if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + i % hd] = 0;
        }
        return;
    }
    const bool vec = ((hd | p.ld | p.koff | p.voff | p.ldp) & 7) == 0;
    const int tq = q0 + wave * 16 + l15;
    bf16x8_t qu[NS], qv[NS];                                        // B fragments: query l15, dimensions 32 s + 8 g .. + 7
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = s * 32 + g * 8 + e;
            const bool in = c < hd;
            const float q = (in && tq < n) ? bf16_to_f32(p.qkv[(rowbase + tq) * p.ld + h * hd + c]) * p.qscale : 0.0f;
            qu[s][e] = (short)f32_to_bf16(in ? q + p.u[h * hd + c] : 0.0f);
            qv[s][e] = (short)f32_to_bf16(in ? q + p.v[h * hd + c] : 0.0f);
        }
    f32x4_t O[2 * NS];                                              // O^T: dimension 16 t + 4 g + e of query l15
#pragma unroll
    for (int t = 0; t < 2 * NS; ++t) O[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.0f;
    const int kr0 = 8 * (l15 >> 2) + (l15 & 3);                     // A row l15 of key tile t reads key kr0 + 4 t: D rows 4 g + e are keys 8 g + 4 t + e
    for (int kb = 0; kb < n; kb += 32) {
        __syncthreads();                                            // the previous tile's reads are done
        for (int i = tid; i < 32 * CH; i += NT) {
            const int r = i / CH, cc = (i % CH) * 8, key = kb + r;
            *reinterpret_cast<uint4*>(&Ks[r][cc]) =
                key < n ? pkb_chunk(p.qkv + (rowbase + key) * p.ld + p.koff + h * hd, cc, hd, vec) : make_uint4(0, 0, 0, 0);
        }
        for (int i = tid; i < 32 * CH; i += NT) {                   // V transposed: consecutive threads, consecutive keys
            const int r = i & 31, cc = (i >> 5) * 8, key = kb + r;
            const uint4 q = key < n ? pkb_chunk(p.qkv + (rowbase + key) * p.ld + p.voff + h * hd, cc, hd, vec) : make_uint4(0, 0, 0, 0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) Vt[cc + e][r] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
        }
        const int base = q0 - kb - 31 + p.Tcap - 1;
        for (int i = tid; i < BR * CH; i += NT) {
            const int r = i / CH, cc = (i % CH) * 8, idx = base + r;
            *reinterpret_cast<uint4*>(&Pb[r][cc]) = (r < PKB_QB + 31 && idx >= 0 && idx < 2 * p.Tcap - 1)
                                                        ? pkb_chunk(p.P + (size_t)idx * p.ldp + h * hd, cc, hd, vec) : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        f32x4_t S0 = {0.f, 0.f, 0.f, 0.f}, S1 = S0, G0 = S0, G1 = S0, G2 = S0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int col = s * 32 + g * 8;
            S0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&Ks[kr0][col]), qu[s], S0, 0, 0, 0);
            S1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&Ks[kr0 + 4][col]), qu[s], S1, 0, 0, 0);
            const bf16_t* band = &Pb[wave * 16 + l15][col];
            G0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(band), qv[s], G0, 0, 0, 0);
            G1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(band + 16 * LDK), qv[s], G1, 0, 0, 0);
            G2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(band + 32 * LDK), qv[s], G2, 0, 0, 0);
        }
        // the wave's patch: band row 16 t + 4 g + e of query l15; then the shifted diagonal, band row l15 - key + 31
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Gp[wave][4 * g + e][l15] = G0[e];
            Gp[wave][16 + 4 * g + e][l15] = G1[e];
            Gp[wave][32 + 4 * g + e][l15] = G2[e];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float sc[8], mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int kk = 8 * g + e;                               // keys 8 g .. 8 g + 7 of the tile
            const float s = (e < 4 ? S0[e & 3] : S1[e & 3]) + Gp[wave][l15 - kk + 31][l15];
            sc[e] = (kb + kk < n) ? s / p.sdk : -INFINITY;
            mx = fmaxf(mx, sc[e]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.0f : m_new;      // (cannot occur: every tile holds a key < n)
        const float alpha = expf(m_run - m_use);
        float psum = 0.0f;
        bf16x8_t pf;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float pe = expf(sc[e] - m_use);
            psum += pe;                                             // the row sum takes the unrounded probability
            pf[e] = (short)f32_to_bf16(pe);
        }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int t = 0; t < 2 * NS; ++t) {
#pragma unroll
            for (int e = 0; e < 4; ++e) O[t][e] *= alpha;
            O[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&Vt[t * 16 + l15][g * 8]), pf, O[t], 0, 0, 0);
        }
    }
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    if (tq >= p.Tp) return;
    bf16_t* orow = p.out + (rowbase + tq) * p.ldo + h * hd;
    const bool vst = ((hd | p.ldo) & 3) == 0;
#pragma unroll
    for (int t = 0; t < 2 * NS; ++t) {
        const int dcol = t * 16 + 4 * g;
        if (dcol >= hd) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tq < n ? O[t][e] / l_tot : 0.0f;
        if (vst) *reinterpret_cast<uint2*>(orow + dcol) = make_uint2(pkb_pack2(v[0], v[1]), pkb_pack2(v[2], v[3]));
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (dcol + e < hd) orow[dcol + e] = f32_to_bf16(v[e]);
        }
    }
}

template <class Ctx>
static void pkb_attn(Ctx* c, const PkbAttn& p, int heads, int hd, int batch) {
    const dim3 grid(cdiv(p.Tp, PKB_QB), heads, batch), block(64 * PKB_QW);
    if (hd <= 32) MIS_LAUNCH(c, k_pk_attn_bf16<1>, grid, block, p);
    else if (hd <= 64) MIS_LAUNCH(c, k_pk_attn_bf16<2>, grid, block, p);
    else if (hd <= 96) MIS_LAUNCH(c, k_pk_attn_bf16<3>, grid, block, p);
    else MIS_LAUNCH(c, k_pk_attn_bf16<4>, grid, block, p);
}

// ============================================================================ conv module
// k_sf_glu_dwconv with bf16 rows in (pw [M][2 C]) and out ([M][C]); the gate, the taps, the folded-BatchNorm shift and SiLU in f32
__global__ void __launch_bounds__(256) k_pk_glu_dwconv_bf16(const bf16_t* __restrict__ pw, const float* __restrict__ taps, const float* __restrict__ shift,
                                                            const int* __restrict__ cnt, bf16_t* __restrict__ out, int Tp, int C, int k) {
    __shared__ float gs[SF_DW_TT + SF_DW_MAXK - 1][64];
    const int cl = threadIdx.x & 63, tl = threadIdx.x >> 6, ch = blockIdx.y * 64 + cl, b = blockIdx.z, t0 = blockIdx.x * SF_DW_TT;
    const int n = min(cnt[b], Tp), padl = (k - 1) >> 1;
    const bool live = ch < C;
    const size_t rowbase = (size_t)b * Tp;
    for (int r = tl; r < SF_DW_TT + k - 1; r += 4) {
        const int t = t0 - padl + r;
        float v = 0.0f;
        if (live && t >= 0 && t < n) {
            const bf16_t* row = pw + (rowbase + t) * 2 * C;
            v = bf16_to_f32(row[ch]) * (1.0f / (1.0f + expf(-bf16_to_f32(row[C + ch]))));
        }
        gs[r][cl] = v;
    }
    __syncthreads();
    if (!live) return;
    float acc[16];
    const float sh = shift[ch];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = sh;
    for (int kk = 0; kk < k; ++kk) {
        const float w = taps[(size_t)kk * C + ch];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = fmaf(w, gs[tl * 16 + i + kk][cl], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = t0 + tl * 16 + i;
        if (t >= Tp) continue;
        const float v = acc[i];
        out[(rowbase + t) * C + ch] = t < n ? f32_to_bf16(v / (1.0f + expf(-v))) : (bf16_t)0;
    }
}

__global__ void __launch_bounds__(256) k_pk_round_bf16(const float* __restrict__ x, bf16_t* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = f32_to_bf16(x[i]);
}

// ============================================================================ host
// f32 (the default) or bf16, before finalize; bf16 needs whole k-slabs (any handle with cfg, finalized and enc_bf16)
template <class Ctx>
static void pk_set_encoder_dtype(Ctx* c, mis_dtype dtype) {
    MIS_REQUIRE(c, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(!c->finalized, MIS_ERR_INVALID_INPUT, "set_encoder_dtype after finalize");
    MIS_REQUIRE(dtype == MIS_F32 || dtype == MIS_BF16, MIS_ERR_INVALID_INPUT, "encoder dtype %d: only MIS_F32 and MIS_BF16 are implemented", (int)dtype);
    if (dtype == MIS_BF16) {
        MIS_REQUIRE(c->cfg.hidden_size % 32 == 0, MIS_ERR_INVALID_INPUT, "hidden_size %d: the bf16 encoder needs a multiple of 32", c->cfg.hidden_size);
        MIS_REQUIRE(c->cfg.intermediate_size % 32 == 0, MIS_ERR_INVALID_INPUT, "intermediate_size %d: the bf16 encoder needs a multiple of 32",
                    c->cfg.intermediate_size);
    }
    c->enc_bf16 = dtype == MIS_BF16;
}

#ifndef PKB_NO_PARAKEET_CHAIN                                        // nemotron_encoder_bf16.h has its own tables and chain
// finalize of bf16 mode: every layer's table projected in f32 by the f32 GEMM, as the f32 mode does, then rounded into ptab16; the f32
// table, the relative_k_proj matrices and the projections live in buffers of this scope only
template <class Ctx>
static void pk_bf16_tables(Ctx* c) {
    const int64_t d = c->d;
    const int Tc = c->Tcap, NP = 2 * Tc - 1;
    HostArena t(c->raw);
    const float* tab = nullptr;
    std::vector<SfLin> rk(c->L);
    const size_t o = t.ftake((size_t)NP * d, tab);
    pk_postab(&t.fhost[o], Tc, d);
    for (int li = 0; li < c->L; ++li) t.fvec("encoder.layers." + std::to_string(li) + ".self_attn.relative_k_proj.weight", {d, d}, d * d, rk[li].w);
    DevBuf<bf16_t> none;
    DevBuf<float> ftmp, proj;
    t.upload(none, ftmp);
    const size_t per = (size_t)NP * d;
    proj.alloc(per);
    c->ptab16.alloc(c->L * per);
    for (int li = 0; li < c->L; ++li) {
        sf_gemm(c, sf_lin(tab, (int)d, rk[li], proj.p, (int)d, nullptr, NP), 1);
        MIS_LAUNCH(c, k_pk_round_bf16, dim3((unsigned)((per + 255) / 256)), dim3(256), proj.p, c->ptab16.p + li * per, per);
        c->fc16[li].P = c->ptab16.p + li * per;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
#endif

// c->emb -> the Conformer blocks in bf16 mode -> c->h (1 + 15 L launches, as pk_encoder).  Any handle whose fc / fc16 layers carry the
// members read here: Parakeet's and Canary's PkEncoder, Sortformer's own (sortformer.hip).
template <class Ctx>
static void pk_encoder_bf16(Ctx* c, int stop) {
    const int B = c->batch, Tp = c->Tp, d = c->d, f = c->f, M = B * Tp;
    const int* cnt = c->cnt3.p;
    const size_t nd = (size_t)M * d;
    MIS_LAUNCH(c, k_sf_intake, dim3((unsigned)((nd + 255) / 256)), dim3(256), c->emb.p, c->h.p, cnt, Tp, d, c->cfg.scale_input ? sqrtf((float)d) : 1.0f, nd);
    auto stats = [&]() { MIS_LAUNCH(c, k_sf_stats, dim3(cdiv(M, 4)), dim3(256), c->h.p, c->stats.p, d, 1e-5f, M); };
    auto gemm = [&](int role, const bf16_t* W, const float* bias, int N, int K, const float* lnw, const float* lnb, const bf16_t* xb, bf16_t* yb, float ra) {
        const PkbRole& r = PKB_ROLE[role];
        PkbGemm p{};
        p.W = W; p.bias = bias; p.cnt = cnt; p.Tp = Tp; p.K = K; p.N = N; p.epi = r.epi; p.ldx = K; p.ldy = N;
        if (r.load == PKB_LOAD_LN) { p.Xf = c->h.p; p.stats = c->stats.p; p.lnw = lnw; p.lnb = lnb; }
        else p.Xb = xb;
        if (r.epi == PKB_EPI_RES) { p.Yf = c->h.p; p.R = c->h.p; p.ldr = N; p.ra = ra; }
        else p.Yb = yb;
        pkb_gemm_launch(c, p, r.load, r.rule, B);
    };
    bf16_t *big = c->big16.p, *qkv = c->qkv16.p, *att = c->att16.p;
    for (int li = 0; li < c->L; ++li) {                            // 15 launches a block
        const auto& l = c->fc[li];
        const auto& w = c->fc16[li];
        stats();
        gemm(PKB_FF1A, w.ff1a, l.ff1a.b, f, d, l.ln1w, l.ln1b, nullptr, big, 0.0f);
        gemm(PKB_FF1B, w.ff1b, l.ff1b.b, d, f, nullptr, nullptr, big, nullptr, 0.5f);
        stats();
        gemm(PKB_QKV, w.qkv, l.qkv.b, 3 * d, d, l.lnaw, l.lnab, nullptr, qkv, 0.0f);
        PkbAttn ap{qkv, 3 * d, d, 2 * d, att, d, cnt, Tp, c->hd, 1.0f, sqrtf((float)c->hd), l.u, l.v, w.P, d, c->Tcap};
        pkb_attn(c, ap, c->H, c->hd, B);
        gemm(PKB_O, w.o, l.o.b, d, d, nullptr, nullptr, att, nullptr, 1.0f);
        stats();
        gemm(PKB_PW1, w.pw1, l.pw1.b, 2 * d, d, l.lncw, l.lncb, nullptr, big, 0.0f);
        MIS_LAUNCH(c, k_pk_glu_dwconv_bf16, dim3(cdiv(Tp, SF_DW_TT), cdiv(d, 64), B), dim3(256), big, l.dw, l.dwshift, cnt, att, Tp, d, c->ck);
        gemm(PKB_PW2, w.pw2, l.pw2.b, d, d, nullptr, nullptr, att, nullptr, 1.0f);
        stats();
        gemm(PKB_FF2A, w.ff2a, l.ff2a.b, f, d, l.ln2w, l.ln2b, nullptr, big, 0.0f);
        gemm(PKB_FF2B, w.ff2b, l.ff2b.b, d, f, nullptr, nullptr, big, nullptr, 0.5f);
        MIS_LAUNCH(c, k_sf_ln, dim3(cdiv(M, 4)), dim3(256), c->h.p, c->h.p, l.lnow, l.lnob, d, 1e-5f, M, cnt, Tp);
        if (stop == li + 1) return;
    }
}

}  // namespace
