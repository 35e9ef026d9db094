// nemotron_encoder_bf16.h - the opt-in bf16 form of the Nemotron ASR block chain (nm_encoder of nemotron.hip), offline engine only: include it
// behind nemotron_kernels.h.  Selected per handle before finalize (mis_nemotron_set_encoder_dtype); the f32 chain, its bits, its launch
// counts and its resident buffers are untouched, and the chain here keeps the same 1 + 15 L launches (k_sf_intake, k_sf_stats and k_sf_ln are
// reused: the residual stream is f32 in both modes).  Front end, stem, prompt kernel, joint.enc and the RNN-T decode stay f32.
//
// PRECISION CONTRACT of bf16 mode: parakeet_encoder_bf16.h's, plus the conv module's two points.
//   f32: the residual stream h, every LayerNorm statistic (the conv module's included: mean and rstd are taken over the UNROUNDED f32
//        depthwise outputs), biases, LayerNorm parameters, bias_u / bias_v, the depthwise taps; every accumulation, the softmax, every epilogue.
//   bf16, round-to-nearest-even, once, at each of these points: the eight block matrices and each layer's projected distance table (projected
//        in f32 for the widest listed context, then rounded); the operand a contraction stages; the big, qkv and att buffers; inside
//        attention q + u, q + v and the probabilities in front of P V (the row sum adds the unrounded probabilities); the conv module's
//        depthwise output.  pointwise_conv2's load forms SiLU((x - mean) rstd w + b) in f32 from the widened bf16 x and rounds it as it is staged.
//   Both modes: an excluded key has weight exactly 0; a row's output is bit-identical whatever its batch, its padding or what lies behind
//        lens[b] (NaN included).
//
// Kernels (k_pk_gemm_bf16, k_pk_round_bf16 and the role table are parakeet_encoder_bf16.h's; resources off
// -Rpass-analysis=kernel-resource-usage, gfx950):
//   k_nm_attn_bf16<NS>   k_pk_attn_bf16's split (32 queries x head x row a block on two waves, a wave 16 queries over ALL head dimensions,
//                        K, transposed V and the band rows staged per 32-key tile, the band product through a wave-private LDS patch, f32
//                        online softmax with one fixed combine order) under k_nm_attn's rule: (a) the block walks only the 32-key tiles
//                        that intersect [(q0 / C - L) C, (q_last / C + 1) C) and [0, n); (b) inside a tile two compares per (query, key)
//                        against the lane's own [lo, hi), made once per query: an excluded key adds nothing to m, l or P V, a query that
//                        sees nothing of a tile keeps m = -inf, and the rescale exp(m_old - m_new) takes m_new = 0 there so that
//                        -inf - -inf never forms; (c) the bf16 table holds the distances dlo .. dhi of the widest listed pair alone
//                        (row = distance + poff); band rows outside the CALL's [dlo, dhi] are staged as zeros and never read.
//                        NS 1 / 2 / 3 / 4: LDS 16768 / 25472 / 34176 / 42880 bytes (three blocks a CU at NS 4), 84 / 100 / 122 / 148 VGPRs +
//                        16 / 20 / 24 / 32 AGPRs, scratch 0.
//   k_nm_glu_dwconv_ln_bf16   k_nm_glu_dwconv_ln's ownership (16 frames of one row across every channel, 64 channels at a time, tile + halo
//                        of gated frames in LDS) with bf16 pw1 rows in (16-byte chunks where aligned) and a bf16 row out, arithmetic in
//                        f32.  Two passes over the channels: the first sums the outputs, the second RECOMPUTES them (one loop body, the
//                        same bits), sums the squared distances to the mean and stores the rounded values - the rounded stores are never
//                        re-read.  Both sums meet in wave_sum's fixed order.  LDS 11776 bytes, 69 VGPRs, scratch 0.
//   k_pk_gemm_bf16<PKB_LOAD_LN_SILU, TI>   the third operand load of the contraction: 59 VGPRs + 4 (TI 1) / 16 (TI 2) AGPRs, scratch 0.
#pragma once

#define PKB_NO_PARAKEET_CHAIN
#include "parakeet_encoder_bf16.h"

namespace {

static const PkbRole NMB_PW2 = {PKB_LOAD_LN_SILU, PKB_EPI_RES, PKB_TILE64};   // pointwise_conv2 [d][d] over SiLU(LayerNorm(.))

template <class Ctx>
static void nmb_gemm_launch(Ctx* c, const PkbGemm& p, int load, int rule, int B) {
    if (load != PKB_LOAD_LN_SILU) { pkb_gemm_launch(c, p, load, rule, B); return; }
    const int bt = rule == PKB_TILE32 ? 32 : 64;
    const dim3 grid(cdiv(p.Tp, bt), cdiv(p.N, bt), B);
    if (rule == PKB_TILE32) MIS_LAUNCH(c, (k_pk_gemm_bf16<PKB_LOAD_LN_SILU, 1>), grid, dim3(256), p);
    else MIS_LAUNCH(c, (k_pk_gemm_bf16<PKB_LOAD_LN_SILU, 2>), grid, dim3(256), p);
}

// ============================================================================ chunked-limited attention
struct NmbAttn {
    const bf16_t* qkv; int ld, koff, voff;                   // q at column h hd, k at koff + h hd, v at voff + h hd
    bf16_t* out; int ldo;
    const int* cnt; int Tp, hd;
    float qscale, sdk;                                       // q x qscale at staging; score / sdk
    const float *u, *v;                                      // [H][hd]
    const bf16_t* P; int ldp, poff;                          // projected table by distance: row = distance + poff
    int C, L, dlo, dhi;                                      // chunk size, left chunks; the distances the call's rule lets occur
};

template <int NS>
__global__ void __launch_bounds__(64 * PKB_QW) k_nm_attn_bf16(NmbAttn p) {
    constexpr int HP = 32 * NS, LDK = HP + 8, CH = HP / 8, NT = 64 * PKB_QW, BR = PKB_QB + 32;
    __shared__ __attribute__((aligned(16))) bf16_t Ks[32][LDK];
    __shared__ __attribute__((aligned(16))) bf16_t Vt[HP][BF16_LD];    // [dimension][key]
    __shared__ __attribute__((aligned(16))) bf16_t Pb[BR][LDK];        // band row r = distance q0 - kb - 31 + r
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
    // the rule: the lane's query sees the keys [vlo, vhi); the block walks the tiles that the first and the last live query of it see
    const int qc = tq / p.C, vlo = max(qc - p.L, 0) * p.C, vhi = (qc + 1) * p.C;
    const int wlo = (max(q0 / p.C - p.L, 0) * p.C) & ~31, whi = min(n, (min(q0 + PKB_QB - 1, n - 1) / p.C + 1) * p.C);
    for (int kb = wlo; kb < whi; kb += 32) {
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
        const int base = q0 - kb - 31;                              // distance of band row 0
        for (int i = tid; i < BR * CH; i += NT) {
            const int r = i / CH, cc = (i % CH) * 8, dist = base + r;
            *reinterpret_cast<uint4*>(&Pb[r][cc]) = (r < PKB_QB + 31 && dist >= p.dlo && dist <= p.dhi)
                                                        ? pkb_chunk(p.P + (size_t)(dist + p.poff) * p.ldp + h * hd, cc, hd, vec) : make_uint4(0, 0, 0, 0);
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
            const int kk = 8 * g + e, key = kb + kk;                // keys 8 g .. 8 g + 7 of the tile
            const float s = (e < 4 ? S0[e & 3] : S1[e & 3]) + Gp[wave][l15 - kk + 31][l15];
            sc[e] = (key < n && key >= vlo && key < vhi) ? s / p.sdk : -INFINITY;
            mx = fmaxf(mx, sc[e]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.0f : m_new;      // the query has seen no key yet: every weight below is exp(-inf) = 0
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
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);                // > 0 for a live query: it sees itself
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
static void nmb_attn(Ctx* c, const NmbAttn& p, int heads, int hd, int batch) {
    const dim3 grid(cdiv(p.Tp, PKB_QB), heads, batch), block(64 * PKB_QW);
    if (hd <= 32) MIS_LAUNCH(c, k_nm_attn_bf16<1>, grid, block, p);
    else if (hd <= 64) MIS_LAUNCH(c, k_nm_attn_bf16<2>, grid, block, p);
    else if (hd <= 96) MIS_LAUNCH(c, k_nm_attn_bf16<3>, grid, block, p);
    else MIS_LAUNCH(c, k_nm_attn_bf16<4>, grid, block, p);
}

// ============================================================================ conv module: GLU + depthwise conv + LayerNorm statistics
// pw bf16 [M][2 C] (pointwise_conv1) -> out bf16 [M][C] and stats f32 [M][2] = mean, rstd over the C UNROUNDED outputs of a frame; padl zero
// frames before the row and zeros from its count on, taps f32 [k][C], bias f32 [C] or null.  Frames behind the count: zeros, stats 0, 0.
__global__ void __launch_bounds__(256) k_nm_glu_dwconv_ln_bf16(const bf16_t* __restrict__ pw, const float* __restrict__ taps, const float* __restrict__ bias,
                                                               const int* __restrict__ cnt, bf16_t* __restrict__ out, float* __restrict__ stats, int Tp, int C,
                                                               int k, int padl, float eps) {
    __shared__ __attribute__((aligned(16))) float g[NM_DW_TT + SF_DW_MAXK - 1][64];
    const int tid = threadIdx.x, cl = tid & 63, tl = tid >> 6, b = blockIdx.y, t0 = blockIdx.x * NM_DW_TT, tw = t0 + tl * 4;
    const int n = min(cnt[b], Tp);
    const size_t rowbase = (size_t)b * Tp;
    const bool vec = (C & 7) == 0;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, q[4] = {0.0f, 0.0f, 0.0f, 0.0f}, mean[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int pass = 0; pass < 2; ++pass) {                          // 0: the sums; 1: the same values again, their squared distances, the stores
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int ch = c0 + cl;
            __syncthreads();                                        // the previous 64 channels are read
            for (int i = tid; i < (NM_DW_TT + k - 1) * 8; i += 256) {   // a thread: 8 channels of a frame, a and its gate in one chunk each
                const int r = i >> 3, cc = (i & 7) * 8, t = t0 - padl + r;
                float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (t >= 0 && t < n && c0 + cc < C) {
                    const bf16_t* row = pw + (rowbase + t) * 2 * C;
                    const uint4 xa = pkb_chunk(row, c0 + cc, C, vec), xg = pkb_chunk(row + C, c0 + cc, C, vec);
                    float al[4], ah[4], gl[4], gh[4];
                    bf16x4_unpack(make_uint2(xa.x, xa.y), al);
                    bf16x4_unpack(make_uint2(xa.z, xa.w), ah);
                    bf16x4_unpack(make_uint2(xg.x, xg.y), gl);
                    bf16x4_unpack(make_uint2(xg.z, xg.w), gh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        a[e] = al[e] * (1.0f / (1.0f + expf(-gl[e])));
                        a[4 + e] = ah[e] * (1.0f / (1.0f + expf(-gh[e])));
                    }
                }
                *reinterpret_cast<float4*>(&g[r][cc]) = make_float4(a[0], a[1], a[2], a[3]);
                *reinterpret_cast<float4*>(&g[r][cc + 4]) = make_float4(a[4], a[5], a[6], a[7]);
            }
            __syncthreads();
            if (ch >= C) continue;                                  // (the barriers above are reached: the loop bound is uniform)
            float acc[4];
            const float bv = bias ? bias[ch] : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = bv;
            for (int kk = 0; kk < k; ++kk) {
                const float w = taps[(size_t)kk * C + ch];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(w, g[tl * 4 + i + kk][cl], acc[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = tw + i;
                const float v = t < n ? acc[i] : 0.0f;
                if (pass == 0) { s[i] += v; continue; }
                const float dv = v - mean[i];
                if (t < n) q[i] = fmaf(dv, dv, q[i]);
                if (t < Tp) out[(rowbase + t) * C + ch] = t < n ? f32_to_bf16(v) : (bf16_t)0;
            }
        }
        if (pass == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) mean[i] = wave_sum(s[i]) / (float)C;   // the wave's four frames: the lanes hold the channels cl, cl + 64, ..
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = tw + i;
        const float rstd = 1.0f / sqrtf(wave_sum(q[i]) / (float)C + eps);
        if (cl == 0 && t < Tp) { stats[2 * (rowbase + t)] = t < n ? mean[i] : 0.0f; stats[2 * (rowbase + t) + 1] = t < n ? rstd : 0.0f; }
    }
}

template <class Ctx>
static void nmb_glu_dwconv_ln(Ctx* c, const bf16_t* pw, const float* taps, const float* bias, const int* cnt, bf16_t* out, float* stats, int Tp, int C,
                              int k, int padl, int batch) {
    MIS_LAUNCH(c, k_nm_glu_dwconv_ln_bf16, dim3(cdiv(Tp, NM_DW_TT), batch), dim3(256), pw, taps, bias, cnt, out, stats, Tp, C, k, padl, 1e-5f);
}

// ============================================================================ host
// finalize of bf16 mode.  wm holds the eight block matrices of every layer and wt the relative_k_proj matrices and the sinusoid table (rows
// tab_lo .. tab_hi), both f32 and bound to the handle's f32 members: uploaded into buffers of this scope, the matrices rounded on the device
// into warena at the same offsets, every layer's table projected in f32 by the f32 GEMM and rounded into ptab16.  The f32 copies of those
// (and of nothing else) end with this scope.
static void nm_bf16_tables(mis_nemotron* c, const HostArena& wm, const HostArena& wt, const float* const& tab, const std::vector<SfLin>& rk) {
    const size_t d = c->d, per = (size_t)(c->tab_hi - c->tab_lo + 1) * d, nw = wm.fhost.size();
    DevBuf<bf16_t> none, none2;
    DevBuf<float> fm, ft, proj;
    wm.upload(none, fm);
    wt.upload(none2, ft);
    c->warena.alloc(nw);
    MIS_LAUNCH(c, k_pk_round_bf16, dim3((unsigned)((nw + 255) / 256)), dim3(256), fm.p, c->warena.p, nw);
    c->fc16.assign(c->L, mis_nemotron::Layer16{});
    proj.alloc(per);
    c->ptab16.alloc(c->L * per);
    for (int li = 0; li < c->L; ++li) {
        mis_nemotron::Layer& l = c->fc[li];
        mis_nemotron::Layer16& w = c->fc16[li];
        auto take = [&](SfLin& lin, bf16_t*& dst) { dst = c->warena.p + (lin.w - fm.p); lin.w = nullptr; };
        take(l.ff1a, w.ff1a); take(l.ff1b, w.ff1b); take(l.qkv, w.qkv); take(l.o, w.o);
        take(l.pw1, w.pw1); take(l.pw2, w.pw2); take(l.ff2a, w.ff2a); take(l.ff2b, w.ff2b);
        sf_gemm(c, sf_lin(tab, (int)d, rk[li], proj.p, (int)d, nullptr, (int)(per / d)), 1);
        w.P = c->ptab16.p + li * per;
        MIS_LAUNCH(c, k_pk_round_bf16, dim3((unsigned)((per + 255) / 256)), dim3(256), proj.p, w.P, per);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// c->emb -> the Conformer blocks in bf16 mode -> c->h (1 + 15 L launches, launch for launch as nm_encoder)
static void nm_encoder_bf16(mis_nemotron* c, int stop) {
    const int B = c->batch, Tp = c->Tp, d = c->d, f = c->f, M = B * Tp;
    const int* cnt = c->cnt3.p;
    const size_t nd = (size_t)M * d;
    MIS_LAUNCH(c, k_sf_intake, dim3((unsigned)((nd + 255) / 256)), dim3(256), c->emb.p, c->h.p, cnt, Tp, d, c->cfg.scale_input ? sqrtf((float)d) : 1.0f, nd);
    auto stats = [&]() { MIS_LAUNCH(c, k_sf_stats, dim3(cdiv(M, 4)), dim3(256), c->h.p, c->stats.p, d, 1e-5f, M); };
    auto gemm = [&](const PkbRole& r, const bf16_t* W, const float* bias, int N, int K, const float* lnw, const float* lnb, const bf16_t* xb, bf16_t* yb, float ra) {
        PkbGemm p{};
        p.W = W; p.bias = bias; p.cnt = cnt; p.Tp = Tp; p.K = K; p.N = N; p.epi = r.epi; p.ldx = K; p.ldy = N;
        if (r.load != PKB_LOAD_BF16) { p.stats = c->stats.p; p.lnw = lnw; p.lnb = lnb; }
        if (r.load == PKB_LOAD_LN) p.Xf = c->h.p;
        else p.Xb = xb;
        if (r.epi == PKB_EPI_RES) { p.Yf = c->h.p; p.R = c->h.p; p.ldr = N; p.ra = ra; }
        else p.Yb = yb;
        nmb_gemm_launch(c, p, r.load, r.rule, B);
    };
    bf16_t *big = c->big16.p, *qkv = c->qkv16.p, *att = c->att16.p;
    for (int li = 0; li < c->L; ++li) {                            // 15 launches a block
        const mis_nemotron::Layer& l = c->fc[li];
        const mis_nemotron::Layer16& w = c->fc16[li];
        stats();
        gemm(PKB_ROLE[PKB_FF1A], w.ff1a, l.ff1a.b, f, d, l.ln1w, l.ln1b, nullptr, big, 0.0f);
        gemm(PKB_ROLE[PKB_FF1B], w.ff1b, l.ff1b.b, d, f, nullptr, nullptr, big, nullptr, 0.5f);
        stats();
        gemm(PKB_ROLE[PKB_QKV], w.qkv, l.qkv.b, 3 * d, d, l.lnaw, l.lnab, nullptr, qkv, 0.0f);
        NmbAttn ap{qkv, 3 * d, d, 2 * d, att, d, cnt, Tp, c->hd, 1.0f, sqrtf((float)c->hd), l.u, l.v, w.P, d, -c->tab_lo,
                   c->ctx.C, c->ctx.L, c->ctx.dlo, c->ctx.dhi};
        nmb_attn(c, ap, c->H, c->hd, B);
        gemm(PKB_ROLE[PKB_O], w.o, l.o.b, d, d, nullptr, nullptr, att, nullptr, 1.0f);
        stats();
        gemm(PKB_ROLE[PKB_PW1], w.pw1, l.pw1.b, 2 * d, d, l.lncw, l.lncb, nullptr, big, 0.0f);
        nmb_glu_dwconv_ln(c, big, l.dw, l.dwb, cnt, att, c->stats.p, Tp, d, c->ck, c->padl, B);
        gemm(NMB_PW2, w.pw2, l.pw2.b, d, d, l.cnw, l.cnb, att, nullptr, 1.0f);
        stats();
        gemm(PKB_ROLE[PKB_FF2A], w.ff2a, l.ff2a.b, f, d, l.ln2w, l.ln2b, nullptr, big, 0.0f);
        gemm(PKB_ROLE[PKB_FF2B], w.ff2b, l.ff2b.b, d, f, nullptr, nullptr, big, nullptr, 0.5f);
        MIS_LAUNCH(c, k_sf_ln, dim3(cdiv(M, 4)), dim3(256), c->h.p, c->h.p, l.lnow, l.lnob, d, 1e-5f, M, cnt, Tp);
        if (stop == li + 1) return;
    }
}

}  // namespace
