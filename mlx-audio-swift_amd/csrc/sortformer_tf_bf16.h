// sortformer_tf_bf16.h - the opt-in bf16 form of Sortformer's post-LN BART tower (sortformer.hip, behind parakeet_encoder_bf16.h, whose
// k_pk_gemm_bf16, k_pk_round_bf16 and pkb_chunk it reuses).  The tower is d_model 192, 8 heads of 24, ffn 768 at the published shape:
// seven launches a layer in f32 mode, each a 64 x 64-tile GEMM, an attention launch or a LayerNorm over a matrix only 192 wide - launch-
// and fill-bound.  Here a layer is THREE launches: q | k | v (k_pk_gemm_bf16, bf16 rows in and out), k_sf_tf_attn_bf16, k_sf_tf_tail_bf16.
//
// PRECISION CONTRACT of the bf16 tower.
//   f32: the stream g, positions, biases, LayerNorm parameters and statistics, the softmax, every accumulator and epilogue.
//   bf16, round-to-nearest-even, once, at each of these points: the matrices q | k | v (packed), out_proj, fc1, fc2; g16 = bf16(g), the
//        q | k | v operand; the gq16 store; q hd^-0.5 (scaled in f32, then rounded); the probabilities in front of P V (the row sum adds the
//        unrounded ones); the ga16 store; x1 as fc1's operand (its f32 value is kept for the residual); the ReLU hidden tile.
//   As in f32 mode a row's bits do not depend on its batch, on the longest row or on what lies behind cnt[b] (NaN included): every output
//   element is one accumulator over k-slabs in ascending order, tiles depend on the widths only, no atomics.
//
// Kernels:
//   k_sf_tf_attn_bf16<NS>  plain flash attention for small heads, head sizes 1..64 zero-padded to NS = 1, 2 slabs of 32.  A block is 16
//                          queries x 4 heads x row: four waves, wave w owns head 4 blockIdx.y + w of those queries and never meets another
//                          wave (no block barrier, no atomics).  Scores are formed transposed, S^T[key][query]: the K rows are the MFMA A
//                          operand, read straight from gq16 in 16-byte chunks in the order 8 (r >> 2) + 4 t + (r & 3), so a lane ends up
//                          with the eight CONSECUTIVE keys 8 g .. 8 g + 7 of its query - exactly the B fragment of P V (the trick of
//                          k_pk_attn_bf16).  V is transposed through the wave's own LDS patch [32 NS][40] bf16.  32-key tiles ascending over
//                          the row's own cnt[b] keys; online softmax in f32.  LDS: 4 x 32 NS x 80 = 10240 NS bytes.
//   k_sf_tf_tail_bf16      everything behind attention: x1 = LN1(g + o(att) + b_o), g' = LN2(x1 + fc2(ReLU(fc1(x1) + b1)) + b2).  A block
//                          owns 16 rows of one batch entry at full width (d_model <= 256, ffn <= 1024); four waves split the output
//                          columns of each contraction in 16-column MFMA tiles, tile 4 i + wave.  The weights (bf16 [N][K]) are the A
//                          operand and stream from global / L2 straight into registers, 16 bytes a lane and tile, TWO k-slabs ahead of
//                          the MFMAs (as k_cn_lin_bf16 of canary.hip, one slab deeper); the 16 activation rows are the B operand from
//                          LDS.  LDS: the att tile, later x1 as bf16 (one buffer: att is dead behind out_proj) 16 x 264 x 2 = 8448, the
//                          f32 row tile (residual, then x1, then the sum LN2 reads) 16 x 260 x 4 = 16640, the hidden tile 16 x 1032 x 2 =
//                          33024: 58112 bytes reserved, of which the published shape 192 / 768 uses 6400 + 12544 + 24832 = 43776.  Both
//                          LayerNorms in f32 over the unrounded sums, one wave a row (wave_mean_rstd).  Writes g' (f32: the stream, the
//                          taps) and g16 = bf16(g'); rows behind cnt[b] are zeros in both.
//   A 32-row tail block needs 12288 + 24576 + 49152 = 86016 bytes at 192 / 768: over the 64 KiB static limit, so 16 rows stand.
#pragma once

#include "bf16_tile.h"

namespace {

constexpr int SFT_DT_MAX = 256, SFT_FT_MAX = 1024;          // the tail's LDS tile

// ============================================================================ attention
struct SftAttn {
    const bf16_t* qkv; int ld, koff, voff;                   // q at column h hd, k at koff + h hd, v at voff + h hd
    bf16_t* out; int ldo;
    const int* cnt; int Tp, hd, heads;
    float qscale;                                            // q x qscale in f32, then rounded
};

__device__ __forceinline__ void sft_wave_sync() {            // LDS writes of this wave are visible to its own later reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NS>
__global__ void __launch_bounds__(256) k_sf_tf_attn_bf16(SftAttn p) {
    constexpr int HP = 32 * NS, CH = HP / 8;
    __shared__ __attribute__((aligned(16))) bf16_t Vt[4][HP][BF16_LD];  // a wave's V tile [dimension][key]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y * 4 + wave, q0 = blockIdx.x * 16, n = min(p.cnt[b], p.Tp), hd = p.hd;
    if (h >= p.heads) return;                                       // (uniform over the wave; nothing below waits for another wave)
    const size_t rowbase = (size_t)b * p.Tp;
    if (q0 >= n) {                                                  // (uniform over the block)
        for (int i = lane; i < 16 * hd; i += 64) {
            const int t = q0 + i / hd;
            if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + i % hd] = 0;
        }
        return;
    }
    const bool vec = ((hd | p.ld | p.koff | p.voff) & 7) == 0;
    const int tq = q0 + l15;
    bf16x8_t qf[NS];                                                // B fragments: query l15, dimensions 32 s + 8 g .. + 7
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = s * 32 + g * 8 + e;
            qf[s][e] = (short)f32_to_bf16((c < hd && tq < n) ? bf16_to_f32(p.qkv[(rowbase + tq) * p.ld + h * hd + c]) * p.qscale : 0.0f);
        }
    f32x4_t O[2 * NS];                                              // O^T: dimension 16 t + 4 g + e of query l15
#pragma unroll
    for (int t = 0; t < 2 * NS; ++t) O[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.0f;
    const int kr0 = 8 * (l15 >> 2) + (l15 & 3);                     // A row l15 of key tile t reads key kr0 + 4 t: D rows 4 g + e are keys 8 g + 4 t + e
    bf16_t (*vt)[BF16_LD] = Vt[wave];
    const bf16_t* kbase = p.qkv + p.koff + h * hd;
    const bf16_t* vbase = p.qkv + p.voff + h * hd;
    for (int kb = 0; kb < n; kb += 32) {
        uint4 ka[2][NS];                                            // K rows as A fragments, straight from global; keys behind n are zeros
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int key = kb + kr0 + 4 * t;
#pragma unroll
            for (int s = 0; s < NS; ++s)
                ka[t][s] = key < n ? pkb_chunk(kbase + (rowbase + key) * p.ld, s * 32 + g * 8, hd, vec) : make_uint4(0, 0, 0, 0);
        }
        sft_wave_sync();                                            // the previous tile's reads of the patch are done
        for (int i = lane; i < 32 * CH; i += 64) {                  // V transposed: consecutive lanes, consecutive keys
            const int r = i & 31, cc = (i >> 5) * 8, key = kb + r;
            const uint4 q = key < n ? pkb_chunk(vbase + (rowbase + key) * p.ld, cc, hd, vec) : make_uint4(0, 0, 0, 0);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) vt[cc + e][r] = (bf16_t)(w[e >> 1] >> (16 * (e & 1)));
        }
        sft_wave_sync();
        f32x4_t S0 = {0.f, 0.f, 0.f, 0.f}, S1 = S0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            S0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ka[0][s]), qf[s], S0, 0, 0, 0);
            S1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ka[1][s]), qf[s], S1, 0, 0, 0);
        }
        float sc[8], mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {                               // keys 8 g .. 8 g + 7 of the tile
            sc[e] = (kb + 8 * g + e < n) ? (e < 4 ? S0[e & 3] : S1[e & 3]) : -INFINITY;
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
            O[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&vt[t * 16 + l15][g * 8]), pf, O[t], 0, 0, 0);
        }
    }
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);                // the four lane groups of a query, one fixed order
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
static void sft_attn(Ctx* c, const SftAttn& p, int batch) {
    const dim3 grid(cdiv(p.Tp, 16), cdiv(p.heads, 4), batch);
    if (p.hd <= 32) MIS_LAUNCH(c, k_sf_tf_attn_bf16<1>, grid, dim3(256), p);
    else MIS_LAUNCH(c, k_sf_tf_attn_bf16<2>, grid, dim3(256), p);
}

// ============================================================================ the layer's tail
// dt % 32 == 0, dt <= SFT_DT_MAX, ft % 32 == 0, ft <= SFT_FT_MAX; g and gout may be the same buffer (a block reads its rows, then writes them)
struct SftTail {
    const bf16_t* att; const float* g;                       // [B Tp][dt]: the attention output, the stream
    float* gout; bf16_t* g16;                                // [B Tp][dt]: g' and bf16(g')
    const int* cnt; int Tp, dt, ft; float eps;
    const bf16_t *Wo, *W1, *W2;                              // [dt][dt], [ft][dt], [dt][ft]
    const float *bo, *b1, *b2, *ln1w, *ln1b, *ln2w, *ln2b;
};

// acc[i] = the 16-column tile tbase + 4 i + wave of Y^T = W X^T, X the block's 16 rows in LDS (row stride ldx): D row 4 g + e is column
// 16 tile + 4 g + e, D column l15 is row l15.  One accumulator an element, k-slabs of 32 ascending; the weights of two slabs in flight.
template <int TW>
__device__ __forceinline__ void sft_contract(const bf16_t* __restrict__ W, int K, int N, int tbase, const bf16_t* Xs, int ldx, f32x4_t (&acc)[TW]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
    const bf16_t* wrow[TW];
    bool live[TW];
#pragma unroll
    for (int i = 0; i < TW; ++i) {
        const int n = 16 * (tbase + 4 * i + wave);
        live[i] = n < N;
        wrow[i] = W + (size_t)(live[i] ? n + l15 : 0) * K + 8 * g;
        acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
    if (!live[0]) return;                                           // (uniform over the wave) no tile of this pass is this wave's
    const bf16_t* xrow = Xs + l15 * ldx + 8 * g;
    const int ns = K / BF16_BK;
    uint4 w0[TW], w1[TW];
    auto load = [&](uint4 (&w)[TW], int sl) {
#pragma unroll
        for (int i = 0; i < TW; ++i) w[i] = live[i] ? *reinterpret_cast<const uint4*>(wrow[i] + sl * BF16_BK) : make_uint4(0, 0, 0, 0);
    };
    auto step = [&](const uint4 (&w)[TW], int sl) {
        const bf16x8_t x = *reinterpret_cast<const bf16x8_t*>(xrow + sl * BF16_BK);
#pragma unroll
        for (int i = 0; i < TW; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w[i]), x, acc[i], 0, 0, 0);
    };
    load(w0, 0);
    if (ns > 1) load(w1, 1);
    for (int sl = 0; sl < ns; sl += 2) {
        step(w0, sl);
        if (sl + 2 < ns) load(w0, sl + 2);
        if (sl + 1 < ns) {
            step(w1, sl + 1);
            if (sl + 3 < ns) load(w1, sl + 3);
        }
    }
}

__global__ void __launch_bounds__(256) k_sf_tf_tail_bf16(SftTail p) {
    __shared__ __attribute__((aligned(16))) float Rs[16 * (SFT_DT_MAX + 4)];    // g, then g + o(att) + b_o, then x1, then x1 + fc2(.) + b2
    __shared__ __attribute__((aligned(16))) bf16_t Ab[16 * (SFT_DT_MAX + 8)];   // the att tile, then bf16(x1)
    __shared__ __attribute__((aligned(16))) bf16_t Hs[16 * (SFT_FT_MAX + 8)];   // ReLU(fc1(x1) + b1)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, m0 = blockIdx.x * 16, T = min(p.cnt[b], p.Tp), dt = p.dt, ft = p.ft;
    const int ldr = dt + 4, lda = dt + 8, ldh = ft + 8;
    const size_t row0 = (size_t)b * p.Tp;
    if (m0 >= T) {                                                  // (uniform over the block) nothing live: zeros
        for (int i = tid; i < 16 * dt; i += 256) {
            const int m = m0 + i / dt;
            if (m >= p.Tp) continue;
            p.gout[(row0 + m) * dt + i % dt] = 0.0f;
            p.g16[(row0 + m) * dt + i % dt] = 0;
        }
        return;
    }
    for (int i = tid; i < 16 * (dt / 8); i += 256) {                // rows behind T are staged as zeros, whatever lies there
        const int r = i / (dt / 8), cc = (i % (dt / 8)) * 8;
        *reinterpret_cast<uint4*>(&Ab[r * lda + cc]) =
            m0 + r < T ? *reinterpret_cast<const uint4*>(p.att + (row0 + m0 + r) * dt + cc) : make_uint4(0, 0, 0, 0);
    }
    for (int i = tid; i < 16 * (dt / 4); i += 256) {
        const int r = i / (dt / 4), cc = (i % (dt / 4)) * 4;
        *reinterpret_cast<float4*>(&Rs[r * ldr + cc]) =
            m0 + r < T ? *reinterpret_cast<const float4*>(p.g + (row0 + m0 + r) * dt + cc) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    // R + (acc + bias) into the f32 tile: every element has one owner
    auto residual = [&](const f32x4_t (&acc)[4], const float* bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = 16 * (4 * i + wave) + 4 * g;
            if (n >= dt) continue;
            const float4 add = *reinterpret_cast<const float4*>(bias + n);
            float4* r = reinterpret_cast<float4*>(&Rs[l15 * ldr + n]);
            float4 v = *r;
            v.x += acc[i][0] + add.x; v.y += acc[i][1] + add.y; v.z += acc[i][2] + add.z; v.w += acc[i][3] + add.w;
            *r = v;
        }
    };
    {
        f32x4_t acc[4];
        sft_contract<4>(p.Wo, dt, dt, 0, Ab, lda, acc);
        residual(acc, p.bo);
    }
    __syncthreads();
    for (int r = wave; r < 16; r += 4) {                            // x1 = LN1(.), f32 for the residual and rounded once for fc1
        float* x = &Rs[r * ldr];
        float mean, rstd;
        wave_mean_rstd(x, dt, p.eps, mean, rstd);
        for (int c = lane; c < dt; c += 64) {
            const float v = fmaf((x[c] - mean) * rstd, p.ln1w[c], p.ln1b[c]);
            x[c] = v;
            Ab[r * lda + c] = f32_to_bf16(v);
        }
    }
    __syncthreads();
    for (int tb = 0; 16 * tb < ft; tb += 16) {                      // fc1 in passes of 256 columns; the hidden tile never leaves the CU
        f32x4_t acc[4];
        sft_contract<4>(p.W1, dt, ft, tb, Ab, lda, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = 16 * (tb + 4 * i + wave) + 4 * g;
            if (n >= ft) continue;
            const float4 add = *reinterpret_cast<const float4*>(p.b1 + n);
            *reinterpret_cast<uint2*>(&Hs[l15 * ldh + n]) = make_uint2(pkb_pack2(fmaxf(acc[i][0] + add.x, 0.0f), fmaxf(acc[i][1] + add.y, 0.0f)),
                                                                       pkb_pack2(fmaxf(acc[i][2] + add.z, 0.0f), fmaxf(acc[i][3] + add.w, 0.0f)));
        }
    }
    __syncthreads();
    {
        f32x4_t acc[4];
        sft_contract<4>(p.W2, ft, dt, 0, Hs, ldh, acc);
        residual(acc, p.b2);
    }
    __syncthreads();
    for (int r = wave; r < 16; r += 4) {                            // g' = LN2(.): the stream in f32 and its bf16 copy
        const int m = m0 + r;
        if (m >= p.Tp) continue;
        float* go = p.gout + (row0 + m) * dt;
        bf16_t* gb = p.g16 + (row0 + m) * dt;
        if (m >= T) {
            for (int c = lane; c < dt; c += 64) { go[c] = 0.0f; gb[c] = 0; }
            continue;
        }
        const float* x = &Rs[r * ldr];
        float mean, rstd;
        wave_mean_rstd(x, dt, p.eps, mean, rstd);
        for (int c = lane; c < dt; c += 64) {
            const float v = fmaf((x[c] - mean) * rstd, p.ln2w[c], p.ln2b[c]);
            go[c] = v;
            gb[c] = f32_to_bf16(v);
        }
    }
}

template <class Ctx>
static void sft_tail(Ctx* c, const SftTail& p, int batch) {
    MIS_LAUNCH(c, k_sf_tf_tail_bf16, dim3(cdiv(p.Tp, 16), batch), dim3(256), p);
}

// ============================================================================ host
struct SfTfLayer16 { bf16_t *qkv, *o, *fc1, *fc2; };

// what bf16 mode asks of the tower's widths (the Conformer half: pk_set_encoder_dtype)
template <class Cfg>
static void sft_check(const Cfg& cfg) {
    MIS_REQUIRE(cfg.tf_d_model % 32 == 0, MIS_ERR_INVALID_INPUT, "tf_d_model %d: the bf16 encoder needs a multiple of 32", cfg.tf_d_model);
    MIS_REQUIRE(cfg.encoder_ffn_dim % 32 == 0, MIS_ERR_INVALID_INPUT, "encoder_ffn_dim %d: the bf16 encoder needs a multiple of 32", cfg.encoder_ffn_dim);
    MIS_REQUIRE(cfg.tf_d_model <= SFT_DT_MAX, MIS_ERR_INVALID_INPUT, "tf_d_model %d: the bf16 encoder holds up to %d (the tail's LDS tile)", cfg.tf_d_model,
                SFT_DT_MAX);
    MIS_REQUIRE(cfg.encoder_ffn_dim <= SFT_FT_MAX, MIS_ERR_INVALID_INPUT, "encoder_ffn_dim %d: the bf16 encoder holds up to %d (the tail's LDS tile)",
                cfg.encoder_ffn_dim, SFT_FT_MAX);
}

// c->g (the projection + positions) -> the BART layers in bf16 mode -> c->g: 1 + 3 Lt launches.  stop as sf_encoder's.
template <class Ctx>
static void sf_tower_bf16(Ctx* c, int stop) {
    const int B = c->batch, Tp = c->Tp, dt = c->dt, ft = c->ft;
    const int* cnt = c->cnt3.p;
    const size_t n = (size_t)B * Tp * dt;
    MIS_LAUNCH(c, k_pk_round_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), c->g.p, c->g16.p, n);
    for (int li = 0; li < c->Lt; ++li) {                           // 3 launches a layer
        const auto& l = c->tf[li];
        const SfTfLayer16& w = c->tf16[li];
        PkbGemm q{};
        q.Xb = c->g16.p; q.ldx = dt; q.W = w.qkv; q.bias = l.qkv.b; q.Yb = c->gq16.p; q.ldy = 3 * dt; q.cnt = cnt; q.Tp = Tp; q.K = dt; q.N = 3 * dt;
        q.epi = PKB_EPI_NONE;
        pkb_gemm_launch(c, q, PKB_LOAD_BF16, PKB_TILE64, B);
        sft_attn(c, SftAttn{c->gq16.p, 3 * dt, dt, 2 * dt, c->ga16.p, dt, cnt, Tp, c->hdt, c->Ht, powf((float)c->hdt, -0.5f)}, B);
        sft_tail(c, SftTail{c->ga16.p, c->g.p, c->g.p, c->g16.p, cnt, Tp, dt, ft, c->cfg.layer_norm_eps, w.o, w.fc1, w.fc2, l.o.b, l.fc1.b, l.fc2.b,
                            l.ln1w, l.ln1b, l.ln2w, l.ln2b}, B);
        if (stop == c->L + 2 + li) return;
    }
}

}  // namespace
