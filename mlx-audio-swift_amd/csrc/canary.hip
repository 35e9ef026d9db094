// canary.hip - Canary speech-to-text and translation: 16 kHz samples -> Parakeet's encoder (parakeet_encoder.h: NeMo log-mel, dw-striding
// stem, FastConformer blocks) -> optional projection -> the cross-attention K and V of every decoder layer, once -> a pre-LN Transformer
// decoder run ONE TOKEN A STEP over cached K/V, with the vocabulary head fused with the arg-max and the token bookkeeping on the device.
// Exact f32 throughout, unless mis_canary_set_encoder_dtype(MIS_BF16) selects the bf16 form of the encoder's Conformer blocks
// (parakeet_encoder_bf16.h) and mis_canary_set_decoder_dtype(MIS_BF16) the bf16 form of the decoder's step: the step matrices and both
// K | V stores as bf16, k_cn_lin_bf16 and k_cn_attn_step_bf16 in place of k_cn_lin and k_cn_attn_step (precision contract: mi_speech.h).
//
// Reference being replaced: CanaryModel (Sources/MLXAudioSTT/Models/Canary/CanaryModel.swift generate :385-432, CanaryDecoder :288-329,
// CanaryDecoderBlock :245-286, CanaryAttention :200-243, CanaryFixedPositionalEncoding :166-198).  The reference re-runs the whole prefix
// at every token; here a step costs one token.
//
// The step's kernels:
//   k_cn_lin        Y[M, N] = X[M, K] W[N, K]^T for M = 1..64 rows on v_mfma_f32_32x32x2_f32.  A block owns 32 output columns and MT = 1 or 2
//                   32-row tiles; grid (ceil(N / 32), S).  K goes by slabs of 128: the block stages X[0..M)[slab] through LDS (row stride
//                   129), and wave w owns the slab's columns 32 w .. 32 w + 31: its lane (l31, kh) loads the 16 consecutive floats
//                   W[n0 + l31][slab + 32 w + 16 kh ..] as four 16-byte loads and feeds them as the MFMA's B operand, so every weight byte
//                   is read once, by one wave, straight into registers.  The four accumulators are added through LDS in wave order.
//                   S = 1: bias, optional ReLU, optional scatter of columns >= kvoff into the self-attention cache at pos[m], optional
//                   (max, lowest index) pair of the tile per row (the head: no logit reaches memory unless Y is given).  Partial mode:
//                   the raw sums go to part[s][m][n].  No atomics; a row's value depends on its own X row and W only.
//   k_cn_rows       one block a row: x += bias + sum_s part[s] (ascending s), then the next sub-layer's LayerNorm -> xn.
//   k_cn_attn_step  one block a (row, head), four waves: one query against n keys of a [rows][2 h] K | V store.  32-key tiles go to the
//                   waves round-robin; a lane pair (key, half of the head) forms the score; online softmax per wave; the lane owns output
//                   dimensions lane and lane + 64; the four (m, l, acc) are merged through LDS in wave order.
//   k_cn_select     one block a row: combines the head's pairs in tile order (ties to the lower index), takes the prompt token while the
//                   row is inside its prompt, applies the reference's loop rule (eos ends the row and is not appended; max_tokens ends it),
//                   counts finished rows, advances pos and forms the next input: LayerNorm_e(embedding[token] + sinusoid[min(pos, 1023)])
//                   -> x, then layer 0's self_attn_norm -> xn.
//
// Launches: encode = 7 + 15 L_enc (+ 1 with a projection); generate = that + L_dec (cross K/V) + 1 (first input) + steps (11 L_dec + 2).
// The bf16 decoder keeps the f32 projection of the cross K/V and rounds each layer into its bf16 store: 2 L_dec there, the step unchanged.
#include "common.h"
#define AUDIO_FRONT_NEMO_KERNELS
#include "audio_front.h"
#include "f32_tile.h"
#include "host_weights.h"
#include "step_loop.h"
#include "sortformer_kernels.h"
#include "parakeet_encoder.h"
#include "parakeet_encoder_bf16.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <memory>

#define CN_KS 128                    // K columns of a slab
#define CN_LDX 129                   // LDS row stride of the staged X slab
#define CN_MAXH 4096                 // decoder width
#define CN_POS_ROWS 1024
#define CN_MAX_STORE_BYTES ((int64_t)4 << 30)

// ============================================================================ the skinny contraction
struct CnLin {
    const float* X; int ldx;
    const float* W; const float* bias;
    int M, K, N, sps;                                                // sps: slabs a split takes
    float* Y; int ldy;                                               // direct output (null: none)
    float* part;                                                     // partial mode: [S][M][N], no bias
    int relu;
    float* kv; const int* pos; int cap, kvoff;                       // columns >= kvoff -> kv[(m cap + pos[m]) (N - kvoff) + n - kvoff]
    float* amv; int* ami; int nt;                                    // the head: per row and tile (max, lowest index) [M][nt]
    const bf16_t* Wb; bf16_t* kvb;                                   // the bf16 decoder (k_cn_lin_bf16): W and the self K/V cache as bf16
};

template <int MT>
__global__ void __launch_bounds__(256) k_cn_lin(CnLin p) {
    __shared__ float Xs[MT * 32 * CN_LDX];                           // the staged slab; afterwards the four waves' accumulators
    __shared__ float Fin[MT * 32][33];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int n0 = blockIdx.x * 32, s = blockIdx.y, nrow = n0 + l31;
    const bool wlive = nrow < p.N, wide = (p.K & 3) == 0;
    const float* wrow = p.W + (size_t)(wlive ? nrow : 0) * p.K;
    f32x16_t acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
    const int ns = (p.K + CN_KS - 1) / CN_KS, sl1 = min((s + 1) * p.sps, ns);
    for (int sl = s * p.sps; sl < sl1; ++sl) {
        const int k0 = sl * CN_KS, kw = k0 + 32 * wave + 16 * kh;
        float wf[16];
        if (wlive && wide && kw + 16 <= p.K) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4_t v = *reinterpret_cast<const f32x4_t*>(wrow + kw + 4 * j);
                wf[4 * j] = v[0]; wf[4 * j + 1] = v[1]; wf[4 * j + 2] = v[2]; wf[4 * j + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) wf[i] = (wlive && kw + i < p.K) ? wrow[kw + i] : 0.0f;
        }
        __syncthreads();                                             // the previous slab's reads are done
        for (int i = tid; i < MT * 32 * CN_KS; i += 256) {
            const int r = i >> 7, c = i & 127;
            Xs[r * CN_LDX + c] = (r < p.M && k0 + c < p.K) ? p.X[(size_t)r * p.ldx + k0 + c] : 0.0f;
        }
        __syncthreads();
        const float* xa = Xs + l31 * CN_LDX + 32 * wave + 16 * kh;
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[mt * 32 * CN_LDX + i], wf[i], acc[mt], 0, 0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) Xs[((wave * MT + mt) * 16 + r) * 64 + lane] = acc[mt][r];
    __syncthreads();
    for (int e = tid; e < MT * 1024; e += 256) {                     // wave 0 + 1 + 2 + 3, in that order
        const int mt = e >> 10, r = (e >> 6) & 15, ln = e & 63;
        float v = Xs[((0 * MT + mt) * 16 + r) * 64 + ln];
#pragma unroll
        for (int w = 1; w < 4; ++w) v += Xs[((w * MT + mt) * 16 + r) * 64 + ln];
        Fin[mt * 32 + f32_tile_row(r, ln >> 5)][ln & 31] = v;
    }
    __syncthreads();
    for (int e = tid; e < MT * 1024; e += 256) {
        const int m = e >> 5, ci = e & 31, n = n0 + ci;
        if (m >= p.M || n >= p.N) continue;
        float v = Fin[m][ci];
        if (p.part) { p.part[((size_t)s * p.M + m) * p.N + n] = v; continue; }
        if (p.bias) v += p.bias[n];
        if (p.relu) v = fmaxf(v, 0.0f);
        Fin[m][ci] = v;
        if (p.kv && n >= p.kvoff) p.kv[((size_t)m * p.cap + min(p.pos[m], p.cap - 1)) * (p.N - p.kvoff) + (n - p.kvoff)] = v;
        else if (p.Y) p.Y[(size_t)m * p.ldy + n] = v;
    }
    if (p.amv) {
        __syncthreads();
        if (tid < MT * 32 && tid < p.M) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int ci = 0; ci < 32 && n0 + ci < p.N; ++ci)
                if (Fin[tid][ci] > bv) { bv = Fin[tid][ci]; bi = n0 + ci; }
            p.amv[(size_t)tid * p.nt + blockIdx.x] = bv;
            p.ami[(size_t)tid * p.nt + blockIdx.x] = bi;
        }
    }
}

// ---------------------------------------------------------------------------- the same contraction with bf16 weights (the bf16 decoder)
// Y[M, N] = bf16(X)[M, K] Wb[N, K]^T on v_mfma_f32_16x16x32_bf16, f32 accumulators; the outer shape is k_cn_lin's (32 columns a block,
// grid (ceil(N / 32), S), slabs of 128, wave w owns the slab's columns 32 w .. 32 w + 31 = one MFMA k-step) and so are cn_split_for, part,
// k_cn_rows, the pairs and k_cn_select.  W is the A operand: lane (n = lane & 15, kq = lane >> 4) loads the 8 bf16
// W[n0 + 16 t + n][k0 + 32 w + 8 kq ..] of tile t = 0, 1 as one 16-byte load, straight into registers, the next slab's while this one is
// contracted: every weight byte is read once, by one wave.  X is the B operand: the block stages X[0..16 MT)[slab] through LDS, rounded to
// bf16 as it is staged (row stride 136 elements = 272 bytes: 16-byte fragments stay aligned and the 16 rows of one kq start 4 banks apart),
// and both column tiles share the fragment.  C/D: lane l, element e = column 16 t + 4 (l >> 4) + e of row 16 mt + (l & 15): four
// consecutive n of one row, so Y, part and cache stores are 16 (bf16: 8) bytes along n.  Waves 1..3 hand their accumulators to wave 0
// through LDS; wave 0 adds them in wave order and runs k_cn_lin's epilogue.  K % 32 == 0; N, M and the last slab are guarded.
#define CNB_LDX 136

__device__ __forceinline__ uint32_t cnb_pack2(float a, float b) { return (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16); }

template <int MT>
__global__ void __launch_bounds__(256) k_cn_lin_bf16(CnLin p) {
    __shared__ f32x4_t Red[3 * 2 * MT * 64];                         // first the staged slab (4352 MT of its 6144 MT bytes), then the accumulators of waves 1..3
    bf16_t* Xs = reinterpret_cast<bf16_t*>(Red);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 32, s = blockIdx.y, kl = 32 * wave + 8 * kq;
    const bf16_t* wrow[2];
    bool wlive[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int nrow = n0 + 16 * t + l15;
        wlive[t] = nrow < p.N;
        wrow[t] = p.Wb + (size_t)(wlive[t] ? nrow : 0) * p.K + kl;
    }
    f32x4_t acc[2][MT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[t][mt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const int ns = (p.K + CN_KS - 1) / CN_KS, sl0 = s * p.sps, sl1 = min((s + 1) * p.sps, ns);
    bf16x8_t wn[2];
    auto loadw = [&](int sl) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
            wn[t] = (wlive[t] && sl * CN_KS + kl + 8 <= p.K) ? *reinterpret_cast<const bf16x8_t*>(wrow[t] + (size_t)sl * CN_KS) : (bf16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
    };
    if (sl0 < sl1) loadw(sl0);
    for (int sl = sl0; sl < sl1; ++sl) {
        const int k0 = sl * CN_KS;
        __syncthreads();                                             // the previous slab's reads are done
        for (int i = tid; i < MT * 16 * (CN_KS / 4); i += 256) {     // four floats a thread -> four bf16, rounded here, once
            const int r = i >> 5, cc = (i & 31) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < p.M && k0 + cc < p.K) v = *reinterpret_cast<const float4*>(p.X + (size_t)r * p.ldx + k0 + cc);
            *reinterpret_cast<uint2*>(Xs + r * CNB_LDX + cc) = make_uint2(cnb_pack2(v.x, v.y), cnb_pack2(v.z, v.w));
        }
        __syncthreads();
        const bf16x8_t w0 = wn[0], w1 = wn[1];
        if (sl + 1 < sl1) loadw(sl + 1);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const bf16x8_t x = *reinterpret_cast<const bf16x8_t*>(Xs + (mt * 16 + l15) * CNB_LDX + kl);
            acc[0][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, x, acc[0][mt], 0, 0, 0);
            acc[1][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, x, acc[1][mt], 0, 0, 0);
        }
    }
    __syncthreads();
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) Red[(((wave - 1) * 2 + t) * MT + mt) * 64 + lane] = acc[t][mt];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 1; w < 4; ++w)                                      // wave 0 + 1 + 2 + 3, in that order
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const f32x4_t o = Red[(((w - 1) * 2 + t) * MT + mt) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t][mt][e] += o[e];
            }
    const bool vec = ((p.N | p.ldy | p.kvoff) & 3) == 0;             // a lane's four columns are one aligned store
    const int kvw = p.N - p.kvoff;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = mt * 16 + l15;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int nq = n0 + 16 * t + 4 * kq;
            if (m >= p.M || nq >= p.N) continue;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[t][mt][e];
            if (p.part) {
                float* dst = p.part + ((size_t)s * p.M + m) * p.N + nq;
                if (vec) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (nq + e < p.N) dst[e] = v[e];
                }
                continue;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (nq + e >= p.N) continue;
                if (p.bias) v[e] += p.bias[nq + e];
                if (p.relu) v[e] = fmaxf(v[e], 0.0f);
                if (v[e] > bv) { bv = v[e]; bi = nq + e; }               // columns ascend inside the lane: the lowest index of equal maxima
            }
            const size_t kvrow = p.kvb ? ((size_t)m * p.cap + min(p.pos[m], p.cap - 1)) * kvw : 0;
            if (vec) {
                if (p.kvb && nq >= p.kvoff) *reinterpret_cast<uint2*>(p.kvb + kvrow + (nq - p.kvoff)) = make_uint2(cnb_pack2(v[0], v[1]), cnb_pack2(v[2], v[3]));
                else if (p.Y) *reinterpret_cast<float4*>(p.Y + (size_t)m * p.ldy + nq) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int n = nq + e;
                    if (n >= p.N) continue;
                    if (p.kvb && n >= p.kvoff) p.kvb[kvrow + (n - p.kvoff)] = f32_to_bf16(v[e]);
                    else if (p.Y) p.Y[(size_t)m * p.ldy + n] = v[e];
                }
            }
        }
        if (p.amv) {                                                 // (uniform) the four lanes of a row, by k_cn_select's rule
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (kq == 0 && m < p.M) { p.amv[(size_t)m * p.nt + blockIdx.x] = bv; p.ami[(size_t)m * p.nt + blockIdx.x] = bi; }
        }
    }
}

// S for a split role, from N alone: the power of two up to 8 with which ceil(N / 32) S first reaches 256 blocks
static int cn_split_for(int N) {
    const int tiles = cdiv(N, 32);
    int S = 1;
    while (S < 8 && tiles * S < 256) S *= 2;
    return S;
}

template <class Ctx>
static void cn_lin(Ctx* c, CnLin p, int S) {
    p.sps = cdiv(cdiv(p.K, CN_KS), S);
    const dim3 grid(cdiv(p.N, 32), S);
    if (p.Wb) {                                                      // the bf16 decoder: 16-row tiles, M <= 16 / 32 / 64
        if (p.M <= 16) MIS_LAUNCH(c, k_cn_lin_bf16<1>, grid, dim3(256), p);
        else if (p.M <= 32) MIS_LAUNCH(c, k_cn_lin_bf16<2>, grid, dim3(256), p);
        else MIS_LAUNCH(c, k_cn_lin_bf16<4>, grid, dim3(256), p);
    } else if (p.M <= 32) MIS_LAUNCH(c, k_cn_lin<1>, grid, dim3(256), p);
    else MIS_LAUNCH(c, k_cn_lin<2>, grid, dim3(256), p);
}

// ============================================================================ one block a row: residual + split-K reduction + LayerNorm
// the sum of one value a thread over the block: xor-tree inside a wave, then wave 0 + 1 + 2 + 3
__device__ __forceinline__ float cn_block_sum(float v, float* sh) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// v: the thread's values of columns tid + 256 j (zero behind h); torch.nn.LayerNorm, eps 1e-5, two passes
__device__ __forceinline__ void cn_layernorm(const float (&v)[CN_MAXH / 256], int h, const float* __restrict__ w, const float* __restrict__ b,
                                             float (&o)[CN_MAXH / 256], float* sh) {
    const int tid = threadIdx.x;
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < CN_MAXH / 256; ++j) s += v[j];
    const float mean = cn_block_sum(s, sh) / (float)h;
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < CN_MAXH / 256; ++j) { const int cc = tid + 256 * j; if (cc < h) { const float dlt = v[j] - mean; q += dlt * dlt; } }
    const float rstd = 1.0f / sqrtf(cn_block_sum(q, sh) / (float)h + 1e-5f);
#pragma unroll
    for (int j = 0; j < CN_MAXH / 256; ++j) { const int cc = tid + 256 * j; o[j] = cc < h ? fmaf((v[j] - mean) * rstd, w[cc], b[cc]) : 0.0f; }
}

struct CnRows { float* x; float* xn; const float* bias; const float* part; int S, M, h; const float *lnw, *lnb; };

__global__ void __launch_bounds__(256) k_cn_rows(CnRows p) {
    __shared__ float sh[4];
    const int m = blockIdx.x, tid = threadIdx.x;
    if (m >= p.M) return;
    float v[CN_MAXH / 256], o[CN_MAXH / 256];
#pragma unroll
    for (int j = 0; j < CN_MAXH / 256; ++j) {
        const int cc = tid + 256 * j;
        float a = 0.0f;
        if (cc < p.h) {
            a = p.x[(size_t)m * p.h + cc] + p.bias[cc];
            for (int s = 0; s < p.S; ++s) a += p.part[((size_t)s * p.M + m) * p.h + cc];
            p.x[(size_t)m * p.h + cc] = a;
        }
        v[j] = a;
    }
    cn_layernorm(v, p.h, p.lnw, p.lnb, o, sh);
#pragma unroll
    for (int j = 0; j < CN_MAXH / 256; ++j) { const int cc = tid + 256 * j; if (cc < p.h) p.xn[(size_t)m * p.h + cc] = o[j]; }
}

// ============================================================================ one query against cached keys
struct CnAttn {
    const float* q; int ldq;                                         // query of row m, head hh: q[m ldq + hh hd ..]
    const float* kv; int ld, voff;                                   // key j of row m: kv[(m cap + j) ld + hh hd ..], its value voff further
    int cap; const int* capd;                                        // rows of a batch entry (capd: read from the device instead)
    const int* cnt; int cnt_add;                                     // keys of row m: cnt[m] + cnt_add, at most cap
    float* out; int ldo; int hd; float scale;
    const bf16_t* kvb;                                               // the bf16 decoder (k_cn_attn_step_bf16): the store as bf16, same layout
};

__global__ void __launch_bounds__(256) k_cn_attn_step(CnAttn p) {
    __shared__ float Qs[128], Ms[4], Ls[4], As[4][128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int m = blockIdx.x, hh = blockIdx.y, hd = p.hd, cap = p.capd ? *p.capd : p.cap, n = max(1, min(p.cnt[m] + p.cnt_add, cap));
    const int HP = hd <= 64 ? 64 : 128, half = HP / 2;               // the head, zero-padded to 64 or 128
    if (tid < 128) Qs[tid] = tid < hd ? p.q[(size_t)m * p.ldq + hh * hd + tid] : 0.0f;
    __syncthreads();
    const float* base = p.kv + (size_t)m * cap * p.ld + hh * hd;
    float m_run = -INFINITY, l_run = 0.0f, a0 = 0.0f, a1 = 0.0f;
    for (int kb = 32 * wave; kb < n; kb += 128) {
        const int key = kb + l31;
        float part = 0.0f;
        if (key < n) {
            const float* kr = base + (size_t)key * p.ld;
            for (int dd = kh * half; dd < min(hd, (kh + 1) * half); ++dd) part = fmaf(Qs[dd], kr[dd], part);
        }
        const float other = __shfl_xor(part, 32, 64);
        const float sc = key < n ? (kh == 0 ? part + other : other + part) * p.scale : -INFINITY;   // lower half + upper half, on both lanes
        float mx = sc;
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const float m_new = fmaxf(m_run, mx);                        // finite: key kb < n
        const float alpha = expf(m_run - m_new), pr = key < n ? expf(sc - m_new) : 0.0f;
        float ps = pr;
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) ps += __shfl_xor(ps, o, 64);
        l_run = l_run * alpha + ps;
        m_run = m_new;
        a0 *= alpha; a1 *= alpha;
        const int nk = min(32, n - kb);
        for (int j = 0; j < nk; ++j) {                               // keys in order; the lane owns dimensions lane and lane + 64
            const float pj = __shfl(pr, j, 64);
            const float* vr = base + (size_t)(kb + j) * p.ld + p.voff;
            if (lane < hd) a0 = fmaf(pj, vr[lane], a0);
            if (lane + 64 < hd) a1 = fmaf(pj, vr[lane + 64], a1);
        }
    }
    if (lane == 0) { Ms[wave] = m_run; Ls[wave] = l_run; }
    As[wave][lane] = a0; As[wave][lane + 64] = a1;
    __syncthreads();
    if (tid < hd) {
        const float mt = fmaxf(fmaxf(Ms[0], Ms[1]), fmaxf(Ms[2], Ms[3]));    // wave 0 always holds key 0
        float l = 0.0f, a = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const float f = expf(Ms[w] - mt); l += Ls[w] * f; a += As[w][tid] * f; }
        p.out[(size_t)m * p.ldo + hh * hd + tid] = a / l;
    }
}

// k_cn_attn_step over a bf16 K | V store: the same split (a block a (row, head), 32-key tiles round-robin over four waves, online softmax per
// wave, the four (m, l, acc) merged through LDS in wave order) and the same f32 arithmetic on the widened values - no MFMA, nothing rounded.
// Score: the lane pair (key, half of the head) reads its half of the key row as 16-byte chunks of 8 bf16 and accumulates in ascending
// dimension against the f32 query in LDS.  P V: the lane owns dimensions 2 lane and 2 lane + 1, one 4-byte load a key.
__global__ void __launch_bounds__(256) k_cn_attn_step_bf16(CnAttn p) {
    __shared__ float Qs[128], Ms[4], Ls[4], As[4][128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int m = blockIdx.x, hh = blockIdx.y, hd = p.hd, cap = p.capd ? *p.capd : p.cap, n = max(1, min(p.cnt[m] + p.cnt_add, cap));
    const int HP = hd <= 64 ? 64 : 128, half = HP / 2;               // the head, zero-padded to 64 or 128
    const int d0 = kh * half, d1 = min(hd, (kh + 1) * half);
    const bool vec = ((hd | p.ld) & 7) == 0, pair = ((hd | p.ld | p.voff) & 1) == 0;
    if (tid < 128) Qs[tid] = tid < hd ? p.q[(size_t)m * p.ldq + hh * hd + tid] : 0.0f;
    __syncthreads();
    const bf16_t* base = p.kvb + (size_t)m * cap * p.ld + hh * hd;
    float m_run = -INFINITY, l_run = 0.0f, a0 = 0.0f, a1 = 0.0f;
    for (int kb = 32 * wave; kb < n; kb += 128) {
        const int key = kb + l31;
        float part = 0.0f;
        if (key < n) {
            const bf16_t* kr = base + (size_t)key * p.ld;
            for (int dd = d0; dd < d1; dd += 8) {                    // (columns >= d1 of the last chunk: zeros against Qs' zeros)
                const uint4 c = pkb_chunk(kr, dd, d1, vec);
                const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    part = fmaf(Qs[dd + 2 * e], __uint_as_float(w[e] << 16), part);
                    part = fmaf(Qs[dd + 2 * e + 1], __uint_as_float(w[e] & 0xffff0000u), part);
                }
            }
        }
        const float other = __shfl_xor(part, 32, 64);
        const float sc = key < n ? (kh == 0 ? part + other : other + part) * p.scale : -INFINITY;   // lower half + upper half, on both lanes
        float mx = sc;
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const float m_new = fmaxf(m_run, mx);                        // finite: key kb < n
        const float alpha = expf(m_run - m_new), pr = key < n ? expf(sc - m_new) : 0.0f;
        float ps = pr;
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) ps += __shfl_xor(ps, o, 64);
        l_run = l_run * alpha + ps;
        m_run = m_new;
        a0 *= alpha; a1 *= alpha;
        const int nk = min(32, n - kb);
        for (int j = 0; j < nk; ++j) {                               // keys in order
            const float pj = __shfl(pr, j, 64);
            const bf16_t* vr = base + (size_t)(kb + j) * p.ld + p.voff;
            if (pair) {
                if (2 * lane < hd) {
                    const uint32_t u = *reinterpret_cast<const uint32_t*>(vr + 2 * lane);
                    a0 = fmaf(pj, __uint_as_float(u << 16), a0);
                    a1 = fmaf(pj, __uint_as_float(u & 0xffff0000u), a1);
                }
            } else {
                if (2 * lane < hd) a0 = fmaf(pj, bf16_to_f32(vr[2 * lane]), a0);
                if (2 * lane + 1 < hd) a1 = fmaf(pj, bf16_to_f32(vr[2 * lane + 1]), a1);
            }
        }
    }
    if (lane == 0) { Ms[wave] = m_run; Ls[wave] = l_run; }
    As[wave][2 * lane] = a0; As[wave][2 * lane + 1] = a1;
    __syncthreads();
    if (tid < hd) {
        const float mt = fmaxf(fmaxf(Ms[0], Ms[1]), fmaxf(Ms[2], Ms[3]));    // wave 0 always holds key 0
        float l = 0.0f, a = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const float f = expf(Ms[w] - mt); l += Ls[w] * f; a += As[w][tid] * f; }
        p.out[(size_t)m * p.ldo + hh * hd + tid] = a / l;
    }
}

// the cross K | V of one layer between the f32 projection and the bf16 store (k_pk_round_bf16 rounds it in), and back for mis_canary_tap
__global__ void __launch_bounds__(256) k_cn_widen_bf16(const bf16_t* __restrict__ x, float* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = bf16_to_f32(x[i]);
}

// ============================================================================ token bookkeeping and the next input
struct CnSel {
    const float* amv; const int* ami; int nt;
    const int* prompt; int Pmax; const int* plen;
    int *pos, *ngen, *done, *done_count, *tokens;
    int eos, max_tokens, init, V, h;
    const float *embed, *postab, *ew, *eb, *lw, *lb;
    float *x, *xn;
};

__device__ __forceinline__ bool cn_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__global__ void __launch_bounds__(256) k_cn_select(CnSel p) {
    __shared__ float sh[4];
    __shared__ int dec[2];                                           // token, position (-1: the row writes nothing)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (tid < 64) {
        int token = 0, at = -1;
        if (p.init) {
            if (lane == 0) {
                p.pos[b] = 0; p.ngen[b] = 0; p.done[b] = 0;
                if (b == 0) *p.done_count = 0;
            }
            token = p.prompt[(size_t)b * p.Pmax]; at = 0;
        } else if (!p.done[b]) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int t = lane; t < p.nt; t += 64) {
                const float v = p.amv[(size_t)b * p.nt + t];
                const int i = p.ami[(size_t)b * p.nt + t];
                if (cn_better(v, i, bv, bi)) { bv = v; bi = i; }
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (cn_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            const int np = p.pos[b] + 1;
            bool ended = false;
            if (np < p.plen[b]) token = p.prompt[(size_t)b * p.Pmax + np];
            else {
                token = bi < p.V ? bi : 0;                           // (no finite logit at all: index 0)
                const int g = p.ngen[b];
                if (token == p.eos) ended = true;
                else if (lane == 0) { p.tokens[(size_t)b * p.max_tokens + g] = token; p.ngen[b] = g + 1; }
                if (!ended && g + 1 >= p.max_tokens) ended = true;
            }
            if (ended) { if (lane == 0) { p.done[b] = 1; atomicAdd(p.done_count, 1); } }
            else { at = np; if (lane == 0) p.pos[b] = np; }
        }
        if (lane == 0) { dec[0] = min(max(token, 0), p.V - 1); dec[1] = at; }
    }
    __syncthreads();
    const int token = dec[0], at = dec[1];
    if (at < 0) return;                                              // (uniform over the block)
    const float* e = p.embed + (size_t)token * p.h;
    const float* ps = p.postab + (size_t)min(at, CN_POS_ROWS - 1) * p.h;
    float v[CN_MAXH / 256], o[CN_MAXH / 256];
#pragma unroll
    for (int j = 0; j < CN_MAXH / 256; ++j) { const int cc = tid + 256 * j; v[j] = cc < p.h ? e[cc] + ps[cc] : 0.0f; }
    cn_layernorm(v, p.h, p.ew, p.eb, o, sh);
#pragma unroll
    for (int j = 0; j < CN_MAXH / 256; ++j) { const int cc = tid + 256 * j; if (cc < p.h) p.x[(size_t)b * p.h + cc] = o[j]; }
    cn_layernorm(o, p.h, p.lw, p.lb, v, sh);
#pragma unroll
    for (int j = 0; j < CN_MAXH / 256; ++j) { const int cc = tid + 256 * j; if (cc < p.h) p.xn[(size_t)b * p.h + cc] = v[j]; }
}

// ============================================================================ host
struct mis_canary : PkEncoder {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_canary_config cfg{};
    int hw = 0, Ld = 0, Hd = 0, hdd = 0, inner = 0, V = 0, NT = 0, cap = 0, S_h = 1;   // hw: the decoder width (enc_output_dim)
    HostWeights raw{"Canary", MIS_ERR_INVALID_INPUT};
    bool finalized = false, use_graph = true;
    SfLin proj, head;
    const float *embed = nullptr, *postab_dec = nullptr, *ew = nullptr, *eb = nullptr, *fw = nullptr, *fb_ = nullptr;
    struct DLayer {
        const float *n1w, *n1b, *n2w, *n2b, *n3w, *n3b;
        SfLin qkv, so, cq, ckv, co, ff1, ff2;
        bf16_t *qkv16, *so16, *cq16, *co16, *ff116, *ff216;          // dec_bf16: these six matrices live in the bf16 arena only (SfLin::w null)
    };
    std::vector<DLayer> dl;
    bool dec_bf16 = false;                                           // mis_canary_set_decoder_dtype(MIS_BF16)
    bf16_t* head16 = nullptr;
    DevBuf<bf16_t> ckv16, skv16;                                     // dec_bf16: the K | V stores, in place of ckv and skv
    DevBuf<float> ckvf;                                              // dec_bf16: one layer of cross K | V in f32, between the projection and the store
    DevBuf<float> encp, ckv, skv, x, xn, q, att, ff, part, amv, logits;
    DevBuf<int> ami, toks, st, prompt;                               // st: pos, ngen, done, plen [B] each, then done_count, Tp
    PinnedBuf<int> done_host;
    std::unique_ptr<StepGraph> graphs[PK_MAX_BATCH + 1];
    int g_eos[PK_MAX_BATCH + 1] = {}, g_max[PK_MAX_BATCH + 1] = {}, g_pmax[PK_MAX_BATCH + 1] = {};
    HipEvents<6> ev;
    bool timed = false, timed_done = false, has_kv = false;
    int steps_run = 0;
    int* pos() { return st.p; }
    int* ngen() { return st.p + cfg.max_batch; }
    int* done() { return st.p + 2 * cfg.max_batch; }
    int* plen() { return st.p + 3 * cfg.max_batch; }
    int* done_count() { return st.p + 4 * cfg.max_batch; }
    int* tp_dev() { return st.p + 4 * cfg.max_batch + 1; }
    const float* enc_out() const { return d == hw ? h.p : encp.p; }
    size_t ckv_layer() const { return (size_t)cfg.max_batch * Tcap * 2 * hw; }
    size_t skv_layer() const { return (size_t)cfg.max_batch * cap * 2 * hw; }
};

static void cn_check_decoder(const mis_canary_config* cfg) {
    const int h = cfg->enc_output_dim;
    MIS_REQUIRE(h >= 8 && h <= CN_MAXH, MIS_ERR_INVALID_INPUT, "enc_output_dim %d outside 8..%d", h, CN_MAXH);
    MIS_REQUIRE(cfg->dec_hidden_size == h, MIS_ERR_INVALID_INPUT,
                "decoder.hidden_size %d differs from enc_output_dim %d: the embedding, norms and head are built from one and the blocks from the other",
                cfg->dec_hidden_size, h);
    MIS_REQUIRE(cfg->dec_layers >= 1 && cfg->dec_layers <= 32, MIS_ERR_INVALID_INPUT, "decoder.num_layers %d outside 1..32", cfg->dec_layers);
    MIS_REQUIRE(cfg->dec_heads >= 1 && h % cfg->dec_heads == 0 && h / cfg->dec_heads <= 128, MIS_ERR_INVALID_INPUT,
                "decoder.num_attention_heads %d: head size hidden_size / num_attention_heads must be a whole number up to 128", cfg->dec_heads);
    MIS_REQUIRE(cfg->dec_inner_size >= 1 && cfg->dec_inner_size <= 16384, MIS_ERR_INVALID_INPUT, "decoder.inner_size %d outside 1..16384", cfg->dec_inner_size);
    MIS_REQUIRE(cfg->vocab_size >= 2 && cfg->vocab_size <= 65536, MIS_ERR_INVALID_INPUT, "vocab_size %d outside 2..65536", cfg->vocab_size);
    MIS_REQUIRE(cfg->max_tokens >= 1 && cfg->max_tokens <= 4096, MIS_ERR_INVALID_INPUT, "max_tokens %d outside 1..4096", cfg->max_tokens);
    MIS_REQUIRE(cfg->max_prompt >= 1 && cfg->max_prompt <= 256, MIS_ERR_INVALID_INPUT, "max_prompt %d outside 1..256", cfg->max_prompt);
}

extern "C" mis_status mis_canary_create(const mis_canary_config* cfg, int device, mis_canary** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    pk_encoder_check(cfg);
    cn_check_decoder(cfg);
    const int Tcap = pk_half(pk_half(pk_half(pk_frames((int64_t)cfg->max_seconds * 16000))));
    const int64_t store = (int64_t)cfg->max_batch * Tcap * cfg->dec_layers * 2 * cfg->enc_output_dim * 4;
    MIS_REQUIRE(store <= CN_MAX_STORE_BYTES, MIS_ERR_INVALID_INPUT,
                "the cross-attention K/V store of max_batch %d x %d frames (max_seconds %d) x %d layers needs %lld bytes, above the cap of %lld: lower max_seconds or max_batch",
                cfg->max_batch, Tcap, cfg->max_seconds, cfg->dec_layers, (long long)store, (long long)CN_MAX_STORE_BYTES);
    hipStream_t stream = mis_open_stream(device);      // first: the handle's events belong to this device
    auto c = std::make_unique<mis_canary>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    pk_encoder_dims(c.get());
    c->hw = cfg->enc_output_dim; c->Ld = cfg->dec_layers; c->Hd = cfg->dec_heads; c->hdd = c->hw / c->Hd; c->inner = cfg->dec_inner_size;
    c->V = cfg->vocab_size; c->NT = cdiv(c->V, 32); c->cap = cfg->max_prompt + cfg->max_tokens; c->S_h = cn_split_for(c->hw);
    c->use_graph = getenv("MIS_NO_GRAPH") == nullptr;
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_canary_destroy(mis_canary* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& g : c->graphs) g.reset();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" mis_status mis_canary_set_tensor(mis_canary* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 4, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

extern "C" mis_status mis_canary_set_encoder_dtype(mis_canary* c, mis_dtype dtype) {
    MIS_API_BEGIN
    pk_set_encoder_dtype(c, dtype);
    MIS_API_END
}

// f32 (the default) or bf16, before finalize, whatever the encoder's dtype; bf16 needs whole MFMA k-steps in both contraction lengths
extern "C" mis_status mis_canary_set_decoder_dtype(mis_canary* c, mis_dtype dtype) {
    MIS_API_BEGIN
    MIS_REQUIRE(c, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(!c->finalized, MIS_ERR_INVALID_INPUT, "set_decoder_dtype after finalize");
    MIS_REQUIRE(dtype == MIS_F32 || dtype == MIS_BF16, MIS_ERR_INVALID_INPUT, "decoder dtype %d: only MIS_F32 and MIS_BF16 are implemented", (int)dtype);
    if (dtype == MIS_BF16) {
        MIS_REQUIRE(c->cfg.enc_output_dim % 32 == 0, MIS_ERR_INVALID_INPUT, "enc_output_dim %d: the bf16 decoder needs a multiple of 32", c->cfg.enc_output_dim);
        MIS_REQUIRE(c->cfg.dec_inner_size % 32 == 0, MIS_ERR_INVALID_INPUT, "dec_inner_size %d: the bf16 decoder needs a multiple of 32", c->cfg.dec_inner_size);
    }
    c->dec_bf16 = dtype == MIS_BF16;
    MIS_API_END
}

static const char* const CN_ATT[4] = {"q_proj", "k_proj", "v_proj", "out_proj"};

extern "C" mis_status mis_canary_finalize(mis_canary* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t d = c->d, h = c->hw, inner = c->inner, V = c->V;
    HostArena a(c->raw);
    pk_encoder_weights(c, a);
    std::vector<float>& fh = a.fhost;
    auto lin = [&](const std::string& p, int64_t N, int64_t K, SfLin& l) { a.fvec(p + ".weight", {N, K}, N * K, l.w); a.fvec(p + ".bias", {N}, N, l.b); };
    const bool b16 = c->dec_bf16;
    // a matrix of the step: the f32 arena, or rounded once into the bf16 arena (and then there only); the bias is f32 in both modes
    auto slin = [&](const std::string& p, int64_t N, int64_t K, SfLin& l, bf16_t*& wb) {
        if (!b16) { lin(p, N, K, l); return; }
        a.bmat(p + ".weight", N, K, wb);
        a.fvec(p + ".bias", {N}, N, l.b);
    };
    auto norm = [&](const std::string& p, const float*& w, const float*& b) { a.fvec(p + ".weight", {h}, h, w); a.fvec(p + ".bias", {h}, h, b); };
    // several projections over the same input as one [n h][h], bias [n h]
    auto stacked = [&](const std::string& p, int first, int n, SfLin& l, bf16_t** wb) {      // wb null: f32 in both modes
        const bool to16 = b16 && wb;
        const size_t ow = to16 ? a.btake((size_t)n * h * h, *wb) : a.ftake((size_t)n * h * h, l.w), ob = a.ftake(n * h, l.b);
        for (int i = 0; i < n; ++i) {
            const HostTensor& w = c->raw.need(p + CN_ATT[first + i] + ".weight", {h, h});
            const HostTensor& bb = c->raw.need(p + CN_ATT[first + i] + ".bias", {h});
            if (to16) for (int64_t j = 0; j < h * h; ++j) a.host[ow + (size_t)i * h * h + j] = f32_to_bf16(w.v[j]);
            else std::copy(w.v.begin(), w.v.end(), fh.begin() + ow + (size_t)i * h * h);
            std::copy(bb.v.begin(), bb.v.end(), fh.begin() + ob + (size_t)i * h);
        }
    };
    if (d != h) lin("encoder.projection", h, d, c->proj);
    a.fvec("decoder.embedding.weight", {V, h}, V * h, c->embed);
    norm("decoder.embedding_layer_norm", c->ew, c->eb);
    c->dl.assign(c->Ld, mis_canary::DLayer{});
    for (int li = 0; li < c->Ld; ++li) {
        const std::string q = "decoder.blocks." + std::to_string(li) + ".";
        mis_canary::DLayer& l = c->dl[li];
        norm(q + "self_attn_norm", l.n1w, l.n1b);
        stacked(q + "self_attn.", 0, 3, l.qkv, &l.qkv16);
        slin(q + "self_attn.out_proj", h, h, l.so, l.so16);
        norm(q + "cross_attn_norm", l.n2w, l.n2b);
        stacked(q + "cross_attn.", 0, 1, l.cq, &l.cq16);
        stacked(q + "cross_attn.", 1, 2, l.ckv, nullptr);              // projected once a call by the f32 GEMM in both modes: stays f32
        slin(q + "cross_attn.out_proj", h, h, l.co, l.co16);
        norm(q + "ff_norm", l.n3w, l.n3b);
        slin(q + "ff1", inner, h, l.ff1, l.ff116); slin(q + "ff2", h, inner, l.ff2, l.ff216);
    }
    norm("decoder.final_norm", c->fw, c->fb_);
    slin("decoder.output_proj", V, h, c->head, c->head16);
    {   // the fixed sinusoid: sin | cos interleaved, frequency 10000^(-c / h) with c the even column, all over sqrt(h); formed in double, rounded once
        const size_t o = a.ftake((size_t)CN_POS_ROWS * h, c->postab_dec);
        const double rs = 1.0 / sqrt((double)h);
        for (int r = 0; r < CN_POS_ROWS; ++r)
            for (int64_t ch = 0; ch < h; ch += 2) {
                const double ang = (double)r * exp(-log(10000.0) * (double)ch / (double)h);
                fh[o + (size_t)r * h + ch] = (float)(sin(ang) * rs);
                if (ch + 1 < h) fh[o + (size_t)r * h + ch + 1] = (float)(cos(ang) * rs);
            }
    }
    a.upload(c->warena, c->farena);
    pk_encoder_workspace(c);
    const size_t B = c->cfg.max_batch, M = B * c->Tcap;
    if (d != h) c->encp.alloc(M * h);
    if (b16) { c->ckv16.alloc(c->ckv_layer() * c->Ld); c->skv16.alloc(c->skv_layer() * c->Ld); c->ckvf.alloc(c->ckv_layer()); }
    else { c->ckv.alloc(c->ckv_layer() * c->Ld); c->skv.alloc(c->skv_layer() * c->Ld); }
    c->x.alloc(B * h); c->xn.alloc(B * h); c->q.alloc(B * h); c->att.alloc(B * h); c->ff.alloc(B * inner); c->part.alloc((size_t)8 * B * h);
    c->amv.alloc(B * c->NT); c->ami.alloc(B * c->NT); c->logits.alloc(B * V);
    c->st.alloc(4 * B + 2); c->prompt.alloc(B * c->cfg.max_prompt); c->toks.alloc(B * c->cfg.max_tokens);
    c->done_host.alloc(1);
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of the engine
extern "C" mis_status mis_canary_init_synthetic(mis_canary* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    const int64_t d = c->d, h = c->hw, inner = c->inner, V = c->V;
    pk_encoder_synthetic(c, sw);
    if (d != h) sw.lin("encoder.projection", h, d, true, 1.0);
    sw.put("decoder.embedding.weight", {V, h}, 1.0, 0.0f);
    sw.norm("decoder.embedding_layer_norm", h);
    for (int li = 0; li < c->Ld; ++li) {
        const std::string q = "decoder.blocks." + std::to_string(li) + ".";
        for (const char* n : {"self_attn_norm", "cross_attn_norm", "ff_norm"}) sw.norm(q + n, h);
        for (const char* at : {"self_attn.", "cross_attn."})
            for (int i = 0; i < 4; ++i) sw.lin(q + at + CN_ATT[i], h, h, true, i == 3 ? 0.5 : 1.0);
        sw.lin(q + "ff1", inner, h, true, 1.0); sw.lin(q + "ff2", h, inner, true, 0.5);
    }
    sw.norm("decoder.final_norm", h);
    sw.lin("decoder.output_proj", V, h, true, 4.0);
    MIS_API_END
}

// ============================================================================ the chain
// (the bf16 decoder: the cross K/V form built is the f32 sf_gemm projection + k_pk_round_bf16 a layer, L_dec launches more in generate)
extern "C" int mis_canary_launches(const mis_canary* c) { return c ? c->launches : 0; }

extern "C" mis_status mis_canary_frames(const mis_canary* c, const int64_t* lens, int batch, int32_t* F_out, int32_t* T_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && lens && batch >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    const int64_t cap = (int64_t)c->cfg.max_seconds * 16000;
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(lens[b] >= 0 && lens[b] <= cap, MIS_ERR_INVALID_INPUT, "row %d: %lld samples outside 0..%lld (max_seconds %d)", b, (long long)lens[b],
                    (long long)cap, c->cfg.max_seconds);
        const int F = pk_frames(lens[b]);
        if (F_out) F_out[b] = F;
        if (T_out) T_out[b] = pk_half(pk_half(pk_half(F)));
    }
    MIS_API_END
}

static void cn_sync(mis_canary* c) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// the encoder's output of the batch in c->enc_out() (1 launch with a projection)
static void cn_project(mis_canary* c) {
    if (c->d != c->hw) sf_gemm(c, sf_lin(c->h.p, c->d, c->proj, c->encp.p, c->hw, c->cnt3.p, c->Tp), c->batch);
}

// K | V of every decoder layer over all B Tp frames: L_dec launches of width 2 h, rows [b Tp + t]
// dec_bf16: each layer through the one-layer f32 buffer, rounded into the bf16 store (2 L_dec launches)
static void cn_cross_kv(mis_canary* c) {
    const size_t n = (size_t)c->batch * c->Tp * 2 * c->hw;
    for (int li = 0; li < c->Ld; ++li) {
        float* dst = c->dec_bf16 ? c->ckvf.p : c->ckv.p + li * c->ckv_layer();
        sf_gemm(c, sf_lin(c->enc_out(), c->hw, c->dl[li].ckv, dst, 2 * c->hw, c->cnt3.p, c->Tp), c->batch);
        if (c->dec_bf16) MIS_LAUNCH(c, k_pk_round_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), dst, c->ckv16.p + li * c->ckv_layer(), n);
    }
    HIP_CHECK(hipMemcpyAsync(c->tp_dev(), &c->Tp, 4, hipMemcpyHostToDevice, c->stream));
    c->has_kv = true;
}

// wb: the matrix in the bf16 arena (the bf16 decoder; l.w is null then), which selects k_cn_lin_bf16 in cn_lin
static CnLin cn_lin_args(const float* X, int K, const SfLin& l, int M, int N, const bf16_t* wb = nullptr) {
    CnLin p{};
    p.X = X; p.ldx = K; p.W = l.w; p.Wb = wb; p.bias = l.b; p.M = M; p.K = K; p.N = N;
    return p;
}

// one layer of the step: qkv . attn . out . rows . q . attn . out . rows . ff1 . ff2 . rows (11 launches); next: the LayerNorm behind it
static void cn_layer(mis_canary* c, int li, int B, const float* nextw, const float* nextb) {
    const mis_canary::DLayer& l = c->dl[li];
    const int h = c->hw, S = c->S_h;
    const float scale = 1.0f / sqrtf((float)c->hdd);
    const bool b16 = c->dec_bf16;
    auto split = [&](const float* X, int K, const SfLin& w, const bf16_t* wb) {
        CnLin p = cn_lin_args(X, K, w, B, h, wb);
        p.bias = nullptr; p.part = c->part.p;
        cn_lin(c, p, S);
    };
    auto rows = [&](const SfLin& w, const float* lw, const float* lb) {
        CnRows r{c->x.p, c->xn.p, w.b, c->part.p, S, B, h, lw, lb};
        MIS_LAUNCH(c, k_cn_rows, dim3(B), dim3(256), r);
    };
    auto attn = [&](const CnAttn& a) {
        if (b16) MIS_LAUNCH(c, k_cn_attn_step_bf16, dim3(B, c->Hd), dim3(256), a);
        else MIS_LAUNCH(c, k_cn_attn_step, dim3(B, c->Hd), dim3(256), a);
    };
    float* skv = b16 ? nullptr : c->skv.p + li * c->skv_layer();
    bf16_t* skv16 = b16 ? c->skv16.p + li * c->skv_layer() : nullptr;
    {
        CnLin p = cn_lin_args(c->xn.p, h, l.qkv, B, 3 * h, l.qkv16);
        p.Y = c->q.p; p.ldy = h; p.kv = skv; p.kvb = skv16; p.pos = c->pos(); p.cap = c->cap; p.kvoff = h;
        cn_lin(c, p, 1);
    }
    attn(CnAttn{c->q.p, h, skv, 2 * h, h, c->cap, nullptr, c->pos(), 1, c->att.p, h, c->hdd, scale, skv16});
    split(c->att.p, h, l.so, l.so16);
    rows(l.so, l.n2w, l.n2b);
    {
        CnLin p = cn_lin_args(c->xn.p, h, l.cq, B, h, l.cq16);
        p.Y = c->q.p; p.ldy = h;
        cn_lin(c, p, 1);
    }
    attn(CnAttn{c->q.p, h, b16 ? nullptr : c->ckv.p + li * c->ckv_layer(), 2 * h, h, 0, c->tp_dev(), c->cnt3.p, 0, c->att.p, h, c->hdd, scale,
                b16 ? c->ckv16.p + li * c->ckv_layer() : nullptr});
    split(c->att.p, h, l.co, l.co16);
    rows(l.co, l.n3w, l.n3b);
    {
        CnLin p = cn_lin_args(c->xn.p, h, l.ff1, B, c->inner, l.ff116);
        p.Y = c->ff.p; p.ldy = c->inner; p.relu = 1;
        cn_lin(c, p, 1);
    }
    split(c->ff.p, c->inner, l.ff2, l.ff216);
    rows(l.ff2, nextw, nextb);
}

static void cn_layers(mis_canary* c, int B) {
    for (int li = 0; li < c->Ld; ++li) {
        const bool last = li + 1 == c->Ld;
        cn_layer(c, li, B, last ? c->fw : c->dl[li + 1].n1w, last ? c->fb_ : c->dl[li + 1].n1b);
    }
}

static void cn_head(mis_canary* c, int B, float* logits) {
    CnLin p = cn_lin_args(c->xn.p, c->hw, c->head, B, c->V, c->head16);
    p.Y = logits; p.ldy = c->V; p.amv = c->amv.p; p.ami = c->ami.p; p.nt = c->NT;
    cn_lin(c, p, 1);
}

static void cn_select(mis_canary* c, int B, int Pmax, int eos, int max_tokens, int init, int* tokens) {
    CnSel s{c->amv.p, c->ami.p, c->NT, c->prompt.p, Pmax, c->plen(), c->pos(), c->ngen(), c->done(), c->done_count(), tokens, eos, max_tokens, init, c->V,
            c->hw, c->embed, c->postab_dec, c->ew, c->eb, c->dl[0].n1w, c->dl[0].n1b, c->x.p, c->xn.p};
    MIS_LAUNCH(c, k_cn_select, dim3(B), dim3(256), s);
}

// judged, then uploaded: prompt ids [B][Pmax] and plen [B]
static void cn_take_prompt(mis_canary* c, const int32_t* prompt, const int32_t* plen, int B, int Pmax) {
    MIS_REQUIRE(Pmax >= 1 && Pmax <= c->cfg.max_prompt, MIS_ERR_INVALID_INPUT, "prompt width %d outside 1..%d (max_prompt)", Pmax, c->cfg.max_prompt);
    for (int b = 0; b < B; ++b) {
        MIS_REQUIRE(plen[b] >= 1 && plen[b] <= Pmax, MIS_ERR_INVALID_INPUT, "row %d: prompt length %d outside 1..%d", b, plen[b], Pmax);
        for (int i = 0; i < plen[b]; ++i)
            MIS_REQUIRE(prompt[(size_t)b * Pmax + i] >= 0 && prompt[(size_t)b * Pmax + i] < c->V, MIS_ERR_INVALID_INPUT, "row %d: prompt token %d outside the vocabulary",
                        b, prompt[(size_t)b * Pmax + i]);
    }
}

extern "C" mis_status mis_canary_encode(mis_canary* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    c->has_kv = false;
    pk_front_stem(c, pcm, lens, batch, stride);
    pk_encoder(c, -1);
    cn_project(c);
    const int kept = c->launches;
    cn_cross_kv(c);                                                  // (kept for mis_canary_forward; not counted as encode's)
    c->launches = kept;
    HIP_CHECK(hipMemcpyAsync(out, c->enc_out(), (size_t)batch * c->Tp * c->hw * 4, hipMemcpyDeviceToHost, c->stream));
    cn_sync(c);
    MIS_API_END
}

extern "C" mis_status mis_canary_generate(mis_canary* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, const int32_t* prompt,
                                          const int32_t* plen, int Pmax, int eos, int max_tokens, int32_t* tokens, int32_t* counts, int32_t* flags,
                                          int32_t* steps) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && prompt && plen && tokens && counts && flags, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch %d outside 1..%d (max_batch)", batch, c->cfg.max_batch);
    MIS_REQUIRE(max_tokens >= 1 && max_tokens <= c->cfg.max_tokens, MIS_ERR_INVALID_INPUT, "max_tokens %d outside 1..%d", max_tokens, c->cfg.max_tokens);
    cn_take_prompt(c, prompt, plen, batch, Pmax);
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->has_kv = false;
    pk_front_stem(c, pcm, lens, batch, stride);
    pk_encoder(c, -1);
    cn_project(c);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[2], s));
    cn_cross_kv(c);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[3], s));
    const int B = batch;
    int maxp = 0;
    for (int b = 0; b < B; ++b) maxp = std::max(maxp, plen[b]);
    HIP_CHECK(hipMemcpyAsync(c->prompt.p, prompt, (size_t)B * Pmax * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->plen(), plen, B * 4, hipMemcpyHostToDevice, s));
    int* dtok = c->toks.p;                                           // [B][max_tokens]
    cn_select(c, B, Pmax, eos, max_tokens, 1, dtok);
    const int per_step = 11 * c->Ld + 2;
    auto step = [&]() { cn_layers(c, B); cn_head(c, B, nullptr); cn_select(c, B, Pmax, eos, max_tokens, 0, dtok); };
    if (c->use_graph) {
        std::unique_ptr<StepGraph>& g = c->graphs[B];
        if (!g || c->g_eos[B] != eos || c->g_max[B] != max_tokens || c->g_pmax[B] != Pmax) {
            const int kept = c->launches;
            g = std::make_unique<StepGraph>();
            g->capture(s, step);
            c->launches = kept;
            c->g_eos[B] = eos; c->g_max[B] = max_tokens; c->g_pmax[B] = Pmax;
            MIS_REQUIRE(g->nodes() == per_step, MIS_ERR_GENERATION_FAILED, "the captured step holds %d nodes where %d were meant", g->nodes(), per_step);
        }
    }
    int nsteps = 0;
    run_frame_loop(maxp + max_tokens, B, nullptr, nullptr,
        [&]() { if (c->use_graph) { c->graphs[B]->launch(s); c->launches += per_step; } else step(); ++nsteps; },
        [&]() { HIP_CHECK(hipMemcpyAsync(c->done_host.p, c->done_count(), 4, hipMemcpyDeviceToHost, s)); },
        [&]() { cn_sync(c); return c->done_host.p[0]; },
        [&]() { HIP_CHECK(hipGetLastError()); },
        [&]() { return 0; });
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[4], s));
    c->steps_run = nsteps;
    std::vector<int32_t> hn(B), hd(B);
    HIP_CHECK(hipMemcpyAsync(hn.data(), c->ngen(), B * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(hd.data(), c->done(), B * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(tokens, dtok, (size_t)B * max_tokens * 4, hipMemcpyDeviceToHost, s));
    cn_sync(c);
    for (int b = 0; b < B; ++b) { counts[b] = hn[b]; flags[b] = hd[b] ? 0 : 1; }       // flag: the row never ended (cannot happen inside the step bound)
    if (steps) *steps = nsteps;
    c->timed_done = c->timed;
    MIS_API_END
}

// The decoder teacher-forced over per-row prompts against the cross K/V of the last encode / generate: for every row the logits [B][V] behind
// its LAST prompt token (the first decoded step) and the hidden state [B][h] in front of final_norm at that step.  Plain launches.
extern "C" mis_status mis_canary_forward(mis_canary* c, const int32_t* prompt, const int32_t* plen, int Pmax, float* logits, float* hidden) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && prompt && plen && logits, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized && c->batch > 0 && c->has_kv, MIS_ERR_NOT_INITIALIZED, "no cross K/V: the last call must be encode or generate");
    const int B = c->batch;
    cn_take_prompt(c, prompt, plen, B, Pmax);
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int kept = c->launches;
    int maxp = 0;
    for (int b = 0; b < B; ++b) maxp = std::max(maxp, plen[b]);
    HIP_CHECK(hipMemcpyAsync(c->prompt.p, prompt, (size_t)B * Pmax * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->plen(), plen, B * 4, hipMemcpyHostToDevice, s));
    cn_select(c, B, Pmax, -1, c->cfg.max_tokens, 1, c->toks.p);
    for (int t = 0; t < maxp; ++t) {
        cn_layers(c, B);
        cn_head(c, B, c->logits.p);
        for (int b = 0; b < B; ++b)
            if (plen[b] - 1 == t) {
                HIP_CHECK(hipMemcpyAsync(logits + (size_t)b * c->V, c->logits.p + (size_t)b * c->V, (size_t)c->V * 4, hipMemcpyDeviceToHost, s));
                if (hidden) HIP_CHECK(hipMemcpyAsync(hidden + (size_t)b * c->hw, c->x.p + (size_t)b * c->hw, (size_t)c->hw * 4, hipMemcpyDeviceToHost, s));
            }
        if (t + 1 < maxp) cn_select(c, B, Pmax, -1, c->cfg.max_tokens, 0, c->toks.p);
    }
    cn_sync(c);
    c->launches = kept;
    MIS_API_END
}

// tensors of the last encode / generate, f32, zero rows behind T_b: stage 0 the stem's embeddings [B, T, hidden_size], 1..L_enc that Conformer
// block, L_enc + 1 the encoder's output behind the projection [B, T, h], L_enc + 2 + l the cross K | V of decoder layer l [B, T, 2 h].
extern "C" mis_status mis_canary_tap(mis_canary* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && dims, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized && c->batch > 0 && c->has_emb && c->has_kv, MIS_ERR_NOT_INITIALIZED, "no call to tap: the last call must be encode or generate");
    const int last = c->L + 1 + c->Ld;
    MIS_REQUIRE(stage >= 0 && stage <= last, MIS_ERR_INVALID_INPUT, "stage %d outside 0..%d", stage, last);
    HIP_CHECK(hipSetDevice(c->device));
    const int width = stage <= c->L ? c->d : stage == c->L + 1 ? c->hw : 2 * c->hw;
    dims[0] = c->batch; dims[1] = c->Tp; dims[2] = width;
    if (!out) return MIS_OK;
    const size_t n = (size_t)c->batch * c->Tp * width;
    MIS_REQUIRE((int64_t)n <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    const int kept = c->launches;
    if (stage >= 1) pk_encoder(c, stage > c->L ? -1 : stage);        // the chain is deterministic: recomputed from the embeddings
    if (stage == c->L + 1) cn_project(c);
    if (stage > c->L + 1 && c->dec_bf16)                             // the bf16 store, widened
        MIS_LAUNCH(c, k_cn_widen_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), c->ckv16.p + (stage - c->L - 2) * c->ckv_layer(), c->ckvf.p, n);
    c->launches = kept;
    const float* src = stage == 0 ? c->emb.p : stage <= c->L ? c->h.p : stage == c->L + 1 ? c->enc_out()
                     : c->dec_bf16 ? c->ckvf.p : c->ckv.p + (stage - c->L - 2) * c->ckv_layer();
    HIP_CHECK(hipMemcpyAsync(out, src, n * 4, hipMemcpyDeviceToHost, c->stream));
    cn_sync(c);
    MIS_API_END
}

// ============================================================================ test and bench scaffolding (include/mi_speech_debug.h)
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

// benches: device milliseconds of the next / last mis_canary_generate: front end, encoder (+ projection), cross K/V, the decode steps
extern "C" mis_status mis_debug_canary_timing(mis_canary* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c, MIS_ERR_INVALID_INPUT, "null argument");
    if (!ms) { c->timed = true; return MIS_OK; }
    MIS_REQUIRE(c->timed && c->timed_done, MIS_ERR_NOT_INITIALIZED, "no timed generate: the last call must be mis_canary_generate");
    for (int i = 0; i < 4; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
    MIS_API_END
}

namespace {
struct CndCtx { hipStream_t stream = nullptr; int launches = 0; };
constexpr int64_t CND_MAX_ELEMS = (int64_t)1 << 28;
void cnd_sync(const CndCtx& c, int want) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    MIS_REQUIRE(c.launches == want, MIS_ERR_GENERATION_FAILED, "%d launches where %d were meant", c.launches, want);
}
const float* cnd_fp(const DevBuf<uint32_t>& d) { return reinterpret_cast<const float*>(d.p); }
}  // namespace

// k_cn_lin on caller-supplied host data with S forced by the caller (1, 2, 4 or 8): X [Mrows][K] of which the first M rows are live (the rest
// may hold anything), W [N][K], bias [N] or NULL, relu.  S = 1: ONE launch, out [M][N] written directly.  S > 1: the partial launch and one
// k_cn_rows (x = 0, bias) - out is the reduced sum + bias, relu refused.  Every input is followed by NaNs; the output is guarded.
extern "C" mis_status mis_debug_canary_lin(int device, const float* X, int Mrows, int M, int K, int N, const float* W, const float* bias, int relu, int S,
                                           float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(X && W && out && M >= 1 && M <= 64 && Mrows >= M && K >= 1 && N >= 1, MIS_ERR_INVALID_INPUT, "Canary lin: pointers, 1..64 live rows, positive K and N");
    MIS_REQUIRE(S == 1 || S == 2 || S == 4 || S == 8, MIS_ERR_INVALID_INPUT, "Canary lin: S must be 1, 2, 4 or 8");
    MIS_REQUIRE(S == 1 || (!relu && N <= CN_MAXH), MIS_ERR_INVALID_INPUT, "Canary lin: a split contraction has no ReLU and at most %d columns", CN_MAXH);
    MIS_REQUIRE((int64_t)Mrows * K <= CND_MAX_ELEMS && (int64_t)N * K <= CND_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Canary lin: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    CndCtx c;
    DevBuf<uint32_t> dx, dw, db;
    alloc32(dx, X, (size_t)Mrows * K, F32_NAN);
    alloc32(dw, W, (size_t)N * K, F32_NAN);
    std::vector<float> zero(N, 0.0f);
    alloc32(db, bias ? bias : zero.data(), N, F32_NAN);
    GuardedOut o;
    o.alloc((size_t)M * N * 4, (size_t)64 * N * 4);
    float* y = reinterpret_cast<float*>(o.p());
    SfLin l{cnd_fp(dw), cnd_fp(db)};
    CnLin p = cn_lin_args(cnd_fp(dx), K, l, M, N);
    p.relu = relu;
    DevBuf<float> part, xn, lw;
    if (S == 1) {
        p.Y = y; p.ldy = N;
        cn_lin(&c, p, 1);
    } else {
        part.alloc((size_t)S * M * N); xn.alloc((size_t)M * N); lw.alloc(N);
        HIP_CHECK(hipMemset(y, 0, (size_t)M * N * 4));
        HIP_CHECK(hipMemset(lw.p, 0, (size_t)N * 4));
        p.bias = nullptr; p.part = part.p;
        cn_lin(&c, p, S);
        CnRows r{y, xn.p, cnd_fp(db), part.p, S, M, N, lw.p, lw.p};
        MIS_LAUNCH(&c, k_cn_rows, dim3(M), dim3(256), r);
    }
    cnd_sync(c, S == 1 ? 1 : 2);
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, y, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// ONE launch of k_cn_attn_step: q [B][heads hd], kv [B][cap][2 heads hd] (K | V), cnt [B] keys a row (1..cap) -> out [B][heads hd].  The
// store is NaN behind each row's count if the caller made it so; every input is followed by NaNs, the output is guarded.
extern "C" mis_status mis_debug_canary_attn_step(int device, const float* q, const float* kv, const int32_t* cnt, int batch, int cap, int heads, int hd, float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(q && kv && cnt && out && batch >= 1 && batch <= 65535 && cap >= 1 && heads >= 1 && heads <= 65535 && hd >= 1 && hd <= 128, MIS_ERR_INVALID_INPUT,
                "Canary attention step: pointers, positive batch, cap, heads and a head size up to 128");
    const int64_t h = (int64_t)heads * hd;
    MIS_REQUIRE((int64_t)batch * cap * 2 * h <= CND_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Canary attention step: tensor too large");
    for (int b = 0; b < batch; ++b) MIS_REQUIRE(cnt[b] >= 1 && cnt[b] <= cap, MIS_ERR_INVALID_INPUT, "Canary attention step: row %d has %d keys outside 1..%d", b, cnt[b], cap);
    HIP_CHECK(hipSetDevice(device));
    CndCtx c;
    DevBuf<uint32_t> dq, dkv, dc;
    alloc32(dq, q, (size_t)batch * h, F32_NAN);
    alloc32(dkv, kv, (size_t)batch * cap * 2 * h, F32_NAN);
    alloc32(dc, cnt, batch, 0x7FFFFFFFu);
    GuardedOut o;
    o.alloc((size_t)batch * h * 4, (size_t)64 * h * 4);
    CnAttn a{cnd_fp(dq), (int)h, cnd_fp(dkv), (int)(2 * h), (int)h, cap, nullptr, reinterpret_cast<const int*>(dc.p), 0, reinterpret_cast<float*>(o.p()), (int)h, hd,
             1.0f / sqrtf((float)hd)};
    MIS_LAUNCH(&c, k_cn_attn_step, dim3(batch, heads), dim3(256), a);
    cnd_sync(c, 1);
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), (size_t)batch * h * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// The head as the step runs it, then the pairs combined as k_cn_select does: xn [M][K], W [V][K], bias [V] -> logits [M][V] (may be NULL: then
// no logit reaches memory), index [M], value [M].  ONE launch (k_cn_lin, S = 1, pairs); the pairs are combined here by k_cn_select's rule.
extern "C" mis_status mis_debug_canary_head_argmax(int device, const float* xn, int M, int K, int V, const float* W, const float* bias, float* logits,
                                                   int32_t* index, float* value) {
    MIS_API_BEGIN
    MIS_REQUIRE(xn && W && bias && index && M >= 1 && M <= 64 && K >= 1 && V >= 2 && V <= 65536, MIS_ERR_INVALID_INPUT, "Canary head: pointers, 1..64 rows, a vocabulary of 2..65536");
    HIP_CHECK(hipSetDevice(device));
    CndCtx c;
    const int nt = cdiv(V, 32);
    DevBuf<uint32_t> dx, dw, db;
    alloc32(dx, xn, (size_t)M * K, F32_NAN);
    alloc32(dw, W, (size_t)V * K, F32_NAN);
    alloc32(db, bias, V, F32_NAN);
    GuardedOut o, pairs;
    o.alloc((size_t)M * V * 4, (size_t)64 * V * 4);
    pairs.alloc((size_t)2 * M * nt * 4, 4096);
    SfLin l{cnd_fp(dw), cnd_fp(db)};
    CnLin p = cn_lin_args(cnd_fp(dx), K, l, M, V);
    p.Y = logits ? reinterpret_cast<float*>(o.p()) : nullptr; p.ldy = V;
    p.amv = reinterpret_cast<float*>(pairs.p()); p.ami = reinterpret_cast<int*>(pairs.p()) + (size_t)M * nt; p.nt = nt;
    cn_lin(&c, p, 1);
    cnd_sync(c, 1);
    o.check_guards(); pairs.check_guards();
    std::vector<float> hv((size_t)M * nt);
    std::vector<int> hi((size_t)M * nt);
    HIP_CHECK(hipMemcpy(hv.data(), p.amv, hv.size() * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hi.data(), p.ami, hi.size() * 4, hipMemcpyDeviceToHost));
    for (int m = 0; m < M; ++m) {                                    // k_cn_select's rule: tile order, ties to the lower index
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int t = 0; t < nt; ++t) if (hv[(size_t)m * nt + t] > bv || (hv[(size_t)m * nt + t] == bv && hi[(size_t)m * nt + t] < bi)) { bv = hv[(size_t)m * nt + t]; bi = hi[(size_t)m * nt + t]; }
        index[m] = bi;
        if (value) value[m] = bv;
    }
    if (logits) HIP_CHECK(hipMemcpy(logits, o.p(), (size_t)M * V * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// k_cn_lin_bf16 on caller-supplied host data, as mis_debug_canary_lin: X f32 [Mrows][K] (M live rows), W bf16 bits [N][K], K % 32 == 0, bias
// [N] or NULL, S forced by the caller.  index NULL: S = 1 is ONE launch into out [M][N]; S > 1 the partial launch and one k_cn_rows (x = 0,
// bias; relu refused).  index [M] given: the launch as the head runs it (S = 1, pairs; out may be NULL: then no logit reaches memory), the
// pairs combined here by k_cn_select's rule.  Every input is followed by NaNs; every output is guarded.
extern "C" mis_status mis_debug_canary_lin_bf16(int device, const float* X, int Mrows, int M, int K, int N, const uint16_t* W, const float* bias, int relu, int S,
                                                float* out, int32_t* index) {
    MIS_API_BEGIN
    MIS_REQUIRE(X && W && (out || index) && M >= 1 && M <= 64 && Mrows >= M && K >= 32 && K % 32 == 0 && N >= 1, MIS_ERR_INVALID_INPUT,
                "Canary bf16 lin: pointers, 1..64 live rows, K a positive multiple of 32, positive N");
    MIS_REQUIRE(S == 1 || S == 2 || S == 4 || S == 8, MIS_ERR_INVALID_INPUT, "Canary bf16 lin: S must be 1, 2, 4 or 8");
    MIS_REQUIRE(S == 1 || (!relu && !index && N <= CN_MAXH), MIS_ERR_INVALID_INPUT, "Canary bf16 lin: a split contraction has no ReLU, no pairs and at most %d columns", CN_MAXH);
    MIS_REQUIRE((int64_t)Mrows * K <= CND_MAX_ELEMS && (int64_t)N * K <= CND_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Canary bf16 lin: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    CndCtx c;
    const int nt = cdiv(N, 32);
    DevBuf<uint32_t> dx, db;
    DevBuf<uint16_t> dw;
    alloc32(dx, X, (size_t)Mrows * K, F32_NAN);
    alloc16(dw, W, (size_t)N * K, BF16_NAN);
    std::vector<float> zero(N, 0.0f);
    alloc32(db, bias ? bias : zero.data(), N, F32_NAN);
    GuardedOut o, pairs;
    o.alloc((size_t)M * N * 4, (size_t)64 * N * 4);
    pairs.alloc((size_t)2 * M * nt * 4, 4096);
    float* y = reinterpret_cast<float*>(o.p());
    SfLin l{nullptr, cnd_fp(db)};
    CnLin p = cn_lin_args(cnd_fp(dx), K, l, M, N, dw.p);
    p.relu = relu;
    DevBuf<float> part, xn, lw;
    if (S == 1) {
        p.Y = out ? y : nullptr; p.ldy = N;
        if (index) { p.amv = reinterpret_cast<float*>(pairs.p()); p.ami = reinterpret_cast<int*>(pairs.p()) + (size_t)M * nt; p.nt = nt; }
        cn_lin(&c, p, 1);
    } else {
        part.alloc((size_t)S * M * N); xn.alloc((size_t)M * N); lw.alloc(N);
        HIP_CHECK(hipMemset(y, 0, (size_t)M * N * 4));
        HIP_CHECK(hipMemset(lw.p, 0, (size_t)N * 4));
        p.bias = nullptr; p.part = part.p;
        cn_lin(&c, p, S);
        CnRows r{y, xn.p, cnd_fp(db), part.p, S, M, N, lw.p, lw.p};
        MIS_LAUNCH(&c, k_cn_rows, dim3(M), dim3(256), r);
    }
    cnd_sync(c, S == 1 ? 1 : 2);
    o.check_guards(); pairs.check_guards();
    if (index) {
        std::vector<float> hv((size_t)M * nt);
        std::vector<int> hi((size_t)M * nt);
        HIP_CHECK(hipMemcpy(hv.data(), p.amv, hv.size() * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(hi.data(), p.ami, hi.size() * 4, hipMemcpyDeviceToHost));
        for (int m = 0; m < M; ++m) {                                // k_cn_select's rule: tile order, ties to the lower index
            float bv = -INFINITY; int bi = 0x7fffffff;
            for (int t = 0; t < nt; ++t) if (hv[(size_t)m * nt + t] > bv || (hv[(size_t)m * nt + t] == bv && hi[(size_t)m * nt + t] < bi)) { bv = hv[(size_t)m * nt + t]; bi = hi[(size_t)m * nt + t]; }
            index[m] = bi;
        }
    }
    if (out) HIP_CHECK(hipMemcpy(out, y, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// ONE launch of k_cn_attn_step_bf16: as mis_debug_canary_attn_step with the K | V store given as bf16 bits
extern "C" mis_status mis_debug_canary_attn_step_bf16(int device, const float* q, const uint16_t* kv, const int32_t* cnt, int batch, int cap, int heads, int hd,
                                                      float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(q && kv && cnt && out && batch >= 1 && batch <= 65535 && cap >= 1 && heads >= 1 && heads <= 65535 && hd >= 1 && hd <= 128, MIS_ERR_INVALID_INPUT,
                "Canary bf16 attention step: pointers, positive batch, cap, heads and a head size up to 128");
    const int64_t h = (int64_t)heads * hd;
    MIS_REQUIRE((int64_t)batch * cap * 2 * h <= CND_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Canary bf16 attention step: tensor too large");
    for (int b = 0; b < batch; ++b) MIS_REQUIRE(cnt[b] >= 1 && cnt[b] <= cap, MIS_ERR_INVALID_INPUT, "Canary bf16 attention step: row %d has %d keys outside 1..%d", b, cnt[b], cap);
    HIP_CHECK(hipSetDevice(device));
    CndCtx c;
    DevBuf<uint32_t> dq, dc;
    DevBuf<uint16_t> dkv;
    alloc32(dq, q, (size_t)batch * h, F32_NAN);
    alloc16(dkv, kv, (size_t)batch * cap * 2 * h, BF16_NAN);
    alloc32(dc, cnt, batch, 0x7FFFFFFFu);
    GuardedOut o;
    o.alloc((size_t)batch * h * 4, (size_t)64 * h * 4);
    CnAttn a{cnd_fp(dq), (int)h, nullptr, (int)(2 * h), (int)h, cap, nullptr, reinterpret_cast<const int*>(dc.p), 0, reinterpret_cast<float*>(o.p()), (int)h, hd,
             1.0f / sqrtf((float)hd), dkv.p};
    MIS_LAUNCH(&c, k_cn_attn_step_bf16, dim3(batch, heads), dim3(256), a);
    cnd_sync(c, 1);
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), (size_t)batch * h * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}
