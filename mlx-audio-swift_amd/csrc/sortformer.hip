// sortformer.hip - Sortformer speaker diarization: 16 kHz samples -> NeMo log-mel -> depthwise-striding Conv2d stem (factor 8) ->
// FastConformer blocks with Transformer-XL relative-position attention -> encoder_proj + learned positions -> post-LN BART layers ->
// speaker sigmoids.  Exact f32 on v_mfma_f32_32x32x2_f32 throughout, as ecapa_lid.hip, fsmn_vad.hip and mossformer2.hip (f32_tile.h).
//
// Reference being replaced: SortformerModel (Sources/MLXAudioVAD/Models/Sortformer/Sortformer.swift: ConvSubsampling :16-87,
// RelPositionalEncoding :90-116, RelPositionMultiHeadAttention :119-196, ConformerConvolution :237-278, ConformerLayer :281-329,
// TransformerAttention / TransformerEncoderLayer / TransformerEncoder :381-487, SortformerModules :492-521, callAsFunction :548-559)
// and extractMelFeatures (SortformerFeatures.swift:28-112).  Silence trimming, segments and the streaming state stay on the host.
//
// Ragged batch.  Row b of n samples has F = 1 + n / 160 feature frames (rounded up to a multiple of pad_to when that is set: the
// padded frames are zeros and count as frames, as generate passes features.dim(2)), and T1 = (F - 1) / 2 + 1, T2, T3 = T frames behind
// the three stride-2 stages.  Every buffer is laid out with the longest row's counts; every kernel takes the row's own: the
// statistics run over the row's own frames, each stem stage reads zeros behind the row's own count of its input (the zero padding
// the row would see alone) and writes zeros behind its own output count, attention runs over the row's own T keys, every GEMM writes
// zero rows behind T.  Each output element is one fixed-order sum over data of its own row: bit for bit the same in any batch.
//
//   k_sf_peak      scale[b] = 1 / (max|x| + 1e-3) over the row's own samples (1 when the option is off)
//   k_nemo_log_mel<true>  scale, pre-emphasis, 512-point FFT of one frame in LDS, power, slaney filters over each filter's own bins,
//                  log(. + 2^-24)                                                          (audio_front.h: the front end shared
//   k_nemo_norm    per bin mean / unbiased variance over the row's own frames, (x - mean) / (std + 1e-5), or the copy    with lasr.hip)
//   k_sf_conv0     Conv2d 1 -> C, 3 x 3, stride 2, pad 1, ReLU; channels last [B][T1][F1][C]
//   k_sf_gemm      the one contraction (on f32_tile.h): 64 x 64 tile, every dimension guarded.  Loads: plain, LayerNorm (statistics from k_sf_stats),
//                  ReLU, and the stem's depthwise 3 x 3 stride-2 conv FOLDED into the operand load of the pointwise GEMM that follows
//                  it (nine taps of a channels-last tensor are nine coalesced reads; its own kernel would write and re-read the
//                  largest tensors of the model).  Epilogue: bias, SiLU / ReLU / sigmoid, R + a v, positional table, zero rows behind T
//   k_sf_stats     mean and 1 / sqrt(var + eps) of a frame, one wave per frame (wave_mean_rstd of common.h)
//   k_sf_ln        LayerNorm with weight and bias (norm_out, the BART post-norms), zero rows behind T
//   k_sf_intake    x sqrt(hidden) (scale_input) of the stem's embeddings, zero rows behind T
//   k_sf_attn      flash attention, 64 queries x head x row per block (two waves of 32), 32-key tiles through LDS, online softmax in
//                  f32.  Relative positions: score[i][j] = ((q_i + u) k_j + (q_i + v) P[i - j]) / sqrt(d_k); a query tile x key tile needs
//                  the 64 + 32 - 1 consecutive rows P[q0 - k0 - 31 ..] of the projected table.  Each wave forms its 32 x 64 band product on
//                  MFMA, writes it to LDS and reads the shifted diagonal band[i - j + 31][i] back next to its content score.  The BART
//                  layers run the same kernel without the band (head sizes up to 64: 24 and 64 published).
//                  LDS at head size 64 with the band: Q 64 x 65 + K, V 2 x 32 x 65 + u, v 2 x 64 + band 96 x 65 floats = 58752 bytes.
//   k_sf_glu_dwconv GLU -> depthwise conv (odd k <= 31) with the inference BatchNorm folded into the taps -> SiLU, time tile + halo in LDS
//
// The sinusoid table [2 Tcap - 1][hidden], row d + Tcap - 1 for distance d = i - j, is formed on the host in double and rounded once;
// each layer's relative_k_proj of it is ONE GEMM at finalize (weights x a constant), so a call does not repeat it.  Row b reads P[d] by
// distance, whatever the longest row is.
//
// Launches (derived from the chain below): forward 11 + 15 L_fc + 7 L_tf; forward_features 8 + 15 L_fc + 7 L_tf;
// encode_embeddings 4 + 15 L_fc + 7 L_tf; pre_encode 4; features 3.
#include "common.h"
#define AUDIO_FRONT_NEMO_KERNELS
#include "audio_front.h"
#include "f32_tile.h"
#include "host_weights.h"
#include "step_loop.h"

#include <math.h>
#include <string.h>
#include <memory>

#define SF_MAX_BATCH 64
#define SF_MAX_SECONDS 120
#define SF_DW_TT 64
#define SF_DW_MAXK 31

enum { SF_LOAD_ACT = 0, SF_LOAD_LN, SF_LOAD_RELU, SF_LOAD_DW };
enum { SF_ACT_NONE = 0, SF_ACT_SILU, SF_ACT_RELU, SF_ACT_SIGMOID };

// ============================================================================ front end
__global__ void __launch_bounds__(256) k_sf_peak(const float* __restrict__ pcm, int64_t stride, const int* __restrict__ N, int on,
                                                 float* __restrict__ scale) {
    __shared__ float red[4];
    const int b = blockIdx.x, n = N[b];
    const float* x = pcm + (size_t)b * stride;
    float m = 0.0f;
    if (on) for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(x[i]));
    m = block_max_256(m, red);
    if (threadIdx.x == 0) scale[b] = on ? 1.0f / (m + 1e-3f) : 1.0f;
}

// k_nemo_log_mel<true> (every sample times scale[b]) and k_nemo_norm of audio_front.h follow it.

// ============================================================================ stem
// out[b][t][f][c] = ReLU(bias[c] + sum_ij w[3 i + j][c] feats[b][2 t + i - 1][2 f + j - 1]) for t < T1[b]; the features are zero outside
// the row's own F[b] frames and the mel range
__global__ void __launch_bounds__(256) k_sf_conv0(const float* __restrict__ feats, const int* __restrict__ F, const int* __restrict__ T1,
                                                  const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ out, int Fp,
                                                  int mels, int T1p, int F1, int C, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    size_t r = i / C;
    const int f = (int)(r % F1);
    r /= F1;
    const int t = (int)(r % T1p), b = (int)(r / T1p);
    float v = 0.0f;
    if (t < T1[b]) {
        const int n = min(F[b], Fp);
        const float* x = feats + (size_t)b * Fp * mels;
        float acc = bias[c];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int ti = 2 * t + a - 1;
            if (ti < 0 || ti >= n) continue;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int fi = 2 * f + j - 1;
                if (fi >= 0 && fi < mels) acc = fmaf(w[(3 * a + j) * C + c], x[(size_t)ti * mels + fi], acc);
            }
        }
        v = fmaxf(acc, 0.0f);
    }
    out[i] = v;
}

// ============================================================================ the contraction
// Y[b][r][n] = epilogue(sum_k load(X)[b][r][k] W[n][k]); a batch entry has nr = Tp rowmul rows of which min(cnt[b], Tp) rowmul are live
// (cnt null: all); rows behind them are written as zero.
struct SfGemm {
    const float* X; int ldx;
    const float* W; const float* bias;
    float* Y; int ldy;
    const int* cnt; int Tp, rowmul, K, N, load, act;
    const float *stats, *lnw, *lnb;                          // LN load: stats [rows][2] = mean, rstd
    const float* R; int ldr; float ra;                       // Y = R + ra v (R null: v)
    const float* pos;                                        // [Tp][N] added last
    // DW load: X [B][Tin][Fin][K] channels last, row r = t Fout + f, value = dwb[k] + sum_ij dww[3 i + j][k] X[2 t + i - 1][2 f + j - 1][k]
    const int* cnt_in; int Tin, Fin, Fout; const float *dww, *dwb;
};

template <int LOAD>
__device__ __forceinline__ float sf_load(const SfGemm& p, int b, size_t row, int r, int ci) {
    switch (LOAD) {
        case SF_LOAD_LN: return fmaf((p.X[row * p.ldx + ci] - p.stats[2 * row]) * p.stats[2 * row + 1], p.lnw[ci], p.lnb[ci]);
        case SF_LOAD_RELU: return fmaxf(p.X[row * p.ldx + ci], 0.0f);
        case SF_LOAD_DW: {
            const int t = r / p.Fout, f = r - t * p.Fout, n = min(p.cnt_in[b], p.Tin);
            const float* x = p.X + (size_t)b * p.Tin * p.Fin * p.K;
            float acc = p.dwb[ci];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int ti = 2 * t + a - 1;
                if (ti < 0 || ti >= n) continue;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int fi = 2 * f + j - 1;
                    if (fi >= 0 && fi < p.Fin) acc = fmaf(p.dww[(3 * a + j) * p.K + ci], x[((size_t)ti * p.Fin + fi) * p.K + ci], acc);
                }
            }
            return acc;
        }
        default: return p.X[row * p.ldx + ci];
    }
}

template <int LOAD>
__global__ void __launch_bounds__(256) k_sf_gemm(SfGemm p) {
    constexpr int TT = F32_TILE, TC = F32_TILE;
    __shared__ float As[TT][F32_KC + 1];
    __shared__ float Bs[TC][F32_KC + 1];
    const int b = blockIdx.z, t0 = blockIdx.x * TT, c0 = blockIdx.y * TC, nr = p.Tp * p.rowmul;
    const int T = (p.cnt ? min(p.cnt[b], p.Tp) : p.Tp) * p.rowmul, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t row0 = (size_t)b * nr;
    if (t0 >= T) { f32_tile_zero<TT, TC>(p.Y, p.ldy, row0, t0, c0, nr, p.N); return; }
    f32x16_t acc[1] = {};
    const int wt = (wave & 1) * 32, wc = (wave >> 1) * 32, kh = lane >> 5, l31 = lane & 31;
    for (int ci0 = 0; ci0 < p.K; ci0 += F32_KC) {
#pragma unroll
        for (int n = 0; n < TT * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, ci = ci0 + (i & 31), t = t0 + r;
            As[r][i & 31] = (ci < p.K && t < T) ? sf_load<LOAD>(p, b, row0 + t, t, ci) : 0.0f;
        }
#pragma unroll
        for (int n = 0; n < TC * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, ci = ci0 + (i & 31), co = c0 + r;
            Bs[r][i & 31] = (co < p.N && ci < p.K) ? p.W[(size_t)co * p.K + ci] : 0.0f;
        }
        __syncthreads();
        f32_tile_mfma(As, Bs, wt + l31, wc + l31, kh, acc);
        __syncthreads();
    }
    const int co = c0 + wc + l31;                                   // C/D: column = lane & 31, row = f32_tile_row(r, lane >> 5)
    if (co >= p.N) return;
    const float add = p.bias ? p.bias[co] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = t0 + wt + f32_tile_row(r, kh);
        if (t >= nr) continue;
        const size_t row = row0 + t;
        float v = 0.0f;
        if (t < T) {
            v = acc[0][r] + add;
            if (p.act == SF_ACT_SILU) v = v / (1.0f + expf(-v));
            else if (p.act == SF_ACT_RELU) v = fmaxf(v, 0.0f);
            else if (p.act == SF_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
            if (p.R) v = fmaf(p.ra, v, p.R[row * p.ldr + co]);
            if (p.pos) v += p.pos[(size_t)(t / p.rowmul) * p.N + co];
        }
        p.Y[row * p.ldy + co] = v;
    }
}

// ============================================================================ a wave per frame
__global__ void __launch_bounds__(256) k_sf_stats(const float* __restrict__ X, float* __restrict__ stats, int d, float eps, int M) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float mean, rstd;
    wave_mean_rstd(X + (size_t)row * d, d, eps, mean, rstd);
    if (lane == 0) { stats[2 * (size_t)row] = mean; stats[2 * (size_t)row + 1] = rstd; }
}

__global__ void __launch_bounds__(256) k_sf_ln(const float* X, float* Y, const float* __restrict__ w,
                                               const float* __restrict__ bias, int d, float eps, int M, const int* __restrict__ cnt, int Tp) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* x = X + (size_t)row * d;
    float* y = Y + (size_t)row * d;
    if ((row % Tp) >= cnt[row / Tp]) {
        for (int c = lane; c < d; c += 64) y[c] = 0.0f;
        return;
    }
    float mean, rstd;
    wave_mean_rstd(x, d, eps, mean, rstd);
    for (int c = lane; c < d; c += 64) y[c] = fmaf((x[c] - mean) * rstd, w[c], bias[c]);
}

// y = x g for the row's own frames, zero behind them
__global__ void __launch_bounds__(256) k_sf_intake(const float* __restrict__ X, float* __restrict__ Y, const int* __restrict__ cnt, int Tp, int d,
                                                   float g, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / d;
    Y[i] = (int)(row % Tp) < cnt[row / Tp] ? X[i] * g : 0.0f;
}

// ============================================================================ attention
struct SfAttn {
    const float* qkv; int ld, koff, voff;                    // q at column h hd, k at koff + h hd, v at voff + h hd
    float* out; int ldo;
    const int* cnt; int Tp, hd;
    float qscale, sdk;                                       // q x qscale at staging; score / sdk
    const float *u, *v;                                      // [H][hd]
    const float* P; int ldp, Tcap;                           // projected table [2 Tcap - 1][ldp], row d + Tcap - 1
};

template <int ND, bool REL>
__global__ void __launch_bounds__(128) k_sf_attn(SfAttn p) {
    constexpr int HD = 32 * ND, LDH = HD + 1, PB = REL ? (96 * LDH > 4096 ? 96 * LDH : 4096) : 1;
    __shared__ float Qs[64][LDH];
    __shared__ float Ks[32][LDH];
    __shared__ float Vs[32][LDH];
    __shared__ float Ub[2][HD];
    __shared__ float Pb[PB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 64, n = min(p.cnt[b], p.Tp), hd = p.hd;
    const size_t rowbase = (size_t)b * p.Tp;
    if (q0 >= n) {                                                  // (uniform over the block)
        for (int i = tid; i < 64 * hd; i += 128) {
            const int t = q0 + i / hd;
            if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + i % hd] = 0.0f;
        }
        return;
    }
    for (int i = tid; i < 64 * HD; i += 128) {
        const int r = i / HD, c = i - r * HD, tq = q0 + r;
        Qs[r][c] = (tq < n && c < hd) ? p.qkv[(rowbase + tq) * p.ld + h * hd + c] * p.qscale : 0.0f;
    }
    for (int i = tid; i < 2 * HD; i += 128) {
        const int c = i % HD;
        Ub[i / HD][c] = (REL && c < hd) ? (i < HD ? p.u : p.v)[h * hd + c] : 0.0f;
    }
    const int wq = wave * 32;
    f32x16_t O[ND];
#pragma unroll
    for (int dn = 0; dn < ND; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dn][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    for (int kb = 0; kb < n; kb += 32) {
        __syncthreads();                                            // the previous tile's reads are done (first pass: Qs, Ub staged)
        for (int i = tid; i < 32 * HD; i += 128) {
            const int r = i / HD, c = i - r * HD, key = kb + r;
            const bool ok = key < n && c < hd;
            const size_t at = (rowbase + key) * p.ld + h * hd + c;
            Ks[r][c] = ok ? p.qkv[at + p.koff] : 0.0f;
            Vs[r][c] = ok ? p.qkv[at + p.voff] : 0.0f;
        }
        if constexpr (REL) {
            const int base = q0 - kb - 31 + p.Tcap - 1;             // table row of band row 0
            for (int i = tid; i < 96 * HD; i += 128) {
                const int r = i / HD, c = i - r * HD, idx = base + r;
                Pb[r * LDH + c] = (idx >= 0 && idx < 2 * p.Tcap - 1 && c < hd) ? p.P[(size_t)idx * p.ldp + h * hd + c] : 0.0f;
            }
        }
        __syncthreads();
        // S^T[key][query] = K (Q + u)^T: the lane holds query l31 and keys (r & 3) + 8 (r >> 2) + 4 kh
        f32x16_t S;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] = 0.0f;
#pragma unroll 8
        for (int kk = 0; kk < HD; kk += 2)
            S = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[l31][kk + kh], Qs[wq + l31][kk + kh] + Ub[0][kk + kh], S, 0, 0, 0);
        if constexpr (REL) {
            f32x16_t G0, G1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { G0[r] = 0.0f; G1[r] = 0.0f; }
#pragma unroll 8
            for (int kk = 0; kk < HD; kk += 2) {
                const float qv = Qs[wq + l31][kk + kh] + Ub[1][kk + kh];
                G0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[(wq + l31) * LDH + kk + kh], qv, G0, 0, 0, 0);
                G1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[(wq + 32 + l31) * LDH + kk + kh], qv, G1, 0, 0, 0);
            }
            __syncthreads();                                        // every wave has read its band rows: the space becomes the products'
            float* Bd = Pb + wave * 2048;                           // [64 band rows][32 queries]
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int br = (r & 3) + 8 * (r >> 2) + 4 * kh;
                Bd[br * 32 + l31] = G0[r];
                Bd[(br + 32) * 32 + l31] = G1[r];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = (r & 3) + 8 * (r >> 2) + 4 * kh;
                S[r] += Bd[(l31 - j + 31) * 32 + l31];              // distance i - j, the literal rel-shift's entry
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = (r & 3) + 8 * (r >> 2) + 4 * kh;
            const float s = (kb + j < n) ? S[r] / p.sdk : -INFINITY;
            S[r] = s;
            mx = fmaxf(mx, s);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);                       // finite: every tile holds a key < n
        const float alpha = expf(m_run - m_new);
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = expf(S[r] - m_new); psum += S[r]; }
        l_run = l_run * alpha + psum;
        m_run = m_new;
        // O^T[d][query] += V^T P^T, the keys contracted in the order the lanes hold them
#pragma unroll
        for (int dn = 0; dn < ND; ++dn) {
#pragma unroll
            for (int r = 0; r < 16; ++r) O[dn][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = (r & 3) + 8 * (r >> 2) + 4 * kh;
                O[dn] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[j][dn * 32 + l31], S[r], O[dn], 0, 0, 0);
            }
        }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    __syncthreads();                                                // Qs is free: the outputs go through it for coalesced stores
#pragma unroll
    for (int dn = 0; dn < ND; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) Qs[wq + l31][dn * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh] = O[dn][r] / l_tot;
    __syncthreads();
    for (int i = tid; i < 64 * hd; i += 128) {
        const int r = i / hd, c = i - r * hd, t = q0 + r;
        if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + c] = t < n ? Qs[r][c] : 0.0f;
    }
}

// ============================================================================ conv module
// pw [M][2 C] (pointwise_conv1) -> out [M][C]: g = a sigmoid(b) (a the first C columns, b the last), (k - 1) / 2 zero frames on both
// sides of the row's own n frames, depthwise conv with the BatchNorm folded in (taps [k][C], shift [C]), SiLU.  A block is 64 output
// frames x 64 channels of one row: the tile's 64 + k - 1 gated frames sit in LDS; a wave is 16 frames, a lane a channel.
__global__ void __launch_bounds__(256) k_sf_glu_dwconv(const float* __restrict__ pw, const float* __restrict__ taps, const float* __restrict__ shift,
                                                       const int* __restrict__ cnt, float* __restrict__ out, int Tp, int C, int k) {
    __shared__ float g[SF_DW_TT + SF_DW_MAXK - 1][64];
    const int cl = threadIdx.x & 63, tl = threadIdx.x >> 6, ch = blockIdx.y * 64 + cl, b = blockIdx.z, t0 = blockIdx.x * SF_DW_TT;
    const int n = min(cnt[b], Tp), padl = (k - 1) >> 1;
    const bool live = ch < C;
    const size_t rowbase = (size_t)b * Tp;
    for (int r = tl; r < SF_DW_TT + k - 1; r += 4) {
        const int t = t0 - padl + r;
        float v = 0.0f;
        if (live && t >= 0 && t < n) {
            const float* row = pw + (rowbase + t) * 2 * C;
            v = row[ch] * (1.0f / (1.0f + expf(-row[C + ch])));
        }
        g[r][cl] = v;
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
        for (int i = 0; i < 16; ++i) acc[i] = fmaf(w, g[tl * 16 + i + kk][cl], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = t0 + tl * 16 + i;
        if (t >= Tp) continue;
        const float v = acc[i];
        out[(rowbase + t) * C + ch] = t < n ? v / (1.0f + expf(-v)) : 0.0f;
    }
}

// ============================================================================ host
struct SfLin { const float *w = nullptr, *b = nullptr; };
struct SfFcLayer {
    const float *ln1w, *ln1b, *lnaw, *lnab, *lncw, *lncb, *ln2w, *ln2b, *lnow, *lnob, *u, *v, *P, *dw, *dwshift;
    SfLin ff1a, ff1b, qkv, o, pw1, pw2, ff2a, ff2b;
};
struct SfTfLayer { SfLin qkv, o, fc1, fc2; const float *ln1w, *ln1b, *ln2w, *ln2b; };

struct mis_sortformer {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_sortformer_config cfg{};
    int mels = 0, C = 0, d = 0, H = 0, hd = 0, f = 0, L = 0, ck = 0, dt = 0, Ht = 0, hdt = 0, ft = 0, Lt = 0, S = 0, F1 = 0, F2 = 0, F3 = 0;
    HostWeights raw{"Sortformer", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<float> farena, ptab;
    DevBuf<int> fbr;
    const float *window = nullptr, *twc = nullptr, *tws = nullptr, *fb = nullptr, *c0w = nullptr, *c0b = nullptr, *dw2w = nullptr, *dw2b = nullptr,
                *dw5w = nullptr, *dw5b = nullptr, *pos = nullptr;
    SfLin pw3, pw6, lin, proj, h2h, spk;
    std::vector<SfFcLayer> fc;
    std::vector<SfTfLayer> tf;
    // workspace (sized at finalize)
    int64_t maxN = 0;
    int Fcap = 0, T1cap = 0, T2cap = 0, Tcap = 0;
    DevBuf<float> pcm, scale, melraw, feats, s0, s1, s2, emb, h, x, stats, big, qkv, att, g, gx, gq, ga, gf, probs;
    DevBuf<int> cntN, cntF0, cntF, cnt1, cnt2, cnt3;
    // state of the last call
    int batch = 0, Fp = 0, T1p = 0, T2p = 0, Tp = 0, launches = 0;
    std::vector<int> hN, hF0, hF, hT1, hT2, hT3;
    HipEvents<5> ev;
    bool timed = false;
    bool has_emb = false;        // the last call left the stem's embeddings of ITS rows in emb
    bool timed_done = false;     // the last call was a timed forward: all five events are recorded
};

static inline int sf_half(int t) { return t >= 1 ? (t - 1) / 2 + 1 : 0; }
static inline int sf_frames(int64_t n, int pad_to) {
    const int F = (int)(1 + n / NEMO_HOP);
    return pad_to > 0 ? (int)round_up(F, pad_to) : F;
}

static void sf_check_pad(int pad_to) {
    MIS_REQUIRE(pad_to >= 0 && pad_to <= 16 && (pad_to == 0 || 16 % pad_to == 0), MIS_ERR_INVALID_INPUT, "pad_to %d unsupported (0, 1, 2, 4, 8 or 16)", pad_to);
}

extern "C" mis_status mis_sortformer_frames(const mis_sortformer* c, const int64_t* lens, int batch, int pad_to, int32_t* F_out, int32_t* T_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && lens && batch >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    sf_check_pad(pad_to);
    const int64_t cap = (int64_t)c->cfg.max_seconds * 16000;
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(lens[b] >= 0 && lens[b] <= cap, MIS_ERR_INVALID_INPUT, "row %d: %lld samples outside 0..%lld (max_seconds %d)", b, (long long)lens[b],
                    (long long)cap, c->cfg.max_seconds);
        const int F = sf_frames(lens[b], pad_to);
        if (F_out) F_out[b] = F;
        if (T_out) T_out[b] = sf_half(sf_half(sf_half(F)));
    }
    MIS_API_END
}

extern "C" mis_status mis_sortformer_create(const mis_sortformer_config* cfg, int device, mis_sortformer** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    const int d = cfg->hidden_size, H = cfg->num_attention_heads, dt = cfg->tf_d_model, Ht = cfg->encoder_attention_heads;
    MIS_REQUIRE(cfg->sampling_rate == 16000 && cfg->n_fft == NEMO_NFFT && cfg->hop_length == NEMO_HOP && cfg->win_length == NEMO_WIN, MIS_ERR_INVALID_INPUT,
                "sampling_rate / n_fft / hop_length / win_length: only 16000 / 512 / 160 / 400 are implemented");
    MIS_REQUIRE(cfg->preemphasis >= 0.0f && cfg->preemphasis <= 1.0f, MIS_ERR_INVALID_INPUT, "preemphasis outside 0..1");
    MIS_REQUIRE(cfg->num_mel_bins >= 8 && cfg->num_mel_bins <= 256, MIS_ERR_INVALID_INPUT, "num_mel_bins %d outside 8..256", cfg->num_mel_bins);
    MIS_REQUIRE(cfg->subsampling_factor == 8 && cfg->subsampling_conv_kernel_size == 3 && cfg->subsampling_conv_stride == 2, MIS_ERR_INVALID_INPUT,
                "subsampling_factor / subsampling_conv_kernel_size / subsampling_conv_stride: only 8 / 3 / 2 are implemented");
    MIS_REQUIRE(cfg->subsampling_conv_channels >= 1 && cfg->subsampling_conv_channels <= 1024, MIS_ERR_INVALID_INPUT,
                "subsampling_conv_channels %d outside 1..1024", cfg->subsampling_conv_channels);
    MIS_REQUIRE(d >= 8 && d <= 4096, MIS_ERR_INVALID_INPUT, "hidden_size %d outside 8..4096", d);
    MIS_REQUIRE(H >= 1 && d % H == 0 && d / H <= 64, MIS_ERR_INVALID_INPUT,
                "num_attention_heads %d: head size hidden_size / num_attention_heads must be a whole number up to 64", H);
    MIS_REQUIRE(cfg->num_key_value_heads == H, MIS_ERR_INVALID_INPUT, "num_key_value_heads %d must equal num_attention_heads %d", cfg->num_key_value_heads, H);
    MIS_REQUIRE(cfg->intermediate_size >= 1 && cfg->intermediate_size <= 16384, MIS_ERR_INVALID_INPUT, "intermediate_size %d outside 1..16384",
                cfg->intermediate_size);
    MIS_REQUIRE(cfg->num_hidden_layers >= 1 && cfg->num_hidden_layers <= 64, MIS_ERR_INVALID_INPUT, "num_hidden_layers %d outside 1..64", cfg->num_hidden_layers);
    MIS_REQUIRE(cfg->conv_kernel_size >= 3 && cfg->conv_kernel_size <= SF_DW_MAXK && cfg->conv_kernel_size % 2 == 1, MIS_ERR_INVALID_INPUT,
                "conv_kernel_size %d unsupported (odd, 3..%d)", cfg->conv_kernel_size, SF_DW_MAXK);
    MIS_REQUIRE(dt >= 8 && dt <= 4096, MIS_ERR_INVALID_INPUT, "d_model %d outside 8..4096", dt);
    MIS_REQUIRE(Ht >= 1 && dt % Ht == 0 && dt / Ht <= 64, MIS_ERR_INVALID_INPUT,
                "encoder_attention_heads %d: head size d_model / encoder_attention_heads must be a whole number up to 64", Ht);
    MIS_REQUIRE(cfg->encoder_ffn_dim >= 1 && cfg->encoder_ffn_dim <= 16384, MIS_ERR_INVALID_INPUT, "encoder_ffn_dim %d outside 1..16384", cfg->encoder_ffn_dim);
    MIS_REQUIRE(cfg->encoder_layers >= 1 && cfg->encoder_layers <= 64, MIS_ERR_INVALID_INPUT, "encoder_layers %d outside 1..64", cfg->encoder_layers);
    MIS_REQUIRE(cfg->max_source_positions >= 1, MIS_ERR_INVALID_INPUT, "max_source_positions %d must be positive", cfg->max_source_positions);
    MIS_REQUIRE(cfg->layer_norm_eps > 0.0f, MIS_ERR_INVALID_INPUT, "layer_norm_eps must be positive");
    MIS_REQUIRE(cfg->fc_d_model == d && cfg->tf_d_model_modules == dt, MIS_ERR_INVALID_INPUT,
                "fc_d_model %d / tf_d_model %d of the modules differ from hidden_size %d / d_model %d", cfg->fc_d_model, cfg->tf_d_model_modules, d, dt);
    MIS_REQUIRE(cfg->num_speakers >= 1 && cfg->num_speakers <= 64, MIS_ERR_INVALID_INPUT, "num_speakers %d outside 1..64", cfg->num_speakers);
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= SF_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch %d outside 1..%d", cfg->max_batch, SF_MAX_BATCH);
    MIS_REQUIRE(cfg->max_seconds >= 1 && cfg->max_seconds <= SF_MAX_SECONDS, MIS_ERR_INVALID_INPUT, "max_seconds %d outside 1..%d", cfg->max_seconds,
                SF_MAX_SECONDS);
    hipStream_t stream = mis_open_stream(device);      // first: the handle's events belong to this device
    auto c = std::make_unique<mis_sortformer>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->mels = cfg->num_mel_bins; c->C = cfg->subsampling_conv_channels; c->d = d; c->H = H; c->hd = d / H; c->f = cfg->intermediate_size;
    c->L = cfg->num_hidden_layers; c->ck = cfg->conv_kernel_size; c->dt = dt; c->Ht = Ht; c->hdt = dt / Ht; c->ft = cfg->encoder_ffn_dim;
    c->Lt = cfg->encoder_layers; c->S = cfg->num_speakers;
    c->F1 = sf_half(c->mels); c->F2 = sf_half(c->F1); c->F3 = sf_half(c->F2);
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_sortformer_destroy(mis_sortformer* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    delete c;
}

extern "C" mis_status mis_sortformer_set_tensor(mis_sortformer* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 4, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

// c: whatever carries the stream and the launch counter (the handle; the debug entry points' bare context)
template <class Ctx>
static void sf_gemm(Ctx* c, SfGemm p, int B) {
    const dim3 grid(cdiv((int64_t)p.Tp * p.rowmul, 64), cdiv(p.N, 64), B);
    switch (p.load) {
        case SF_LOAD_LN: MIS_LAUNCH(c, k_sf_gemm<SF_LOAD_LN>, grid, dim3(256), p); break;
        case SF_LOAD_RELU: MIS_LAUNCH(c, k_sf_gemm<SF_LOAD_RELU>, grid, dim3(256), p); break;
        case SF_LOAD_DW: MIS_LAUNCH(c, k_sf_gemm<SF_LOAD_DW>, grid, dim3(256), p); break;
        default: MIS_LAUNCH(c, k_sf_gemm<SF_LOAD_ACT>, grid, dim3(256), p); break;
    }
}
// plain rows [B Tp][K] x lin -> Y [B Tp][N]
static SfGemm sf_lin(const float* X, int K, const SfLin& l, float* Y, int N, const int* cnt, int Tp, int act = SF_ACT_NONE) {
    SfGemm p{};
    p.X = X; p.ldx = K; p.W = l.w; p.bias = l.b; p.Y = Y; p.ldy = N; p.cnt = cnt; p.Tp = Tp; p.rowmul = 1; p.K = K; p.N = N; p.act = act;
    return p;
}

extern "C" mis_status mis_sortformer_finalize(mis_sortformer* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t mels = c->mels, C = c->C, d = c->d, f = c->f, ck = c->ck, dt = c->dt, ft = c->ft, S = c->S, F3 = c->F3, H = c->H, hd = c->hd;
    const bool ab = c->cfg.attention_bias != 0, kb = c->cfg.k_proj_bias != 0;
    HostArena a(c->raw);
    std::vector<float>& fh = a.fhost;
    // ---- front end tables: window 400 -> 512, FFT twiddles, slaney filters [257][mels] and each filter's bin range
    const size_t o_win = a.ftake(NEMO_NFFT, c->window), o_twc = a.ftake(NEMO_NFFT / 2, c->twc), o_tws = a.ftake(NEMO_NFFT / 2, c->tws);
    hann_padded(&fh[o_win], NEMO_WIN, NEMO_NFFT);
    fft512_twiddles(&fh[o_twc], &fh[o_tws]);
    const size_t o_fb = a.ftake((size_t)NEMO_BINS * mels, c->fb);
    std::vector<int> ranges(2 * mels, 0);
    slaney_filterbank(&fh[o_fb], ranges.data(), NEMO_BINS, (int)mels, 16000.0, NEMO_NFFT);
    // ---- workspace extents
    c->maxN = (int64_t)c->cfg.max_seconds * 16000;
    c->Fcap = sf_frames(c->maxN, 16); c->T1cap = sf_half(c->Fcap); c->T2cap = sf_half(c->T1cap); c->Tcap = sf_half(c->T2cap);
    const int Tc = c->Tcap, NP = 2 * Tc - 1;
    // ---- weights; an absent bias stays nullptr
    auto lin = [&](const std::string& p, int64_t N, int64_t K, bool bias, SfLin& l) {
        l = SfLin{};
        a.fvec(p + ".weight", {N, K}, N * K, l.w);
        if (bias) a.fvec(p + ".bias", {N}, N, l.b);
    };
    // three linears over the same input as one [N0 + N1 + N2][K]; an absent bias is zero
    auto lin3 = [&](const std::string& p, const char* n0, const char* n1, const char* n2, int64_t N, bool b0, bool b1, bool b2, SfLin& l) {
        const size_t ow = a.ftake((size_t)3 * N * N, l.w), ob = a.ftake(3 * N, l.b);
        const char* names[3] = {n0, n1, n2};
        const bool has[3] = {b0, b1, b2};
        for (int i = 0; i < 3; ++i) {
            const HostTensor& w = c->raw.need(p + names[i] + ".weight", {N, N});
            std::copy(w.v.begin(), w.v.end(), fh.begin() + ow + (size_t)i * N * N);
            if (has[i]) { const HostTensor& bb = c->raw.need(p + names[i] + ".bias", {N}); std::copy(bb.v.begin(), bb.v.end(), fh.begin() + ob + (size_t)i * N); }
        }
    };
    auto norm = [&](const std::string& p, int64_t n, const float*& w, const float*& b) { a.fvec(p + ".weight", {n}, n, w); a.fvec(p + ".bias", {n}, n, b); };
    const std::string SUB = "fc_encoder.subsampling.";
    // conv taps [C][3][3][1] -> [9][C]
    auto taps9 = [&](const std::string& name, const float*& dst) {
        const HostTensor& t = c->raw.need(name, {C, 3, 3, 1});
        const size_t off = a.ftake(9 * C, dst);
        for (int64_t ch = 0; ch < C; ++ch) for (int k = 0; k < 9; ++k) fh[off + k * C + ch] = t.v[ch * 9 + k];
    };
    taps9(SUB + "layers_0.weight", c->c0w); a.fvec(SUB + "layers_0.bias", {C}, C, c->c0b);
    taps9(SUB + "layers_2.weight", c->dw2w); a.fvec(SUB + "layers_2.bias", {C}, C, c->dw2b);
    a.fvec(SUB + "layers_3.weight", {C, 1, 1, C}, C * C, c->pw3.w); a.fvec(SUB + "layers_3.bias", {C}, C, c->pw3.b);
    taps9(SUB + "layers_5.weight", c->dw5w); a.fvec(SUB + "layers_5.bias", {C}, C, c->dw5b);
    a.fvec(SUB + "layers_6.weight", {C, 1, 1, C}, C * C, c->pw6.w); a.fvec(SUB + "layers_6.bias", {C}, C, c->pw6.b);
    // linear [d][C F3] reads the flattening (c, f); the stem keeps channels last, so its columns are re-ordered to (f, c) once, here
    {
        const size_t ow = a.ftake((size_t)d * C * F3, c->lin.w);
        a.fvec(SUB + "linear.bias", {d}, d, c->lin.b);
        const HostTensor& w = c->raw.need(SUB + "linear.weight", {d, C * F3});
        for (int64_t n = 0; n < d; ++n) for (int64_t ch = 0; ch < C; ++ch) for (int64_t fq = 0; fq < F3; ++fq)
            fh[ow + (n * F3 + fq) * C + ch] = w.v[n * C * F3 + ch * F3 + fq];
    }
    c->fc.assign(c->L, SfFcLayer{});
    std::vector<SfLin> rk(c->L);                         // relative_k_proj: used once, below
    for (int li = 0; li < c->L; ++li) {
        const std::string q = "fc_encoder.layers." + std::to_string(li) + ".";
        SfFcLayer& l = c->fc[li];
        norm(q + "norm_feed_forward1", d, l.ln1w, l.ln1b);
        lin(q + "feed_forward1.linear1", f, d, true, l.ff1a); lin(q + "feed_forward1.linear2", d, f, true, l.ff1b);
        norm(q + "norm_self_att", d, l.lnaw, l.lnab);
        lin3(q + "self_attn.", "q_proj", "k_proj", "v_proj", d, ab, ab, ab, l.qkv);
        lin(q + "self_attn.o_proj", d, d, ab, l.o);
        a.fvec(q + "self_attn.relative_k_proj.weight", {d, d}, d * d, rk[li].w);
        a.fvec(q + "self_attn.bias_u", {H, hd}, d, l.u); a.fvec(q + "self_attn.bias_v", {H, hd}, d, l.v);
        norm(q + "norm_conv", d, l.lncw, l.lncb);
        a.fvec(q + "conv.pointwise_conv1.weight", {2 * d, 1, d}, 2 * d * d, l.pw1.w); a.fvec(q + "conv.pointwise_conv1.bias", {2 * d}, 2 * d, l.pw1.b);
        a.fvec(q + "conv.pointwise_conv2.weight", {d, 1, d}, d * d, l.pw2.w); a.fvec(q + "conv.pointwise_conv2.bias", {d}, d, l.pw2.b);
        // inference BatchNorm folded into the depthwise taps and a shift
        const HostTensor& dw = c->raw.need(q + "conv.depthwise_conv.weight", {d, ck, 1});
        const HostTensor& dwb = c->raw.need(q + "conv.depthwise_conv.bias", {d});
        const HostTensor& bw = c->raw.need(q + "conv.norm.weight", {d}); const HostTensor& bb = c->raw.need(q + "conv.norm.bias", {d});
        const HostTensor& bm = c->raw.need(q + "conv.norm.running_mean", {d}); const HostTensor& bv = c->raw.need(q + "conv.norm.running_var", {d});
        const size_t o_dw = a.ftake((size_t)ck * d, l.dw), o_sh = a.ftake(d, l.dwshift);
        fold_bn_dwconv(&fh[o_dw], &fh[o_sh], dw.v.data(), dwb.v.data(), bw.v.data(), bb.v.data(), bm.v.data(), bv.v.data(), d, ck);
        norm(q + "norm_feed_forward2", d, l.ln2w, l.ln2b);
        lin(q + "feed_forward2.linear1", f, d, true, l.ff2a); lin(q + "feed_forward2.linear2", d, f, true, l.ff2b);
        norm(q + "norm_out", d, l.lnow, l.lnob);
    }
    const int64_t msp = c->cfg.max_source_positions;
    a.fvec("tf_encoder.embed_positions.weight", {msp, dt}, msp * dt, c->pos);
    c->tf.assign(c->Lt, SfTfLayer{});
    for (int li = 0; li < c->Lt; ++li) {
        const std::string q = "tf_encoder.layers." + std::to_string(li) + ".";
        SfTfLayer& l = c->tf[li];
        lin3(q + "self_attn.", "q_proj", "k_proj", "v_proj", dt, true, kb, true, l.qkv);
        lin(q + "self_attn.out_proj", dt, dt, true, l.o);
        norm(q + "self_attn_layer_norm", dt, l.ln1w, l.ln1b);
        lin(q + "fc1", ft, dt, true, l.fc1); lin(q + "fc2", dt, ft, true, l.fc2);
        norm(q + "final_layer_norm", dt, l.ln2w, l.ln2b);
    }
    const std::string SM = "sortformer_modules.";
    lin(SM + "encoder_proj", dt, d, true, c->proj); lin(SM + "first_hidden_to_hidden", dt, dt, true, c->h2h);
    lin(SM + "single_hidden_to_spks", S, dt, true, c->spk);
    c->raw.need(SM + "hidden_to_spks.weight", {S, 2 * dt}); c->raw.need(SM + "hidden_to_spks.bias", {S});   // loaded and checked, unused
    // ---- the sinusoid table by distance: row d + Tcap - 1, columns interleaved sin, cos; formed in double, rounded once
    const float* tab = nullptr;
    const size_t o_tab = a.ftake((size_t)NP * d, tab);
    for (int r = 0; r < NP; ++r) {
        const double dist = (double)(r - (Tc - 1));
        for (int64_t k = 0; 2 * k < d; ++k) {
            const double ang = dist * exp(-(double)(2 * k) * log(10000.0) / (double)d);
            fh[o_tab + (size_t)r * d + 2 * k] = (float)sin(ang);
            if (2 * k + 1 < d) fh[o_tab + (size_t)r * d + 2 * k + 1] = (float)cos(ang);
        }
    }
    // ---- upload: every pointer bound above now addresses the device arena
    DevBuf<bf16_t> none;
    a.upload(none, c->farena);
    c->fbr.alloc(2 * mels);
    HIP_CHECK(hipMemcpy(c->fbr.p, ranges.data(), 2 * mels * sizeof(int), hipMemcpyHostToDevice));
    // each layer's relative_k_proj of the table: one GEMM, once
    c->ptab.alloc((size_t)c->L * NP * d);
    for (int li = 0; li < c->L; ++li) {
        float* dst = c->ptab.p + (size_t)li * NP * d;
        sf_gemm(c, sf_lin(tab, (int)d, rk[li], dst, (int)d, nullptr, NP), 1);
        c->fc[li].P = dst;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->launches = 0;
    // ---- the workspace: every buffer a call touches, for max_batch rows of max_seconds
    const size_t B = c->cfg.max_batch, M = B * Tc;
    c->pcm.alloc(B * c->maxN); c->scale.alloc(B); c->melraw.alloc(B * c->Fcap * mels); c->feats.alloc(B * c->Fcap * mels);
    c->s0.alloc(B * c->T1cap * c->F1 * C); c->s1.alloc(B * c->T2cap * c->F2 * C); c->s2.alloc(M * F3 * C); c->emb.alloc(M * d);
    c->h.alloc(M * d); c->x.alloc(M * d); c->stats.alloc(M * 2); c->big.alloc(M * std::max<size_t>(f, 2 * d)); c->qkv.alloc(M * 3 * d); c->att.alloc(M * d);
    c->g.alloc(M * dt); c->gx.alloc(M * dt); c->gq.alloc(M * 3 * dt); c->ga.alloc(M * dt); c->gf.alloc(M * ft); c->probs.alloc(M * S);
    c->cntN.alloc(B); c->cntF0.alloc(B); c->cntF.alloc(B); c->cnt1.alloc(B); c->cnt2.alloc(B); c->cnt3.alloc(B);
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of SortformerModel
extern "C" mis_status mis_sortformer_init_synthetic(mis_sortformer* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    const int64_t C = c->C, d = c->d, f = c->f, ck = c->ck, dt = c->dt, ft = c->ft;
    const bool ab = c->cfg.attention_bias != 0;
    const std::string SUB = "fc_encoder.subsampling.";
    sw.put(SUB + "layers_0.weight", {C, 3, 3, 1}, sqrt(3.0 / 9.0), 0.0f); sw.put(SUB + "layers_0.bias", {C}, 0.05, 0.0f);
    for (const char* n : {"layers_2", "layers_5"}) { sw.put(SUB + n + ".weight", {C, 3, 3, 1}, sqrt(3.0 / 9.0), 0.0f); sw.put(SUB + n + ".bias", {C}, 0.05, 0.0f); }
    for (const char* n : {"layers_3", "layers_6"}) { sw.put(SUB + n + ".weight", {C, 1, 1, C}, sqrt(3.0 / (double)C), 0.0f); sw.put(SUB + n + ".bias", {C}, 0.05, 0.0f); }
    sw.lin(SUB + "linear", d, C * c->F3, true, 1.0);
    for (int li = 0; li < c->L; ++li) {
        const std::string q = "fc_encoder.layers." + std::to_string(li) + ".";
        for (const char* n : {"norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"}) sw.norm(q + n, d);
        for (const char* n : {"feed_forward1", "feed_forward2"}) { sw.lin(q + n + ".linear1", f, d, true, 1.0); sw.lin(q + n + ".linear2", d, f, true, 0.5); }
        for (const char* n : {"q_proj", "k_proj", "v_proj"}) sw.lin(q + "self_attn." + n, d, d, ab, 1.0);
        sw.lin(q + "self_attn.o_proj", d, d, ab, 0.5);
        sw.lin(q + "self_attn.relative_k_proj", d, d, false, 1.0);
        sw.put(q + "self_attn.bias_u", {c->H, c->hd}, 0.1, 0.0f); sw.put(q + "self_attn.bias_v", {c->H, c->hd}, 0.1, 0.0f);
        sw.put(q + "conv.pointwise_conv1.weight", {2 * d, 1, d}, sqrt(3.0 / (double)d), 0.0f); sw.put(q + "conv.pointwise_conv1.bias", {2 * d}, 0.05, 0.0f);
        sw.put(q + "conv.pointwise_conv2.weight", {d, 1, d}, 0.5 * sqrt(3.0 / (double)d), 0.0f); sw.put(q + "conv.pointwise_conv2.bias", {d}, 0.05, 0.0f);
        sw.put(q + "conv.depthwise_conv.weight", {d, ck, 1}, sqrt(3.0 / (double)ck), 0.0f); sw.put(q + "conv.depthwise_conv.bias", {d}, 0.05, 0.0f);
        sw.put(q + "conv.norm.weight", {d}, 0.1, 1.0f); sw.put(q + "conv.norm.bias", {d}, 0.05, 0.0f);
        sw.put(q + "conv.norm.running_mean", {d}, 0.05, 0.0f); sw.put(q + "conv.norm.running_var", {d}, 0.1, 1.0f);
    }
    sw.put("tf_encoder.embed_positions.weight", {c->cfg.max_source_positions, dt}, 0.1, 0.0f);
    for (int li = 0; li < c->Lt; ++li) {
        const std::string q = "tf_encoder.layers." + std::to_string(li) + ".";
        sw.lin(q + "self_attn.q_proj", dt, dt, true, 1.0); sw.lin(q + "self_attn.k_proj", dt, dt, c->cfg.k_proj_bias != 0, 1.0);
        sw.lin(q + "self_attn.v_proj", dt, dt, true, 1.0); sw.lin(q + "self_attn.out_proj", dt, dt, true, 0.5);
        sw.norm(q + "self_attn_layer_norm", dt); sw.norm(q + "final_layer_norm", dt);
        sw.lin(q + "fc1", ft, dt, true, 1.0); sw.lin(q + "fc2", dt, ft, true, 0.5);
    }
    const std::string SM = "sortformer_modules.";
    sw.lin(SM + "encoder_proj", dt, d, true, 1.0); sw.lin(SM + "first_hidden_to_hidden", dt, dt, true, 1.0);
    sw.lin(SM + "single_hidden_to_spks", c->S, dt, true, 1.0); sw.lin(SM + "hidden_to_spks", c->S, 2 * dt, true, 1.0);
    MIS_API_END
}

// ============================================================================ the chain
static void sf_check_ready(const mis_sortformer* c, int batch) {
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch %d outside 1..%d (max_batch)", batch, c->cfg.max_batch);
}
// A call is judged first (sf_check_*: nothing of the handle is written), then taken (sf_take_*: the last call's state is replaced).
static void sf_check_T(const mis_sortformer* c, const std::vector<int>& T, int Tp) {
    MIS_REQUIRE(Tp >= 1 && Tp <= c->Tcap, MIS_ERR_INVALID_INPUT, "%d encoder frames exceed the workspace of %d (max_seconds %d)", Tp, c->Tcap, c->cfg.max_seconds);
    MIS_REQUIRE(Tp <= c->cfg.max_source_positions, MIS_ERR_INVALID_INPUT, "%d encoder frames exceed max_source_positions %d", Tp, c->cfg.max_source_positions);
    for (size_t b = 0; b < T.size(); ++b) MIS_REQUIRE(T[b] >= 1 && T[b] <= Tp, MIS_ERR_INVALID_INPUT, "row %d: %d encoder frames outside 1..%d", (int)b, T[b], Tp);
}
// the encoder's frame counts of every row; the longest row's are the strides.  A new call starts here: no embeddings, no timestamps yet.
static void sf_take_T(mis_sortformer* c, const std::vector<int>& T, int Tp) {
    c->hT3 = T; c->batch = (int)T.size(); c->Tp = Tp; c->launches = 0; c->has_emb = false; c->timed_done = false;
    HIP_CHECK(hipMemcpyAsync(c->cnt3.p, c->hT3.data(), T.size() * 4, hipMemcpyHostToDevice, c->stream));
}
// feature frames F[b] (padding included) of every row at the stride Fp
static void sf_check_frames(const mis_sortformer* c, const std::vector<int>& F, int Fp) {
    MIS_REQUIRE(Fp >= 1 && Fp <= c->Fcap, MIS_ERR_INVALID_INPUT, "%d feature frames exceed the workspace of %d (max_seconds %d)", Fp, c->Fcap, c->cfg.max_seconds);
    std::vector<int> t3(F.size());
    for (size_t b = 0; b < F.size(); ++b) {
        MIS_REQUIRE(F[b] >= 1 && F[b] <= Fp, MIS_ERR_INVALID_INPUT, "row %d: %d feature frames outside 1..%d (the row stride)", (int)b, F[b], Fp);
        t3[b] = sf_half(sf_half(sf_half(F[b])));
    }
    sf_check_T(c, t3, sf_half(sf_half(sf_half(Fp))));
}
static void sf_take_frames(mis_sortformer* c, const std::vector<int>& F, int Fp) {
    const int B = (int)F.size();
    std::vector<int> t1(B), t2(B), t3(B);
    for (int b = 0; b < B; ++b) { t1[b] = sf_half(F[b]); t2[b] = sf_half(t1[b]); t3[b] = sf_half(t2[b]); }
    c->Fp = Fp; c->T1p = sf_half(Fp); c->T2p = sf_half(c->T1p);
    sf_take_T(c, t3, sf_half(c->T2p));
    c->hF = F; c->hT1 = t1; c->hT2 = t2;
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpyAsync(c->cntF.p, c->hF.data(), B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt1.p, c->hT1.data(), B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt2.p, c->hT2.data(), B * 4, hipMemcpyHostToDevice, s));
}

// pcm f32 [B][stride] -> c->feats [B][Fp][mels]
static void sf_front(mis_sortformer* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int peak, int normalize, int pad_to) {
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    sf_check_pad(pad_to);
    std::vector<int> N(batch), F0(batch), F(batch);
    int Fp = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 0 && n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the row stride %lld", b, (long long)n, (long long)stride);
        MIS_REQUIRE(n <= c->maxN, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the workspace of %d seconds (max_seconds)", b, (long long)n,
                    c->cfg.max_seconds);
        N[b] = (int)n; F0[b] = sf_frames(n, 0); F[b] = sf_frames(n, pad_to);
        Fp = std::max(Fp, F[b]);
    }
    sf_check_frames(c, F, Fp);
    sf_take_frames(c, F, Fp);
    c->hN = N; c->hF0 = F0;
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpyAsync(c->cntN.p, c->hN.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cntF0.p, c->hF0.data(), batch * 4, hipMemcpyHostToDevice, s));
    const int64_t ws = std::min<int64_t>(stride, c->maxN);
    HIP_CHECK(hipMemcpy2DAsync(c->pcm.p, ws * 4, pcm, stride * 4, ws * 4, batch, hipMemcpyDefault, s));
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[0], s));
    MIS_LAUNCH(c, k_sf_peak, dim3(batch), dim3(256), c->pcm.p, ws, c->cntN.p, peak, c->scale.p);
    MIS_LAUNCH(c, k_nemo_log_mel<true>, dim3(Fp, batch), dim3(256), c->pcm.p, ws, c->cntN.p, c->cntF0.p, c->scale.p, c->cfg.preemphasis, c->window, c->twc, c->tws,
              c->fb, c->fbr.p, c->melraw.p, Fp, c->mels);
    MIS_LAUNCH(c, k_nemo_norm, dim3(cdiv(c->mels, 64), batch), dim3(256), c->melraw.p, c->cntF0.p, c->feats.p, Fp, c->mels, normalize);
}

// c->feats -> c->emb [B][Tp][d] (ConvSubsampling), 4 launches
static void sf_stem(mis_sortformer* c) {
    const int B = c->batch, C = c->C, F1 = c->F1, F2 = c->F2, F3 = c->F3;
    const size_t n0 = (size_t)B * c->T1p * F1 * C;
    MIS_LAUNCH(c, k_sf_conv0, dim3((unsigned)((n0 + 255) / 256)), dim3(256), c->feats.p, c->cntF.p, c->cnt1.p, c->c0w, c->c0b, c->s0.p, c->Fp, c->mels, c->T1p,
              F1, C, n0);
    auto dwpw = [&](const float* in, const int* cin, int Tin, int Fin, const float* dww, const float* dwb, const SfLin& pw, float* out, const int* cout,
                    int Tout, int Fout) {
        SfGemm p{};
        p.X = in; p.ldx = C; p.W = pw.w; p.bias = pw.b; p.Y = out; p.ldy = C; p.cnt = cout; p.Tp = Tout; p.rowmul = Fout; p.K = C; p.N = C;
        p.load = SF_LOAD_DW; p.act = SF_ACT_RELU; p.cnt_in = cin; p.Tin = Tin; p.Fin = Fin; p.Fout = Fout; p.dww = dww; p.dwb = dwb;
        sf_gemm(c, p, B);
    };
    dwpw(c->s0.p, c->cnt1.p, c->T1p, F1, c->dw2w, c->dw2b, c->pw3, c->s1.p, c->cnt2.p, c->T2p, F2);
    dwpw(c->s1.p, c->cnt2.p, c->T2p, F2, c->dw5w, c->dw5b, c->pw6, c->s2.p, c->cnt3.p, c->Tp, F3);
    sf_gemm(c, sf_lin(c->s2.p, F3 * C, c->lin, c->emb.p, c->d, c->cnt3.p, c->Tp), B);
    c->has_emb = true;
}

template <bool REL, class Ctx>
static void sf_attn(Ctx* c, const SfAttn& p, int heads, int hd, int batch) {
    const dim3 grid(cdiv(p.Tp, 64), heads, batch);
    if (hd <= 32) MIS_LAUNCH(c, (k_sf_attn<1, REL>), grid, dim3(128), p);
    else MIS_LAUNCH(c, (k_sf_attn<2, REL>), grid, dim3(128), p);
}

// c->emb -> Conformer blocks -> projection -> BART layers -> c->probs.  stop: -1 everything; 1 .. L behind that block (c->h);
// L + 1 behind the projection, L + 2 .. L + 1 + Lt behind that BART layer (c->g).
static void sf_encoder(mis_sortformer* c, int stop) {
    const int B = c->batch, Tp = c->Tp, d = c->d, f = c->f, dt = c->dt, ft = c->ft, M = B * Tp, L = c->L;
    const int* cnt = c->cnt3.p;
    hipStream_t s = c->stream;
    const size_t nd = (size_t)M * d;
    MIS_LAUNCH(c, k_sf_intake, dim3((unsigned)((nd + 255) / 256)), dim3(256), c->emb.p, c->h.p, cnt, Tp, d,
              c->cfg.scale_input ? sqrtf((float)d) : 1.0f, nd);
    auto stats = [&](const float* x) { MIS_LAUNCH(c, k_sf_stats, dim3(cdiv(M, 4)), dim3(256), x, c->stats.p, d, 1e-5f, M); };
    auto ln_lin = [&](const float* x, const float* w, const float* b, const SfLin& l, float* y, int N, int act) {
        SfGemm p = sf_lin(x, d, l, y, N, cnt, Tp, act);
        p.load = SF_LOAD_LN; p.stats = c->stats.p; p.lnw = w; p.lnb = b;
        sf_gemm(c, p, B);
    };
    auto res_lin = [&](const float* x, int K, const SfLin& l, float* hres, int N, float ra) {
        SfGemm p = sf_lin(x, K, l, hres, N, cnt, Tp);
        p.R = hres; p.ldr = N; p.ra = ra;
        sf_gemm(c, p, B);
    };
    for (int li = 0; li < L; ++li) {                               // 15 launches a block
        const SfFcLayer& l = c->fc[li];
        stats(c->h.p);
        ln_lin(c->h.p, l.ln1w, l.ln1b, l.ff1a, c->big.p, f, SF_ACT_SILU);
        res_lin(c->big.p, f, l.ff1b, c->h.p, d, 0.5f);
        stats(c->h.p);
        ln_lin(c->h.p, l.lnaw, l.lnab, l.qkv, c->qkv.p, 3 * d, SF_ACT_NONE);
        SfAttn ap{c->qkv.p, 3 * d, d, 2 * d, c->att.p, d, cnt, Tp, c->hd, 1.0f, sqrtf((float)c->hd), l.u, l.v, l.P, d, c->Tcap};
        sf_attn<true>(c, ap, c->H, c->hd, B);
        res_lin(c->att.p, d, l.o, c->h.p, d, 1.0f);
        stats(c->h.p);
        ln_lin(c->h.p, l.lncw, l.lncb, l.pw1, c->big.p, 2 * d, SF_ACT_NONE);
        MIS_LAUNCH(c, k_sf_glu_dwconv, dim3(cdiv(Tp, SF_DW_TT), cdiv(d, 64), B), dim3(256), c->big.p, l.dw, l.dwshift, cnt, c->att.p, Tp, d, c->ck);
        res_lin(c->att.p, d, l.pw2, c->h.p, d, 1.0f);
        stats(c->h.p);
        ln_lin(c->h.p, l.ln2w, l.ln2b, l.ff2a, c->big.p, f, SF_ACT_SILU);
        res_lin(c->big.p, f, l.ff2b, c->h.p, d, 0.5f);
        MIS_LAUNCH(c, k_sf_ln, dim3(cdiv(M, 4)), dim3(256), c->h.p, c->h.p, l.lnow, l.lnob, d, 1e-5f, M, cnt, Tp);
        if (stop == li + 1) return;
    }
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[3], s));
    {   // encoder_proj + embed_positions[0 .. T)
        SfGemm p = sf_lin(c->h.p, d, c->proj, c->g.p, dt, cnt, Tp);
        p.pos = c->pos;
        sf_gemm(c, p, B);
    }
    if (stop == L + 1) return;
    const float eps = c->cfg.layer_norm_eps;
    for (int li = 0; li < c->Lt; ++li) {                           // 7 launches a layer
        const SfTfLayer& l = c->tf[li];
        sf_gemm(c, sf_lin(c->g.p, dt, l.qkv, c->gq.p, 3 * dt, cnt, Tp), B);
        SfAttn ap{c->gq.p, 3 * dt, dt, 2 * dt, c->ga.p, dt, cnt, Tp, c->hdt, powf((float)c->hdt, -0.5f), 1.0f, nullptr, nullptr, nullptr, 0, 0};
        sf_attn<false>(c, ap, c->Ht, c->hdt, B);
        {
            SfGemm p = sf_lin(c->ga.p, dt, l.o, c->gx.p, dt, cnt, Tp);
            p.R = c->g.p; p.ldr = dt; p.ra = 1.0f;
            sf_gemm(c, p, B);
        }
        MIS_LAUNCH(c, k_sf_ln, dim3(cdiv(M, 4)), dim3(256), c->gx.p, c->g.p, l.ln1w, l.ln1b, dt, eps, M, cnt, Tp);
        sf_gemm(c, sf_lin(c->g.p, dt, l.fc1, c->gf.p, ft, cnt, Tp, SF_ACT_RELU), B);
        {
            SfGemm p = sf_lin(c->gf.p, ft, l.fc2, c->gx.p, dt, cnt, Tp);
            p.R = c->g.p; p.ldr = dt; p.ra = 1.0f;
            sf_gemm(c, p, B);
        }
        MIS_LAUNCH(c, k_sf_ln, dim3(cdiv(M, 4)), dim3(256), c->gx.p, c->g.p, l.ln2w, l.ln2b, dt, eps, M, cnt, Tp);
        if (stop == L + 2 + li) return;
    }
    {   // ReLU -> first_hidden_to_hidden -> ReLU -> single_hidden_to_spks -> sigmoid
        SfGemm p = sf_lin(c->g.p, dt, c->h2h, c->gx.p, dt, cnt, Tp, SF_ACT_RELU);
        p.load = SF_LOAD_RELU;
        sf_gemm(c, p, B);
        sf_gemm(c, sf_lin(c->gx.p, dt, c->spk, c->probs.p, c->S, cnt, Tp, SF_ACT_SIGMOID), B);
    }
}

extern "C" int mis_sortformer_launches(const mis_sortformer* c) { return c ? c->launches : 0; }

static void sf_finish(mis_sortformer* c, const float* dev, float* out, size_t n) {
    HIP_CHECK(hipMemcpyAsync(out, dev, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));                    // the call's one synchronisation
}

extern "C" mis_status mis_sortformer_features(mis_sortformer* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int peak_normalize,
                                              int normalize, int pad_to, float* feats_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && feats_out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    sf_check_ready(c, batch);
    sf_front(c, pcm, lens, batch, stride, peak_normalize, normalize, pad_to);
    sf_finish(c, c->feats.p, feats_out, (size_t)batch * c->Fp * c->mels);
    MIS_API_END
}

static void sf_take_features(mis_sortformer* c, const float* feats, const int32_t* frames, int batch, int F) {
    MIS_REQUIRE(F >= 1, MIS_ERR_INVALID_INPUT, "bad frame count");
    std::vector<int> fr(batch, F);
    if (frames) for (int b = 0; b < batch; ++b) fr[b] = frames[b];
    sf_check_frames(c, fr, F);
    sf_take_frames(c, fr, F);
    HIP_CHECK(hipMemcpyAsync(c->feats.p, feats, (size_t)batch * F * c->mels * 4, hipMemcpyDefault, c->stream));
}

extern "C" mis_status mis_sortformer_forward_features(mis_sortformer* c, const float* feats, const int32_t* frames, int batch, int F, float* probs_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && feats && probs_out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    sf_check_ready(c, batch);
    sf_take_features(c, feats, frames, batch, F);
    sf_stem(c);
    sf_encoder(c, -1);
    sf_finish(c, c->probs.p, probs_out, (size_t)batch * c->Tp * c->S);
    MIS_API_END
}

extern "C" mis_status mis_sortformer_forward(mis_sortformer* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int peak_normalize,
                                             int normalize, int pad_to, float* probs_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && probs_out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    sf_check_ready(c, batch);
    hipStream_t s = c->stream;
    sf_front(c, pcm, lens, batch, stride, peak_normalize, normalize, pad_to);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[1], s));
    sf_stem(c);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[2], s));
    sf_encoder(c, -1);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[4], s));
    sf_finish(c, c->probs.p, probs_out, (size_t)batch * c->Tp * c->S);
    c->timed_done = c->timed;
    MIS_API_END
}

extern "C" mis_status mis_sortformer_pre_encode(mis_sortformer* c, const float* feats, const int32_t* frames, int batch, int F, float* emb_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && feats && emb_out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    sf_check_ready(c, batch);
    sf_take_features(c, feats, frames, batch, F);
    sf_stem(c);
    sf_finish(c, c->emb.p, emb_out, (size_t)batch * c->Tp * c->d);
    MIS_API_END
}

extern "C" mis_status mis_sortformer_encode_embeddings(mis_sortformer* c, const float* emb, const int32_t* counts, int batch, int T, float* probs_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && emb && probs_out, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    sf_check_ready(c, batch);
    std::vector<int> t(batch, T);
    if (counts) for (int b = 0; b < batch; ++b) t[b] = counts[b];
    sf_check_T(c, t, T);
    sf_take_T(c, t, T);
    HIP_CHECK(hipMemcpyAsync(c->emb.p, emb, (size_t)batch * T * c->d * 4, hipMemcpyDefault, c->stream));
    c->has_emb = true;
    sf_encoder(c, -1);
    sf_finish(c, c->probs.p, probs_out, (size_t)batch * c->Tp * c->S);
    MIS_API_END
}

// tensors of the last call (any but features, which leaves no embeddings), f32, zero rows behind a row's own T: stage 0 the stem's embeddings [B, T, hidden] (what the call left),
// 1 .. L that Conformer block, L + 1 the projection + positions [B, T, d_model], L + 2 .. L + 1 + Lt that BART layer, L + 2 + Lt the
// probabilities.  The chain is deterministic and the embeddings are still in the workspace: stages >= 1 are recomputed from them.
extern "C" mis_status mis_sortformer_tap(mis_sortformer* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && dims, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized && c->batch > 0 && c->has_emb, MIS_ERR_NOT_INITIALIZED,
                "no call to tap: the last call must be forward, forward_features, pre_encode or encode_embeddings");
    const int last = c->L + c->Lt + 2;
    MIS_REQUIRE(stage >= 0 && stage <= last, MIS_ERR_INVALID_INPUT, "stage %d outside 0..%d", stage, last);
    HIP_CHECK(hipSetDevice(c->device));
    const int width = stage <= c->L ? c->d : stage < last ? c->dt : c->S;
    dims[0] = c->batch; dims[1] = c->Tp; dims[2] = width;
    if (!out) return MIS_OK;
    const size_t n = (size_t)c->batch * c->Tp * width;
    MIS_REQUIRE((int64_t)n <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    const int kept = c->launches;
    const bool timed = c->timed;
    c->timed = false;
    if (stage >= 1) sf_encoder(c, stage == last ? -1 : stage);
    c->timed = timed;
    c->launches = kept;
    const float* src = stage == 0 ? c->emb.p : stage <= c->L ? c->h.p : stage < last ? c->g.p : c->probs.p;
    sf_finish(c, src, out, n);
    MIS_API_END
}

// benches: device milliseconds of the next / last mis_sortformer_forward: front end, stem, Conformer blocks, projection + BART + head
extern "C" mis_status mis_debug_sortformer_timing(mis_sortformer* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c, MIS_ERR_INVALID_INPUT, "null argument");
    if (!ms) { c->timed = true; return MIS_OK; }
    MIS_REQUIRE(c->timed && c->timed_done, MIS_ERR_NOT_INITIALIZED, "no timed forward: the last call must be mis_sortformer_forward");
    for (int i = 0; i < 4; ++i) HIP_CHECK(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
    MIS_API_END
}

// ============================================================================ test scaffolding (include/mi_speech_debug.h)
// ONE call of sf_gemm / sf_attn, or one launch line of sf_front / sf_stem / sf_encoder, on caller-supplied host data, so that
// tests/test_gpu_sortformer_ops.py can hold the kernels above to an operator-level reference.  Nothing is computed here: the operands are
// uploaded as given and what the launch wrote is copied back.  Guards as the LASR entry points (debug_guard.h): every output is
// [guard | body | guard], all of it the byte 0xFF before the launch (an output that also goes IN - the in-place residual, the in-place
// LayerNorm - holds the caller's data instead); a changed guard byte or padding column fails the call; every input is followed by
// IN_GUARD NaNs (ints: 0x7FFFFFFF).  The entry points refuse only what would make a KERNEL leave these buffers.  The launches run on a
// bare context (the null stream and a launch counter): the launchers need nothing else of the handle.
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

namespace {

constexpr int64_t SFD_MAX_ELEMS = (int64_t)1 << 28;          // per tensor

struct SfdCtx { hipStream_t stream = nullptr; int launches = 0; };

void sfd_sync(const SfdCtx& c) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    MIS_REQUIRE(c.launches == 1, MIS_ERR_GENERATION_FAILED, "%d launches where one was meant", c.launches);
}
void sfd_f32(DevBuf<uint32_t>& d, const float* src, size_t n) { alloc32(d, src, n, F32_NAN); }
// counts [n] followed by 0x7FFFFFFF (a row count that masks nothing)
void sfd_counts(DevBuf<uint32_t>& d, const int32_t* cnt, size_t n) { alloc32(d, cnt, n, 0x7FFFFFFFu); }
const float* sfd_fp(const DevBuf<uint32_t>& d) { return reinterpret_cast<const float*>(d.p); }
const int* sfd_ip(const DevBuf<uint32_t>& d) { return reinterpret_cast<const int*>(d.p); }
float* sfd_out(GuardedOut& o) { return reinterpret_cast<float*>(o.p()); }
// rows of ld words with `cols` live columns -> the live columns, as bits; the columns behind must still hold the fill
void sfd_fetch_rows(GuardedOut& o, size_t rows, size_t ld, size_t cols, float* out) {
    o.check_guards();
    std::vector<uint32_t> h(o.body / 4);
    HIP_CHECK(hipMemcpy(h.data(), o.p(), o.body, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        memcpy(out + r * cols, h.data() + r * ld, cols * 4);
        for (size_t c = cols; c < ld; ++c)
            MIS_REQUIRE(h[r * ld + c] == 0xFFFFFFFFu, MIS_ERR_GENERATION_FAILED, "the kernel wrote column %zu of row %zu behind its %zu columns", c, r, cols);
    }
}
// dense rows [rows][cols] into the body of an output of row stride ld; the padding columns keep the fill
void sfd_put_rows(GuardedOut& o, size_t rows, size_t ld, size_t cols, const float* src) {
    HIP_CHECK(hipMemcpy2D(o.p(), ld * 4, src, cols * 4, cols * 4, rows, hipMemcpyHostToDevice));
}

}  // namespace

extern "C" mis_status mis_debug_sortformer_gemm(int device, int load, int act, const float* X, int ldx, const float* W, const float* bias, const int32_t* cnt,
                                                int batch, int Tp, int rowmul, int K, int N, int ldy, const float* stats, const float* lnw, const float* lnb,
                                                const float* R, int ldr, float ra, int in_place, const float* pos, const int32_t* cnt_in, int Tin, int Fin,
                                                int Fout, const float* dww, const float* dwb, float* Y_out, float* R_after, int32_t* report) {
    MIS_API_BEGIN
    if (report) report[0] = -1;
    MIS_REQUIRE(X && W && Y_out && batch >= 1 && Tp >= 1 && rowmul >= 1 && K >= 1 && N >= 1 && ldy >= N, MIS_ERR_INVALID_INPUT,
                "Sortformer GEMM: X, W, Y_out, positive batch, Tp, rowmul, K, N and ldy >= N are required");
    MIS_REQUIRE(load >= SF_LOAD_ACT && load <= SF_LOAD_DW && act >= SF_ACT_NONE && act <= SF_ACT_SIGMOID, MIS_ERR_INVALID_INPUT, "Sortformer GEMM: load 0..3, act 0..3");
    const int64_t rows = (int64_t)batch * Tp * rowmul;
    MIS_REQUIRE(rows * ldy <= SFD_MAX_ELEMS && (int64_t)N * K <= SFD_MAX_ELEMS && batch <= 65535 && cdiv(N, 64) <= 65535, MIS_ERR_INVALID_INPUT,
                "Sortformer GEMM: tensor too large");
    MIS_REQUIRE(load != SF_LOAD_LN || (stats && lnw && lnb), MIS_ERR_INVALID_INPUT, "Sortformer GEMM: the LayerNorm load needs stats, lnw and lnb");
    MIS_REQUIRE(!in_place || R, MIS_ERR_INVALID_INPUT, "Sortformer GEMM: in_place needs R");
    MIS_REQUIRE(!R || in_place || ldr >= N, MIS_ERR_INVALID_INPUT, "Sortformer GEMM: ldr >= N");
    size_t nx;
    if (load == SF_LOAD_DW) {
        MIS_REQUIRE(cnt_in && dww && dwb && Tin >= 1 && Fin >= 1 && Fout >= 1 && (int64_t)batch * Tin * Fin * K <= SFD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                    "Sortformer GEMM: the depthwise load needs cnt_in, dww, dwb and positive Tin, Fin, Fout");
        nx = (size_t)batch * Tin * Fin * K;
    } else {
        MIS_REQUIRE(ldx >= K && (rows - 1) * ldx + K <= SFD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Sortformer GEMM: ldx >= K");
        nx = (size_t)(rows - 1) * ldx + K;
    }
    HIP_CHECK(hipSetDevice(device));
    SfdCtx c;
    DevBuf<uint32_t> dX, dW, dB, dcnt, dst, dlw, dlb, dR, dpos, dcin, ddw, ddb;
    sfd_f32(dX, X, nx);
    sfd_f32(dW, W, (size_t)N * K);
    if (bias) sfd_f32(dB, bias, N);
    if (cnt) sfd_counts(dcnt, cnt, batch);
    if (load == SF_LOAD_LN) { sfd_f32(dst, stats, (size_t)rows * 2); sfd_f32(dlw, lnw, K); sfd_f32(dlb, lnb, K); }
    if (load == SF_LOAD_DW) { sfd_counts(dcin, cnt_in, batch); sfd_f32(ddw, dww, (size_t)9 * K); sfd_f32(ddb, dwb, K); }
    if (pos) sfd_f32(dpos, pos, (size_t)Tp * N);
    const bool sep = R && !in_place;
    const size_t nr = sep ? (size_t)(rows - 1) * ldr + N : 0;
    if (sep) sfd_f32(dR, R, nr);
    GuardedOut o;
    o.alloc((size_t)rows * ldy * 4, (size_t)64 * ldy * 4);         // a guard is one 64-row tile of output
    if (in_place) sfd_put_rows(o, rows, ldy, N, R);
    SfGemm p{};
    p.X = sfd_fp(dX); p.ldx = ldx; p.W = sfd_fp(dW); p.bias = bias ? sfd_fp(dB) : nullptr; p.Y = sfd_out(o); p.ldy = ldy;
    p.cnt = cnt ? sfd_ip(dcnt) : nullptr; p.Tp = Tp; p.rowmul = rowmul; p.K = K; p.N = N; p.load = load; p.act = act;
    if (load == SF_LOAD_LN) { p.stats = sfd_fp(dst); p.lnw = sfd_fp(dlw); p.lnb = sfd_fp(dlb); }
    if (in_place) { p.R = sfd_out(o); p.ldr = ldy; p.ra = ra; }
    else if (sep) { p.R = sfd_fp(dR); p.ldr = ldr; p.ra = ra; }
    p.pos = pos ? sfd_fp(dpos) : nullptr;
    if (load == SF_LOAD_DW) { p.cnt_in = sfd_ip(dcin); p.Tin = Tin; p.Fin = Fin; p.Fout = Fout; p.dww = sfd_fp(ddw); p.dwb = sfd_fp(ddb); }
    sf_gemm(&c, p, batch);
    sfd_sync(c);
    if (report) report[0] = load;
    sfd_fetch_rows(o, rows, ldy, N, Y_out);
    if (sep && R_after) HIP_CHECK(hipMemcpy(R_after, dR.p, nr * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_sortformer_attn(int device, int rel, const float* qkv, int ld, int koff, int voff, const int32_t* cnt, int batch, int Tp,
                                                int heads, int hd, float qscale, float sdk, const float* u, const float* v, const float* P, int ldp, int Tcap,
                                                int ldo, float* out, int32_t* report) {
    MIS_API_BEGIN
    if (report) { report[0] = -1; report[1] = -1; }
    MIS_REQUIRE(qkv && cnt && out && batch >= 1 && Tp >= 1 && heads >= 1 && hd >= 1 && hd <= 64, MIS_ERR_INVALID_INPUT,
                "Sortformer attention: qkv, cnt, out, positive batch, Tp, heads and a head size of 1..64 (the LDS tiles) are required");
    const int64_t width = (int64_t)heads * hd;
    MIS_REQUIRE(koff >= 0 && voff >= 0 && width <= ld && koff + width <= ld && voff + width <= ld && width <= ldo, MIS_ERR_INVALID_INPUT,
                "Sortformer attention: q, k and v must lie inside a row of ld columns, the output inside ldo");
    MIS_REQUIRE((int64_t)batch * Tp * ld <= SFD_MAX_ELEMS && (int64_t)batch * Tp * ldo <= SFD_MAX_ELEMS && batch <= 65535 && heads <= 65535, MIS_ERR_INVALID_INPUT,
                "Sortformer attention: tensor too large");
    MIS_REQUIRE(!rel || (u && v && P && Tcap >= 1 && ldp >= width && (int64_t)(2 * (int64_t)Tcap - 1) * ldp <= SFD_MAX_ELEMS), MIS_ERR_INVALID_INPUT,
                "Sortformer attention: relative positions need u, v, P, Tcap >= 1 and ldp >= heads hd");
    HIP_CHECK(hipSetDevice(device));
    SfdCtx c;
    const size_t rows = (size_t)batch * Tp;
    DevBuf<uint32_t> dq, dcnt, du, dv, dP;
    sfd_f32(dq, qkv, rows * ld);
    sfd_counts(dcnt, cnt, batch);
    if (rel) { sfd_f32(du, u, width); sfd_f32(dv, v, width); sfd_f32(dP, P, (size_t)(2 * Tcap - 1) * ldp); }
    GuardedOut o;
    o.alloc(rows * ldo * 4, (size_t)64 * ldo * 4);
    SfAttn p{sfd_fp(dq), ld, koff, voff, sfd_out(o), ldo, sfd_ip(dcnt), Tp, hd, qscale, sdk, rel ? sfd_fp(du) : nullptr, rel ? sfd_fp(dv) : nullptr,
             rel ? sfd_fp(dP) : nullptr, rel ? ldp : 0, rel ? Tcap : 0};
    if (rel) sf_attn<true>(&c, p, heads, hd, batch);
    else sf_attn<false>(&c, p, heads, hd, batch);
    sfd_sync(c);
    if (report) { report[0] = hd <= 32 ? 1 : 2; report[1] = rel ? 1 : 0; }
    sfd_fetch_rows(o, rows, ldo, width, out);
    MIS_API_END
}

extern "C" mis_status mis_debug_sortformer_conv0(int device, const float* feats, const int32_t* F, const int32_t* T1, const float* w, const float* bias, int batch,
                                                 int Fp, int mels, int T1p, int F1, int C, float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(feats && F && T1 && w && bias && out && batch >= 1 && Fp >= 1 && mels >= 1 && T1p >= 1 && F1 >= 1 && C >= 1, MIS_ERR_INVALID_INPUT,
                "Sortformer conv0: every pointer and positive batch, Fp, mels, T1p, F1, C are required");
    const int64_t n = (int64_t)batch * T1p * F1 * C;
    MIS_REQUIRE(n <= SFD_MAX_ELEMS && (int64_t)batch * Fp * mels <= SFD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Sortformer conv0: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    SfdCtx c;
    DevBuf<uint32_t> df, dF, dT, dw, db;
    sfd_f32(df, feats, (size_t)batch * Fp * mels);
    sfd_counts(dF, F, batch);
    sfd_counts(dT, T1, batch);
    sfd_f32(dw, w, (size_t)9 * C);
    sfd_f32(db, bias, C);
    GuardedOut o;
    o.alloc((size_t)n * 4, (size_t)F1 * C * 4);
    MIS_LAUNCH(&c, k_sf_conv0, dim3((unsigned)((n + 255) / 256)), dim3(256), sfd_fp(df), sfd_ip(dF), sfd_ip(dT), sfd_fp(dw), sfd_fp(db), sfd_out(o), Fp, mels, T1p, F1,
              C, (size_t)n);
    sfd_sync(c);
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_sortformer_stats(int device, const float* x, int M, int d, float eps, float* stats_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(x && stats_out && M >= 1 && d >= 1 && (int64_t)M * d <= SFD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "Sortformer stats: x, stats_out and positive M, d are required");
    HIP_CHECK(hipSetDevice(device));
    SfdCtx c;
    DevBuf<uint32_t> dx;
    sfd_f32(dx, x, (size_t)M * d);
    GuardedOut o;
    o.alloc((size_t)M * 2 * 4, 256);
    MIS_LAUNCH(&c, k_sf_stats, dim3(cdiv(M, 4)), dim3(256), sfd_fp(dx), sfd_out(o), d, eps, M);
    sfd_sync(c);
    o.check_guards();
    HIP_CHECK(hipMemcpy(stats_out, o.p(), o.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_sortformer_ln(int device, const float* x, const float* w, const float* b, int M, int d, float eps, const int32_t* cnt, int Tp,
                                              int in_place, float* y_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(x && w && b && cnt && y_out && M >= 1 && d >= 1 && Tp >= 1 && (int64_t)M * d <= SFD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "Sortformer LayerNorm: x, w, b, cnt, y_out and positive M, d, Tp are required");
    HIP_CHECK(hipSetDevice(device));
    SfdCtx c;
    DevBuf<uint32_t> dx, dw, db, dcnt;
    if (!in_place) sfd_f32(dx, x, (size_t)M * d);
    sfd_f32(dw, w, d);
    sfd_f32(db, b, d);
    sfd_counts(dcnt, cnt, (size_t)cdiv(M, Tp));
    GuardedOut y;
    y.alloc((size_t)M * d * 4, (size_t)4 * d * 4);
    if (in_place) HIP_CHECK(hipMemcpy(y.p(), x, y.body, hipMemcpyHostToDevice));
    MIS_LAUNCH(&c, k_sf_ln, dim3(cdiv(M, 4)), dim3(256), in_place ? sfd_out(y) : sfd_fp(dx), sfd_out(y), sfd_fp(dw), sfd_fp(db), d, eps, M, sfd_ip(dcnt), Tp);
    sfd_sync(c);
    y.check_guards();
    HIP_CHECK(hipMemcpy(y_out, y.p(), y.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_sortformer_intake(int device, const float* x, const int32_t* cnt, int batch, int Tp, int d, float g, float* y_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(x && cnt && y_out && batch >= 1 && Tp >= 1 && d >= 1 && (int64_t)batch * Tp * d <= SFD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "Sortformer intake: x, cnt, y_out and positive batch, Tp, d are required");
    HIP_CHECK(hipSetDevice(device));
    SfdCtx c;
    const size_t n = (size_t)batch * Tp * d;
    DevBuf<uint32_t> dx, dcnt;
    sfd_f32(dx, x, n);
    sfd_counts(dcnt, cnt, batch);
    GuardedOut o;
    o.alloc(n * 4, (size_t)d * 4);
    MIS_LAUNCH(&c, k_sf_intake, dim3((unsigned)((n + 255) / 256)), dim3(256), sfd_fp(dx), sfd_out(o), sfd_ip(dcnt), Tp, d, g, n);
    sfd_sync(c);
    o.check_guards();
    HIP_CHECK(hipMemcpy(y_out, o.p(), o.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_sortformer_glu_dwconv(int device, const float* pw, const float* taps, const float* shift, const int32_t* cnt, int batch, int Tp,
                                                      int C, int k, float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(pw && taps && shift && cnt && out && batch >= 1 && Tp >= 1 && C >= 1, MIS_ERR_INVALID_INPUT,
                "Sortformer GLU + depthwise conv: every pointer and positive batch, Tp, C are required");
    MIS_REQUIRE(k >= 1 && k <= SF_DW_MAXK, MIS_ERR_INVALID_INPUT, "Sortformer GLU + depthwise conv: k %d outside 1..%d (the LDS tile)", k, SF_DW_MAXK);
    MIS_REQUIRE((int64_t)batch * Tp * 2 * C <= SFD_MAX_ELEMS && batch <= 65535 && cdiv(C, 64) <= 65535, MIS_ERR_INVALID_INPUT,
                "Sortformer GLU + depthwise conv: tensor too large");
    HIP_CHECK(hipSetDevice(device));
    SfdCtx c;
    const size_t rows = (size_t)batch * Tp;
    DevBuf<uint32_t> dp, dt, ds, dcnt;
    sfd_f32(dp, pw, rows * 2 * C);
    sfd_f32(dt, taps, (size_t)k * C);
    sfd_f32(ds, shift, C);
    sfd_counts(dcnt, cnt, batch);
    GuardedOut o;
    o.alloc(rows * C * 4, (size_t)SF_DW_TT * C * 4);
    MIS_LAUNCH(&c, k_sf_glu_dwconv, dim3(cdiv(Tp, SF_DW_TT), cdiv(C, 64), batch), dim3(256), sfd_fp(dp), sfd_fp(dt), sfd_fp(ds), sfd_ip(dcnt), sfd_out(o), Tp, C, k);
    sfd_sync(c);
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_sortformer_peak(int device, const float* pcm, int64_t stride, const int32_t* N, int batch, int on, float* scale_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(pcm && N && scale_out && batch >= 1 && stride >= 1 && batch * stride <= SFD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "Sortformer peak: pcm, N, scale_out and positive batch, stride are required");
    for (int b = 0; b < batch; ++b)
        MIS_REQUIRE(N[b] <= stride, MIS_ERR_INVALID_INPUT, "Sortformer peak: row %d: %d samples exceed the row stride %lld", b, N[b], (long long)stride);
    HIP_CHECK(hipSetDevice(device));
    SfdCtx c;
    DevBuf<uint32_t> dx, dn;
    sfd_f32(dx, pcm, (size_t)batch * stride);
    sfd_counts(dn, N, batch);
    GuardedOut o;
    o.alloc((size_t)batch * 4, 256);
    MIS_LAUNCH(&c, k_sf_peak, dim3(batch), dim3(256), sfd_fp(dx), stride, sfd_ip(dn), on, sfd_out(o));
    sfd_sync(c);
    o.check_guards();
    HIP_CHECK(hipMemcpy(scale_out, o.p(), o.body, hipMemcpyDeviceToHost));
    MIS_API_END
}
