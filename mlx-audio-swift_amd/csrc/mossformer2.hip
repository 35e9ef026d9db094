// mossformer2.hip - MossFormer2-SE speech enhancement: waveform -> Kaldi-style fbank + deltas -> MossFormer mask network -> mask on the
// row's STFT -> inverse STFT and overlap-add.  Exact f32 throughout, as the reference runs it.
//
// Reference being replaced: MossFormer2SEModel.enhance (Sources/MLXAudioSTS/Models/MossFormer2SE/MossFormer2Model.swift:395-470),
// MossFormerMaskNet (:76-199), the layers of MossFormer2Layers.swift and MossFormer2DSP.swift (computeFbankKaldi, computeDeltasKaldi,
// stft, istft).
//
// One call serves 1..max_batch ragged rows.  Row b has n_b samples and T_b = n_b < win_len ? 0 : 1 + (n_b - win_len) / win_inc frames;
// every activation is f32 [B][nr][C] with nr the call's longest row, a row's own frames first and zeros behind them.  Every output
// element is one fixed-order sum over data of its own row, so a row's result is bit for bit the same whatever batch it travels in.
//
//   k_mf2_fbank    one frame per block: x 32768, minus the frame mean, pre-emphasis (first sample x0 - c x0), window, power-of-two FFT of
//                  up to 2048 points in LDS, power, the Hz triangles (Nyquist bin included), log max(., 1e-10)
//   k_mf2_deltas   [fbank | delta | delta-delta], the 5-tap filter with edge padding written as k / 10 (x[t + k] - x[t - k])
//   k_mf2_gln      GlobalLayerNorm over a row's [T, C]: one block a row, mean then variance, each one fixed-order sum
//   k_mf2_row      a wave per frame: ScaleNorm's scale (with the token shift), CLayerNorm (+ the statistics of the LayerNorm that follows),
//                  or the tail LayerNorm o LayerNorm + skip + PReLU
//   k_mf2_gemm     the one contraction, exact f32 on v_mfma_f32_32x32x2_f32, 64 x 64 tile, every dimension guarded.  Loads: activations,
//                  token shift, LayerNorm, the product of the two gate halves, windowed frames of the waveform, spectrum x mask.  Epilogue: row scale,
//                  bias, SiLU / ReLU / PReLU / tanh | sigmoid, column scale, residual, positional table (on f32_tile.h)
//   k_mf2_dwconv   y + depthwise(y) from a time tile + halo in LDS, 17 taps (FFConvM; the qk channels go on through OffsetScale and
//                  RoPE; to_out adds the layer's input) or 39 (UniDeepFsmn, fused with the gate xv (.) + residual)
//   k_mf2_linkv    linK^T [V | U] of one group of 256 frames: the linear attention's partials (its own transposed staging)
//   k_mf2_linsum   the partials summed once in group order, / n
//   k_mf2_attn     relu(Q K^T / 256)^2 [V | U] inside the group + linQ x that sum, then the gate
//   k_mf2_ola      overlap-add as a gather, / max(sum w^2, 1e-8), / 32768
//
// Launches: enhance 11 + 18 num_blocks; mask 8 + 18 num_blocks; mask_features 6 + 18 num_blocks; features 2; synthesize 3.
#include "common.h"
#include "audio_front.h"
#include "f32_tile.h"
#include "host_weights.h"
#include "step_loop.h"

#include <math.h>
#include <string.h>
#include <memory>

#define MF_MAX_BATCH 64
#define MF_GROUP 256              // constants of the reference: group size, query / key width, FSMN inner width, lorder, taps
#define MF_QK 128
#define MF_INNER 256
#define MF_ROPE 32
#define MF_FF_TAPS 17
#define MF_FSMN_TAPS 39
#define MF_MAX_NFFT 2048

enum { MF_LOAD_ACT = 0, MF_LOAD_SHIFT, MF_LOAD_LN, MF_LOAD_GATE, MF_LOAD_FRAME, MF_LOAD_MASKED };
enum { MF_ACT_NONE = 0, MF_ACT_SILU, MF_ACT_RELU, MF_ACT_PRELU, MF_ACT_TANH_SIGMOID };
enum { MF_ROW_SCALE = 0, MF_ROW_CLN, MF_ROW_TAIL };
enum { MF_DW_FF = 0, MF_DW_FSMN };

__device__ __forceinline__ float mf_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---------------------------------------------------------------------------- front end
struct MfFront {
    const float* pcm; int64_t pcm_stride;
    const float *win, *twc, *tws, *fb; const int32_t* fbr;  // window [wlen], twiddles [1024], filters [nfft / 2 + 1][nm], bin ranges
    float* fbank; const int32_t* cnt;
    int nr, wlen, hop, nm, nfft, log2n; float preemph, log_floor;
};

__global__ void __launch_bounds__(256) k_mf2_fbank(MfFront p) {
    __shared__ float re[MF_MAX_NFFT], im[MF_MAX_NFFT], red[4];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, N = p.nfft;
    float* o = p.fbank + ((size_t)b * p.nr + f) * p.nm;
    if (f >= p.cnt[b]) {
        for (int m = tid; m < p.nm; m += 256) o[m] = 0.0f;
        return;
    }
    const float* x = p.pcm + (size_t)b * p.pcm_stride + (size_t)f * p.hop;
    float part = 0.0f;
    for (int j = tid; j < p.wlen; j += 256) part += x[j] * 32768.0f;
    const float mean = block_sum_256(part, red) / (float)p.wlen;
    for (int j = tid; j < N; j += 256) im[j] = j < p.wlen ? x[j] * 32768.0f - mean : 0.0f;
    __syncthreads();
    for (int j = tid; j < N; j += 256) {
        float y = 0.0f;
        if (j < p.wlen && j < N) {
            y = __fsub_rn(im[j], __fmul_rn(p.preemph, im[j == 0 ? 0 : j - 1]));
            y = __fmul_rn(y, p.win[j]);
        }
        re[__brev((unsigned)j) >> (32 - p.log2n)] = y;
    }
    __syncthreads();
    for (int j = tid; j < N; j += 256) im[j] = 0.0f;
    __syncthreads();
    const int tstride = MF_MAX_NFFT / N;
    for (int half = 1; half < N; half <<= 1) {
        for (int q = tid; q < N / 2; q += 256) {
            const int k = q & (half - 1), i0 = ((q - k) << 1) + k, i1 = i0 + half, ti = k * (N / 2 / half) * tstride;
            const float c = p.twc[ti], s = p.tws[ti];
            const float xr = re[i1], xi = im[i1];
            const float pr = xr * c - xi * s, pi = xr * s + xi * c;
            const float ar = re[i0], ai = im[i0];
            re[i0] = ar + pr; im[i0] = ai + pi; re[i1] = ar - pr; im[i1] = ai - pi;
        }
        __syncthreads();
    }
    for (int j = tid; j <= N / 2; j += 256) { const float a = re[j], c = im[j]; re[j] = a * a + c * c; }
    __syncthreads();
    for (int m = tid; m < p.nm; m += 256) {
        float acc = 0.0f;
        for (int i = p.fbr[2 * m]; i < p.fbr[2 * m + 1]; ++i) acc = fmaf(re[i], p.fb[(size_t)i * p.nm + m], acc);
        o[m] = acc > 1e-10f ? logf(acc) : p.log_floor;
    }
}

__device__ __forceinline__ float mf_delta(const float* fb, int nm, int m, int t, int T) {
    float a = 0.0f;
#pragma unroll
    for (int k = 1; k <= 2; ++k) {
        const float hi = fb[(size_t)min(t + k, T - 1) * nm + m], lo = fb[(size_t)max(t - k, 0) * nm + m];
        a = fmaf((float)k / 10.0f, hi - lo, a);
    }
    return a;
}

// feat[b][t][.] = fbank | delta | delta-delta; delta-delta reads the deltas at the clamped frames (edge padding of the deltas)
__global__ void __launch_bounds__(256) k_mf2_deltas(const float* __restrict__ fbank, float* __restrict__ feat, const int32_t* cnt, int nr,
                                                    int nm, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int m = (int)(i % nm);
    const size_t r = i / nm;
    const int t = (int)(r % nr), b = (int)(r / nr), T = cnt[b];
    float* o = feat + r * 3 * nm;
    if (t >= T) { o[m] = 0.0f; o[nm + m] = 0.0f; o[2 * nm + m] = 0.0f; return; }
    const float* fb = fbank + (size_t)b * nr * nm;
    o[m] = fb[(size_t)t * nm + m];
    o[nm + m] = mf_delta(fb, nm, m, t, T);
    float a = 0.0f;
#pragma unroll
    for (int k = 1; k <= 2; ++k)
        a = fmaf((float)k / 10.0f, mf_delta(fb, nm, m, min(t + k, T - 1), T) - mf_delta(fb, nm, m, max(t - k, 0), T), a);
    o[2 * nm + m] = a;
}

// GlobalLayerNorm over the row's T_b x C values (eps 1e-8): mean, then the mean of the squared distances, each a fixed-order sum
__global__ void __launch_bounds__(256) k_mf2_gln(const float* __restrict__ X, float* __restrict__ Y, const float* __restrict__ w,
                                                 const float* __restrict__ bias, const int32_t* cnt, int nr, int C) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t n = (size_t)cnt[b] * C, all = (size_t)nr * C;
    const float* x = X + (size_t)b * all;
    float* y = Y + (size_t)b * all;
    float s = 0.0f;
    for (size_t i = tid; i < n; i += 256) s += x[i];
    const float mean = block_sum_256(s, red) / (float)(n ? n : 1);
    float q = 0.0f;
    for (size_t i = tid; i < n; i += 256) { const float d = x[i] - mean; q = fmaf(d, d, q); }
    const float var = block_sum_256(q, red) / (float)(n ? n : 1);
    const float den = sqrtf(var + 1e-8f);
    for (size_t i = tid; i < all; i += 256) {
        const int c = (int)(i % C);
        y[i] = i < n ? fmaf(w[c], (x[i] - mean) / den, bias[c]) : 0.0f;
    }
}

// ---------------------------------------------------------------------------- a wave per frame
struct MfRow {
    const float* X; int ldx; float* Y; int ldy; float* stats;      // stats [B nr][2]
    const float *w1, *b1, *w2, *b2, *R, *slope; int ldr;
    const int32_t* cnt; int nr, C, mode, half; float eps, eps_next;
};

__global__ void __launch_bounds__(256) k_mf2_row(MfRow p) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (t >= p.nr) return;
    const int T = p.cnt[b], C = p.C;
    const size_t row = (size_t)b * p.nr + t;
    const float* x = p.X + row * p.ldx;
    if (p.mode == MF_ROW_SCALE) {                                     // 1 / max(|x| C^-1/2, 1e-8) of the (shifted) frame
        float q = 0.0f;
        if (t < T)
            for (int c = lane; c < C; c += 64) {
                float v = x[c];
                if (c < p.half && T > 1) v = t > 0 ? x[c - (ptrdiff_t)p.ldx] : 0.0f;
                q = fmaf(v, v, q);
            }
        q = wave_sum(q);
        if (lane == 0) { p.stats[2 * row] = t < T ? 1.0f / fmaxf(sqrtf(q) * (1.0f / sqrtf((float)C)), 1e-8f) : 0.0f; p.stats[2 * row + 1] = 0.0f; }
        return;
    }
    float* y = p.Y + row * p.ldy;
    if (t >= T) {
        for (int c = lane; c < C; c += 64) y[c] = 0.0f;
        if (p.stats && lane == 0) { p.stats[2 * row] = 0.0f; p.stats[2 * row + 1] = 0.0f; }
        return;
    }
    float mean, rstd, m2, r2;
    wave_mean_rstd(x, C, p.eps, mean, rstd);
    const auto ln1 = [&](int c) { return fmaf((x[c] - mean) * rstd, p.w1[c], p.b1[c]); };
    if (p.mode == MF_ROW_CLN) {
        float s2 = 0.0f;                                            // (the sum rides on the pass that writes y: not wave_mean_rstd)
        for (int c = lane; c < C; c += 64) { const float v = ln1(c); y[c] = v; s2 += v; }
        if (!p.stats) return;
        m2 = wave_sum(s2) / (float)C;                                // the LayerNorm in front of to_u / to_v reads these
        float q2 = 0.0f;
        for (int c = lane; c < C; c += 64) { const float d = ln1(c) - m2; q2 = fmaf(d, d, q2); }
        q2 = wave_sum(q2);
        if (lane == 0) { p.stats[2 * row] = m2; p.stats[2 * row + 1] = 1.0f / sqrtf(q2 / (float)C + p.eps_next); }
        return;
    }
    // tail: LayerNorm (intra_mdl.norm), LayerNorm (intra_norm), + the network's input, PReLU
    wave_mean_rstd_of(ln1, C, p.eps, m2, r2);
    const float a = p.slope[0];
    for (int c = lane; c < C; c += 64) {
        const float v = fmaf((ln1(c) - m2) * r2, p.w2[c], p.b2[c]) + p.R[row * p.ldr + c];
        y[c] = fmaxf(v, 0.0f) + a * fminf(v, 0.0f);
    }
}

// ---------------------------------------------------------------------------- the contraction
struct MfGemm {
    const float* X; int ldx;
    const float* W; int ldw; const float* bias;
    float* Y; int ldy;
    const int32_t* cnt; int nr, Cin, Cout, load, act;
    const float* stats;                                     // LN load: mean, rstd; row scale epilogue: the scale
    int half;                                               // SHIFT: channels below it come from the frame before
    const float* pcm; int64_t pcm_stride; int hop; const float* win;   // FRAME
    const float* M; int ldm, F;                             // MASKED: X [.][2 F] x M [.][F]
    const float *g0, *g1; int gsplit;                       // row scale: stats[row][0] x (co < gsplit ? g0[0] : g1[0]); g0 null: none
                                                            // (TANH_SIGMOID: tanh below gsplit, sigmoid from it on)
    const float* slope;                                     // PReLU
    const float* cscale;                                    // column scale (after the activation)
    const float* R; int ldr;                                // residual
    const float* pos;                                       // [nr][Cout] added last
};

__device__ __forceinline__ float mf_load(const MfGemm& p, int b, size_t row, int t, int T, int ci) {
    switch (p.load) {
        case MF_LOAD_SHIFT:
            if (ci < p.half && T > 1) return t > 0 ? p.X[(row - 1) * p.ldx + ci] : 0.0f;
            return p.X[row * p.ldx + ci];
        case MF_LOAD_LN: return (p.X[row * p.ldx + ci] - p.stats[2 * row]) * p.stats[2 * row + 1];
        case MF_LOAD_GATE: return p.X[row * p.ldx + ci] * p.X[row * p.ldx + p.Cin + ci];
        case MF_LOAD_FRAME: return __fmul_rn(__fmul_rn(p.pcm[(size_t)b * p.pcm_stride + (size_t)t * p.hop + ci], 32768.0f), p.win[ci]);
        case MF_LOAD_MASKED: return p.X[row * p.ldx + ci] * p.M[row * p.ldm + (ci >= p.F ? ci - p.F : ci)];
        default: return p.X[row * p.ldx + ci];
    }
}

__global__ void __launch_bounds__(256) k_mf2_gemm(MfGemm p) {
    constexpr int TT = F32_TILE, TC = F32_TILE;
    __shared__ float As[TT][F32_KC + 1];
    __shared__ float Bs[TC][F32_KC + 1];
    const int b = blockIdx.z, t0 = blockIdx.x * TT, c0 = blockIdx.y * TC, nr = p.nr;
    const int T = min(p.cnt[b], nr), tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t row0 = (size_t)b * nr;
    if (t0 >= T) { f32_tile_zero<TT, TC>(p.Y, p.ldy, row0, t0, c0, nr, p.Cout); return; }
    f32x16_t acc[1] = {};
    const int wt = (wave & 1) * 32, wc = (wave >> 1) * 32, kh = lane >> 5, l31 = lane & 31;
    for (int ci0 = 0; ci0 < p.Cin; ci0 += F32_KC) {
#pragma unroll
        for (int n = 0; n < TT * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, ci = ci0 + (i & 31), t = t0 + r;
            As[r][i & 31] = (ci < p.Cin && t < T) ? mf_load(p, b, row0 + t, t, T, ci) : 0.0f;
        }
#pragma unroll
        for (int n = 0; n < TC * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, ci = ci0 + (i & 31), co = c0 + r;
            Bs[r][i & 31] = (co < p.Cout && ci < p.Cin) ? p.W[(size_t)co * p.ldw + ci] : 0.0f;
        }
        __syncthreads();
        f32_tile_mfma(As, Bs, wt + l31, wc + l31, kh, acc);
        __syncthreads();
    }
    const int co = c0 + wc + l31;                                   // C/D: column = lane & 31, row = f32_tile_row(r, lane >> 5)
    if (co >= p.Cout) return;
    const float add = p.bias ? p.bias[co] : 0.0f;
    const float g = p.g0 ? (co < p.gsplit ? p.g0[0] : p.g1[0]) : 1.0f;
    const float cs = p.cscale ? p.cscale[co] : 1.0f;
    const float slope = p.act == MF_ACT_PRELU ? p.slope[0] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = t0 + wt + f32_tile_row(r, kh);
        if (t >= nr) continue;
        const size_t row = row0 + t;
        float v = acc[0][r];
        if (t < T) {
            if (p.g0) v *= p.stats[2 * row] * g;
            v += add;
            if (p.act == MF_ACT_SILU) v = v * mf_sigmoid(v);
            else if (p.act == MF_ACT_RELU) v = fmaxf(v, 0.0f);
            else if (p.act == MF_ACT_PRELU) v = fmaxf(v, 0.0f) + slope * fminf(v, 0.0f);
            else if (p.act == MF_ACT_TANH_SIGMOID) v = co < p.gsplit ? tanhf(v) : mf_sigmoid(v);
            if (p.cscale) v *= cs;
            if (p.R) v += p.R[row * p.ldr + co];
            if (p.pos) v += p.pos[(size_t)t * p.Cout + co];
        } else v = 0.0f;
        p.Y[row * p.ldy + co] = v;
    }
}

// ---------------------------------------------------------------------------- depthwise + residual
struct MfDw {
    const float* X; int ldx, xoff;                           // the conv's input: channels xoff .. xoff + C of X
    const float* dw; int K;                                 // [C][K]
    float* Y; int ldy;                                      // FF: channels < Cmain; FSMN: all
    int C, Cmain, mode;
    float* qk4; const float *gamma, *beta, *rc, *rs;        // FF, channels >= Cmain: [.][4][128]; gamma / beta [4][128]; RoPE tables [nr][16]
    const float* R; int ldr;                                // FF: added to the main channels (null: none)
    const float *U; int ldu, uoff; const float* V; int ldv, voff; const float* N; int ldn;   // FSMN: xv (p + conv(p) + xu) + n
    const int32_t* cnt; int nr;
};

__global__ void __launch_bounds__(256) k_mf2_dwconv(MfDw p) {
    constexpr int TT = 32, CC = 64;
    __shared__ float Hs[TT + MF_FSMN_TAPS - 1][CC];
    __shared__ float Ws[CC][MF_FSMN_TAPS + 1];
    __shared__ float Ys[TT][CC + 1];
    const int b = blockIdx.z, t0 = blockIdx.x * TT, c0 = blockIdx.y * CC, tid = threadIdx.x, nr = p.nr, K = p.K, pad = (K - 1) / 2;
    const int T = min(p.cnt[b], nr);
    const size_t row0 = (size_t)b * nr;
    const bool qk = p.mode == MF_DW_FF && c0 >= p.Cmain;
    if (t0 >= T) {
        for (int i = tid; i < TT * CC; i += 256) {
            const int t = t0 + i / CC, c = c0 + i % CC;
            if (t >= nr || c >= p.C) continue;
            if (qk) { for (int h = 0; h < 4; ++h) p.qk4[((row0 + t) * 4 + h) * MF_QK + (c - p.Cmain)] = 0.0f; }
            else p.Y[(row0 + t) * p.ldy + c] = 0.0f;
        }
        return;
    }
    for (int i = tid; i < (TT + K - 1) * CC; i += 256) {
        const int h = i / CC, c = c0 + i % CC, t = t0 - pad + h;
        Hs[h][i % CC] = (c < p.C && t >= 0 && t < T) ? p.X[(row0 + t) * p.ldx + p.xoff + c] : 0.0f;
    }
    for (int i = tid; i < CC * K; i += 256) {
        const int c = i / K, j = i - c * K;
        Ws[c][j] = c0 + c < p.C ? p.dw[(size_t)(c0 + c) * K + j] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < TT * CC / 256; ++n) {                        // x[t] + sum_j w[j] x[t + j - pad], taps ascending
        const int i = tid + n * 256, r = i / CC, cc = i % CC;
        float a = 0.0f;
        for (int j = 0; j < K; ++j) a = fmaf(Ws[cc][j], Hs[r + j][cc], a);
        Ys[r][cc] = Hs[r + pad][cc] + a;
    }
    __syncthreads();
    if (qk) {                                                         // OffsetScale into four heads, RoPE on the first 32 dims (pairs 2 i, 2 i + 1)
        for (int i = tid; i < TT * (CC / 2) * 4; i += 256) {
            const int pr = i % (CC / 2), h = (i / (CC / 2)) & 3, r = i / (CC / 2 * 4), t = t0 + r;
            if (t >= nr) continue;
            const int d = c0 - p.Cmain + 2 * pr;
            float a = fmaf(Ys[r][2 * pr], p.gamma[h * MF_QK + d], p.beta[h * MF_QK + d]);
            float c = fmaf(Ys[r][2 * pr + 1], p.gamma[h * MF_QK + d + 1], p.beta[h * MF_QK + d + 1]);
            if (d < MF_ROPE) {
                const float cs = p.rc[(size_t)t * (MF_ROPE / 2) + d / 2], sn = p.rs[(size_t)t * (MF_ROPE / 2) + d / 2];
                const float ra = a * cs - c * sn, rb = a * sn + c * cs;
                a = ra; c = rb;
            }
            float* o = p.qk4 + ((row0 + t) * 4 + h) * MF_QK + d;
            o[0] = t < T ? a : 0.0f; o[1] = t < T ? c : 0.0f;
        }
        return;
    }
    for (int i = tid; i < TT * CC; i += 256) {
        const int r = i / CC, cc = i % CC, t = t0 + r, c = c0 + cc;
        if (t >= nr || c >= p.C) continue;
        const size_t row = row0 + t;
        float v = Ys[r][cc];
        if (p.mode == MF_DW_FSMN) v = fmaf(p.V[row * p.ldv + p.voff + c], v + p.U[row * p.ldu + p.uoff + c], p.N[row * p.ldn + c]);
        else if (p.R) v += p.R[row * p.ldr + c];
        p.Y[row * p.ldy + c] = t < T ? v : 0.0f;
    }
}

// ---------------------------------------------------------------------------- attention
// P[b][g][d][c] = sum over the frames t of group g (in order, t < T_b) of linK[t][d] vu[t][c]
struct MfLinKV { const float* qk4; const float* vu; float* P; const int32_t* cnt; int nr, G, N; };   // N = 4 dim, the width of vu

__global__ void __launch_bounds__(256) k_mf2_linkv(MfLinKV p) {
    __shared__ float As[F32_TILE][F32_KC + 1];
    __shared__ float Bs[F32_TILE][F32_KC + 1];
    const int g = blockIdx.z % p.G, b = blockIdx.z / p.G, d0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int T = min(p.cnt[b], p.nr), tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t row0 = (size_t)b * p.nr;
    const int ta = g * MF_GROUP, tb = min(T, ta + MF_GROUP);
    f32x16_t acc[1] = {};
    const int wd = (wave & 1) * 32, wc = (wave >> 1) * 32, kh = lane >> 5, l31 = lane & 31;
    for (int k0 = ta; k0 < tb; k0 += F32_KC) {                        // (frames are the K index here: both operands are staged transposed)
#pragma unroll
        for (int n = 0; n < F32_TILE * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i & 63, kk = i >> 6, t = k0 + kk;
            As[r][kk] = t < tb ? p.qk4[((row0 + t) * 4 + 3) * MF_QK + d0 + r] : 0.0f;
            Bs[r][kk] = (t < tb && c0 + r < p.N) ? p.vu[(row0 + t) * p.N + c0 + r] : 0.0f;
        }
        __syncthreads();
        f32_tile_mfma(As, Bs, wd + l31, wc + l31, kh, acc);
        __syncthreads();
    }
    const int c = c0 + wc + l31;
    if (c >= p.N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int d = d0 + wd + f32_tile_row(r, kh);
        p.P[(((size_t)b * p.G + g) * MF_QK + d) * p.N + c] = acc[0][r];
    }
}

// S[b][d][c] = (P[b][0][d][c] + P[b][1][d][c] + ...) / T_b over the row's live groups, in group order
__global__ void __launch_bounds__(256) k_mf2_linsum(const float* __restrict__ P, float* __restrict__ S, const int32_t* cnt, int nr, int G, int per_row) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= per_row) return;
    const int T = min(cnt[b], nr), Gr = (T + MF_GROUP - 1) / MF_GROUP;
    float s = 0.0f;
    for (int g = 0; g < Gr; ++g) s += P[((size_t)b * G + g) * per_row + i];
    S[(size_t)b * per_row + i] = T > 0 ? s / (float)T : 0.0f;
}

// out[t][c] = (attU[t][c] v[t][c]) sigmoid(attV[t][c] u[t][c]), att. = relu(quadQ quadK^T / 256)^2 [v | u] over the keys of t's group
// + linQ S[b] (k_mf2_linsum).  A block: 32 queries x 128 of the 2 dim columns (the v column and its u column together).
struct MfAttn { const float* qk4; const float* vu; const float* S; float* out; const int32_t* cnt; int nr, D2; };

__global__ void __launch_bounds__(256) k_mf2_attn(MfAttn p) {
    __shared__ float Ss[32][MF_GROUP + 1];
    __shared__ float Rb[5280];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 128, nr = p.nr, D2 = p.D2, N = 2 * D2;
    const int T = min(p.cnt[b], nr), tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kh = lane >> 5, l31 = lane & 31;
    const size_t row0 = (size_t)b * nr;
    if (t0 >= T) {
        for (int i = tid; i < 32 * 128; i += 256) {
            const int t = t0 + i / 128, c = c0 + i % 128;
            if (t < nr && c < D2) p.out[(row0 + t) * D2 + c] = 0.0f;
        }
        return;
    }
    const int k0 = (t0 / MF_GROUP) * MF_GROUP, nk = min(T - k0, MF_GROUP);        // the group's first key frame and its live keys
    // ---- scores, two halves of 128 keys
    {
        float (*Qs)[33] = reinterpret_cast<float (*)[33]>(Rb);
        float (*Ks)[33] = reinterpret_cast<float (*)[33]>(Rb + 32 * 33);
        for (int hk = 0; hk < 2; ++hk) {
            f32x16_t acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            for (int d0 = 0; d0 < MF_QK; d0 += 32) {
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int i = tid + n * 256, r = i >> 5, kk = i & 31, t = t0 + r;
                    Qs[r][kk] = t < T ? p.qk4[((row0 + t) * 4 + 0) * MF_QK + d0 + kk] : 0.0f;
                }
#pragma unroll
                for (int n = 0; n < 16; ++n) {
                    const int i = tid + n * 256, r = i >> 5, kk = i & 31, key = hk * 128 + r;
                    Ks[r][kk] = key < nk ? p.qk4[((row0 + k0 + key) * 4 + 2) * MF_QK + d0 + kk] : 0.0f;
                }
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < 32; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[l31][kk + kh], Ks[wave * 32 + l31][kk + kh], acc, 0, 0, 0);
                __syncthreads();
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = fmaxf(acc[r] * (1.0f / MF_GROUP), 0.0f);
                Ss[(r & 3) + 8 * (r >> 2) + 4 * kh][hk * 128 + wave * 32 + l31] = s * s;
            }
        }
    }
    __syncthreads();
    f32x16_t aV, aU;
#pragma unroll
    for (int r = 0; r < 16; ++r) { aV[r] = 0.0f; aU[r] = 0.0f; }
    float (*Vs)[17] = reinterpret_cast<float (*)[17]>(Rb);
    float (*Us)[17] = reinterpret_cast<float (*)[17]>(Rb + 128 * 17);
    float (*Ls)[17] = reinterpret_cast<float (*)[17]>(Rb + 256 * 17);
    // ---- scores x [v | u], the keys in slabs of 16
    for (int ks = 0; ks < nk; ks += 16) {
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int i = tid + n * 256, c = i & 127, kk = i >> 7, key = ks + kk, col = c0 + c;
            const bool ok = key < nk && col < D2;
            const size_t at = (row0 + k0 + key) * N + col;
            Vs[c][kk] = ok ? p.vu[at] : 0.0f;
            Us[c][kk] = ok ? p.vu[at + D2] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2) {
            const float a = Ss[l31][ks + kk + kh];
            aV = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Vs[wave * 32 + l31][kk + kh], aV, 0, 0, 0);
            aU = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Us[wave * 32 + l31][kk + kh], aU, 0, 0, 0);
        }
        __syncthreads();
    }
    // ---- linQ x S
    for (int d0 = 0; d0 < MF_QK; d0 += 16) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int i = tid + n * 256, r = i >> 4, kk = i & 15, t = t0 + r;
            Ls[r][kk] = t < T ? p.qk4[((row0 + t) * 4 + 1) * MF_QK + d0 + kk] : 0.0f;
        }
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int i = tid + n * 256, c = i & 127, kk = i >> 7, col = c0 + c;
            const size_t at = ((size_t)b * MF_QK + d0 + kk) * N + col;
            Vs[c][kk] = col < D2 ? p.S[at] : 0.0f; Us[c][kk] = col < D2 ? p.S[at + D2] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2) {
            const float a = Ls[l31][kk + kh];
            aV = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Vs[wave * 32 + l31][kk + kh], aV, 0, 0, 0);
            aU = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Us[wave * 32 + l31][kk + kh], aU, 0, 0, 0);
        }
        __syncthreads();
    }
    const int col = c0 + wave * 32 + l31;
    if (col >= D2) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (t >= nr) continue;
        float o = 0.0f;
        if (t < T) {
            const float v = p.vu[(row0 + t) * N + col], u = p.vu[(row0 + t) * N + D2 + col];
            o = (aU[r] * v) * mf_sigmoid(aV[r] * u);
        }
        p.out[(row0 + t) * D2 + col] = o;
    }
}

// ---------------------------------------------------------------------------- overlap-add
// out[b][s] = sum over the frames f covering s, in frame order, of fr[f][s - f hop], / max(sum w^2, 1e-8), / 32768
__global__ void __launch_bounds__(256) k_mf2_ola(const float* __restrict__ fr, const float* __restrict__ win, float* __restrict__ out,
                                                 const int32_t* cnt, int nr, int W, int hop, int64_t out_stride) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y, T = cnt[b];
    if (s >= out_stride) return;
    float v = 0.0f;
    if (T > 0 && s < (int64_t)(T - 1) * hop + W) {
        const int64_t lo = s - W + 1;
        const int fa = lo <= 0 ? 0 : (int)((lo + hop - 1) / hop), fb = s / hop > T - 1 ? T - 1 : (int)(s / hop);
        float acc = 0.0f, ws = 0.0f;
        for (int f = fa; f <= fb; ++f) {
            const int j = (int)(s - (int64_t)f * hop);
            acc += fr[((size_t)b * nr + f) * W + j];
            ws = fmaf(win[j], win[j], ws);
        }
        v = acc / fmaxf(ws, 1e-8f) / 32768.0f;
    }
    out[(size_t)b * out_stride + s] = v;
}

// ============================================================================ host
struct MfLin { const float *w, *b; int cin, cout; };
struct MfFlash { MfLin hq, out; const float *g_h, *g_qk, *g_out, *dw_hq, *dw_out, *gamma, *beta; };
struct MfFsmn { MfLin conv1, uv, lin, proj, conv2; const float *prelu, *n1w, *n1b, *n2w, *n2b, *dw_uv, *dw39; };

struct mis_mossformer2 {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_mossformer2_config cfg{};
    int wlen = 0, hop = 0, nfft = 0, log2n = 0, nm = 0, Cin = 0, D = 0, F = 0, NB = 0, N = 0, W = 0, Tcap = 0, Gcap = 0;
    int64_t out_cap = 0;
    HostWeights raw{"MossFormer2", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<float> farena, work, pcm;
    DevBuf<int32_t> counts, iarena;
    std::vector<int32_t> h_T;
    const float *win = nullptr, *twc = nullptr, *tws = nullptr, *fb = nullptr, *pos = nullptr, *rc = nullptr, *rs = nullptr, *dft = nullptr,
                *idft = nullptr, *gln_w = nullptr, *gln_b = nullptr, *ln1w = nullptr, *ln1b = nullptr, *ln2w = nullptr, *ln2b = nullptr,
                *prelu = nullptr;
    const int32_t* fbr = nullptr;
    MfLin enc{}, cout0{}, og{}, dec{};
    std::vector<MfFlash> flash;
    std::vector<MfFsmn> fsmn;
    float *fbank = nullptr, *feat = nullptr, *xn = nullptr, *hq = nullptr, *vu = nullptr, *qk4 = nullptr, *P = nullptr, *S = nullptr, *att = nullptr, *y = nullptr,
          *c1 = nullptr, *n1 = nullptr, *uv = nullptr, *uv2 = nullptr, *f1 = nullptr, *p1 = nullptr, *gt = nullptr, *n2 = nullptr, *sa = nullptr,
          *sb = nullptr, *tail = nullptr, *co = nullptr, *ogb = nullptr, *mask = nullptr, *spec = nullptr, *fr = nullptr, *wave = nullptr;
    std::vector<float*> xs;                                 // x0 and every layer's / block's output: 2 NB + 1 buffers
    int last_batch = 0, last_nr = 0, last_launches = 0;
    int64_t last_out = 0;
    bool last_front = false, last_net = false, last_synth = false;
    HipEvents<4> ev;
    float ms[3] = {0.0f, 0.0f, 0.0f};
};

static int mf_frames_of(const mis_mossformer2* c, int64_t n) { return n < c->wlen ? 0 : (int)(1 + (n - c->wlen) / c->hop); }

extern "C" mis_status mis_mossformer2_create(const mis_mossformer2_config* cfg, int device, mis_mossformer2** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    // the configuration is judged before the device is touched
    MIS_REQUIRE(cfg->sample_rate >= 1000 && cfg->sample_rate <= 192000, MIS_ERR_INVALID_INPUT, "sample_rate %d unsupported", cfg->sample_rate);
    MIS_REQUIRE(cfg->win_len >= 33 && cfg->win_len <= MF_MAX_NFFT, MIS_ERR_INVALID_INPUT,
                "win_len %d unsupported (33..%d: the fbank's power-of-two FFT has at most %d points)", cfg->win_len, MF_MAX_NFFT, MF_MAX_NFFT);
    MIS_REQUIRE(cfg->win_inc >= 1 && cfg->win_inc <= cfg->win_len, MIS_ERR_INVALID_INPUT, "win_inc %d unsupported (1..win_len)", cfg->win_inc);
    MIS_REQUIRE(cfg->fft_len >= 2 && cfg->fft_len <= 4096 && cfg->fft_len % 2 == 0, MIS_ERR_INVALID_INPUT, "fft_len %d unsupported (even, 2..4096)",
                cfg->fft_len);
    MIS_REQUIRE(cfg->out_channels_final == cfg->fft_len / 2 + 1, MIS_ERR_INVALID_INPUT,
                "out_channels_final %d is not fft_len / 2 + 1 = %d: the mask would not cover the spectrum", cfg->out_channels_final, cfg->fft_len / 2 + 1);
    MIS_REQUIRE(cfg->num_mels >= 1 && cfg->num_mels <= 256, MIS_ERR_INVALID_INPUT, "num_mels %d unsupported (1..256)", cfg->num_mels);
    MIS_REQUIRE(cfg->in_channels == 3 * cfg->num_mels, MIS_ERR_INVALID_INPUT, "in_channels %d is not 3 x num_mels = %d", cfg->in_channels,
                3 * cfg->num_mels);
    MIS_REQUIRE(cfg->out_channels >= 16 && cfg->out_channels <= 2048 && cfg->out_channels % 16 == 0, MIS_ERR_INVALID_INPUT,
                "out_channels %d unsupported (a multiple of 16, 16..2048)", cfg->out_channels);
    MIS_REQUIRE(cfg->num_blocks >= 1 && cfg->num_blocks <= 64, MIS_ERR_INVALID_INPUT, "num_blocks %d unsupported (1..64)", cfg->num_blocks);
    MIS_REQUIRE(cfg->preemphasis >= 0.0f && cfg->preemphasis <= 1.0f, MIS_ERR_INVALID_INPUT, "preemphasis outside 0..1");
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= MF_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch must be 1..%d", MF_MAX_BATCH);
    MIS_REQUIRE(cfg->max_samples >= cfg->win_len && cfg->max_samples <= ((int64_t)1 << 28), MIS_ERR_INVALID_INPUT,
                "max_samples must be win_len..2^28");
    hipStream_t stream = mis_open_stream(device);
    auto c = std::make_unique<mis_mossformer2>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->wlen = cfg->win_len; c->hop = cfg->win_inc; c->nm = cfg->num_mels; c->Cin = cfg->in_channels; c->D = cfg->out_channels;
    c->F = cfg->out_channels_final; c->NB = cfg->num_blocks; c->N = cfg->fft_len; c->W = std::min(cfg->win_len, cfg->fft_len);
    c->nfft = 1; c->log2n = 0;
    while (c->nfft < c->wlen) { c->nfft <<= 1; ++c->log2n; }
    c->Tcap = mf_frames_of(c.get(), cfg->max_samples); c->Gcap = cdiv(c->Tcap, MF_GROUP);
    c->out_cap = (int64_t)(c->Tcap - 1) * c->hop + c->W;
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_mossformer2_destroy(mis_mossformer2* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// names below "model.mossformer." of a sanitized checkpoint; scalars ([] in the checkpoint) arrive as [1]; host pointers
extern "C" mis_status mis_mossformer2_set_tensor(mis_mossformer2* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape,
                                                 int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 4, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

static std::string mf_layer(int i) { return "mdl.intra_mdl.mossformerM.layers." + std::to_string(i); }
static std::string mf_fsmn(int i) { return "mdl.intra_mdl.mossformerM.fsmn." + std::to_string(i); }

extern "C" mis_status mis_mossformer2_finalize(mis_mossformer2* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t D = c->D, Ci = c->Cin, F = c->F, I = MF_INNER, Q = MF_QK, nm = c->nm, N = c->N, W = c->W, Tc = c->Tcap;
    const double PI = 3.14159265358979323846;
    HostArena a(c->raw);
    std::vector<float>& fh = a.fhost;
    auto lin = [&](const std::string& p, std::initializer_list<int64_t> shape, int64_t cout, int64_t cin, bool bias, MfLin& l) {
        l = MfLin{nullptr, nullptr, (int)cin, (int)cout};
        a.fvec(p + ".weight", shape, cout * cin, l.w);
        if (bias) a.fvec(p + ".bias", {cout}, cout, l.b);
    };
    // a weight [cout][cin] at ow and a bias [cout] at ob for a packer below to fill
    auto packed = [&](int64_t cout, int64_t cin, MfLin& l, size_t& ow, size_t& ob) {
        l = MfLin{nullptr, nullptr, (int)cin, (int)cout};
        ow = a.ftake((size_t)cout * cin, l.w); ob = a.ftake(cout, l.b);
    };
    auto vec = [&](const std::string& name, std::initializer_list<int64_t> shape, int64_t n, const float*& dst) { a.fvec(name, shape, n, dst); };
    vec("norm.weight", {Ci, 1}, Ci, c->gln_w); vec("norm.bias", {Ci, 1}, Ci, c->gln_b);
    lin("conv1d_encoder", {D, 1, Ci}, D, Ci, false, c->enc);
    c->flash.assign(c->NB, MfFlash{}); c->fsmn.assign(c->NB, MfFsmn{});
    size_t ow, ob;
    for (int i = 0; i < c->NB; ++i) {
        const std::string q = mf_layer(i);
        MfFlash& f = c->flash[i];
        // to_hidden and to_qk read the same shifted, scale-normed frame: one weight [4 D + 128][D], one bias, one set of taps
        packed(4 * D + Q, D, f.hq, ow, ob);
        {
            const HostTensor &wh = c->raw.need(q + ".to_hidden.linear.weight", {4 * D, D}), &wq = c->raw.need(q + ".to_qk.linear.weight", {Q, D});
            const HostTensor &bh = c->raw.need(q + ".to_hidden.linear.bias", {4 * D}), &bq = c->raw.need(q + ".to_qk.linear.bias", {Q});
            std::copy(wh.v.begin(), wh.v.end(), fh.begin() + ow); std::copy(wq.v.begin(), wq.v.end(), fh.begin() + ow + 4 * D * D);
            std::copy(bh.v.begin(), bh.v.end(), fh.begin() + ob); std::copy(bq.v.begin(), bq.v.end(), fh.begin() + ob + 4 * D);
            const HostTensor &dh = c->raw.need(q + ".to_hidden.conv_module.weight", {4 * D, MF_FF_TAPS, 1}),
                             &dq = c->raw.need(q + ".to_qk.conv_module.weight", {Q, MF_FF_TAPS, 1});
            const size_t o_dw = a.ftake((size_t)(4 * D + Q) * MF_FF_TAPS, f.dw_hq);
            std::copy(dh.v.begin(), dh.v.end(), fh.begin() + o_dw); std::copy(dq.v.begin(), dq.v.end(), fh.begin() + o_dw + 4 * D * MF_FF_TAPS);
        }
        vec(q + ".to_hidden.norm.g", {1}, 1, f.g_h); vec(q + ".to_qk.norm.g", {1}, 1, f.g_qk); vec(q + ".to_out.norm.g", {1}, 1, f.g_out);
        vec(q + ".qk_offset_scale.gamma", {4, Q}, 4 * Q, f.gamma); vec(q + ".qk_offset_scale.beta", {4, Q}, 4 * Q, f.beta);
        lin(q + ".to_out.linear", {D, 2 * D}, D, 2 * D, true, f.out);
        vec(q + ".to_out.conv_module.weight", {D, MF_FF_TAPS, 1}, D * MF_FF_TAPS, f.dw_out);
        const std::string s = mf_fsmn(i), gq = s + ".gated_fsmn";
        MfFsmn& z = c->fsmn[i];
        lin(s + ".conv1", {I, 1, D}, I, D, true, z.conv1);
        vec(s + ".prelu.weight", {1}, 1, z.prelu);
        vec(s + ".norm1.weight", {I}, I, z.n1w); vec(s + ".norm1.bias", {I}, I, z.n1b);
        vec(s + ".norm2.weight", {I}, I, z.n2w); vec(s + ".norm2.bias", {I}, I, z.n2b);
        // to_u | to_v: the LayerNorm's weight and bias are folded into the Linear (formed in double, rounded once); the kernel
        // normalises on load
        packed(2 * I, I, z.uv, ow, ob);
        const size_t o_dwuv = a.ftake((size_t)2 * I * MF_FF_TAPS, z.dw_uv);
        for (int h = 0; h < 2; ++h) {
            const std::string t = gq + (h ? ".to_v" : ".to_u");
            const HostTensor &w = c->raw.need(t + ".linear.weight", {I, I}), &bl = c->raw.need(t + ".linear.bias", {I});
            const HostTensor &nw = c->raw.need(t + ".norm.weight", {I}), &nb = c->raw.need(t + ".norm.bias", {I});
            const HostTensor& dw = c->raw.need(t + ".conv_module.weight", {I, MF_FF_TAPS, 1});
            for (int64_t o = 0; o < I; ++o) {
                double acc = bl.v[o];
                for (int64_t k = 0; k < I; ++k) {
                    fh[ow + (h * I + o) * I + k] = (float)((double)w.v[o * I + k] * (double)nw.v[k]);
                    acc += (double)w.v[o * I + k] * (double)nb.v[k];
                }
                fh[ob + h * I + o] = (float)acc;
            }
            std::copy(dw.v.begin(), dw.v.end(), fh.begin() + o_dwuv + h * I * MF_FF_TAPS);
        }
        lin(gq + ".fsmn.linear", {I, I}, I, I, true, z.lin);
        lin(gq + ".fsmn.project", {I, I}, I, I, false, z.proj);
        vec(gq + ".fsmn.conv1.weight", {I, MF_FSMN_TAPS, 1, 1}, I * MF_FSMN_TAPS, z.dw39);
        lin(s + ".conv2", {D, 1, I}, D, I, true, z.conv2);
    }
    vec("mdl.intra_mdl.norm.weight", {D}, D, c->ln1w); vec("mdl.intra_mdl.norm.bias", {D}, D, c->ln1b);
    vec("mdl.intra_norm.weight", {D}, D, c->ln2w); vec("mdl.intra_norm.bias", {D}, D, c->ln2b);
    vec("prelu.weight", {1}, 1, c->prelu);
    // speaker 0 is the first out_channels outputs of conv1d_out; the reference returns nothing of the second speaker
    c->cout0 = MfLin{nullptr, nullptr, (int)D, (int)D};
    a.fvec("conv1d_out.weight", {2 * D, 1, D}, D * D, c->cout0.w); a.fvec("conv1d_out.bias", {2 * D}, D, c->cout0.b);
    packed(2 * D, D, c->og, ow, ob);
    {
        const HostTensor &wo = c->raw.need("output.weight", {D, 1, D}), &wg = c->raw.need("output_gate.weight", {D, 1, D});
        const HostTensor &bo = c->raw.need("output.bias", {D}), &bg = c->raw.need("output_gate.bias", {D});
        std::copy(wo.v.begin(), wo.v.end(), fh.begin() + ow); std::copy(wg.v.begin(), wg.v.end(), fh.begin() + ow + D * D);
        std::copy(bo.v.begin(), bo.v.end(), fh.begin() + ob); std::copy(bg.v.begin(), bg.v.end(), fh.begin() + ob + D);
    }
    lin("conv1_decoder", {F, 1, D}, F, D, false, c->dec);
    // ---- tables
    const HostTensor &pscale = c->raw.need("pos_enc.scale", {1}), &pfreq = c->raw.need("pos_enc.inv_freq", {D / 2});
    const size_t o_pos = a.ftake((size_t)Tc * D, c->pos), o_rc = a.ftake((size_t)Tc * (MF_ROPE / 2), c->rc), o_rs = a.ftake((size_t)Tc * (MF_ROPE / 2), c->rs);
    for (int64_t t = 0; t < Tc; ++t) {
        for (int64_t i = 0; i < D / 2; ++i) {                          // [sin | cos] scale; the angle is the f32 product the reference forms
            const float th = (float)t * pfreq.v[i];
            fh[o_pos + t * D + i] = (float)sin((double)th) * pscale.v[0];
            fh[o_pos + t * D + D / 2 + i] = (float)cos((double)th) * pscale.v[0];
        }
        for (int i = 0; i < MF_ROPE / 2; ++i) {
            const float inv = (float)pow(10000.0, -2.0 * i / (double)MF_ROPE), th = (float)t * inv;
            fh[o_rc + t * (MF_ROPE / 2) + i] = (float)cos((double)th); fh[o_rs + t * (MF_ROPE / 2) + i] = (float)sin((double)th);
        }
    }
    const int bins = c->nfft / 2 + 1;
    const size_t o_win = a.ftake(c->wlen, c->win), o_twc = a.ftake(1024, c->twc), o_tws = a.ftake(1024, c->tws), o_fb = a.ftake((size_t)bins * nm, c->fb);
    for (int i = 0; i < c->wlen; ++i) {                                // the reference's own f32 arithmetic (hammingWindow / hannWindow)
        const float phase = 2.0f * (float)M_PI * (float)i / (float)(c->wlen - 1);
        fh[o_win + i] = c->cfg.win_hann ? 0.5f - 0.5f * (float)cos((double)phase) : 0.54f - 0.46f * (float)cos((double)phase);
    }
    fft2048_twiddles(&fh[o_twc], &fh[o_tws]);
    std::vector<int32_t> ih((size_t)round_up(2 * nm, 64), 0);
    {   // melFilters(sampleRate, nFft, nMels, fMin 20, norm nil, htk): triangles in Hz, f32 as the reference
        const float sr = (float)c->cfg.sample_rate, fmax = sr / 2.0f;
        auto h2m = [](float f) { return 2595.0f * log10f(1.0f + f / 700.0f); };
        auto m2h = [](float m) { return 700.0f * (powf(10.0f, m / 2595.0f) - 1.0f); };
        const float mmin = h2m(20.0f), mmax = h2m(fmax);
        std::vector<float> fp(nm + 2);
        for (int i = 0; i < nm + 2; ++i) fp[i] = m2h(mmin + (float)i * (mmax - mmin) / (float)(nm + 1));
        for (int i = 0; i < bins; ++i) {
            const float fq = (float)i * sr / (float)c->nfft;
            for (int j = 0; j < nm; ++j) {
                const float lo = fp[j], ce = fp[j + 1], hi = fp[j + 2];
                float v = 0.0f;
                if (fq >= lo && fq < ce) v = (fq - lo) / (ce - lo);
                else if (fq >= ce && fq <= hi) v = (hi - fq) / (hi - ce);
                fh[o_fb + (size_t)i * nm + j] = v;
            }
        }
        filter_bin_ranges(&fh[o_fb], bins, (int)nm, ih.data());
    }
    // the transform pair as tables formed in double: rows [cos | -sin] over the W samples a frame keeps, and the inverse's weights
    const size_t o_dft = a.ftake((size_t)2 * F * W, c->dft), o_idft = a.ftake((size_t)W * 2 * F, c->idft);
    for (int64_t k = 0; k < F; ++k)
        for (int64_t n = 0; n < W; ++n) {
            const double ang = 2.0 * PI * (double)((k * n) % N) / (double)N;
            fh[o_dft + k * W + n] = (float)cos(ang); fh[o_dft + (F + k) * W + n] = (float)-sin(ang);
            const bool edge = k == 0 || k == N / 2;                    // irfft ignores the imaginary parts of DC and Nyquist
            fh[o_idft + n * 2 * F + k] = (float)((edge ? 1.0 : 2.0) * cos(ang) / (double)N);
            fh[o_idft + n * 2 * F + F + k] = edge ? 0.0f : (float)(-2.0 * sin(ang) / (double)N);
        }
    // ---- the workspace, sized once.  No call reads the handle before finalized is set: a finalize rejected for a missing or misshapen
    // tensor or for its size can be repeated.  A failed device allocation below is not recoverable: destroy the handle.
    const size_t B = c->cfg.max_batch, rows = B * (size_t)Tc;
    const size_t per_row = nm + 2 * Ci + (2 * c->NB + 1) * D + (4 * D + Q) + 4 * D + 4 * Q + 2 * D + D + 2 * I + 2 * 2 * I + 4 * I + 4 + D + D
                           + 2 * D + F + 2 * F + W;
    const size_t total = rows * per_row + B * (size_t)(c->Gcap + 1) * Q * 4 * D + B * (size_t)c->out_cap + 64 * (64 + 2 * (size_t)c->NB);
    MIS_REQUIRE((total + B * (size_t)c->cfg.max_samples) * 4 <= ((size_t)96 << 30), MIS_ERR_INVALID_INPUT,
                "max_batch x max_samples needs a workspace of %zu MiB (at most 96 GiB)", (total + B * (size_t)c->cfg.max_samples) * 4 >> 20);
    DevBuf<bf16_t> none;
    a.upload(none, c->farena);
    c->iarena.alloc(ih.size());
    HIP_CHECK(hipMemcpy(c->iarena.p, ih.data(), ih.size() * 4, hipMemcpyHostToDevice));
    c->work.alloc(total);
    c->pcm.alloc(B * (size_t)c->cfg.max_samples);
    c->counts.alloc(MF_MAX_BATCH);
    c->h_T.assign(MF_MAX_BATCH, 0);
    float* w = c->work.p;
    auto take = [&](size_t n) { float* p = w; w += round_up(n, 64); return p; };
    c->fbank = take(rows * nm); c->feat = take(rows * Ci); c->xn = take(rows * Ci);
    c->xs.clear();
    for (int i = 0; i < 2 * c->NB + 1; ++i) c->xs.push_back(take(rows * D));
    c->hq = take(rows * (4 * D + Q)); c->vu = take(rows * 4 * D); c->qk4 = take(rows * 4 * Q); c->att = take(rows * 2 * D); c->y = take(rows * D);
    c->c1 = take(rows * I); c->n1 = take(rows * I); c->uv = take(rows * 2 * I); c->uv2 = take(rows * 2 * I); c->f1 = take(rows * I);
    c->p1 = take(rows * I); c->gt = take(rows * I); c->n2 = take(rows * I); c->sa = take(rows * 2); c->sb = take(rows * 2);
    c->tail = take(rows * D); c->co = take(rows * D); c->ogb = take(rows * 2 * D); c->mask = take(rows * F); c->spec = take(rows * 2 * F);
    c->fr = take(rows * W); c->P = take(B * (size_t)c->Gcap * Q * 4 * D); c->S = take(B * (size_t)Q * 4 * D); c->wave = take(B * (size_t)c->out_cap);
    MIS_REQUIRE((size_t)(w - c->work.p) <= total, MIS_ERR_GENERATION_FAILED, "workspace layout exceeds its size");
    c->fbr = c->iarena.p;
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of a sanitized checkpoint
extern "C" mis_status mis_mossformer2_init_synthetic(mis_mossformer2* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    const int64_t D = c->D, Ci = c->Cin, F = c->F, I = MF_INNER, Q = MF_QK;
    SynthWeights sw{c->raw, seed * 100000ull};
    auto conv = [&](const std::string& p, int64_t o, int64_t i, bool bias, double gain) {
        sw.put(p + ".weight", {o, 1, i}, gain * sqrt(3.0 / (double)i), 0.0f);
        if (bias) sw.put(p + ".bias", {o}, 0.05, 0.0f);
    };
    auto ff = [&](const std::string& p, int64_t o, int64_t i, bool scale) {
        if (scale) sw.put(p + ".norm.g", {1}, 0.1, 1.0f); else sw.norm(p + ".norm", i);
        sw.lin(p + ".linear", o, i, true, 1.0);
        sw.put(p + ".conv_module.weight", {o, MF_FF_TAPS, 1}, sqrt(3.0 / MF_FF_TAPS), 0.0f);
    };
    sw.put("norm.weight", {Ci, 1}, 0.1, 1.0f); sw.put("norm.bias", {Ci, 1}, 0.05, 0.0f);
    conv("conv1d_encoder", D, Ci, false, 1.0);
    sw.put("pos_enc.scale", {1}, 0.1, 1.0f);
    {
        HostTensor t; t.shape = {D / 2}; t.v.resize(D / 2);
        for (int64_t i = 0; i < D / 2; ++i) t.v[i] = 1.0f / powf(10000.0f, (float)(2 * i) / (float)D);
        c->raw.put("pos_enc.inv_freq", std::move(t));
    }
    for (int i = 0; i < c->NB; ++i) {
        const std::string q = mf_layer(i), s = mf_fsmn(i), gq = s + ".gated_fsmn";
        ff(q + ".to_hidden", 4 * D, D, true); ff(q + ".to_qk", Q, D, true); ff(q + ".to_out", D, 2 * D, true);
        sw.put(q + ".qk_offset_scale.gamma", {4, Q}, 0.5, 1.0f); sw.put(q + ".qk_offset_scale.beta", {4, Q}, 0.5, 0.0f);
        conv(s + ".conv1", I, D, true, 1.0);
        sw.put(s + ".prelu.weight", {1}, 0.05, 0.25f);
        sw.norm(s + ".norm1", I); sw.norm(s + ".norm2", I);
        ff(gq + ".to_u", I, I, false); ff(gq + ".to_v", I, I, false);
        sw.lin(gq + ".fsmn.linear", I, I, true, 1.0); sw.lin(gq + ".fsmn.project", I, I, false, 1.0);
        sw.put(gq + ".fsmn.conv1.weight", {I, MF_FSMN_TAPS, 1, 1}, sqrt(3.0 / MF_FSMN_TAPS), 0.0f);
        conv(s + ".conv2", D, I, true, 0.5);
    }
    sw.norm("mdl.intra_mdl.norm", D); sw.norm("mdl.intra_norm", D);
    sw.put("prelu.weight", {1}, 0.05, 0.25f);
    conv("conv1d_out", 2 * D, D, true, 1.0); conv("output", D, D, true, 1.0); conv("output_gate", D, D, true, 1.0);
    conv("conv1_decoder", F, D, false, 2.0);
    MIS_API_END
}

extern "C" int mis_mossformer2_launches(const mis_mossformer2* c) { return c ? c->last_launches : 0; }

extern "C" mis_status mis_mossformer2_frames(const mis_mossformer2* c, const int64_t* lens, int batch, int32_t* frames, int64_t* out_lens) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && lens && batch >= 0, MIS_ERR_INVALID_INPUT, "bad argument");
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(lens[b] >= 0 && lens[b] < ((int64_t)1 << 40), MIS_ERR_INVALID_INPUT, "row %d: bad length", b);
        const int64_t T = lens[b] < c->wlen ? 0 : 1 + (lens[b] - c->wlen) / c->hop;
        MIS_REQUIRE(T < (1 << 30), MIS_ERR_INVALID_INPUT, "row %d: too many frames", b);
        if (frames) frames[b] = (int32_t)T;
        if (out_lens) out_lens[b] = T ? (T - 1) * c->hop + c->W : 0;
    }
    MIS_API_END
}

// ---------------------------------------------------------------------------- launches
static MfGemm mf_gemm(const MfLin& l, const float* X, int ldx, float* Y, int act) {
    MfGemm g{};
    g.X = X; g.ldx = ldx; g.W = l.w; g.ldw = l.cin; g.bias = l.b; g.Y = Y; g.ldy = l.cout; g.Cin = l.cin; g.Cout = l.cout; g.act = act;
    g.load = MF_LOAD_ACT;
    return g;
}
static void mf_launch_gemm(mis_mossformer2* c, MfGemm g, int nr, int B) {
    g.cnt = c->counts.p; g.nr = nr;
    hipLaunchKernelGGL(k_mf2_gemm, dim3(cdiv(nr, 64), cdiv(g.Cout, 64), B), dim3(256), 0, c->stream, g);
}
static void mf_launch_row(mis_mossformer2* c, MfRow r, int nr, int B) {
    r.cnt = c->counts.p; r.nr = nr;
    hipLaunchKernelGGL(k_mf2_row, dim3(cdiv(nr, 4), B), dim3(256), 0, c->stream, r);
}
static void mf_launch_dw(mis_mossformer2* c, MfDw d, int nr, int B) {
    d.cnt = c->counts.p; d.nr = nr;
    hipLaunchKernelGGL(k_mf2_dwconv, dim3(cdiv(nr, 32), cdiv(d.C, 64), B), dim3(256), 0, c->stream, d);
}

static int mf_enqueue_front(mis_mossformer2* c, int64_t stride, int nr, int B) {
    MfFront fp{c->pcm.p, stride, c->win, c->twc, c->tws, c->fb, c->fbr, c->fbank, c->counts.p, nr, c->wlen, c->hop, c->nm, c->nfft, c->log2n,
               c->cfg.preemphasis, (float)log((double)1e-10f)};
    hipLaunchKernelGGL(k_mf2_fbank, dim3(nr, B), dim3(256), 0, c->stream, fp);
    const size_t total = (size_t)B * nr * c->nm;
    hipLaunchKernelGGL(k_mf2_deltas, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, c->fbank, c->feat, c->counts.p, nr, c->nm, total);
    return 2;
}

// the mask network on c->feat; returns the launches made: 6 + 18 num_blocks
static int mf_enqueue_network(mis_mossformer2* c, int nr, int B) {
    const int D = c->D, I = MF_INNER, Q = MF_QK, G = cdiv(nr, MF_GROUP);
    hipLaunchKernelGGL(k_mf2_gln, dim3(B), dim3(256), 0, c->stream, c->feat, c->xn, c->gln_w, c->gln_b, c->counts.p, nr, c->Cin);
    { MfGemm g = mf_gemm(c->enc, c->xn, c->Cin, c->xs[0], MF_ACT_NONE); g.pos = c->pos; mf_launch_gemm(c, g, nr, B); }
    for (int i = 0; i < c->NB; ++i) {
        const MfFlash& f = c->flash[i];
        const float* x = c->xs[2 * i];
        float* xa = c->xs[2 * i + 1];
        float* xb = c->xs[2 * i + 2];
        // ---- FLASH layer: 9 launches
        { MfRow r{}; r.X = x; r.ldx = D; r.stats = c->sa; r.C = D; r.mode = MF_ROW_SCALE; r.half = D / 2; mf_launch_row(c, r, nr, B); }
        { MfGemm g = mf_gemm(f.hq, x, D, c->hq, MF_ACT_SILU); g.load = MF_LOAD_SHIFT; g.half = D / 2; g.stats = c->sa; g.g0 = f.g_h; g.g1 = f.g_qk;
          g.gsplit = 4 * D; mf_launch_gemm(c, g, nr, B); }
        { MfDw d{}; d.X = c->hq; d.ldx = 4 * D + Q; d.dw = f.dw_hq; d.K = MF_FF_TAPS; d.Y = c->vu; d.ldy = 4 * D; d.C = 4 * D + Q; d.Cmain = 4 * D;
          d.mode = MF_DW_FF; d.qk4 = c->qk4; d.gamma = f.gamma; d.beta = f.beta; d.rc = c->rc; d.rs = c->rs; mf_launch_dw(c, d, nr, B); }
        { MfLinKV l{c->qk4, c->vu, c->P, c->counts.p, nr, G, 4 * D};
          hipLaunchKernelGGL(k_mf2_linkv, dim3(Q / 64, cdiv(4 * D, 64), G * B), dim3(256), 0, c->stream, l); }
        { const int per_row = Q * 4 * D;
          hipLaunchKernelGGL(k_mf2_linsum, dim3(cdiv(per_row, 256), B), dim3(256), 0, c->stream, c->P, c->S, c->counts.p, nr, G, per_row); }
        { MfAttn t{c->qk4, c->vu, c->S, c->att, c->counts.p, nr, 2 * D};
          hipLaunchKernelGGL(k_mf2_attn, dim3(cdiv(nr, 32), cdiv(2 * D, 128), B), dim3(256), 0, c->stream, t); }
        { MfRow r{}; r.X = c->att; r.ldx = 2 * D; r.stats = c->sb; r.C = 2 * D; r.mode = MF_ROW_SCALE; r.half = 0; mf_launch_row(c, r, nr, B); }
        { MfGemm g = mf_gemm(f.out, c->att, 2 * D, c->y, MF_ACT_SILU); g.stats = c->sb; g.g0 = f.g_out; g.g1 = f.g_out; g.gsplit = D;
          mf_launch_gemm(c, g, nr, B); }
        { MfDw d{}; d.X = c->y; d.ldx = D; d.dw = f.dw_out; d.K = MF_FF_TAPS; d.Y = xa; d.ldy = D; d.C = D; d.Cmain = D; d.mode = MF_DW_FF; d.R = x;
          d.ldr = D; mf_launch_dw(c, d, nr, B); }
        // ---- GatedFSMNBlock: 9 launches
        const MfFsmn& s = c->fsmn[i];
        { MfGemm g = mf_gemm(s.conv1, xa, D, c->c1, MF_ACT_PRELU); g.slope = s.prelu; mf_launch_gemm(c, g, nr, B); }
        { MfRow r{}; r.X = c->c1; r.ldx = I; r.Y = c->n1; r.ldy = I; r.stats = c->sa; r.w1 = s.n1w; r.b1 = s.n1b; r.C = I; r.mode = MF_ROW_CLN;
          r.eps = 1e-8f; r.eps_next = 1e-5f; mf_launch_row(c, r, nr, B); }
        { MfGemm g = mf_gemm(s.uv, c->n1, I, c->uv, MF_ACT_SILU); g.load = MF_LOAD_LN; g.stats = c->sa; mf_launch_gemm(c, g, nr, B); }
        { MfDw d{}; d.X = c->uv; d.ldx = 2 * I; d.dw = s.dw_uv; d.K = MF_FF_TAPS; d.Y = c->uv2; d.ldy = 2 * I; d.C = 2 * I; d.Cmain = 2 * I;
          d.mode = MF_DW_FF; mf_launch_dw(c, d, nr, B); }
        mf_launch_gemm(c, mf_gemm(s.lin, c->uv2, 2 * I, c->f1, MF_ACT_RELU), nr, B);
        mf_launch_gemm(c, mf_gemm(s.proj, c->f1, I, c->p1, MF_ACT_NONE), nr, B);
        { MfDw d{}; d.X = c->p1; d.ldx = I; d.dw = s.dw39; d.K = MF_FSMN_TAPS; d.Y = c->gt; d.ldy = I; d.C = I; d.Cmain = I; d.mode = MF_DW_FSMN;
          d.U = c->uv2; d.ldu = 2 * I; d.uoff = 0; d.V = c->uv2; d.ldv = 2 * I; d.voff = I; d.N = c->n1; d.ldn = I; mf_launch_dw(c, d, nr, B); }
        { MfRow r{}; r.X = c->gt; r.ldx = I; r.Y = c->n2; r.ldy = I; r.w1 = s.n2w; r.b1 = s.n2b; r.C = I; r.mode = MF_ROW_CLN; r.eps = 1e-8f;
          mf_launch_row(c, r, nr, B); }
        { MfGemm g = mf_gemm(s.conv2, c->n2, I, xb, MF_ACT_NONE); g.R = xa; g.ldr = D; mf_launch_gemm(c, g, nr, B); }
    }
    { MfRow r{}; r.X = c->xs[2 * c->NB]; r.ldx = D; r.Y = c->tail; r.ldy = D; r.w1 = c->ln1w; r.b1 = c->ln1b; r.w2 = c->ln2w; r.b2 = c->ln2b;
      r.R = c->xs[0]; r.ldr = D; r.slope = c->prelu; r.C = D; r.mode = MF_ROW_TAIL; r.eps = 1e-8f; mf_launch_row(c, r, nr, B); }
    mf_launch_gemm(c, mf_gemm(c->cout0, c->tail, D, c->co, MF_ACT_NONE), nr, B);
    { MfGemm g = mf_gemm(c->og, c->co, D, c->ogb, MF_ACT_TANH_SIGMOID); g.gsplit = D; mf_launch_gemm(c, g, nr, B); }
    { MfGemm g = mf_gemm(c->dec, c->ogb, 2 * D, c->mask, MF_ACT_RELU); g.load = MF_LOAD_GATE; mf_launch_gemm(c, g, nr, B); }
    return 6 + 18 * c->NB;
}

// STFT of the rows in c->pcm, x c->mask, inverse transform x window, overlap-add into c->wave [B][out_stride]: 3 launches
static int mf_enqueue_synthesis(mis_mossformer2* c, int64_t stride, int nr, int B, int64_t out_stride) {
    const int F = c->F, W = c->W;
    { MfGemm g{}; g.W = c->dft; g.ldw = W; g.Y = c->spec; g.ldy = 2 * F; g.Cin = W; g.Cout = 2 * F; g.load = MF_LOAD_FRAME; g.pcm = c->pcm.p;
      g.pcm_stride = stride; g.hop = c->hop; g.win = c->win; mf_launch_gemm(c, g, nr, B); }
    { MfGemm g{}; g.X = c->spec; g.ldx = 2 * F; g.W = c->idft; g.ldw = 2 * F; g.Y = c->fr; g.ldy = W; g.Cin = 2 * F; g.Cout = W;
      g.load = MF_LOAD_MASKED; g.M = c->mask; g.ldm = F; g.F = F; g.cscale = c->win; mf_launch_gemm(c, g, nr, B); }
    hipLaunchKernelGGL(k_mf2_ola, dim3((unsigned)((out_stride + 255) / 256), B), dim3(256), 0, c->stream, c->fr, c->win, c->wave, c->counts.p, nr, W,
                       c->hop, out_stride);
    return 3;
}

enum { MF_WANT_FEATURES = 0, MF_WANT_MASK, MF_WANT_WAVE };

// The one driver.  Source: pcm [B][stride] (h_T set from the lens), features [B][nr][in_channels] or (synthesis alone) pcm + mask.
static void mf_run(mis_mossformer2* c, int want, const float* pcm, int64_t stride, const float* feats, const float* mask_in, int B, int nr,
                   float* out, int64_t out_rows_or_stride) {
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->last_launches = 0; c->ms[0] = c->ms[1] = c->ms[2] = 0.0f;
    c->last_batch = 0;
    if (nr == 0) return;
    MIS_REQUIRE(nr <= c->Tcap, MIS_ERR_INVALID_INPUT, "%d frames, the workspace holds %d (max_samples)", nr, c->Tcap);
    const int D = c->D, F = c->F;
    (void)D;
    int launches = 0;
    HIP_CHECK(hipMemcpyAsync(c->counts.p, c->h_T.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(c->ev[0], s));
    int64_t ns = 0;
    if (pcm) {
        ns = (int64_t)(nr - 1) * c->hop + c->wlen;
        MIS_REQUIRE(ns <= stride && ns <= c->cfg.max_samples, MIS_ERR_GENERATION_FAILED, "samples outside the workspace");
        HIP_CHECK(hipMemcpy2DAsync(c->pcm.p, (size_t)ns * 4, pcm, (size_t)stride * 4, (size_t)ns * 4, B, hipMemcpyHostToDevice, s));
        if (!mask_in) launches += mf_enqueue_front(c, ns, nr, B);
    } else {
        HIP_CHECK(hipMemcpyAsync(c->feat, feats, (size_t)B * nr * c->Cin * 4, hipMemcpyHostToDevice, s));
    }
    HIP_CHECK(hipEventRecord(c->ev[1], s));
    if (mask_in) HIP_CHECK(hipMemcpyAsync(c->mask, mask_in, (size_t)B * nr * F * 4, hipMemcpyHostToDevice, s));
    else if (want != MF_WANT_FEATURES) launches += mf_enqueue_network(c, nr, B);
    HIP_CHECK(hipEventRecord(c->ev[2], s));
    int64_t out_stride = 0;
    if (want == MF_WANT_FEATURES) {
        HIP_CHECK(hipMemcpy2DAsync(out, (size_t)out_rows_or_stride * c->Cin * 4, c->feat, (size_t)nr * c->Cin * 4, (size_t)nr * c->Cin * 4, B,
                                   hipMemcpyDeviceToHost, s));
    } else if (want == MF_WANT_MASK) {
        HIP_CHECK(hipMemcpy2DAsync(out, (size_t)out_rows_or_stride * F * 4, c->mask, (size_t)nr * F * 4, (size_t)nr * F * 4, B, hipMemcpyDeviceToHost, s));
    } else {
        out_stride = (int64_t)(nr - 1) * c->hop + c->W;
        MIS_REQUIRE(out_stride <= c->out_cap && out_stride <= out_rows_or_stride, MIS_ERR_GENERATION_FAILED, "output outside the workspace");
        launches += mf_enqueue_synthesis(c, ns, nr, B, out_stride);
        HIP_CHECK(hipMemcpy2DAsync(out, (size_t)out_rows_or_stride * 4, c->wave, (size_t)out_stride * 4, (size_t)out_stride * 4, B,
                                   hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipEventRecord(c->ev[3], s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));                               // the one synchronisation of a call
    for (int i = 0; i < 3; ++i) HIP_CHECK(hipEventElapsedTime(&c->ms[i], c->ev[i], c->ev[i + 1]));
    c->last_batch = B; c->last_nr = nr; c->last_launches = launches; c->last_out = out_stride;
    c->last_front = pcm != nullptr && !mask_in; c->last_net = !mask_in && want != MF_WANT_FEATURES; c->last_synth = want == MF_WANT_WAVE;
}

// lens -> h_T; returns the longest row's frames
static int mf_take_lens(mis_mossformer2* c, const float* pcm, const int64_t* lens, int batch, int64_t stride) {
    MIS_REQUIRE(c && pcm, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "MossFormer2 model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch must be 1..%d (max_batch)", c->cfg.max_batch);
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    int Tmax = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 0 && n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples, the row stride is %lld", b, (long long)n, (long long)stride);
        MIS_REQUIRE(n <= c->cfg.max_samples, MIS_ERR_INVALID_INPUT, "row %d: %lld samples, the workspace holds %lld (max_samples)", b, (long long)n,
                    (long long)c->cfg.max_samples);
        c->h_T[b] = mf_frames_of(c, n);
        Tmax = std::max(Tmax, c->h_T[b]);
    }
    return Tmax;
}

extern "C" mis_status mis_mossformer2_features(mis_mossformer2* c, const float* pcm, const int64_t* lens, int batch, int64_t stride,
                                               float* features, int rows) {
    MIS_API_BEGIN
    const int Tmax = mf_take_lens(c, pcm, lens, batch, stride);
    MIS_REQUIRE(features && rows >= Tmax, MIS_ERR_INVALID_INPUT, "features: room for %d rows, %d are needed", rows, Tmax);
    mf_run(c, MF_WANT_FEATURES, pcm, stride, nullptr, nullptr, batch, Tmax, features, rows);
    MIS_API_END
}

extern "C" mis_status mis_mossformer2_mask(mis_mossformer2* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* mask,
                                           int rows) {
    MIS_API_BEGIN
    const int Tmax = mf_take_lens(c, pcm, lens, batch, stride);
    MIS_REQUIRE(mask && rows >= Tmax, MIS_ERR_INVALID_INPUT, "mask: room for %d rows, %d are needed", rows, Tmax);
    mf_run(c, MF_WANT_MASK, pcm, stride, nullptr, nullptr, batch, Tmax, mask, rows);
    MIS_API_END
}

static void mf_take_counts(mis_mossformer2* c, const int32_t* counts, int batch, int rows) {
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "MossFormer2 model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch must be 1..%d (max_batch)", c->cfg.max_batch);
    MIS_REQUIRE(rows >= 1 && rows <= c->Tcap, MIS_ERR_INVALID_INPUT, "%d rows, the workspace holds 1..%d (max_samples)", rows, c->Tcap);
    for (int b = 0; b < batch; ++b) {
        const int r = counts ? counts[b] : rows;
        MIS_REQUIRE(r >= 0 && r <= rows, MIS_ERR_INVALID_INPUT, "row %d: %d feature rows (0 .. %d are served)", b, r, rows);
        c->h_T[b] = r;
    }
}

extern "C" mis_status mis_mossformer2_mask_features(mis_mossformer2* c, const float* features, const int32_t* counts, int batch, int rows,
                                                    float* mask) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && features && mask, MIS_ERR_INVALID_INPUT, "null argument");
    mf_take_counts(c, counts, batch, rows);
    mf_run(c, MF_WANT_MASK, nullptr, 0, features, nullptr, batch, rows, mask, rows);
    MIS_API_END
}

extern "C" mis_status mis_mossformer2_enhance(mis_mossformer2* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* out,
                                              int64_t out_stride, int64_t* out_lens) {
    MIS_API_BEGIN
    const int Tmax = mf_take_lens(c, pcm, lens, batch, stride);
    const int64_t need = Tmax ? (int64_t)(Tmax - 1) * c->hop + c->W : 0;
    MIS_REQUIRE(out && out_stride >= need, MIS_ERR_INVALID_INPUT, "out: room for %lld samples a row, %lld are needed", (long long)out_stride,
                (long long)need);
    if (out_lens) for (int b = 0; b < batch; ++b) out_lens[b] = c->h_T[b] ? (int64_t)(c->h_T[b] - 1) * c->hop + c->W : 0;
    mf_run(c, MF_WANT_WAVE, pcm, stride, nullptr, nullptr, batch, Tmax, out, out_stride);
    MIS_API_END
}

// the synthesis alone with a given mask f32 [batch, rows, out_channels_final], rows >= the longest row's frames
extern "C" mis_status mis_mossformer2_synthesize(mis_mossformer2* c, const float* pcm, const int64_t* lens, int batch, int64_t stride,
                                                 const float* mask, int rows, float* out, int64_t out_stride, int64_t* out_lens) {
    MIS_API_BEGIN
    const int Tmax = mf_take_lens(c, pcm, lens, batch, stride);
    const int64_t need = Tmax ? (int64_t)(Tmax - 1) * c->hop + c->W : 0;
    MIS_REQUIRE(mask && rows == Tmax, MIS_ERR_INVALID_INPUT, "mask: %d rows, the longest row has %d frames", rows, Tmax);
    MIS_REQUIRE(out && out_stride >= need, MIS_ERR_INVALID_INPUT, "out: room for %lld samples a row, %lld are needed", (long long)out_stride,
                (long long)need);
    if (out_lens) for (int b = 0; b < batch; ++b) out_lens[b] = c->h_T[b] ? (int64_t)(c->h_T[b] - 1) * c->hop + c->W : 0;
    mf_run(c, MF_WANT_WAVE, pcm, stride, nullptr, mask, batch, Tmax, out, out_stride);
    MIS_API_END
}

// tensors of the last call, f32 [B, rows, width], a row's own frames first and zeros behind them.  With L = num_blocks: stage 0 fbank,
// 1 features, 2 GlobalLayerNorm, 3 encoder + positions, 4 + 2 i FLASH layer i, 5 + 2 i GatedFSMNBlock i; from base = 4 + 2 L: + 0 tail
// norms + skip + PReLU, + 1 conv1d_out (speaker 0), + 2 tanh(output) | sigmoid(output_gate), + 3 mask, + 4 spectrum [re | im],
// + 5 windowed synthesis frames, + 6 waveform [B, samples, 1]; the last block's inner stages from base + 7: + 0 SiLU(to_hidden | to_qk),
// + 1 v | u, + 2 the four heads [quadQ | linQ | quadK | linK] after RoPE, + 3 attention output, + 4 SiLU(to_out), + 5 PReLU(conv1),
// + 6 norm1, + 7 SiLU(to_u | to_v), + 8 after the taps, + 9 ReLU(fsmn.linear), + 10 fsmn.project, + 11 the gate, + 12 norm2
extern "C" mis_status mis_mossformer2_tap(mis_mossformer2* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c, MIS_ERR_INVALID_INPUT, "null argument");
    const int base = 4 + 2 * c->NB, D = c->D, I = MF_INNER;
    MIS_REQUIRE(stage >= 0 && stage < base + 20, MIS_ERR_INVALID_INPUT, "bad stage");
    MIS_REQUIRE(c->last_batch > 0, MIS_ERR_INVALID_INPUT, "no call to tap");
    const bool net = (stage >= 2 && stage <= base + 3) || stage >= base + 7, synth = stage >= base + 4 && stage <= base + 6;
    MIS_REQUIRE((stage != 0 || c->last_front) && (!net || c->last_net || stage == base + 3) && (!synth || c->last_synth), MIS_ERR_INVALID_INPUT,
                "the last call did not compute stage %d", stage);
    HIP_CHECK(hipSetDevice(c->device));
    const float* src; size_t width; size_t n = c->last_nr;
    const float* inner[13] = {c->hq, c->vu, c->qk4, c->att, c->y, c->c1, c->n1, c->uv, c->uv2, c->f1, c->p1, c->gt, c->n2};
    const size_t iw[13] = {(size_t)4 * D + MF_QK, (size_t)4 * D, 4 * MF_QK, (size_t)2 * D, (size_t)D, (size_t)I, (size_t)I, (size_t)2 * I,
                           (size_t)2 * I, (size_t)I, (size_t)I, (size_t)I, (size_t)I};
    if (stage == 0) { src = c->fbank; width = c->nm; }
    else if (stage == 1) { src = c->feat; width = c->Cin; }
    else if (stage == 2) { src = c->xn; width = c->Cin; }
    else if (stage < base) { src = c->xs[stage - 3]; width = D; }
    else if (stage == base) { src = c->tail; width = D; }
    else if (stage == base + 1) { src = c->co; width = D; }
    else if (stage == base + 2) { src = c->ogb; width = 2 * D; }
    else if (stage == base + 3) { src = c->mask; width = c->F; }
    else if (stage == base + 4) { src = c->spec; width = 2 * c->F; }
    else if (stage == base + 5) { src = c->fr; width = c->W; }
    else if (stage == base + 6) { src = c->wave; width = 1; n = (size_t)c->last_out; }
    else { src = inner[stage - base - 7]; width = iw[stage - base - 7]; }
    const size_t B = c->last_batch;
    if (dims) { dims[0] = (int64_t)B; dims[1] = (int64_t)n; dims[2] = (int64_t)width; }
    if (!out) return MIS_OK;
    MIS_REQUIRE((int64_t)(B * n * width) <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    HIP_CHECK(hipMemcpy(out, src, B * n * width * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// measurements: device milliseconds of the last call, ms[3] = front end (copy in + fbank + deltas), mask network, synthesis (+ copy out)
extern "C" mis_status mis_debug_mossformer2_timing(const mis_mossformer2* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && ms, MIS_ERR_INVALID_INPUT, "null argument");
    ms[0] = c->ms[0]; ms[1] = c->ms[1]; ms[2] = c->ms[2];
    MIS_API_END
}
