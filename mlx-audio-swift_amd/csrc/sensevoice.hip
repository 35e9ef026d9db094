// sensevoice.hip - SenseVoice-small speech-to-text: waveform -> Kaldi-style fbank -> LFR stacking + CMVN behind four query rows ->
// SAN-M encoder -> CTC head; language / emotion / event ids and the greedy CTC collapse on the device.
//
// Reference being replaced: SenseVoiceModel (Sources/MLXAudioSTT/Models/SenseVoice/SenseVoiceModel.swift), SenseVoiceAudio.computeFbank /
// applyLFR / applyCMVN (SenseVoiceAudio.swift) and DSP.swift melFilters(htk, norm nil) / hammingWindow / hanningWindow.
//
// One call serves 1..max_batch ragged rows.  Row b has n_b samples, F_b = 1 + (n_b - win) / hop fbank frames (0 below one window) and
// T_b = 4 + ceil(F_b / lfr_n) sequence rows; every buffer of a call is f32 [B][Tp][.] with Tp the longest row's T_b.  A kernel derives
// a row's own count from T[b], loads zeros outside it and writes zeros behind it, and every output element is one fixed-order sum that
// depends on the row alone: a row's bits do not depend on the batch, its neighbours or the padding behind it.
//
//   k_sv_peak      max |x| of a row (block_max_256): the row is multiplied by 32768 iff its own peak <= 1
//   k_sv_fbank     one frame per block: scale, minus the frame mean, pre-emphasis 0.97 with first sample x0 - 0.97 x0, symmetric Hamming
//                  or Hann, 512-point radix-2 FFT in LDS, power over 257 bins, sparse HTK triangles, log max(., 1e-10)
//   k_sv_intake    rows 0..3 from the embedding table, rows >= 4 the clamp form of the LFR stack + CMVN; x sqrt(output_size) + the
//                  sinusoid of position r + 1 (table formed in double at finalize).  Also the plain LFR + CMVN tensor (features).
//   k_sv_gemm      the one contraction, exact f32 on v_mfma_f32_32x32x2_f32 (f32_tile.h), every dimension guarded.  Operand prologue:
//                  plain, or LayerNorm with the statistics of the block's own 64 rows formed first (a wave per row, two passes).
//                  Epilogues: bias / ReLU / residual; <SV_MEM> bias + v + depthwise_conv(v) from a time tile + halo of v in LDS + residual;
//                  <SV_ARGMAX> the column tile's (max, lowest index attaining it) per frame - no logit reaches memory
//   k_sv_attn      f32 flash attention: 64 queries x head x row per block (two waves of 32), 32-key tiles in ascending order through
//                  LDS, QK^T and PV on the f32 MFMA, online softmax in f32, d_k 1..128 zero-padded, the query fragments in registers
//   k_sv_ln        after_norm / tp_norm
//   k_sv_decode    one block per row: the tiles' pairs combined in tile order (ties to the lower index), rows 0..2 -> language / emotion /
//                  event ids, dedupe + drop blank 0 over rows 4.. and compaction
//   k_sv_logsoftmax  (forward only) log-softmax of a chunk of logits in place
//
// Launches: generate 7 + 5 L (peak, fbank, intake, 5 a layer, after_norm, tp_norm, head + arg-max, decode), L = 1 + max(num_blocks - 1, 0) +
// tp_blocks; forward 5 + 5 L + 2 chunks; forward_features 3 + 5 L + 2 chunks; features 3.  No allocation, one synchronisation per generate.
#include "common.h"
#include "audio_front.h"
#include "f32_tile.h"
#include "host_weights.h"
#include "step_loop.h"

#include <math.h>
#include <string.h>
#include <memory>

#define SV_MAX_BATCH 64
#define SV_NFFT 512
#define SV_BINS 257
#define SV_KMAX 32                // fsmn kernel_size
#define SV_TIMED_CHUNKS 64
#define SV_LN_EPS 1e-5f           // MLXNN LayerNorm default

enum { SV_PLAIN = 0, SV_MEM = 1, SV_ARGMAX = 2 };

// the rows a launch covers: batch rows b0 + blockIdx.z, sequence rows [t_lo, t_lo + nr) of each; inputs are [B][Tp][.], outputs [.][nr][.]
struct SvGeom { const int32_t* T; int Tp, b0, t_lo, nr; };

__device__ __forceinline__ int sv_count(const SvGeom& g, int b) {
    const int c = g.T[g.b0 + b] - g.t_lo;
    return c < 0 ? 0 : (c > g.nr ? g.nr : c);
}

// ============================================================================ front end
__global__ void __launch_bounds__(256) k_sv_peak(const float* __restrict__ pcm, int64_t stride, const int32_t* __restrict__ N, float* __restrict__ scale) {
    __shared__ float red[4];
    const int b = blockIdx.x, n = N[b];
    const float* x = pcm + (size_t)b * stride;
    float m = 0.0f;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(x[i]));
    m = block_max_256(m, red);
    if (threadIdx.x == 0) scale[b] = m <= 1.0f ? 32768.0f : 1.0f;
}

struct SvFront {
    const float* pcm; int64_t stride;
    const float *scale, *win, *twc, *tws, *fb; const int32_t *fbr, *F;   // window [wlen], twiddles [256], filters [257][nm], bin range per filter
    float* fbank; int Fp, wlen, hop, nm; float log_floor;                // [B][Fp][nm]
};

__global__ void __launch_bounds__(256) k_sv_fbank(SvFront p) {
    __shared__ float re[SV_NFFT], im[SV_NFFT], red[4];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    float* o = p.fbank + ((size_t)b * p.Fp + f) * p.nm;
    if (f >= p.F[b]) {
        if (tid < p.nm) o[tid] = 0.0f;
        return;
    }
    const float* x = p.pcm + (size_t)b * p.stride + (size_t)f * p.hop;
    const float g = p.scale[b];
    const float s0 = tid < p.wlen ? x[tid] * g : 0.0f, s1 = tid + 256 < p.wlen ? x[tid + 256] * g : 0.0f;
    const float mean = block_sum_256(s0 + s1, red) / (float)p.wlen;
    im[tid] = s0 - mean; im[tid + 256] = s1 - mean;
    __syncthreads();
    for (int j = tid; j < SV_NFFT; j += 256) {
        float y = 0.0f;
        if (j < p.wlen) {
            y = __fsub_rn(im[j], __fmul_rn(0.97f, im[j == 0 ? 0 : j - 1]));
            y = __fmul_rn(y, p.win[j]);
        }
        re[__brev((unsigned)j) >> 23] = y;
    }
    __syncthreads();
    im[tid] = 0.0f; im[tid + 256] = 0.0f;
    __syncthreads();
    for (int half = 1; half < SV_NFFT; half <<= 1) {
        const int k = tid & (half - 1), i0 = ((tid - k) << 1) + k, i1 = i0 + half, ti = k * (SV_NFFT / 2 / half);
        const float c = p.twc[ti], s = p.tws[ti];
        const float xr = re[i1], xi = im[i1];
        const float pr = xr * c - xi * s, pi = xr * s + xi * c;
        const float ar = re[i0], ai = im[i0];
        re[i0] = ar + pr; im[i0] = ai + pi; re[i1] = ar - pr; im[i1] = ai - pi;
        __syncthreads();
    }
    for (int j = tid; j < SV_BINS; j += 256) { const float a = re[j], c = im[j]; re[j] = a * a + c * c; }   // bins 0..256
    __syncthreads();
    if (tid < p.nm) {
        float acc = 0.0f;
        for (int i = p.fbr[2 * tid]; i < p.fbr[2 * tid + 1]; ++i) acc = fmaf(re[i], p.fb[(size_t)i * p.nm + tid], acc);
        o[tid] = acc > 1e-10f ? logf(acc) : p.log_floor;
    }
}

struct SvIntake {
    const float* fbank; int Fp; const int32_t* F;            // LFR source, or
    const float* feats; int Rs;                              // given features [B][Rs][in]
    const float *shift, *scale, *embed, *pos;                // CMVN (null: none), embed [16][in], pos [Tcap][in]
    float g; int nm, n, lp, in, lid, tn, raw;                // raw: the LFR + CMVN tensor alone, no query rows
};

// LFR row r, column ci of row b: slot i = ci / nm of fbank frame clamp(r n + i - lp, 0, F_b - 1), then (x + shift) scale, each rounded
__device__ __forceinline__ float sv_lfr_value(const SvIntake& q, int b, int r, int ci) {
    const int i = ci / q.nm, f = ci - i * q.nm;
    const int src = min(max(r * q.n + i - q.lp, 0), q.F[b] - 1);
    float v = q.fbank[((size_t)b * q.Fp + src) * q.nm + f];
    if (q.shift) v = __fmul_rn(__fadd_rn(v, q.shift[ci]), q.scale[ci]);
    return v;
}

// out [B][nr][in]: raw - the row's T_b - 4 feature rows; else its T_b sequence rows; zeros behind them
__global__ void __launch_bounds__(256) k_sv_intake(SvIntake q, SvGeom g, float* __restrict__ out, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ci = (int)(i % q.in);
    const size_t row = i / q.in;
    const int r = (int)(row % g.nr), b = (int)(row / g.nr), Tb = min(g.T[b], g.Tp);
    float v = 0.0f;
    if (q.raw) {
        if (r < Tb - 4) v = sv_lfr_value(q, b, r, ci);
    } else if (r < Tb) {
        if (r < 4) v = q.embed[(size_t)(r == 0 ? q.lid : (r == 3 ? q.tn : r)) * q.in + ci];
        else v = q.feats ? q.feats[((size_t)b * q.Rs + r - 4) * q.in + ci] : sv_lfr_value(q, b, r - 4, ci);
        v = __fadd_rn(__fmul_rn(v, q.g), q.pos[(size_t)r * q.in + ci]);
    }
    out[i] = v;
}

// ============================================================================ the contraction
struct SvGemm {
    const float* X; int ldx;                                // [B][Tp][ldx]
    const float *lnw, *lnb;                                 // LayerNorm over the K columns in the operand load (null: plain)
    const float* W; const float* bias; int K, N;            // [N][K]; bias may be null
    float* Y; int ldy;                                      // [.][nr][ldy]
    const float* R; int ldr; int relu;                      // residual [B][Tp][ldr] (null: none)
    const float* V; int ldv; const float* dw; int ks, left; // SV_MEM: v [B][Tp][ldv] (N columns), taps [N][ks]
    float* pmax; int32_t* pidx; int nt;                     // SV_ARGMAX: [.][nr][nt]
    SvGeom g;
};

// a 64 x 64 tile, 2 x 2 waves of one 32 x 32 accumulator
template <int MODE>
__global__ void __launch_bounds__(256) k_sv_gemm(SvGemm p) {
    constexpr int TT = 64, TC = 64;
    __shared__ float As[TT][F32_KC + 1];
    __shared__ float Bs[TC][F32_KC + 1];
    __shared__ float St[TT][2];
    __shared__ float Hs[MODE == SV_MEM ? TT + SV_KMAX - 1 : 1][TC + 1];
    __shared__ float Ws[MODE == SV_MEM ? TC : 1][SV_KMAX + 1];
    __shared__ float Rm[MODE == SV_ARGMAX ? TT : 1];
    __shared__ int Ri[MODE == SV_ARGMAX ? TT : 1];
    const int b = blockIdx.z, t0 = blockIdx.x * TT, c0 = blockIdx.y * TC, nr = p.g.nr;
    const int cnt = sv_count(p.g, b), tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t xrow0 = (size_t)(p.g.b0 + b) * p.g.Tp + p.g.t_lo, yrow0 = (size_t)b * nr;
    if (t0 >= cnt) {                                                  // nothing of the row here: zeros (uniform over the block)
        if constexpr (MODE != SV_ARGMAX) f32_tile_zero<TT, TC>(p.Y, p.ldy, yrow0, t0, c0, nr, p.N);
        return;
    }
    if (p.lnw) {                                                      // the statistics of the tile's own rows
        for (int r = wave; r < TT; r += 4) {
            float mean = 0.0f, rstd = 0.0f;
            if (t0 + r < cnt) wave_mean_rstd(p.X + (xrow0 + t0 + r) * p.ldx, p.K, SV_LN_EPS, mean, rstd);
            if (lane == 0) { St[r][0] = mean; St[r][1] = rstd; }
        }
        __syncthreads();
    }
    f32x16_t acc[1] = {};
    const int wt = (wave & 1) * 32, wc = (wave >> 1) * 32, kh = lane >> 5, l31 = lane & 31;
    for (int ci0 = 0; ci0 < p.K; ci0 += F32_KC) {
#pragma unroll
        for (int n = 0; n < TT * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, ci = ci0 + (i & 31), t = t0 + r;
            float v = 0.0f;
            if (ci < p.K && t < cnt) {
                v = p.X[(xrow0 + t) * p.ldx + ci];
                if (p.lnw) v = (v - St[r][0]) * St[r][1] * p.lnw[ci] + p.lnb[ci];
            }
            As[r][i & 31] = v;
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
    // C/D: column (output channel) = lane & 31, row (frame) = f32_tile_row(r, lane >> 5)
    const int co = c0 + wc + l31;
    const float add = (co < p.N && p.bias) ? p.bias[co] : 0.0f;
    if constexpr (MODE == SV_ARGMAX) {
        float bm[16]; int bi[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {                                // over the wave's 32 columns: the lanes of one half
            float v = co < p.N ? acc[0][r] + add : -INFINITY;
            int ix = co < p.N ? co : 0x7fffffff;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) {
                const float ov = __shfl_xor(v, o, 64);
                const int oi = __shfl_xor(ix, o, 64);
                if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
            }
            bm[r] = v; bi[r] = ix;
        }
        if (wc == 32 && l31 == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { Rm[wt + f32_tile_row(r, kh)] = bm[r]; Ri[wt + f32_tile_row(r, kh)] = bi[r]; }
        }
        __syncthreads();
        if (wc == 0 && l31 == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = wt + f32_tile_row(r, kh), t = t0 + rl;
                if (t >= cnt) continue;
                float v = bm[r]; int ix = bi[r];
                if (Rm[rl] > v) { v = Rm[rl]; ix = Ri[rl]; }          // the upper columns win only when greater
                p.pmax[(yrow0 + t) * p.nt + blockIdx.y] = v;
                p.pidx[(yrow0 + t) * p.nt + blockIdx.y] = ix;
            }
        }
        return;
    }
    if constexpr (MODE == SV_MEM) {
        const int L = p.ks, nh = TT + L - 1;
        for (int i = tid; i < nh * TC; i += 256) {
            const int h = i >> 6, cl = i & 63, t = t0 - p.left + h;
            Hs[h][cl] = (c0 + cl < p.N && t >= 0 && t < cnt) ? p.V[(xrow0 + t) * p.ldv + c0 + cl] : 0.0f;
        }
        for (int i = tid; i < TC * L; i += 256) {
            const int cl = i / L, j = i - cl * L;
            Ws[cl][j] = c0 + cl < p.N ? p.dw[(size_t)(c0 + cl) * L + j] : 0.0f;
        }
        __syncthreads();
    }
    if (co >= p.N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rl = wt + f32_tile_row(r, kh), t = t0 + rl;
        if (t >= nr) continue;
        float v = acc[0][r] + add;
        if constexpr (MODE == SV_MEM) {                               // v[t] + sum_j w[j] v[t + j - left], taps ascending
            float a = 0.0f;
            for (int j = 0; j < p.ks; ++j) a = fmaf(Ws[wc + l31][j], Hs[rl + j][wc + l31], a);
            v += Hs[rl + p.left][wc + l31] + a;
        }
        if (p.relu) v = fmaxf(v, 0.0f);
        if (p.R && t < cnt) v = p.R[(xrow0 + t) * p.ldr + co] + v;
        p.Y[(yrow0 + t) * p.ldy + co] = t < cnt ? v : 0.0f;
    }
}

// ============================================================================ attention
struct SvAttn {
    const float* qkv; int ld, koff, voff;                    // q at column h hd, k at koff + h hd, v at voff + h hd
    float* out; int ldo;
    const int32_t* T; int Tp, hd;
    float scale;                                             // q x scale at the load
};

template <int ND>
__global__ void __launch_bounds__(128) k_sv_attn(SvAttn p) {
    constexpr int HD = 32 * ND, LDH = HD + 1;
    __shared__ float Ks[32][LDH];
    __shared__ float Vs[32][LDH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 64, n = min(p.T[b], p.Tp), hd = p.hd;
    const size_t rowbase = (size_t)b * p.Tp;
    if (q0 >= n) {                                                  // (uniform over the block)
        for (int i = tid; i < 64 * hd; i += 128) {
            const int t = q0 + i / hd;
            if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + i % hd] = 0.0f;
        }
        return;
    }
    // the lane's query fragment: query wave 32 + l31, columns 2 i + kh
    float Qr[HD / 2];
    {
        const int tq = q0 + wave * 32 + l31;
#pragma unroll
        for (int i = 0; i < HD / 2; ++i) {
            const int c = 2 * i + kh;
            Qr[i] = (tq < n && c < hd) ? p.qkv[(rowbase + tq) * p.ld + h * hd + c] * p.scale : 0.0f;
        }
    }
    f32x16_t O[ND];
#pragma unroll
    for (int dn = 0; dn < ND; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dn][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    for (int kb = 0; kb < n; kb += 32) {                            // key tiles in ascending order, no split over keys
        __syncthreads();                                            // the previous tile's reads are done
        for (int i = tid; i < 32 * HD; i += 128) {
            const int r = i / HD, c = i - r * HD, key = kb + r;
            const bool ok = key < n && c < hd;
            const size_t at = (rowbase + key) * p.ld + h * hd + c;
            Ks[r][c] = ok ? p.qkv[at + p.koff] : 0.0f;
            Vs[r][c] = ok ? p.qkv[at + p.voff] : 0.0f;
        }
        __syncthreads();
        // S^T[key][query] = K Q^T: the lane holds query l31 and keys f32_tile_row(r, kh)
        f32x16_t S;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[r] = 0.0f;
#pragma unroll
        for (int i = 0; i < HD / 2; ++i) S = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[l31][2 * i + kh], Qr[i], S, 0, 0, 0);
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s = (kb + f32_tile_row(r, kh) < n) ? S[r] : -INFINITY;
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
            for (int r = 0; r < 16; ++r) O[dn] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[f32_tile_row(r, kh)][dn * 32 + l31], S[r], O[dn], 0, 0, 0);
        }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    __syncthreads();                                                // the key tiles are free: a wave's 32 x HD outputs go through one of them
    float* Os = wave == 0 ? &Ks[0][0] : &Vs[0][0];
#pragma unroll
    for (int dn = 0; dn < ND; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) Os[l31 * LDH + dn * 32 + f32_tile_row(r, kh)] = O[dn][r] / l_tot;
    __syncthreads();
    for (int i = tid; i < 64 * hd; i += 128) {
        const int r = i / hd, c = i - r * hd, t = q0 + r;
        if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + c] = t < n ? (r < 32 ? Ks : Vs)[r & 31][c] : 0.0f;
    }
}

// ============================================================================ norms and the tail
// y = LayerNorm(x) over d columns, a wave per row; zero rows behind a row's own T_b.  In place is allowed (a wave reads its row before it writes it).
__global__ void __launch_bounds__(256) k_sv_ln(const float* x, float* y, const float* __restrict__ w, const float* __restrict__ bvec,
                                               const int32_t* __restrict__ T, int Tp, int M, int d) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + (size_t)row * d;
    float* yr = y + (size_t)row * d;
    if (row % Tp >= T[row / Tp]) {
        for (int c = lane; c < d; c += 64) yr[c] = 0.0f;
        return;
    }
    float mean, rstd;
    wave_mean_rstd(xr, d, SV_LN_EPS, mean, rstd);
    for (int c = lane; c < d; c += 64) yr[c] = (xr[c] - mean) * rstd * w[c] + bvec[c];
}

// log-softmax of the rows of a chunk of logits [.][nr][V] in place, a wave per row; dead rows stay zero
__global__ void __launch_bounds__(256) k_sv_logsoftmax(float* __restrict__ lg, int V, int M, SvGeom g) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    if (row % g.nr >= sv_count(g, row / g.nr)) return;
    float* x = lg + (size_t)row * V;
    float mx = -INFINITY;
    for (int i = lane; i < V; i += 64) mx = fmaxf(mx, x[i]);
    mx = wave_max(mx);
    float s = 0.0f;
    for (int i = lane; i < V; i += 64) s += expf(x[i] - mx);
    const float lse = logf(wave_sum(s));
    for (int i = lane; i < V; i += 64) x[i] = (x[i] - mx) - lse;
}

// One block per row.  pred[t] = the arg-max of frame t from the tiles' pairs in tile order (a later tile wins only when greater: MLX argMax);
// rich[b] = pred[0..2]; greedy CTC over frames 4..T_b - 1: a token is kept when it differs from the previous frame's (none before frame 4)
// and is not blank 0; the kept tokens are compacted in frame order into tokens[b][0 .. ntok[b]).
__global__ void __launch_bounds__(256) k_sv_decode(const float* __restrict__ pmax, const int32_t* __restrict__ pidx, int nt, int V,
                                                   const int32_t* __restrict__ T, int Tp, int32_t* __restrict__ pred, int32_t* __restrict__ tokens,
                                                   int32_t* __restrict__ ntok, int32_t* __restrict__ rich) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = min(T[b], Tp);
    int32_t* p = pred + (size_t)b * Tp;
    for (int t = tid; t < n; t += 256) {
        const float* m = pmax + ((size_t)b * Tp + t) * nt;
        const int32_t* ix = pidx + ((size_t)b * Tp + t) * nt;
        float best = -INFINITY;
        int idx = 0x7fffffff;
        for (int k = 0; k < nt; ++k) {
            const float v = m[k];
            if (v > best || (v == best && ix[k] < idx)) { best = v; idx = ix[k]; }
        }
        p[t] = (idx < 0 || idx >= V) ? 0 : idx;                     // (a frame of NaNs: no comparison holds)
    }
    __syncthreads();
    if (tid < 3) rich[b * 3 + tid] = tid < n ? p[tid] : 0;
    int base = 0;
    for (int c0 = 4; c0 < n; c0 += 256) {
        const int t = c0 + tid;
        int tok = 0;
        bool keep = false;
        if (t < n) { tok = p[t]; keep = tok != 0 && tok != (t > 4 ? p[t - 1] : -1); }
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(mask);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        if (keep) tokens[(size_t)b * Tp + off + before] = tok;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) ntok[b] = base;
}

// ============================================================================ host
struct SvLin { const float *w, *b; int cin, cout; };
struct SvLayer { SvLin qkv, out, w1, w2; const float *dw, *n1w, *n1b, *n2w, *n2b; int cin; };

struct mis_sensevoice {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_sensevoice_config cfg{};
    int D = 0, H = 0, dk = 0, Fd = 0, In = 0, V = 0, nm = 0, wlen = 0, hop = 0, m = 0, n = 0, lp = 0, ks = 0, left = 0, N1 = 0, NL = 0, nt = 0;
    int Fcap = 0, Tcap = 0, maxN = 0;
    HostWeights raw{"SenseVoice", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<float> farena, work, pcm;
    DevBuf<int32_t> iarena, counts, iwork;                  // filter bin ranges; N | F | T; pidx | pred | tokens | ntok | rich
    PinnedBuf<int32_t> host_tokens;
    std::vector<int32_t> hN, hF, hT;
    const float *win = nullptr, *twc = nullptr, *tws = nullptr, *fb = nullptr, *shift = nullptr, *scale = nullptr, *embed = nullptr, *pos = nullptr;
    const float *anw = nullptr, *anb = nullptr, *tnw = nullptr, *tnb = nullptr;
    const int32_t* fbr = nullptr;
    SvLin head{};
    std::vector<SvLayer> layers;
    float *rowscale = nullptr, *fbank = nullptr, *x0 = nullptr, *featbuf = nullptr, *hA = nullptr, *hB = nullptr, *qkv = nullptr, *att = nullptr,
          *ff = nullptr, *pmax = nullptr, *logits = nullptr;
    int32_t *pidx = nullptr, *pred = nullptr, *tokens = nullptr, *ntok = nullptr, *rich = nullptr;
    int batch = 0, Tp = 0, Fp = 0, launches = 0;
    bool last_front = false;
    HipEvents<4 + 2 * SV_TIMED_CHUNKS> ev;
    int timed_chunks = -1;                                  // -1: the last call was a generate (ev[2] .. ev[3] is the head)
    float ms[3] = {0.0f, 0.0f, 0.0f};
    bool have_ms = false;
};

static int sv_frames_of(const mis_sensevoice* c, int64_t n) { return n < c->wlen ? 0 : (int)(1 + (n - c->wlen) / c->hop); }
static int sv_rows_of(const mis_sensevoice* c, int F) { return 4 + (F + c->n - 1) / c->n; }

extern "C" mis_status mis_sensevoice_create(const mis_sensevoice_config* cfg, int device, mis_sensevoice** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    // the configuration is judged before the device is touched
    MIS_REQUIRE(cfg->output_size >= 1 && cfg->output_size <= 4096, MIS_ERR_INVALID_INPUT, "output_size %d unsupported (1..4096)", cfg->output_size);
    MIS_REQUIRE(cfg->attention_heads >= 1 && cfg->output_size % cfg->attention_heads == 0, MIS_ERR_INVALID_INPUT,
                "attention_heads %d does not divide output_size %d", cfg->attention_heads, cfg->output_size);
    const int dk = cfg->output_size / cfg->attention_heads;
    MIS_REQUIRE(dk <= 128, MIS_ERR_INVALID_INPUT, "head size %d unsupported (1..128)", dk);
    MIS_REQUIRE(cfg->linear_units >= 1 && cfg->linear_units <= 16384, MIS_ERR_INVALID_INPUT, "linear_units %d unsupported (1..16384)", cfg->linear_units);
    MIS_REQUIRE(cfg->num_blocks >= 0 && cfg->num_blocks <= 256 && cfg->tp_blocks >= 0 && cfg->tp_blocks <= 256, MIS_ERR_INVALID_INPUT,
                "num_blocks %d / tp_blocks %d unsupported (0..256)", cfg->num_blocks, cfg->tp_blocks);
    MIS_REQUIRE(cfg->kernel_size >= 1 && cfg->kernel_size <= SV_KMAX, MIS_ERR_INVALID_INPUT, "kernel_size %d unsupported (1..%d)", cfg->kernel_size, SV_KMAX);
    const int left = (cfg->kernel_size - 1) / 2 + (cfg->sanm_shift > 0 ? cfg->sanm_shift : 0);
    MIS_REQUIRE(left <= cfg->kernel_size - 1, MIS_ERR_INVALID_INPUT, "sanm_shift %d leaves a negative right padding at kernel_size %d", cfg->sanm_shift,
                cfg->kernel_size);
    MIS_REQUIRE(cfg->vocab_size >= 1 && cfg->vocab_size <= (1 << 20), MIS_ERR_INVALID_INPUT, "vocab_size %d unsupported (1..2^20)", cfg->vocab_size);
    MIS_REQUIRE(cfg->n_mels >= 1 && cfg->n_mels <= 128, MIS_ERR_INVALID_INPUT, "n_mels %d unsupported (1..128)", cfg->n_mels);
    MIS_REQUIRE(cfg->lfr_m >= 1 && cfg->lfr_m <= 64 && cfg->lfr_n >= 1 && cfg->lfr_n <= 64, MIS_ERR_INVALID_INPUT, "lfr_m %d / lfr_n %d unsupported (1..64)",
                cfg->lfr_m, cfg->lfr_n);
    MIS_REQUIRE(cfg->input_size == cfg->n_mels * cfg->lfr_m, MIS_ERR_INVALID_INPUT, "input_size %d is not n_mels x lfr_m = %d", cfg->input_size,
                cfg->n_mels * cfg->lfr_m);
    MIS_REQUIRE(cfg->sample_rate >= 1000 && cfg->sample_rate <= 192000 && cfg->frame_length >= 1 && cfg->frame_shift >= 1, MIS_ERR_INVALID_INPUT,
                "sample_rate / frame_length / frame_shift unsupported");
    const int64_t wlen = (int64_t)cfg->sample_rate * cfg->frame_length / 1000, hop = (int64_t)cfg->sample_rate * cfg->frame_shift / 1000;
    MIS_REQUIRE(wlen > SV_NFFT / 2 && wlen <= SV_NFFT, MIS_ERR_INVALID_INPUT,
                "a window of %lld samples is unsupported (257..512: the next power of two must be 512)", (long long)wlen);
    MIS_REQUIRE(hop >= 1 && hop <= 4096, MIS_ERR_INVALID_INPUT, "a frame shift of %lld samples is unsupported (1..4096)", (long long)hop);
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= SV_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch must be 1..%d", SV_MAX_BATCH);
    MIS_REQUIRE(cfg->max_seconds >= 1 && cfg->max_seconds <= 600, MIS_ERR_INVALID_INPUT, "max_seconds must be 1..600");
    MIS_REQUIRE(cfg->head_rows >= 1 && cfg->head_rows <= (1 << 20), MIS_ERR_INVALID_INPUT, "head_rows must be 1..%d", 1 << 20);
    hipStream_t stream = mis_open_stream(device);
    auto c = std::make_unique<mis_sensevoice>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->D = cfg->output_size; c->H = cfg->attention_heads; c->dk = dk; c->Fd = cfg->linear_units; c->In = cfg->input_size; c->V = cfg->vocab_size;
    c->nm = cfg->n_mels; c->wlen = (int)wlen; c->hop = (int)hop; c->m = cfg->lfr_m; c->n = cfg->lfr_n; c->lp = (cfg->lfr_m - 1) / 2;
    c->ks = cfg->kernel_size; c->left = left; c->N1 = 1 + std::max(cfg->num_blocks - 1, 0); c->NL = c->N1 + cfg->tp_blocks;
    c->nt = cdiv(cfg->vocab_size, 64);
    c->maxN = cfg->max_seconds * cfg->sample_rate; c->Fcap = std::max(1, sv_frames_of(c.get(), c->maxN)); c->Tcap = sv_rows_of(c.get(), c->Fcap);
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_sensevoice_destroy(mis_sensevoice* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// names as SenseVoiceModel.sanitize leaves them: embed.weight [16, input_size]; encoder.{encoders0.0, encoders.N, tp_encoders.N}.
// {self_attn.linear_q_k_v, self_attn.linear_out, feed_forward.w_1, feed_forward.w_2, norm1, norm2}.{weight,bias} and
// .self_attn.fsmn_block.weight [output_size, kernel_size, 1] (the torch layout [output_size, 1, kernel_size] holds the same values in
// the same order and is taken too); encoder.after_norm / tp_norm.{weight,bias}; ctc_lo.{weight,bias}; optional cmvn.shift / cmvn.scale
extern "C" mis_status mis_sensevoice_set_tensor(mis_sensevoice* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 3, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

static std::string sv_layer_name(const mis_sensevoice* c, int i) {
    if (i == 0) return "encoder.encoders0.0";
    if (i < c->N1) return "encoder.encoders." + std::to_string(i - 1);
    return "encoder.tp_encoders." + std::to_string(i - c->N1);
}

extern "C" mis_status mis_sensevoice_finalize(mis_sensevoice* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t D = c->D, Fd = c->Fd, In = c->In, V = c->V, nm = c->nm, ks = c->ks;
    HostArena a(c->raw);
    std::vector<float>& fh = a.fhost;
    auto lin = [&](const std::string& p, int64_t cout, int64_t cin, SvLin& l) {
        l = SvLin{nullptr, nullptr, (int)cin, (int)cout};
        a.fvec(p + ".weight", {cout, cin}, cout * cin, l.w);
        a.fvec(p + ".bias", {cout}, cout, l.b);
    };
    a.fvec("embed.weight", {16, In}, 16 * In, c->embed);
    c->layers.assign(c->NL, SvLayer{});
    for (int i = 0; i < c->NL; ++i) {
        const std::string q = sv_layer_name(c, i);
        SvLayer& L = c->layers[i];
        L.cin = i == 0 ? (int)In : (int)D;
        a.fvec(q + ".norm1.weight", {L.cin}, L.cin, L.n1w); a.fvec(q + ".norm1.bias", {L.cin}, L.cin, L.n1b);
        lin(q + ".self_attn.linear_q_k_v", 3 * D, L.cin, L.qkv);
        lin(q + ".self_attn.linear_out", D, D, L.out);
        const HostTensor& dw = c->raw.need(q + ".self_attn.fsmn_block.weight");
        MIS_REQUIRE(dw.shape == std::vector<int64_t>({D, ks, 1}) || dw.shape == std::vector<int64_t>({D, 1, ks}), MIS_ERR_INVALID_INPUT,
                    "SenseVoice weight %s.self_attn.fsmn_block.weight has the wrong shape", q.c_str());
        const size_t o_dw = a.ftake(D * ks, L.dw);
        for (int64_t j = 0; j < D * ks; ++j) fh[o_dw + j] = dw.v[j];
        a.fvec(q + ".norm2.weight", {D}, D, L.n2w); a.fvec(q + ".norm2.bias", {D}, D, L.n2b);
        lin(q + ".feed_forward.w_1", Fd, D, L.w1);
        lin(q + ".feed_forward.w_2", D, Fd, L.w2);
    }
    a.fvec("encoder.after_norm.weight", {D}, D, c->anw); a.fvec("encoder.after_norm.bias", {D}, D, c->anb);
    a.fvec("encoder.tp_norm.weight", {D}, D, c->tnw); a.fvec("encoder.tp_norm.bias", {D}, D, c->tnb);
    lin("ctc_lo", V, D, c->head);
    // CMVN: applied when both tensors are there; they must have the feature width
    const HostTensor *sh = c->raw.find("cmvn.shift"), *sc = c->raw.find("cmvn.scale");
    c->shift = c->scale = nullptr;
    if (sh || sc) {
        MIS_REQUIRE(sh && sc && (int64_t)sh->v.size() == In && (int64_t)sc->v.size() == In, MIS_ERR_INVALID_INPUT,
                    "SenseVoice: cmvn.shift and cmvn.scale must both hold input_size = %lld values", (long long)In);
        const size_t o_shift = a.ftake(In, c->shift), o_scale = a.ftake(In, c->scale);
        for (int64_t i = 0; i < In; ++i) { fh[o_shift + i] = sh->v[i]; fh[o_scale + i] = sc->v[i]; }
    }
    // front end: the window and the filters in the reference's own f32 arithmetic (DSP.swift), [bin][mel]; twiddles
    const size_t o_win = a.ftake(c->wlen, c->win), o_twc = a.ftake(SV_NFFT / 2, c->twc), o_tws = a.ftake(SV_NFFT / 2, c->tws),
                 o_fb = a.ftake((size_t)SV_BINS * nm, c->fb);
    {
        const float pi = 3.14159265358979323846f, denom = (float)(c->wlen - 1);
        for (int i = 0; i < c->wlen; ++i) {
            const float cs = cosf(2.0f * pi * (float)i / denom);
            fh[o_win + i] = c->cfg.window_hann ? 0.5f * (1.0f - cs) : 0.54f - 0.46f * cs;
        }
    }
    fft512_twiddles(&fh[o_twc], &fh[o_tws]);
    std::vector<int32_t> ih((size_t)round_up(2 * nm, 64), 0);
    {
        auto hz_to_mel = [](float f) { return 2595.0f * log10f(1.0f + f / 700.0f); };
        auto mel_to_hz = [](float m) { return 700.0f * (powf(10.0f, m / 2595.0f) - 1.0f); };
        const float sr = (float)c->cfg.sample_rate, m_min = hz_to_mel(20.0f), m_max = hz_to_mel(sr / 2.0f);
        std::vector<float> fp(nm + 2);
        for (int i = 0; i < nm + 2; ++i) fp[i] = mel_to_hz(m_min + (float)i * (m_max - m_min) / (float)(nm + 1));
        for (int i = 0; i < SV_BINS; ++i) {
            const float fr = (float)i * sr / (float)SV_NFFT;
            for (int j = 0; j < nm; ++j) {
                const float low = fp[j], center = fp[j + 1], high = fp[j + 2];
                float w = 0.0f;
                if (fr >= low && fr < center) w = (fr - low) / (center - low);
                else if (fr >= center && fr <= high) w = (high - fr) / (high - center);
                fh[o_fb + (size_t)i * nm + j] = w;
            }
        }
        filter_bin_ranges(&fh[o_fb], SV_BINS, (int)nm, ih.data());
    }
    // the sinusoid of positions 1 .. Tcap over input_size columns: sin | cos halves, zero-padded or cut; formed in double, rounded once
    const size_t o_pos = a.ftake((size_t)c->Tcap * In, c->pos);
    {
        const int half = std::max((int)In / 2, 1);
        const double inc = log(10000.0) / (double)std::max(half - 1, 1);
        for (int r = 0; r < c->Tcap; ++r)
            for (int ci = 0; ci < In && ci < 2 * half; ++ci) {
                const int k = ci < half ? ci : ci - half;
                const double ang = (double)(r + 1) * exp(-inc * (double)k);
                fh[o_pos + (size_t)r * In + ci] = (float)(ci < half ? sin(ang) : cos(ang));
            }
    }
    // ---- the workspace, sized once (no call reads the handle before finalized is set: a rejected finalize can be repeated)
    const size_t B = c->cfg.max_batch, rows = B * (size_t)c->Tcap, frames = B * (size_t)c->Fcap, HR = c->cfg.head_rows;
    const size_t per_row = 2 * In + 6 * D + Fd + c->nt;
    const size_t total = frames * nm + rows * per_row + HR * V + 64 * 32;
    const size_t itotal = rows * (c->nt + 2) + 64 * 16;
    MIS_REQUIRE((total + itotal + B * (size_t)c->maxN) * 4 <= ((size_t)24 << 30), MIS_ERR_INVALID_INPUT,
                "max_batch x max_seconds (+ head_rows) needs a workspace of %zu MiB (at most 24 GiB)", (total + itotal + B * (size_t)c->maxN) * 4 >> 20);
    DevBuf<bf16_t> none;
    a.upload(none, c->farena);
    c->iarena.alloc(ih.size());
    HIP_CHECK(hipMemcpy(c->iarena.p, ih.data(), ih.size() * 4, hipMemcpyHostToDevice));
    c->work.alloc(total);
    c->iwork.alloc(itotal);
    c->pcm.alloc(B * (size_t)c->maxN);
    c->counts.alloc(3 * SV_MAX_BATCH);
    c->host_tokens.alloc(rows + 4 * SV_MAX_BATCH);
    c->hN.assign(SV_MAX_BATCH, 0); c->hF.assign(SV_MAX_BATCH, 0); c->hT.assign(SV_MAX_BATCH, 0);
    float* w = c->work.p;
    auto take = [&](size_t n) { float* p = w; w += round_up(n, 64); return p; };
    c->rowscale = take(64); c->fbank = take(frames * nm); c->x0 = take(rows * In); c->featbuf = take(rows * In); c->hA = take(rows * D);
    c->hB = take(rows * D); c->qkv = take(rows * 3 * D); c->att = take(rows * D); c->ff = take(rows * Fd); c->pmax = take(rows * c->nt);
    c->logits = take(HR * V);
    int32_t* iw = c->iwork.p;
    auto itake = [&](size_t n) { int32_t* p = iw; iw += round_up(n, 64); return p; };
    c->pidx = itake(rows * c->nt); c->pred = itake(rows); c->tokens = itake(rows); c->ntok = itake(64); c->rich = itake(3 * 64);
    c->fbr = c->iarena.p;
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of a sanitized checkpoint and a CMVN
extern "C" mis_status mis_sensevoice_init_synthetic(mis_sensevoice* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    sw.put("embed.weight", {16, c->In}, 0.5, 0.0f);
    for (int i = 0; i < c->NL; ++i) {
        const std::string q = sv_layer_name(c, i);
        const int cin = i == 0 ? c->In : c->D;
        sw.norm(q + ".norm1", cin);
        sw.lin(q + ".self_attn.linear_q_k_v", 3 * c->D, cin, true, 1.0);
        sw.lin(q + ".self_attn.linear_out", c->D, c->D, true, 0.5);
        sw.put(q + ".self_attn.fsmn_block.weight", {c->D, c->ks, 1}, 0.5 * sqrt(3.0 / (double)c->ks), 0.0f);
        sw.norm(q + ".norm2", c->D);
        sw.lin(q + ".feed_forward.w_1", c->Fd, c->D, true, 1.0);
        sw.lin(q + ".feed_forward.w_2", c->D, c->Fd, true, 0.5);
    }
    sw.norm("encoder.after_norm", c->D);
    sw.norm("encoder.tp_norm", c->D);
    sw.lin("ctc_lo", c->V, c->D, true, 2.0);
    sw.put("cmvn.shift", {c->In}, 1.0, -8.0f);
    sw.put("cmvn.scale", {c->In}, 0.05, 0.2f);
    MIS_API_END
}

extern "C" int mis_sensevoice_launches(const mis_sensevoice* c) { return c ? c->launches : 0; }

extern "C" mis_status mis_sensevoice_frames(const mis_sensevoice* c, const int64_t* lens, int batch, int32_t* frames, int32_t* rows) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && lens && batch >= 0, MIS_ERR_INVALID_INPUT, "bad argument");
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(lens[b] >= 0 && lens[b] < ((int64_t)1 << 40), MIS_ERR_INVALID_INPUT, "row %d: bad length", b);
        const int64_t F = lens[b] < c->wlen ? 0 : 1 + (lens[b] - c->wlen) / c->hop;
        MIS_REQUIRE(F < (1 << 30), MIS_ERR_INVALID_INPUT, "row %d: too many frames", b);
        if (frames) frames[b] = (int32_t)F;
        if (rows) rows[b] = sv_rows_of(c, (int)F);
    }
    MIS_API_END
}

// ---------------------------------------------------------------------------- the chain
static void sv_check_ready(const mis_sensevoice* c, int batch, int lid, int textnorm) {
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "SenseVoice model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch must be 1..%d (max_batch)", c->cfg.max_batch);
    MIS_REQUIRE(lid >= 0 && lid < 16 && textnorm >= 0 && textnorm < 16, MIS_ERR_INVALID_INPUT, "query ids %d / %d outside the 16 embeddings", lid, textnorm);
}
static SvGeom sv_geom(const mis_sensevoice* c) { return SvGeom{c->counts.p + 2 * SV_MAX_BATCH, c->Tp, 0, 0, c->Tp}; }

static void sv_upload_counts(mis_sensevoice* c, int B) {
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpyAsync(c->counts.p, c->hN.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->counts.p + SV_MAX_BATCH, c->hF.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->counts.p + 2 * SV_MAX_BATCH, c->hT.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
}

// pcm f32 [B][stride] -> c->fbank [B][Fp][nm]; 2 launches
static void sv_front(mis_sensevoice* c, const float* pcm, const int64_t* lens, int B, int64_t stride) {
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    int64_t nmax = 1;
    int Fp = 1, Tp = 4;
    for (int b = 0; b < B; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 0 && n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples, the row stride is %lld", b, (long long)n, (long long)stride);
        MIS_REQUIRE(n <= c->maxN, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the workspace of %d seconds (max_seconds); rows are not truncated", b,
                    (long long)n, c->cfg.max_seconds);
        c->hN[b] = (int32_t)n; c->hF[b] = sv_frames_of(c, n); c->hT[b] = sv_rows_of(c, c->hF[b]);
        nmax = std::max(nmax, n); Fp = std::max(Fp, c->hF[b]); Tp = std::max(Tp, c->hT[b]);
    }
    MIS_REQUIRE(Fp <= c->Fcap && Tp <= c->Tcap, MIS_ERR_GENERATION_FAILED, "row geometry outside the workspace");
    c->batch = B; c->Fp = Fp; c->Tp = Tp; c->last_front = true;
    hipStream_t s = c->stream;
    HIP_CHECK(hipEventRecord(c->ev[0], s));
    sv_upload_counts(c, B);
    // the rows are packed at the longest row's length: only a row's own samples (and the padding up to the longest) travel
    HIP_CHECK(hipMemcpy2DAsync(c->pcm.p, (size_t)nmax * 4, pcm, (size_t)stride * 4, (size_t)nmax * 4, B, hipMemcpyHostToDevice, s));
    MIS_LAUNCH(c, k_sv_peak, dim3(B), dim3(256), c->pcm.p, nmax, c->counts.p, c->rowscale);
    SvFront fp{c->pcm.p, nmax, c->rowscale, c->win, c->twc, c->tws, c->fb, c->fbr, c->counts.p + SV_MAX_BATCH, c->fbank, Fp, c->wlen, c->hop, c->nm,
               (float)log((double)1e-10f)};
    MIS_LAUNCH(c, k_sv_fbank, dim3(Fp, B), dim3(256), fp);
}

static SvIntake sv_intake_params(const mis_sensevoice* c, int lid, int tn, bool raw, const float* feats, int Rs) {
    return SvIntake{c->fbank, c->Fp, c->counts.p + SV_MAX_BATCH, feats, Rs, c->shift, c->scale, c->embed, c->pos, (float)sqrt((double)c->D),
                    c->nm, c->n, c->lp, c->In, lid, tn, raw ? 1 : 0};
}
// c->x0 [B][Tp][In] from the fbank (feats null) or from given features; 1 launch
static void sv_intake(mis_sensevoice* c, int lid, int tn, const float* feats, int Rs) {
    const size_t total = (size_t)c->batch * c->Tp * c->In;
    MIS_LAUNCH(c, k_sv_intake, dim3((unsigned)((total + 255) / 256)), dim3(256), sv_intake_params(c, lid, tn, false, feats, Rs), sv_geom(c), c->x0, total);
}

template <int MODE>
static void sv_launch_gemm(mis_sensevoice* c, const SvGemm& g, int nb) {
    MIS_LAUNCH(c, (k_sv_gemm<MODE>), dim3(cdiv(g.g.nr, 64), cdiv(g.N, 64), nb), dim3(256), g);
}
static SvGemm sv_lin_gemm(const mis_sensevoice* c, const SvLin& l, const float* X, int ldx, float* Y) {
    SvGemm g{};
    g.X = X; g.ldx = ldx; g.W = l.w; g.bias = l.b; g.K = l.cin; g.N = l.cout; g.Y = Y; g.ldy = l.cout; g.g = sv_geom(c);
    return g;
}
static void sv_launch_attn(mis_sensevoice* c, const SvAttn& p, int heads, int B) {
    const dim3 grid(cdiv(p.Tp, 64), heads, B);
    if (p.hd <= 32) MIS_LAUNCH(c, (k_sv_attn<1>), grid, dim3(128), p);
    else if (p.hd <= 64) MIS_LAUNCH(c, (k_sv_attn<2>), grid, dim3(128), p);
    else MIS_LAUNCH(c, (k_sv_attn<4>), grid, dim3(128), p);
}
static void sv_launch_ln(mis_sensevoice* c, const float* x, float* y, const float* w, const float* b) {
    const int M = c->batch * c->Tp;
    MIS_LAUNCH(c, k_sv_ln, dim3(cdiv(M, 4)), dim3(256), x, y, w, b, c->counts.p + 2 * SV_MAX_BATCH, c->Tp, M, c->D);
}

// The encoder from c->x0.  stop < 0: all of it, the result in c->hA.  Else the stages of the tap: 0 .. NL - 1 the layers in order with
// after_norm behind layer N1 - 1 (stage N1), tp_norm last; returns the buffer that holds stage `stop`.
static const float* sv_encoder(mis_sensevoice* c, int stop) {
    const bool norm = c->cfg.normalize_before != 0;
    const int B = c->batch, D = c->D;
    int stage = 0;
    for (int i = 0; i < c->NL; ++i, ++stage) {
        const SvLayer& L = c->layers[i];
        const float* hin = i == 0 ? c->x0 : c->hB;
        SvGemm g = sv_lin_gemm(c, L.qkv, hin, L.cin, c->qkv);
        if (norm) { g.lnw = L.n1w; g.lnb = L.n1b; }
        sv_launch_gemm<SV_PLAIN>(c, g, B);
        sv_launch_attn(c, SvAttn{c->qkv, 3 * D, D, 2 * D, c->att, D, c->counts.p + 2 * SV_MAX_BATCH, c->Tp, c->dk, 1.0f / sqrtf((float)c->dk)}, c->H, B);
        g = sv_lin_gemm(c, L.out, c->att, D, c->hA);
        g.V = c->qkv + 2 * D; g.ldv = 3 * D; g.dw = L.dw; g.ks = c->ks; g.left = c->left;
        if (i > 0) { g.R = hin; g.ldr = D; }
        sv_launch_gemm<SV_MEM>(c, g, B);
        g = sv_lin_gemm(c, L.w1, c->hA, D, c->ff);
        if (norm) { g.lnw = L.n2w; g.lnb = L.n2b; }
        g.relu = 1;
        sv_launch_gemm<SV_PLAIN>(c, g, B);
        g = sv_lin_gemm(c, L.w2, c->ff, c->Fd, c->hB);
        g.R = c->hA; g.ldr = D;
        sv_launch_gemm<SV_PLAIN>(c, g, B);
        if (stage == stop) return c->hB;
        if (i == c->N1 - 1) {
            sv_launch_ln(c, c->hB, c->hB, c->anw, c->anb);
            ++stage;
            if (stage == stop) return c->hB;
        }
    }
    sv_launch_ln(c, c->hB, c->hA, c->tnw, c->tnb);
    return c->hA;
}

// the forward head: log-probabilities of every (row, frame) through the logits scratch, chunk by chunk, into out [B][Tp][V]
static void sv_head_forward(mis_sensevoice* c, float* out) {
    hipStream_t s = c->stream;
    const int B = c->batch, Tp = c->Tp, HR = c->cfg.head_rows, V = c->V;
    int chunks = 0;
    auto one = [&](int b0, int nb, int t_lo, int nr) {
        SvGemm g = sv_lin_gemm(c, c->head, c->hA, c->D, c->logits);
        g.g = SvGeom{c->counts.p + 2 * SV_MAX_BATCH, Tp, b0, t_lo, nr};
        const bool timed = chunks < SV_TIMED_CHUNKS;
        if (timed) HIP_CHECK(hipEventRecord(c->ev[4 + 2 * chunks], s));
        sv_launch_gemm<SV_PLAIN>(c, g, nb);
        const int M = nb * nr;
        MIS_LAUNCH(c, k_sv_logsoftmax, dim3(cdiv(M, 4)), dim3(256), c->logits, V, M, g.g);
        if (timed) HIP_CHECK(hipEventRecord(c->ev[5 + 2 * chunks], s));
        HIP_CHECK(hipMemcpyAsync(out + ((size_t)b0 * Tp + t_lo) * V, c->logits, (size_t)M * V * 4, hipMemcpyDeviceToHost, s));
        ++chunks;
    };
    if (HR >= Tp) {
        const int per = HR / Tp;
        for (int b0 = 0; b0 < B; b0 += per) one(b0, std::min(per, B - b0), 0, Tp);
    } else {
        for (int b = 0; b < B; ++b)
            for (int t_lo = 0; t_lo < Tp; t_lo += HR) one(b, 1, t_lo, std::min(HR, Tp - t_lo));
    }
    c->timed_chunks = std::min(chunks, SV_TIMED_CHUNKS);
}

// after the call's synchronisation: the three device intervals
static void sv_collect_ms(mis_sensevoice* c, bool front) {
    c->ms[0] = 0.0f;
    if (front) HIP_CHECK(hipEventElapsedTime(&c->ms[0], c->ev[0], c->ev[1]));
    HIP_CHECK(hipEventElapsedTime(&c->ms[1], c->ev[1], c->ev[2]));
    if (c->timed_chunks < 0) HIP_CHECK(hipEventElapsedTime(&c->ms[2], c->ev[2], c->ev[3]));
    else {
        c->ms[2] = 0.0f;
        for (int i = 0; i < c->timed_chunks; ++i) {
            float t = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&t, c->ev[4 + 2 * i], c->ev[5 + 2 * i]));
            c->ms[2] += t;
        }
    }
    c->have_ms = true;
}

// pcm f32 [batch, stride] -> LFR + CMVN features f32 [batch, rows, input_size], rows >= the longest row's T_b - 4; zeros behind a row's own
extern "C" mis_status mis_sensevoice_features(mis_sensevoice* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* features,
                                              int rows) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && features, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    sv_check_ready(c, batch, 0, 0);
    c->launches = 0; c->have_ms = false;
    sv_front(c, pcm, lens, batch, stride);
    const int R = c->Tp - 4;
    MIS_REQUIRE(rows >= std::max(R, 1), MIS_ERR_INVALID_INPUT, "features: room for %d rows, %d are needed", rows, std::max(R, 1));
    const size_t total = (size_t)batch * rows * c->In;
    SvGeom g = sv_geom(c);
    g.nr = rows;
    MIS_REQUIRE((size_t)rows <= (size_t)c->Tcap, MIS_ERR_INVALID_INPUT, "features: %d rows exceed the workspace of %d", rows, c->Tcap);
    MIS_LAUNCH(c, k_sv_intake, dim3((unsigned)((total + 255) / 256)), dim3(256), sv_intake_params(c, 0, 0, true, nullptr, 0), g, c->featbuf, total);
    HIP_CHECK(hipMemcpyAsync(features, c->featbuf, total * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    MIS_API_END
}

static void sv_finish_forward(mis_sensevoice* c, float* logp, bool front) {
    hipStream_t s = c->stream;
    HIP_CHECK(hipEventRecord(c->ev[1], s));
    sv_encoder(c, -1);
    HIP_CHECK(hipEventRecord(c->ev[2], s));
    sv_head_forward(c, logp);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    sv_collect_ms(c, front);
}

// SenseVoiceModel.callAsFunction on given features f32 [batch, rows, input_size], counts[batch] valid rows each (NULL = rows) ->
// log-probabilities f32 [batch, 4 + rows, vocab_size], zeros behind a row's own 4 + counts[b]
extern "C" mis_status mis_sensevoice_forward_features(mis_sensevoice* c, const float* features, const int32_t* counts, int batch, int rows, int lid,
                                                      int textnorm, float* logp) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && features && logp, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    sv_check_ready(c, batch, lid, textnorm);
    MIS_REQUIRE(rows >= 0 && rows + 4 <= c->Tcap, MIS_ERR_INVALID_INPUT, "%d feature rows exceed the workspace of %d (max_seconds %d)", rows, c->Tcap - 4,
                c->cfg.max_seconds);
    for (int b = 0; b < batch; ++b) {
        const int r = counts ? counts[b] : rows;
        MIS_REQUIRE(r >= 0 && r <= rows, MIS_ERR_INVALID_INPUT, "row %d: %d feature rows (0 .. %d are served)", b, r, rows);
        c->hN[b] = 0; c->hF[b] = 0; c->hT[b] = 4 + r;
    }
    c->launches = 0; c->have_ms = false;
    c->batch = batch; c->Tp = 4 + rows; c->Fp = 1; c->last_front = false;
    sv_upload_counts(c, batch);
    if (rows > 0) HIP_CHECK(hipMemcpyAsync(c->featbuf, features, (size_t)batch * rows * c->In * 4, hipMemcpyHostToDevice, c->stream));
    sv_intake(c, lid, textnorm, c->featbuf, rows);
    sv_finish_forward(c, logp, false);
    MIS_API_END
}

// front end + callAsFunction: log-probabilities f32 [batch, Tmax, vocab_size], Tmax the longest row's T_b
extern "C" mis_status mis_sensevoice_forward(mis_sensevoice* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int lid, int textnorm,
                                             float* logp) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && logp, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    sv_check_ready(c, batch, lid, textnorm);
    c->launches = 0; c->have_ms = false;
    sv_front(c, pcm, lens, batch, stride);
    sv_intake(c, lid, textnorm, nullptr, 0);
    sv_finish_forward(c, logp, true);
    MIS_API_END
}

extern "C" mis_status mis_stt_sensevoice_generate(mis_sensevoice* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int lid,
                                                  int textnorm, int32_t* tokens_out, int64_t tokens_stride, int32_t* n_tokens, int32_t* rich_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && tokens_out && n_tokens && rich_out && tokens_stride >= 1, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipSetDevice(c->device));
    sv_check_ready(c, batch, lid, textnorm);
    c->launches = 0; c->have_ms = false;
    hipStream_t s = c->stream;
    sv_front(c, pcm, lens, batch, stride);
    sv_intake(c, lid, textnorm, nullptr, 0);
    HIP_CHECK(hipEventRecord(c->ev[1], s));
    sv_encoder(c, -1);
    HIP_CHECK(hipEventRecord(c->ev[2], s));
    SvGemm g = sv_lin_gemm(c, c->head, c->hA, c->D, nullptr);
    g.pmax = c->pmax; g.pidx = c->pidx; g.nt = c->nt;
    sv_launch_gemm<SV_ARGMAX>(c, g, batch);
    MIS_LAUNCH(c, k_sv_decode, dim3(batch), dim3(256), c->pmax, c->pidx, c->nt, c->V, c->counts.p + 2 * SV_MAX_BATCH, c->Tp, c->pred, c->tokens, c->ntok,
               c->rich);
    HIP_CHECK(hipEventRecord(c->ev[3], s));
    c->timed_chunks = -1;
    const size_t M = (size_t)batch * c->Tp;
    int32_t* ht = c->host_tokens.p;
    HIP_CHECK(hipMemcpyAsync(ht, c->tokens, M * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ht + M, c->ntok, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ht + M + SV_MAX_BATCH, c->rich, (size_t)batch * 12, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));                               // the call's one synchronisation
    for (int b = 0; b < batch; ++b) {
        const int n = (int)std::min<int64_t>(ht[M + b], tokens_stride);
        n_tokens[b] = n;
        memcpy(tokens_out + (size_t)b * tokens_stride, ht + (size_t)b * c->Tp, (size_t)n * 4);
        for (int k = 0; k < 3; ++k) rich_out[b * 3 + k] = ht[M + SV_MAX_BATCH + b * 3 + k];
    }
    sv_collect_ms(c, true);
    MIS_API_END
}

// tensors of the last call, f32, zeros behind a row's own rows.  stage 0 fbank [B, Fmax, n_mels] (a call from pcm), 1 the intake
// [B, Tmax, input_size], 2 + i the stages of the encoder in the order they run [B, Tmax, output_size]: the first stack's layers, after_norm,
// the tp layers, tp_norm (3 + L stages).  The chain is deterministic and the intake is still in the workspace: an encoder stage is
// recomputed from it (the same bits as the call produced).
extern "C" mis_status mis_sensevoice_tap(mis_sensevoice* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && dims, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized && c->batch > 0, MIS_ERR_INVALID_INPUT, "no call to tap");
    MIS_REQUIRE(stage >= 0 && stage <= 3 + c->NL, MIS_ERR_INVALID_INPUT, "stage %d outside 0..%d", stage, 3 + c->NL);
    MIS_REQUIRE(stage >= 1 || c->last_front, MIS_ERR_INVALID_INPUT, "the last call had no front end");
    HIP_CHECK(hipSetDevice(c->device));
    const size_t B = c->batch, n = stage == 0 ? c->Fp : c->Tp, width = stage == 0 ? c->nm : (stage == 1 ? c->In : c->D);
    dims[0] = (int64_t)B; dims[1] = (int64_t)n; dims[2] = (int64_t)width;
    if (!out) return MIS_OK;
    MIS_REQUIRE((int64_t)(B * n * width) <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    const float* src = stage == 0 ? c->fbank : c->x0;
    if (stage >= 2) {
        const int kept = c->launches;
        src = sv_encoder(c, stage - 2);
        c->launches = kept;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(out, src, B * n * width * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// measurements: device milliseconds of the last generate / forward, ms[3] = front end (copy in + peak + fbank + intake), encoder, head
// (generate: the fused head + arg-max and the decode; forward: the head GEMM + log-softmax of its first 64 chunks, copies excluded)
extern "C" mis_status mis_debug_sensevoice_timing(const mis_sensevoice* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && ms, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->have_ms, MIS_ERR_INVALID_INPUT, "no generate or forward to time");
    for (int i = 0; i < 3; ++i) ms[i] = c->ms[i];
    MIS_API_END
}

// ============================================================================ test scaffolding (include/mi_speech_debug.h)
// ONE launch line of sv_encoder / mis_stt_sensevoice_generate on caller-supplied host data.  Nothing is computed here: the operands are
// uploaded as given and what the launch wrote is copied back.  Guards as the other debug entry points (debug_guard.h): every output is
// [guard | body | guard], all of it the byte 0xFF before the launch; every input is followed by IN_GUARD NaNs (ints: 0x7FFFFFFF).
#include "debug_guard.h"

namespace {
constexpr int64_t SVD_MAX_ELEMS = (int64_t)1 << 28;
const float* svd_f(const DevBuf<uint32_t>& d) { return reinterpret_cast<const float*>(d.p); }
const int32_t* svd_i(const DevBuf<uint32_t>& d) { return reinterpret_cast<const int32_t*>(d.p); }
}  // namespace

extern "C" mis_status mis_debug_sensevoice_attn(int device, const float* qkv, int ld, int koff, int voff, const int32_t* cnt, int batch, int Tp, int heads,
                                                int hd, float scale, int ldo, float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(qkv && cnt && out && batch >= 1 && batch <= 65535 && Tp >= 1 && heads >= 1 && heads <= 65535 && hd >= 1 && hd <= 128, MIS_ERR_INVALID_INPUT,
                "SenseVoice attention: qkv, cnt, out, positive batch, Tp, heads and hd 1..128 are required");
    MIS_REQUIRE(koff >= 0 && voff >= 0 && heads * hd <= ld && koff + heads * hd <= ld && voff + heads * hd <= ld && heads * hd <= ldo, MIS_ERR_INVALID_INPUT,
                "SenseVoice attention: the heads leave the rows");
    MIS_REQUIRE((int64_t)batch * Tp * ld <= SVD_MAX_ELEMS && (int64_t)batch * Tp * ldo <= SVD_MAX_ELEMS, MIS_ERR_INVALID_INPUT, "SenseVoice attention: tensor too large");
    mis_sensevoice c;
    HIP_CHECK(hipSetDevice(device));
    c.device = device;
    DevBuf<uint32_t> dq, dc;
    alloc32(dq, qkv, (size_t)batch * Tp * ld, F32_NAN);
    alloc32(dc, cnt, batch, 0x7FFFFFFFu);
    GuardedOut o;
    o.alloc((size_t)batch * Tp * ldo * 4, 1 << 16);
    sv_launch_attn(&c, SvAttn{svd_f(dq), ld, koff, voff, reinterpret_cast<float*>(o.p()), ldo, svd_i(dc), Tp, hd, scale}, heads, batch);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    MIS_REQUIRE(c.launches == 1, MIS_ERR_GENERATION_FAILED, "%d launches where one was meant", c.launches);
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
    MIS_API_END
}

extern "C" mis_status mis_debug_sensevoice_head_argmax(int device, const float* X, const float* W, const float* bias, const int32_t* cnt, int batch, int Tp,
                                                       int K, int N, float* pmax_out, int32_t* pidx_out, int32_t* pred_out, int32_t* tokens_out,
                                                       int32_t* ntok_out, int32_t* rich_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(X && W && cnt && pmax_out && pidx_out && pred_out && tokens_out && ntok_out && rich_out, MIS_ERR_INVALID_INPUT, "SenseVoice head: null argument");
    MIS_REQUIRE(batch >= 1 && batch <= 65535 && Tp >= 1 && K >= 1 && N >= 1, MIS_ERR_INVALID_INPUT, "SenseVoice head: positive batch, Tp, K, N are required");
    const int nt = cdiv(N, 64);
    MIS_REQUIRE((int64_t)batch * Tp * K <= SVD_MAX_ELEMS && (int64_t)N * K <= SVD_MAX_ELEMS && (int64_t)batch * Tp * nt <= SVD_MAX_ELEMS, MIS_ERR_INVALID_INPUT,
                "SenseVoice head: tensor too large");
    mis_sensevoice c;
    HIP_CHECK(hipSetDevice(device));
    c.device = device;
    const size_t M = (size_t)batch * Tp;
    DevBuf<uint32_t> dx, dw, db, dc;
    alloc32(dx, X, M * K, F32_NAN);
    alloc32(dw, W, (size_t)N * K, F32_NAN);
    if (bias) alloc32(db, bias, N, F32_NAN);
    alloc32(dc, cnt, batch, 0x7FFFFFFFu);
    GuardedOut om, oi, op, ot, on, orc;
    om.alloc(M * nt * 4, 1 << 16); oi.alloc(M * nt * 4, 1 << 16); op.alloc(M * 4, 4096); ot.alloc(M * 4, 4096); on.alloc((size_t)batch * 4, 4096);
    orc.alloc((size_t)batch * 12, 4096);
    SvGemm g{};
    g.X = svd_f(dx); g.ldx = K; g.W = svd_f(dw); g.bias = bias ? svd_f(db) : nullptr; g.K = K; g.N = N;
    g.pmax = reinterpret_cast<float*>(om.p()); g.pidx = reinterpret_cast<int32_t*>(oi.p()); g.nt = nt;
    g.g = SvGeom{svd_i(dc), Tp, 0, 0, Tp};
    sv_launch_gemm<SV_ARGMAX>(&c, g, batch);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    MIS_REQUIRE(c.launches == 1, MIS_ERR_GENERATION_FAILED, "%d launches where one was meant", c.launches);
    om.check_guards(); oi.check_guards();
    HIP_CHECK(hipMemcpy(pmax_out, om.p(), om.body, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(pidx_out, oi.p(), oi.body, hipMemcpyDeviceToHost));
    // the combine launch on what the first wrote
    MIS_LAUNCH(&c, k_sv_decode, dim3(batch), dim3(256), g.pmax, g.pidx, nt, N, svd_i(dc), Tp, reinterpret_cast<int32_t*>(op.p()),
               reinterpret_cast<int32_t*>(ot.p()), reinterpret_cast<int32_t*>(on.p()), reinterpret_cast<int32_t*>(orc.p()));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    op.check_guards(); ot.check_guards(); on.check_guards(); orc.check_guards();
    HIP_CHECK(hipMemcpy(pred_out, op.p(), op.body, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(tokens_out, ot.p(), ot.body, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(ntok_out, on.p(), on.body, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(rich_out, orc.p(), orc.body, hipMemcpyDeviceToHost));
    MIS_API_END
}
