// ecapa_lid.hip - spoken language identification: waveform -> SpeechBrain log-mel -> ECAPA-TDNN -> classifier -> log-probabilities, top-k.
//
// Reference being replaced: EcapaTdnn (Sources/MLXAudioLID/Models/EcapaTdnn/EcapaTdnnLID.swift:13-195), EcapaClassifier
// (EcapaTdnnLayers.swift:52-78), EcapaMelSpectrogram.swift:15-55 on stft / melFilters / powerToDB (MLXAudioCore/DSP.swift:25-227), and the
// shared backbone built with reflectPadding false and globalContext true (MLXAudioCodecs/EcapaTdnn/EcapaTdnnBackbone.swift:16-282).
//
// One call serves 1..max_batch ragged rows.  Row b has n_b samples and T_b = n_b / 160 + 1 frames; activations are f32 [B][Ts][C]
// (channels contiguous, Ts = the longest row of the call) inside one workspace sized at finalize.  Every kernel takes the frame counts:
// a load at t outside [0, T_b) is a zero whatever the buffer holds, every epilogue writes zeros at t >= T_b, and every reduction over time
// runs in an order that T_b alone fixes (four interleaved partial sums met in a fixed order), so a row's result is the same bit for bit
// whatever batch it travels in.
//
//   k_lid_gemm      the one contraction of the file, exact f32 on v_mfma_f32_32x32x2_f32: out[t][co] = sum_j sum_ci W[co][j][ci] x[t + (j -
//                   (k - 1) / 2) d][ci], 64 frames x 64 output channels per block, K staged through LDS 32 at a time with the edges of
//                   every dimension guarded (60 mels, C / 8 channels per Res2Net chunk).  Loads: activations (optionally the sum of two, the
//                   Res2Net chunk + previous output), windowed frames of the zero-padded signal (the DFT as a 400 -> 402 product), or the
//                   power of a spectrum (the mel filters).  Epilogues: plain, BN(ReLU(. + bias)), tanh of that, 10 log10 max(., 1e-10);
//                   a per-row bias carries the broadcast mean / std columns of the pooling's attention input. (On f32_tile.h.)
//   k_lid_clamp     the row's maximum over its own frames and all mels, minus 80 dB, as a floor (powerToDB topDB, DSP.swift:68-70)
//   k_lid_meannorm  sentenceMeanNormalize (EcapaTdnnLID.swift:84-86)
//   k_lid_time_stats  per-row, per-channel mean over the valid frames (SE squeeze) and sqrt(population variance + 1e-9) (pooling context)
//   k_lid_se_gate / k_lid_se_apply   1x1 -> ReLU -> 1x1 -> sigmoid; gate * x + residual, masked
//   k_lid_rowbias   the global-context columns of asp.tdnn.conv folded into a bias per row
//   k_lid_asp_pool  softmax over the valid frames, weighted mean, sqrt(max(sum a x^2 - mean^2, 1e-9)) (EcapaTdnnBackbone.swift:275-280)
//   k_lid_tail / k_lid_head   asp_bn + fc; LeakyReLU -> BN -> Linear -> LeakyReLU -> BN -> Linear -> log-softmax -> top-k by rank
//
// The block-wide maximum and sum of k_lid_clamp and k_lid_head are common.h's block_max_256 / block_sum_256.
// The Res2Net chain runs as scale - 1 launches of k_lid_gemm per block (chunk 0 is stored twice by tdnn1's epilogue): 49 launches a call
// at the published depth.  No allocation and no synchronisation between the copy in and the copy out.
#include "common.h"
#include "f32_tile.h"
#include "host_weights.h"
#include "step_loop.h"

#include <math.h>
#include <string.h>
#include <memory>

#define LID_MAX_BATCH 64
#define LID_NFFT 400
#define LID_HOP 160
#define LID_NBIN 201
#define LID_BN_EPS 1e-5           // MLXNN.BatchNorm default

enum { LID_EPI_PLAIN = 0, LID_EPI_RELU_BN = 1, LID_EPI_RELU_BN_TANH = 2, LID_EPI_DB = 3 };
enum { LID_LOAD_ACT = 0, LID_LOAD_FRAMES = 1, LID_LOAD_POWER = 2 };

struct LidGemm {
    const float* X; int ldx;            // ACT / POWER: [B][Ts][ldx]
    const float* X2; int ldx2;          // ACT: optional addend of the same frames
    const float* pcm; int64_t pcm_stride; const int64_t* nsamp; const float* win;      // FRAMES
    const float* W; int ldw;            // [Cout][ldw], the first taps * Cin columns are read
    const float* bias; const float* rowbias; const float* bn_s; const float* bn_b;
    float* Y; int ldy; float* Y2; int ldy2, y2_cols;
    const int32_t* T; int Ts;
    int Cin, Cout, taps, dil, epi, load;
};

__global__ void __launch_bounds__(256) k_lid_gemm(LidGemm p) {
    constexpr int TT = F32_TILE, TC = F32_TILE;
    __shared__ float As[TT][F32_KC + 1];
    __shared__ float Bs[TC][F32_KC + 1];
    const int b = blockIdx.z, t0 = blockIdx.x * TT, c0 = blockIdx.y * TC;
    const int Tb = p.T[b], tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t row0 = (size_t)b * p.Ts;
    if (t0 >= Tb) {                                                   // nothing of the row here: the padding is written as zeros
        f32_tile_zero<TT, TC>(p.Y, p.ldy, row0, t0, c0, p.Ts, p.Cout);
        if (p.Y2) f32_tile_zero<TT, TC>(p.Y2, p.ldy2, row0, t0, c0, p.Ts, min(p.Cout, p.y2_cols));
        return;
    }
    f32x16_t acc[1] = {};
    const int wt = (wave & 1) * 32, wc = (wave >> 1) * 32, kh = lane >> 5, l31 = lane & 31, half = (p.taps - 1) / 2;
    const int64_t ns = p.load == LID_LOAD_FRAMES ? p.nsamp[b] : 0;
    for (int j = 0; j < p.taps; ++j) {
        const int shift = (j - half) * p.dil;
        for (int ci0 = 0; ci0 < p.Cin; ci0 += F32_KC) {
#pragma unroll
            for (int n = 0; n < TT * F32_KC / 256; ++n) {
                const int i = tid + n * 256, r = i >> 5, ci = ci0 + (i & 31), t = t0 + r + shift;
                float v = 0.0f;
                if (ci < p.Cin && t >= 0 && t < Tb) {
                    if (p.load == LID_LOAD_ACT) {
                        v = p.X[(row0 + t) * p.ldx + ci];
                        if (p.X2) v += p.X2[(row0 + t) * p.ldx2 + ci];
                    } else if (p.load == LID_LOAD_FRAMES) {           // sample q of the signal with 200 zeros on each side
                        const int64_t q = (int64_t)t * LID_HOP + ci - LID_NFFT / 2;
                        if (q >= 0 && q < ns) v = p.pcm[(int64_t)b * p.pcm_stride + q] * p.win[ci];
                    } else {
                        const float re = p.X[(row0 + t) * p.ldx + ci], im = p.X[(row0 + t) * p.ldx + LID_NBIN + ci];
                        v = re * re + im * im;
                    }
                }
                As[r][i & 31] = v;
            }
#pragma unroll
            for (int n = 0; n < TC * F32_KC / 256; ++n) {
                const int i = tid + n * 256, r = i >> 5, ci = ci0 + (i & 31), co = c0 + r;
                Bs[r][i & 31] = (co < p.Cout && ci < p.Cin) ? p.W[(size_t)co * p.ldw + (size_t)j * p.Cin + ci] : 0.0f;
            }
            __syncthreads();
            f32_tile_mfma(As, Bs, wt + l31, wc + l31, kh, acc);
            __syncthreads();
        }
    }
    const int co = c0 + wc + l31;                                   // C/D: column = lane & 31, row = f32_tile_row(r, lane >> 5)
    if (co >= p.Cout) return;
    float add = p.bias ? p.bias[co] : 0.0f;
    if (p.rowbias) add += p.rowbias[(size_t)b * p.Cout + co];
    const float s = p.bn_s ? p.bn_s[co] : 1.0f, sh = p.bn_b ? p.bn_b[co] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = t0 + wt + f32_tile_row(r, kh);
        if (t >= p.Ts) continue;
        float v = acc[0][r] + add;
        if (p.epi == LID_EPI_RELU_BN || p.epi == LID_EPI_RELU_BN_TANH) {
            v = fmaxf(v, 0.0f) * s + sh;
            if (p.epi == LID_EPI_RELU_BN_TANH) v = tanhf(v);
        } else if (p.epi == LID_EPI_DB) {
            v = 10.0f * log10f(fmaxf(v, 1e-10f));
        }
        if (t >= Tb) v = 0.0f;
        p.Y[(row0 + t) * p.ldy + co] = v;
        if (p.Y2 && co < p.y2_cols) p.Y2[(row0 + t) * p.ldy2 + co] = v;
    }
}

// mel [B][Ts][nm] in place: floor at (the row's maximum over t < T_b and all mels) - 80; one block per row
__global__ void __launch_bounds__(256) k_lid_clamp(float* __restrict__ mel, const int32_t* __restrict__ T, int Ts, int nm) {
    __shared__ float red[4];
    const int b = blockIdx.x, n = T[b] * nm;
    float* row = mel + (size_t)b * Ts * nm;
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 256) mx = fmaxf(mx, row[i]);
    mx = block_max_256(mx, red);
    const float floor_db = mx - 80.0f;
    for (int i = threadIdx.x; i < n; i += 256) row[i] = fmaxf(row[i], floor_db);
}

// feat[b][t][m] = mel[b][t][m] - mean_t mel[b][.][m]; the mean as four interleaved partial sums; grid (B), zeros at t >= T_b
__global__ void __launch_bounds__(256) k_lid_meannorm(const float* __restrict__ mel, float* __restrict__ feat, const int32_t* __restrict__ T,
                                                      int Ts, int nm) {
    extern __shared__ float sm[];                                     // part[4][nm] | mean[nm]
    const int b = blockIdx.x, Tb = T[b], ph = threadIdx.x >> 6;
    const float* row = mel + (size_t)b * Ts * nm;
    for (int m = threadIdx.x & 63; m < nm; m += 64) {
        float a = 0.0f;
        for (int t = ph; t < Tb; t += 4) a += row[(size_t)t * nm + m];
        sm[ph * nm + m] = a;
    }
    __syncthreads();
    for (int m = threadIdx.x; m < nm; m += 256) sm[4 * nm + m] = ((sm[m] + sm[nm + m]) + (sm[2 * nm + m] + sm[3 * nm + m])) / (float)Tb;
    __syncthreads();
    float* out = feat + (size_t)b * Ts * nm;
    for (int i = threadIdx.x; i < Ts * nm; i += 256) {
        const int t = i / nm, m = i - t * nm;
        out[i] = t < Tb ? row[i] - sm[4 * nm + m] : 0.0f;
    }
}

// mean[b][c] over t < T_b of x[b][t][c] and, with sd, sqrt(population variance + 1e-9) around that mean; grid (ceil(C / 64), B)
__global__ void __launch_bounds__(256) k_lid_time_stats(const float* __restrict__ x, int ldx, const int32_t* __restrict__ T, int Ts, int C,
                                                        float* __restrict__ mean, float* __restrict__ sd) {
    __shared__ float part[4][64];
    __shared__ float mu[64];
    const int b = blockIdx.y, ph = threadIdx.x >> 6, cl = threadIdx.x & 63, c = blockIdx.x * 64 + cl, Tb = T[b];
    const float* col = x + (size_t)b * Ts * ldx + (c < C ? c : 0);
    float a = 0.0f;
    if (c < C) for (int t = ph; t < Tb; t += 4) a += col[(size_t)t * ldx];
    part[ph][cl] = a;
    __syncthreads();
    if (ph == 0) {
        const float m = ((part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl])) / (float)Tb;
        mu[cl] = m;
        if (c < C) mean[(size_t)b * C + c] = m;
    }
    if (!sd) return;
    __syncthreads();
    const float m = mu[cl];
    a = 0.0f;
    if (c < C) for (int t = ph; t < Tb; t += 4) { const float dv = col[(size_t)t * ldx] - m; a += dv * dv; }
    part[ph][cl] = a;
    __syncthreads();
    if (ph == 0 && c < C) sd[(size_t)b * C + c] = sqrtf(((part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl])) / (float)Tb + 1e-9f);
}

// one output per wave: w . x over K (lanes stride the columns, the 64 partial sums meet in wave_sum's fixed order)
__device__ __forceinline__ float lid_wave_dot(const float* __restrict__ w, const float* x, int K) {
    float a = 0.0f;
    for (int k = threadIdx.x & 63; k < K; k += 64) a = fmaf(w[k], x[k], a);
    return wave_sum(a);
}

// gate[b][c] = sigmoid(W2[c] . relu(W1 mean[b] + b1) + b2) (SEBlock, EcapaTdnnBackbone.swift:187-192); grid (ceil(C / 64), B): every
// block forms the se hidden units itself, then its 64 gates
__global__ void __launch_bounds__(256) k_lid_se_gate(const float* __restrict__ mean, const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ w2, const float* __restrict__ b2, int C, int se,
                                                     float* __restrict__ gate) {
    extern __shared__ float sm[];                                     // mean[C] | hidden[se]
    float* hid = sm + C;
    const int b = blockIdx.y, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < C; i += 256) sm[i] = mean[(size_t)b * C + i];
    __syncthreads();
    for (int j = wave; j < se; j += 4) {
        const float v = lid_wave_dot(w1 + (size_t)j * C, sm, C) + b1[j];
        if ((threadIdx.x & 63) == 0) hid[j] = fmaxf(v, 0.0f);
    }
    __syncthreads();
    for (int i = wave; i < 64; i += 4) {
        const int c = blockIdx.x * 64 + i;
        if (c >= C) break;
        const float v = lid_wave_dot(w2 + (size_t)c * se, hid, se) + b2[c];
        if ((threadIdx.x & 63) == 0) gate[(size_t)b * C + c] = 1.0f / (1.0f + expf(-v));
    }
}

// y[b][t][c] = x[b][t][c] gate[b][c] + res[b][t][c], zero at t >= T_b (SERes2NetBlock, :231-238)
__global__ void __launch_bounds__(256) k_lid_se_apply(const float* __restrict__ x, const float* __restrict__ gate, const float* __restrict__ res,
                                                      int ldr, float* __restrict__ y, int ldy, const int32_t* __restrict__ T, int Ts, int C,
                                                      size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const size_t r = i / C;
    const int t = (int)(r % Ts), b = (int)(r / Ts);
    y[r * ldy + c] = t < T[b] ? x[i] * gate[(size_t)b * C + c] + res[r * ldr + c] : 0.0f;
}

// rb[b][a] = W[a][C3 .. 2 C3) . mean[b] + W[a][2 C3 .. 3 C3) . sd[b]: what the broadcast columns of the attention input contribute
// (:260-267); grid (ceil(A / 4), B), a wave per unit
__global__ void __launch_bounds__(256) k_lid_rowbias(const float* __restrict__ w, int C3, int A, const float* __restrict__ mean,
                                                     const float* __restrict__ sd, float* __restrict__ rb) {
    const int b = blockIdx.y, a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= A) return;
    const float* wr = w + (size_t)a * 3 * C3;
    const float v = lid_wave_dot(wr + C3, mean + (size_t)b * C3, C3) + lid_wave_dot(wr + 2 * C3, sd + (size_t)b * C3, C3);
    if ((threadIdx.x & 63) == 0) rb[(size_t)b * A + a] = v;
}

// pooled[b][c] = sum_t a x, pooled[b][C3 + c] = sqrt(max(sum_t a x^2 - mean^2, 1e-9)), a = softmax over t < T_b of the scores (:275-280);
// grid (ceil(C3 / 64), B), four interleaved partial sums per channel
__global__ void __launch_bounds__(256) k_lid_asp_pool(const float* __restrict__ x, const float* __restrict__ sc, const int32_t* __restrict__ T,
                                                      int Ts, int C3, float* __restrict__ pooled) {
    __shared__ float part[3][4][64];
    __shared__ float mxs[64];
    const int b = blockIdx.y, ph = threadIdx.x >> 6, cl = threadIdx.x & 63, c = blockIdx.x * 64 + cl, Tb = T[b];
    const size_t base = (size_t)b * Ts * C3 + (c < C3 ? c : 0);
    float mx = -INFINITY;
    if (c < C3) for (int t = ph; t < Tb; t += 4) mx = fmaxf(mx, sc[base + (size_t)t * C3]);
    part[0][ph][cl] = mx;
    __syncthreads();
    if (ph == 0) mxs[cl] = fmaxf(fmaxf(part[0][0][cl], part[0][1][cl]), fmaxf(part[0][2][cl], part[0][3][cl]));
    __syncthreads();
    mx = mxs[cl];
    float se = 0.0f, sx = 0.0f, sxx = 0.0f;
    if (c < C3) for (int t = ph; t < Tb; t += 4) {
        const float e = expf(sc[base + (size_t)t * C3] - mx), v = x[base + (size_t)t * C3];
        se += e; sx = fmaf(e, v, sx); sxx = fmaf(e * v, v, sxx);
    }
    part[0][ph][cl] = se; part[1][ph][cl] = sx; part[2][ph][cl] = sxx;
    __syncthreads();
    if (ph == 0 && c < C3) {
        const float e = (part[0][0][cl] + part[0][1][cl]) + (part[0][2][cl] + part[0][3][cl]);
        const float m = ((part[1][0][cl] + part[1][1][cl]) + (part[1][2][cl] + part[1][3][cl])) / e;
        const float m2 = ((part[2][0][cl] + part[2][1][cl]) + (part[2][2][cl] + part[2][3][cl])) / e;
        pooled[(size_t)b * 2 * C3 + c] = m;
        // (the product is rounded on its own: contracted into the subtraction, a constant channel would leave its rounding error here)
        pooled[(size_t)b * 2 * C3 + C3 + c] = sqrtf(fmaxf(__fsub_rn(m2, __fmul_rn(m, m)), 1e-9f));
    }
}

// emb[b][e] = fc[e] . asp_bn(pooled[b]) + bias[e]; grid (ceil(E / 8), B), two units a wave
__global__ void __launch_bounds__(256) k_lid_tail(const float* __restrict__ pooled, const float* __restrict__ bn_s, const float* __restrict__ bn_b,
                                                  const float* __restrict__ w, const float* __restrict__ bias, int K, int E,
                                                  float* __restrict__ emb) {
    extern __shared__ float sm[];                                     // asp_bn(pooled)[K]
    const int b = blockIdx.y, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < K; i += 256) sm[i] = pooled[(size_t)b * K + i] * bn_s[i] + bn_b[i];
    __syncthreads();
    for (int i = wave; i < 8; i += 4) {
        const int e = blockIdx.x * 8 + i;
        if (e >= E) break;
        const float v = lid_wave_dot(w + (size_t)e * K, sm, K) + bias[e];
        if ((threadIdx.x & 63) == 0) emb[(size_t)b * E + e] = v;
    }
}

__device__ __forceinline__ float lid_leaky(float x) { return fmaxf(x, 0.01f * x); }

// EcapaClassifier (EcapaTdnnLayers.swift:63-77) and the top-k of predict (EcapaTdnnLID.swift:59-73): one block per row.  Class i has rank
// #{j : v_j > v_i or (v_j == v_i and j < i)}: descending, ties to the lower index.
struct LidHead {
    const float *emb, *n0s, *n0b, *w1, *b1, *n1s, *n1b, *w2, *b2;
    int E, Hd, N, k;
    float *logp, *top_prob; int32_t* top_idx;
};
__global__ void __launch_bounds__(256) k_lid_head(LidHead p) {
    extern __shared__ float sm[];                                     // x[E] | h[Hd] | logits[N]
    __shared__ float red[4];
    float* x = sm;
    float* h = sm + p.E;
    float* lg = h + p.Hd;
    const int b = blockIdx.x, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < p.E; i += 256) x[i] = lid_leaky(p.emb[(size_t)b * p.E + i]) * p.n0s[i] + p.n0b[i];
    __syncthreads();
    for (int j = wave; j < p.Hd; j += 4) {
        const float v = lid_wave_dot(p.w1 + (size_t)j * p.E, x, p.E) + p.b1[j];
        if ((threadIdx.x & 63) == 0) h[j] = lid_leaky(v) * p.n1s[j] + p.n1b[j];
    }
    __syncthreads();
    for (int n = wave; n < p.N; n += 4) {
        const float v = lid_wave_dot(p.w2 + (size_t)n * p.Hd, h, p.Hd) + p.b2[n];
        if ((threadIdx.x & 63) == 0) lg[n] = v;
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int n = threadIdx.x; n < p.N; n += 256) mx = fmaxf(mx, lg[n]);
    mx = block_max_256(mx, red);
    float s = 0.0f;
    for (int n = threadIdx.x; n < p.N; n += 256) s += expf(lg[n] - mx);
    s = block_sum_256(s, red);
    const float lse = mx + logf(s);
    for (int n = threadIdx.x; n < p.N; n += 256) { const float v = lg[n] - lse; lg[n] = v; p.logp[(size_t)b * p.N + n] = v; }
    __syncthreads();
    if (p.k <= 0) return;
    for (int i = threadIdx.x; i < p.N; i += 256) {
        const float v = lg[i];
        int rank = 0;
        for (int j = 0; j < p.N; ++j) { const float u = lg[j]; rank += (u > v || (u == v && j < i)) ? 1 : 0; }
        if (rank < p.k) { p.top_idx[(size_t)b * p.k + rank] = i; p.top_prob[(size_t)b * p.k + rank] = expf(v); }
    }
}

// ============================================================================ host
struct LidBN { const float *s, *b; };
struct LidTdnn { const float *w, *bias; LidBN bn; int cin, cout, k, dil; };
struct LidBlock { LidTdnn tdnn1, tdnn2; std::vector<LidTdnn> res; const float *se_w1, *se_b1, *se_w2, *se_b2; };

struct mis_ecapa_lid {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_ecapa_lid_config cfg{};
    int nm = 0, C = 0, A = 0, SE = 0, E = 0, Hd = 0, N = 0, S = 0, Tcap = 0;
    HostWeights raw{"ECAPA LID", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<float> farena, work, pcm;
    DevBuf<int64_t> nsamp;
    DevBuf<int32_t> frames, top_idx;
    std::vector<int64_t> h_nsamp;
    std::vector<int32_t> h_frames;
    // weights
    const float *win = nullptr, *dft = nullptr, *filt = nullptr;
    LidTdnn block0{}, mfa{}, asp_tdnn{};
    LidBlock blocks[3];
    const float *asp_w = nullptr, *asp_b = nullptr, *fc_w = nullptr, *fc_b = nullptr, *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
    LidBN asp_bn{}, n0{}, n1{};
    // workspace (floats, for max_batch rows of Tcap frames)
    float *spec = nullptr, *mel = nullptr, *feat = nullptr, *h0 = nullptr, *cat = nullptr, *r = nullptr, *q = nullptr, *u = nullptr, *mf = nullptr,
          *att = nullptr, *sc = nullptr, *mean = nullptr, *sd = nullptr, *gate = nullptr, *rb = nullptr, *pooled = nullptr, *emb = nullptr,
          *logp = nullptr, *top_prob = nullptr;
    int last_batch = 0, last_Ts = 0, last_launches = 0;
    HipEvents<3> ev;
    float ms_front = 0.0f, ms_model = 0.0f;
};

extern "C" mis_status mis_ecapa_lid_create(const mis_ecapa_lid_config* cfg, int device, mis_ecapa_lid** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    // the configuration is judged before the device is touched
    MIS_REQUIRE(cfg->n_mels >= 1 && cfg->n_mels <= 256, MIS_ERR_INVALID_INPUT, "n_mels %d unsupported (1..256)", cfg->n_mels);
    MIS_REQUIRE(cfg->res2net_scale >= 2 && cfg->res2net_scale <= 16, MIS_ERR_INVALID_INPUT, "res2net_scale %d unsupported (2..16)", cfg->res2net_scale);
    MIS_REQUIRE(cfg->channels >= cfg->res2net_scale && cfg->channels <= 4096 && cfg->channels % cfg->res2net_scale == 0, MIS_ERR_INVALID_INPUT,
                "channels %d unsupported (a multiple of res2net_scale, at most 4096)", cfg->channels);
    for (int i = 0; i < 5; ++i) {
        const int k = cfg->kernel_sizes[i];
        MIS_REQUIRE(k == 1 || k == 3 || k == 5, MIS_ERR_INVALID_INPUT, "kernel_sizes[%d] = %d unsupported (1, 3 or 5)", i, k);
        MIS_REQUIRE(cfg->dilations[i] >= 1 && cfg->dilations[i] <= 16, MIS_ERR_INVALID_INPUT, "dilations[%d] = %d unsupported (1..16)", i, cfg->dilations[i]);
    }
    MIS_REQUIRE(cfg->attention_channels >= 1 && cfg->attention_channels <= 4096 && cfg->se_channels >= 1 && cfg->se_channels <= 4096,
                MIS_ERR_INVALID_INPUT, "attention_channels / se_channels unsupported (1..4096)");
    MIS_REQUIRE(cfg->embedding_dim >= 1 && cfg->embedding_dim <= 4096 && cfg->classifier_hidden_dim >= 1 && cfg->classifier_hidden_dim <= 4096 &&
                cfg->num_classes >= 1 && cfg->num_classes <= 4096, MIS_ERR_INVALID_INPUT,
                "embedding_dim / classifier_hidden_dim / num_classes unsupported (1..4096)");
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= LID_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch must be 1..%d", LID_MAX_BATCH);
    MIS_REQUIRE(cfg->max_samples >= 1 && cfg->max_samples <= 16000 * 120, MIS_ERR_INVALID_INPUT, "max_samples must be 1..%d", 16000 * 120);
    hipStream_t stream = mis_open_stream(device);
    auto c = std::make_unique<mis_ecapa_lid>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->nm = cfg->n_mels; c->C = cfg->channels; c->A = cfg->attention_channels; c->SE = cfg->se_channels; c->E = cfg->embedding_dim;
    c->Hd = cfg->classifier_hidden_dim; c->N = cfg->num_classes; c->S = cfg->res2net_scale; c->Tcap = (int)(cfg->max_samples / LID_HOP + 1);
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_ecapa_lid_destroy(mis_ecapa_lid* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// names are the ones EcapaTdnn.sanitize leaves (EcapaTdnnLID.swift:99-131); conv weights [out, k, in]; host pointers
extern "C" mis_status mis_ecapa_lid_set_tensor(mis_ecapa_lid* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape,
                                               int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 3, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

// the TDNN blocks of the model in the order finalize and init_synthetic walk them: name, in, out, kernel, dilation
struct LidTdnnSpec { std::string name; int cin, cout, k, dil; };
static std::vector<LidTdnnSpec> lid_tdnn_specs(const mis_ecapa_lid* c) {
    const int C = c->C, H = C / c->S;
    std::vector<LidTdnnSpec> v;
    const std::string E = "embedding_model.";
    v.push_back({E + "block0", c->nm, C, c->cfg.kernel_sizes[0], 1});                  // (dilations[0] is not passed on, Backbone.swift:29-34)
    for (int i = 1; i <= 3; ++i) {
        const std::string q = E + "block" + std::to_string(i);
        v.push_back({q + ".tdnn1", C, C, 1, 1});
        for (int j = 0; j < c->S - 1; ++j)
            v.push_back({q + ".res2net_block.blocks." + std::to_string(j), H, H, c->cfg.kernel_sizes[i], c->cfg.dilations[i]});
        v.push_back({q + ".tdnn2", C, C, 1, 1});
    }
    v.push_back({E + "mfa", 3 * C, 3 * C, c->cfg.kernel_sizes[4], 1});
    v.push_back({E + "asp.tdnn", 9 * C, c->A, 1, 1});
    return v;
}

extern "C" mis_status mis_ecapa_lid_finalize(mis_ecapa_lid* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const int64_t C = c->C, nm = c->nm, A = c->A, SE = c->SE, E = c->E, Hd = c->Hd, N = c->N;
    HostArena a(c->raw);
    std::vector<float>& fh = a.fhost;
    // BatchNorm in eval mode as scale and shift: y = x s + b, s = weight / sqrt(running_var + eps), b = bias - running_mean s
    auto bn = [&](const std::string& p, int64_t n, LidBN& dst) {
        const HostTensor &w = c->raw.need(p + ".weight", {n}), &b = c->raw.need(p + ".bias", {n}), &m = c->raw.need(p + ".running_mean", {n}),
                         &v = c->raw.need(p + ".running_var", {n});
        const size_t os = a.ftake(n, dst.s), ob = a.ftake(n, dst.b);
        for (int64_t i = 0; i < n; ++i) {
            const double s = (double)w.v[i] / sqrt((double)v.v[i] + LID_BN_EPS);
            fh[os + i] = (float)s;
            fh[ob + i] = (float)((double)b.v[i] - (double)m.v[i] * s);
        }
    };
    auto whole = [&](const std::string& name, std::initializer_list<int64_t> shape, const float*& dst) {
        int64_t n = 1;
        for (auto d : shape) n *= d;
        a.fvec(name, shape, n, dst);
    };
    // the handle's TDNN blocks in the order of the specs
    std::vector<LidTdnn*> tdnn{&c->block0};
    for (LidBlock& bl : c->blocks) {
        bl.res.assign(c->S - 1, LidTdnn{});
        tdnn.push_back(&bl.tdnn1);
        for (LidTdnn& r : bl.res) tdnn.push_back(&r);
        tdnn.push_back(&bl.tdnn2);
    }
    tdnn.push_back(&c->mfa); tdnn.push_back(&c->asp_tdnn);
    const std::vector<LidTdnnSpec> specs = lid_tdnn_specs(c);
    for (size_t i = 0; i < specs.size(); ++i) {
        const LidTdnnSpec& s = specs[i];
        LidTdnn& t = *tdnn[i];
        t = LidTdnn{nullptr, nullptr, LidBN{}, s.cin, s.cout, s.k, s.dil};
        whole(s.name + ".conv.weight", {s.cout, s.k, s.cin}, t.w);
        whole(s.name + ".conv.bias", {s.cout}, t.bias);
        bn(s.name + ".norm", s.cout, t.bn);
    }
    for (int i = 1; i <= 3; ++i) {
        const std::string q = "embedding_model.block" + std::to_string(i) + ".se_block.";
        LidBlock& bl = c->blocks[i - 1];
        whole(q + "conv1.weight", {SE, 1, C}, bl.se_w1); whole(q + "conv1.bias", {SE}, bl.se_b1);
        whole(q + "conv2.weight", {C, 1, SE}, bl.se_w2); whole(q + "conv2.bias", {C}, bl.se_b2);
    }
    whole("embedding_model.asp.conv.weight", {3 * C, 1, A}, c->asp_w); whole("embedding_model.asp.conv.bias", {3 * C}, c->asp_b);
    bn("embedding_model.asp_bn", 6 * C, c->asp_bn);
    whole("embedding_model.fc.weight", {E, 1, 6 * C}, c->fc_w); whole("embedding_model.fc.bias", {E}, c->fc_b);
    bn("classifier.norm", E, c->n0);
    whole("classifier.DNN.block_0.linear.w.weight", {Hd, E}, c->w1); whole("classifier.DNN.block_0.linear.w.bias", {Hd}, c->b1);
    bn("classifier.DNN.block_0.norm", Hd, c->n1);
    whole("classifier.out.w.weight", {N, Hd}, c->w2); whole("classifier.out.w.bias", {N}, c->b2);
    // front end: periodic Hamming window (DSP.swift:25-42), the real DFT as [402][400] (cos rows, then sin rows), HTK filters without
    // normalisation as [n_mels][201] (:76-168), all formed in double
    const size_t o_win = a.ftake(LID_NFFT, c->win), o_dft = a.ftake((size_t)2 * LID_NBIN * LID_NFFT, c->dft), o_filt = a.ftake((size_t)nm * LID_NBIN, c->filt);
    const double PI = 3.14159265358979323846;
    for (int n = 0; n < LID_NFFT; ++n) fh[o_win + n] = (float)(0.54 - 0.46 * cos(2.0 * PI * n / LID_NFFT));
    for (int f = 0; f < LID_NBIN; ++f)
        for (int n = 0; n < LID_NFFT; ++n) {
            const double ph = 2.0 * PI * (double)((f * n) % LID_NFFT) / LID_NFFT;
            fh[o_dft + (size_t)f * LID_NFFT + n] = (float)cos(ph);
            fh[o_dft + (size_t)(LID_NBIN + f) * LID_NFFT + n] = (float)-sin(ph);
        }
    {
        const double m_max = 2595.0 * log10(1.0 + 8000.0 / 700.0);
        std::vector<double> fp(nm + 2);
        for (int i = 0; i < nm + 2; ++i) fp[i] = 700.0 * (pow(10.0, (i * m_max / (double)(nm + 1)) / 2595.0) - 1.0);
        for (int j = 0; j < nm; ++j)
            for (int i = 0; i < LID_NBIN; ++i) {
                const double f = i * 16000.0 / LID_NFFT, lo = fp[j], ce = fp[j + 1], hi = fp[j + 2];
                double v = 0.0;
                if (f >= lo && f < ce) v = (f - lo) / (ce - lo);
                else if (f >= ce && f <= hi) v = (hi - f) / (hi - ce);
                fh[o_filt + (size_t)j * LID_NBIN + i] = (float)v;
            }
    }
    // ---- the workspace, sized once (no call reads the handle before finalized is set: a rejected finalize can be repeated)
    const size_t rows = (size_t)c->cfg.max_batch * c->Tcap, B = c->cfg.max_batch;
    const size_t per_frame = 2 * LID_NBIN + 2 * nm + 4 * C + 9 * C + A, per_row = 3 * C + 3 * C + C + A + 6 * C + E + 2 * N;
    const size_t total = rows * per_frame + B * per_row + 64 * 32;
    MIS_REQUIRE(total * 4 <= ((size_t)24 << 30), MIS_ERR_INVALID_INPUT, "max_batch x max_samples needs a workspace of %zu MiB (at most 24 GiB)",
                total * 4 >> 20);
    DevBuf<bf16_t> none;
    a.upload(none, c->farena);
    c->work.alloc(total);
    c->pcm.alloc(B * (size_t)c->cfg.max_samples);
    c->nsamp.alloc(LID_MAX_BATCH); c->frames.alloc(LID_MAX_BATCH); c->top_idx.alloc(B * N);
    c->h_nsamp.resize(LID_MAX_BATCH); c->h_frames.resize(LID_MAX_BATCH);
    float* w = c->work.p;
    auto take = [&](size_t n) { float* p = w; w += round_up(n, 64); return p; };
    c->spec = take(rows * 2 * LID_NBIN); c->mel = take(rows * nm); c->feat = take(rows * nm); c->h0 = take(rows * C); c->cat = take(rows * 3 * C);
    c->r = take(rows * C); c->q = take(rows * C); c->u = take(rows * C); c->mf = take(rows * 3 * C); c->att = take(rows * A);
    c->sc = take(rows * 3 * C); c->mean = take(B * 3 * C); c->sd = take(B * 3 * C); c->gate = take(B * C); c->rb = take(B * A);
    c->pooled = take(B * 6 * C); c->emb = take(B * E); c->logp = take(B * N); c->top_prob = take(B * N);
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of a sanitized checkpoint; running statistics away from (0, 1)
extern "C" mis_status mis_ecapa_lid_init_synthetic(mis_ecapa_lid* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    const int64_t C = c->C;
    auto bn = [&](const std::string& p, int64_t n) {
        sw.norm(p, n);
        sw.put(p + ".running_mean", {n}, 0.1, 0.0f);
        sw.put(p + ".running_var", {n}, 0.3, 1.0f);
    };
    for (const LidTdnnSpec& s : lid_tdnn_specs(c)) {
        sw.put(s.name + ".conv.weight", {s.cout, s.k, s.cin}, sqrt(3.0 / ((double)s.k * s.cin)), 0.0f);
        sw.put(s.name + ".conv.bias", {s.cout}, 0.05, 0.0f);
        bn(s.name + ".norm", s.cout);
    }
    for (int i = 1; i <= 3; ++i) {
        const std::string q = "embedding_model.block" + std::to_string(i) + ".se_block.";
        sw.put(q + "conv1.weight", {c->SE, 1, C}, sqrt(3.0 / (double)C), 0.0f); sw.put(q + "conv1.bias", {c->SE}, 0.05, 0.0f);
        sw.put(q + "conv2.weight", {C, 1, c->SE}, sqrt(3.0 / (double)c->SE), 0.0f); sw.put(q + "conv2.bias", {C}, 0.05, 0.0f);
    }
    sw.put("embedding_model.asp.conv.weight", {3 * C, 1, c->A}, sqrt(3.0 / (double)c->A), 0.0f);
    sw.put("embedding_model.asp.conv.bias", {3 * C}, 0.05, 0.0f);
    bn("embedding_model.asp_bn", 6 * C);
    sw.put("embedding_model.fc.weight", {c->E, 1, 6 * C}, sqrt(3.0 / (6.0 * C)), 0.0f); sw.put("embedding_model.fc.bias", {c->E}, 0.05, 0.0f);
    bn("classifier.norm", c->E);
    sw.lin("classifier.DNN.block_0.linear.w", c->Hd, c->E, true, 1.0);
    bn("classifier.DNN.block_0.norm", c->Hd);
    sw.lin("classifier.out.w", c->N, c->Hd, true, 2.0);
    MIS_API_END
}

static int lid_launch_gemm(mis_ecapa_lid* c, LidGemm g, int B, int Ts) {
    g.T = c->frames.p; g.Ts = Ts;
    if (!g.ldw) g.ldw = g.taps * g.Cin;
    hipLaunchKernelGGL(k_lid_gemm, dim3(cdiv(Ts, F32_TILE), cdiv(g.Cout, F32_TILE), B), dim3(256), 0, c->stream, g);
    return 1;
}
static LidGemm lid_tdnn_gemm(const LidTdnn& t, const float* X, int ldx, float* Y, int ldy) {
    LidGemm g{};
    g.X = X; g.ldx = ldx; g.W = t.w; g.bias = t.bias; g.bn_s = t.bn.s; g.bn_b = t.bn.b; g.Y = Y; g.ldy = ldy;
    g.Cin = t.cin; g.Cout = t.cout; g.taps = t.k; g.dil = t.dil; g.epi = LID_EPI_RELU_BN; g.load = LID_LOAD_ACT;
    return g;
}

// the front end: c->pcm, c->nsamp -> c->mel (stage 0).  Returns the launches made.
static int lid_enqueue_front(mis_ecapa_lid* c, int B, int Ts, int64_t pcm_stride) {
    int n = 0;
    LidGemm g{};
    g.pcm = c->pcm.p; g.pcm_stride = pcm_stride; g.nsamp = c->nsamp.p; g.win = c->win; g.W = c->dft; g.Y = c->spec; g.ldy = 2 * LID_NBIN;
    g.Cin = LID_NFFT; g.Cout = 2 * LID_NBIN; g.taps = 1; g.dil = 1; g.epi = LID_EPI_PLAIN; g.load = LID_LOAD_FRAMES;
    n += lid_launch_gemm(c, g, B, Ts);
    LidGemm m{};
    m.X = c->spec; m.ldx = 2 * LID_NBIN; m.W = c->filt; m.Y = c->mel; m.ldy = c->nm;
    m.Cin = LID_NBIN; m.Cout = c->nm; m.taps = 1; m.dil = 1; m.epi = LID_EPI_DB; m.load = LID_LOAD_POWER;
    n += lid_launch_gemm(c, m, B, Ts);
    hipLaunchKernelGGL(k_lid_clamp, dim3(B), dim3(256), 0, c->stream, c->mel, c->frames.p, Ts, c->nm);
    return n + 1;
}

// c->mel (stage 0) -> log-probabilities and the top k.  Returns the launches made.
static int lid_enqueue_model(mis_ecapa_lid* c, int B, int Ts, int k) {
    hipStream_t s = c->stream;
    const int C = c->C, C3 = 3 * C, H = C / c->S, A = c->A;
    const int32_t* T = c->frames.p;
    int n = 0;
    hipLaunchKernelGGL(k_lid_meannorm, dim3(B), dim3(256), (size_t)5 * c->nm * 4, s, c->mel, c->feat, T, Ts, c->nm); ++n;
    n += lid_launch_gemm(c, lid_tdnn_gemm(c->block0, c->feat, c->nm, c->h0, C), B, Ts);
    for (int bi = 0; bi < 3; ++bi) {
        const LidBlock& bl = c->blocks[bi];
        const float* x = bi == 0 ? c->h0 : c->cat + (size_t)(bi - 1) * C;
        const int ldx = bi == 0 ? C : C3;
        float* y = c->cat + (size_t)bi * C;
        LidGemm g1 = lid_tdnn_gemm(bl.tdnn1, x, ldx, c->r, C);
        g1.Y2 = c->q; g1.ldy2 = C; g1.y2_cols = H;                    // Res2Net chunk 0 passes through (:168-169)
        n += lid_launch_gemm(c, g1, B, Ts);
        for (int j = 0; j < c->S - 1; ++j) {                          // chunk j + 1 = TDNN(chunk + previous output), no add for the first
            LidGemm g = lid_tdnn_gemm(bl.res[j], c->r + (size_t)(j + 1) * H, C, c->q + (size_t)(j + 1) * H, C);
            if (j > 0) { g.X2 = c->q + (size_t)j * H; g.ldx2 = C; }
            n += lid_launch_gemm(c, g, B, Ts);
        }
        n += lid_launch_gemm(c, lid_tdnn_gemm(bl.tdnn2, c->q, C, c->u, C), B, Ts);
        hipLaunchKernelGGL(k_lid_time_stats, dim3(cdiv(C, 64), B), dim3(256), 0, s, c->u, C, T, Ts, C, c->mean, (float*)nullptr);
        hipLaunchKernelGGL(k_lid_se_gate, dim3(cdiv(C, 64), B), dim3(256), (size_t)(C + c->SE) * 4, s, c->mean, bl.se_w1, bl.se_b1, bl.se_w2,
                           bl.se_b2, C, c->SE, c->gate);
        const size_t total = (size_t)B * Ts * C;
        hipLaunchKernelGGL(k_lid_se_apply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, c->u, c->gate, x, ldx, y, C3, T, Ts, C, total);
        n += 3;
    }
    n += lid_launch_gemm(c, lid_tdnn_gemm(c->mfa, c->cat, C3, c->mf, C3), B, Ts);
    // attentive statistics pooling with global context
    hipLaunchKernelGGL(k_lid_time_stats, dim3(cdiv(C3, 64), B), dim3(256), 0, s, c->mf, C3, T, Ts, C3, c->mean, c->sd);
    hipLaunchKernelGGL(k_lid_rowbias, dim3(cdiv(A, 4), B), dim3(256), 0, s, c->asp_tdnn.w, C3, A, c->mean, c->sd, c->rb);
    LidGemm ga = lid_tdnn_gemm(c->asp_tdnn, c->mf, C3, c->att, A);
    ga.Cin = C3; ga.ldw = 3 * C3; ga.rowbias = c->rb; ga.epi = LID_EPI_RELU_BN_TANH;
    n += 2 + lid_launch_gemm(c, ga, B, Ts);
    LidGemm gs{};
    gs.X = c->att; gs.ldx = A; gs.W = c->asp_w; gs.bias = c->asp_b; gs.Y = c->sc; gs.ldy = C3; gs.Cin = A; gs.Cout = C3; gs.taps = 1; gs.dil = 1;
    gs.epi = LID_EPI_PLAIN; gs.load = LID_LOAD_ACT;
    n += lid_launch_gemm(c, gs, B, Ts);
    hipLaunchKernelGGL(k_lid_asp_pool, dim3(cdiv(C3, 64), B), dim3(256), 0, s, c->mf, c->sc, T, Ts, C3, c->pooled);
    hipLaunchKernelGGL(k_lid_tail, dim3(cdiv(c->E, 8), B), dim3(256), (size_t)6 * C * 4, s, c->pooled, c->asp_bn.s, c->asp_bn.b, c->fc_w, c->fc_b,
                       6 * C, c->E, c->emb);
    LidHead hp{c->emb, c->n0.s, c->n0.b, c->w1, c->b1, c->n1.s, c->n1.b, c->w2, c->b2, c->E, c->Hd, c->N, k, c->logp, c->top_prob, c->top_idx.p};
    hipLaunchKernelGGL(k_lid_head, dim3(B), dim3(256), (size_t)(c->E + c->Hd + c->N) * 4, s, hp);
    return n + 3;
}

static int lid_clamp_k(const mis_ecapa_lid* c, int top_k) { return top_k < 0 ? 0 : top_k > c->N ? c->N : top_k; }

// results of the chain to the host; the one synchronisation of a call
static void lid_finish(mis_ecapa_lid* c, int B, int Ts, int k, float* log_probs, float* embedding, int32_t* top_idx, float* top_prob) {
    hipStream_t s = c->stream;
    HIP_CHECK(hipGetLastError());
    if (log_probs) HIP_CHECK(hipMemcpyAsync(log_probs, c->logp, (size_t)B * c->N * 4, hipMemcpyDeviceToHost, s));
    if (embedding) HIP_CHECK(hipMemcpyAsync(embedding, c->emb, (size_t)B * c->E * 4, hipMemcpyDeviceToHost, s));
    if (top_idx && k > 0) HIP_CHECK(hipMemcpyAsync(top_idx, c->top_idx.p, (size_t)B * k * 4, hipMemcpyDeviceToHost, s));
    if (top_prob && k > 0) HIP_CHECK(hipMemcpyAsync(top_prob, c->top_prob, (size_t)B * k * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    c->last_batch = B; c->last_Ts = Ts;
}

extern "C" int mis_ecapa_lid_launches(const mis_ecapa_lid* c) { return c ? c->last_launches : 0; }

extern "C" mis_status mis_ecapa_lid_predict(mis_ecapa_lid* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, int top_k,
                                            float* log_probs, float* embedding, int32_t* top_idx, float* top_prob) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "ECAPA LID model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch must be 1..%d (max_batch)", c->cfg.max_batch);
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    int64_t longest = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 1, MIS_ERR_INVALID_INPUT, "row %d is empty (the reference would return NaN)", b);
        MIS_REQUIRE(n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples, the row stride is %lld", b, (long long)n, (long long)stride);
        MIS_REQUIRE(n <= c->cfg.max_samples, MIS_ERR_INVALID_INPUT, "row %d: %lld samples, max_samples is %lld", b, (long long)n,
                    (long long)c->cfg.max_samples);
        c->h_nsamp[b] = n; c->h_frames[b] = (int32_t)(n / LID_HOP + 1);
        longest = std::max(longest, n);
    }
    const int Ts = (int)(longest / LID_HOP + 1), k = lid_clamp_k(c, top_k);
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpy2DAsync(c->pcm.p, (size_t)longest * 4, pcm, (size_t)stride * 4, (size_t)longest * 4, batch, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->nsamp.p, c->h_nsamp.data(), (size_t)batch * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->frames.p, c->h_frames.data(), (size_t)batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(c->ev[0], s));
    int n = lid_enqueue_front(c, batch, Ts, longest);
    HIP_CHECK(hipEventRecord(c->ev[1], s));
    n += lid_enqueue_model(c, batch, Ts, k);
    HIP_CHECK(hipEventRecord(c->ev[2], s));
    lid_finish(c, batch, Ts, k, log_probs, embedding, top_idx, top_prob);
    c->last_launches = n;
    HIP_CHECK(hipEventElapsedTime(&c->ms_front, c->ev[0], c->ev[1]));
    HIP_CHECK(hipEventElapsedTime(&c->ms_model, c->ev[1], c->ev[2]));
    MIS_API_END
}

extern "C" mis_status mis_ecapa_lid_forward_features(mis_ecapa_lid* c, const float* mel, const int32_t* frames, int batch, int T, int top_k,
                                                     float* log_probs, float* embedding, int32_t* top_idx, float* top_prob) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && mel, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "ECAPA LID model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch must be 1..%d (max_batch)", c->cfg.max_batch);
    MIS_REQUIRE(T >= 1 && T <= c->Tcap, MIS_ERR_INVALID_INPUT, "%d frames: 1..%d (max_samples / 160 + 1) are served", T, c->Tcap);
    for (int b = 0; b < batch; ++b) {
        const int t = frames ? frames[b] : T;
        MIS_REQUIRE(t >= 1 && t <= T, MIS_ERR_INVALID_INPUT, "row %d: %d frames (1 .. %d are served)", b, t, T);
        c->h_frames[b] = t;
    }
    const int k = lid_clamp_k(c, top_k);
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpyAsync(c->mel, mel, (size_t)batch * T * c->nm * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->frames.p, c->h_frames.data(), (size_t)batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(c->ev[1], s));
    const int n = lid_enqueue_model(c, batch, T, k);
    HIP_CHECK(hipEventRecord(c->ev[2], s));
    lid_finish(c, batch, T, k, log_probs, embedding, top_idx, top_prob);
    c->last_launches = n;
    c->ms_front = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&c->ms_model, c->ev[1], c->ev[2]));
    MIS_API_END
}

// tensors of the last call, f32, a row's own frames first and zeros behind them.  stage 0 mel dB [B, Ts, n_mels], 1 normalised features,
// 2 block0 [B, Ts, C], 3-5 the SE-Res2Net blocks, 6 mfa [B, Ts, 3 C], 7 pooled [B, 6 C], 8 embedding [B, E], 9 log-probabilities [B, N].
// dims[3]: B, Ts (1 from stage 7 on), width; out may be NULL for the dims alone.
extern "C" mis_status mis_ecapa_lid_tap(mis_ecapa_lid* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && stage >= 0 && stage <= 9, MIS_ERR_INVALID_INPUT, "bad argument");
    MIS_REQUIRE(c->last_batch > 0, MIS_ERR_INVALID_INPUT, "no call to tap");
    HIP_CHECK(hipSetDevice(c->device));
    const size_t B = c->last_batch, Ts = stage >= 7 ? 1 : c->last_Ts, C = c->C;
    const size_t width = stage <= 1 ? c->nm : stage <= 5 ? C : stage == 6 ? 3 * C : stage == 7 ? 6 * C : stage == 8 ? c->E : c->N;
    if (dims) { dims[0] = (int64_t)B; dims[1] = (int64_t)Ts; dims[2] = (int64_t)width; }
    if (!out) return MIS_OK;
    MIS_REQUIRE((int64_t)(B * Ts * width) <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    const float* src = stage == 0 ? c->mel : stage == 1 ? c->feat : stage == 2 ? c->h0 : stage <= 5 ? c->cat + (size_t)(stage - 3) * C :
                       stage == 6 ? c->mf : stage == 7 ? c->pooled : stage == 8 ? c->emb : c->logp;
    const size_t pitch = (stage >= 3 && stage <= 5 ? 3 * C : width) * 4;
    HIP_CHECK(hipMemcpy2D(out, width * 4, src, pitch, width * 4, B * Ts, hipMemcpyDeviceToHost));
    MIS_API_END
}

// measurements: device milliseconds of the last call, ms[2] = front end (0 after forward_features), model
extern "C" mis_status mis_debug_ecapa_lid_timing(const mis_ecapa_lid* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && ms, MIS_ERR_INVALID_INPUT, "null argument");
    ms[0] = c->ms_front; ms[1] = c->ms_model;
    MIS_API_END
}
