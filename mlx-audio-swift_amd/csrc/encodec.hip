// encodec.hip - EnCodec (SEANet) decoder: residual-VQ codes -> waveform, float32.  Both model families: 24 kHz (mono, causal padding,
// plain convs) and 48 kHz (stereo, non-causal padding, GroupNorm(1 group) after every conv - in the transposed-conv layer before the trim).
//
// Reference being replaced: Encodec.decodeFrame / EncodecDecoder (Sources/MLXAudioCodecs/Encodec/Encodec.swift:94-170,295-302),
// EncodecLSTM / EncodecLSTMBlock, EncodecConv1d (causal + reflect padding), EncodecConvTranspose1dLayer, EncodecResnetBlock, ELU
// (EncodecLayers.swift:15-450), EncodecResidualVectorQuantizer.decode (EncodecQuantization.swift:117-133).  The reference runs its
// transposed conv as scalar host loops over asArray copies (EncodecLayers.swift:395-420) and the LSTM as a per-step host loop.
// Here: convs are exact-f32 MFMA contractions (k_conv_taps on a reflect-padded, ELU-activated copy; transposed convs as per-phase
// GEMMs), and the LSTM recurrence is ONE persistent launch: every block keeps its slice of W_h resident in LDS for all T steps,
// the hidden state is exchanged through global memory, one monotonic counter barrier per step (release fence -> atomic arrive;
// agent-scope poll -> acquire fence), bounded spins so a lost block cannot hang the GPU.
//
// Encode side (Encodec.encodeFrame / EncodecEncoder, Encodec.swift:17-89,212-238; EncodecResidualVectorQuantizer.encode,
// EncodecQuantization.swift:22-32,100-114): per-row loudness normalisation (fixed partition, sums in double), the SEANet encoder on the
// decoder's conv / resnet / LSTM pieces plus a strided conv (pad + ELU + phase split, then a two-tap contraction over Cin * r channels),
// and the residual-VQ search of all quantizers in ONE launch (k_encodec_rvq: 32 frames per block, residuals resident in LDS).
#include "common.h"
#include "host_weights.h"
#include "kernels.h"
#include "codec_kernels.h"
#include "f32_tile.h"
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <map>

struct mis_encodec {
    int device = 0;
    mis_encodec_config cfg{};
    hipStream_t stream = nullptr;
    HostWeights raw{"Encodec"};
    bool finalized = false;
    int n_q = 0, dim0 = 0;
    DevBuf<float> arena;
    struct Lin : F32Lin {                                                        // nw / nb: GroupNorm weight / bias (group_norm models)
        size_t nw = 0, nb = 0;
        Lin() {}
        Lin(const F32Lin& l) : F32Lin(l) {}
    };
    size_t tables = 0, zeros = 0;
    Lin conv0, last;
    struct Lstm { Lin xproj; size_t wh = 0; };
    std::vector<Lstm> lstm;
    struct Res { Lin c1, c2, sc; int dil; bool has_sc; };
    struct Up { Lin ct; int s, cin, cout; std::vector<Res> res; };
    std::vector<Up> ups;
    // encoder (optional: a decoder-only checkpoint finalizes without it)
    bool has_encoder = false;
    size_t e2 = 0;                       // |e|^2 of every codebook row [n_q][codebook_size]
    Lin enc_conv0, enc_last;
    std::vector<Lstm> enc_lstm;
    struct Down { Lin cv; int r, cin, cout; std::vector<Res> res; };   // resnets at cin, then ELU + conv (kernel 2r, stride r) cin -> cout
    std::vector<Down> downs;
    DevBuf<float> audio_dev, scale_dev;
    DevBuf<uint8_t> mask_dev;
    DevBuf<double> rms_part;             // loudness partial sums [rows][RMS_BLOCKS]
    DevBuf<float> buf[4], hstate;
    CodecPack pack;                      // split-bf16 weight fragments + activation scratch (codec_bf3.hip)
    DevBuf<int32_t> codes_dev, sync;
    DevBuf<double> gn_part;              // GroupNorm partial sums [batch][GN_BLOCKS][2]
    DevBuf<float> gn_stat;               // [batch][2]: mean, 1 / sqrt(var + eps)
};

// ---------------------------------------------------------------------------- kernels
// y[c][i], i in [0, left + T + right): EncodecConv1d.pad1d (EncodecLayers.swift:130-171) then optional ELU (:340-350).
// reflect: left sample i <- x[min(left - i, T-1)], right sample i <- x[max(T-2-i, 0)]; zero mode: zeros.
// elu 1: expf(v) - 1 (the decode chain, whose bits are pinned); elu 2: expm1f(v) (the encode chain: no cancellation near 0, which a
// one-frame input would otherwise carry through all seven taps of the last conv at once).
__global__ void k_encodec_pad_act(const float* __restrict__ x, float* __restrict__ y, int C, int T, int left, int right, int reflect, int elu) {
    const int Tp = left + T + right;
    int i = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (i >= Tp) return;
    const float* xr = x + ((size_t)b * C + c) * T;
    float v;
    if (i < left) v = reflect ? xr[min(left - i, T - 1)] : 0.0f;
    else if (i < left + T) v = xr[i - left];
    else v = reflect ? xr[max(T - 2 - (i - left - T), 0)] : 0.0f;
    if (elu) v = v > 0.0f ? v : (elu == 2 ? expm1f(v) : expf(v) - 1.0f);
    y[((size_t)b * C + c) * Tp + i] = v;
}

__global__ void k_encodec_scale(float* __restrict__ x, const float* __restrict__ scale, int64_t n_per_row) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int b = blockIdx.y;
    if (i < n_per_row) x[(size_t)b * n_per_row + i] *= scale[b];
}


// ---- GroupNorm(1 group, pytorchCompatible) over the (C, T) block of one sample (EncodecLayers.swift:128-131): two deterministic
// reduction stages (fixed partition, fixed summation order; sums in double), then the affine apply - which also crops a column window
// out of a wider buffer (the transposed-conv layer normalises BEFORE it trims, :244-262) and adds the residual of a resnet block.
#define GN_BLOCKS 64
__global__ void __launch_bounds__(256) k_gn_partial(const float* __restrict__ x, double* __restrict__ part, int64_t n) {
    __shared__ double s1[256], s2[256];
    const int blk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int64_t len = (n + GN_BLOCKS - 1) / GN_BLOCKS, lo = (int64_t)blk * len, hi = lo + len < n ? lo + len : n;
    const float* xb = x + (size_t)b * n;
    double a = 0.0, q = 0.0;
    for (int64_t i = lo + tid; i < hi; i += 256) { const double v = (double)xb[i]; a += v; q += v * v; }
    s1[tid] = a; s2[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { s1[tid] += s1[tid + o]; s2[tid] += s2[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { part[((size_t)b * GN_BLOCKS + blk) * 2] = s1[0]; part[((size_t)b * GN_BLOCKS + blk) * 2 + 1] = s2[0]; }
}
__global__ void k_gn_final(const double* __restrict__ part, float* __restrict__ stat, double n, float eps) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    double a = 0.0, q = 0.0;
    for (int i = 0; i < GN_BLOCKS; ++i) { a += part[((size_t)b * GN_BLOCKS + i) * 2]; q += part[((size_t)b * GN_BLOCKS + i) * 2 + 1]; }
    const double mu = a / n;
    double var = q / n - mu * mu;
    if (var < 0.0) var = 0.0;
    stat[b * 2] = (float)mu;
    stat[b * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
}
// y[b][c][t] = norm(xf[b][c][off + t]) * w[c] + bsh[c] (+ R[b][c][t]); stat null: plain crop.  xf rows are ldf wide, y / R rows T.
__global__ void k_gn_apply(const float* xf, int64_t ldf, int off, float* y, const float* __restrict__ stat, const float* __restrict__ w,
                           const float* __restrict__ bsh, const float* R, int C, int T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    float v = xf[((size_t)b * C + c) * ldf + off + t];
    if (stat) v = (v - stat[b * 2]) * stat[b * 2 + 1] * w[c] + bsh[c];
    const size_t o = ((size_t)b * C + c) * T + t;
    if (R) v += R[o];
    y[o] = v;
}

// LSTM recurrence (EncodecLSTM :33-61), persistent: block blk owns hidden units [blk*U, blk*U + U) = 4U gate rows of W_h
// (rows g*H + j, g = i,f,g,o) held in LDS.  xp [B][4H][T] = x W_x^T + b (computed by a GEMM), out [B][H][T], hbuf [2][B][H].
struct LstmArgs {
    const float* wh;     // [4H][H]
    const float* xp;     // [B][4H][T]
    const float* resid;  // optional [B][H][T] added to the output (EncodecLSTMBlock: h + hiddenStates), null for inner layers
    float* out;          // [B][H][T]
    float* hbuf;         // [2][B][H]
    int* counter;        // monotonic arrivals
    int* error;          // set to 1 on a barrier timeout
    int H, T, B, U, NB;
};
__global__ void __launch_bounds__(256) k_encodec_lstm(LstmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, blk = blockIdx.x;
    const int H = a.H, U = a.U, R = 4 * U;
    float* wsl = lds;                 // [R][H]
    float* hs = lds + (size_t)R * H;  // [H]
    float* dots = hs + H;             // [R]
    float* cst = dots + R;            // [B][U] cell state
    for (int idx = tid; idx < R * H; idx += 256) {
        int r = idx / H, k = idx - r * H;
        int g = r / U, u = r - g * U;
        wsl[idx] = a.wh[((size_t)g * H + blk * U + u) * H + k];
    }
    for (int idx = tid; idx < a.B * U; idx += 256) cst[idx] = 0.0f;
    __syncthreads();
    // thread groups: G threads per gate row
    int G = 256 / R;
    if (G < 1) G = 1;
    if (G > 64) G = 64;
    while (G & (G - 1)) G &= G - 1;   // power of two
    const int rows_per_pass = 256 / G;
    for (int t = 0; t < a.T; ++t) {
        if (t > 0) {                  // wait for every block's step t-1
            if (tid == 0) {
                const int target = a.NB * t;
                int spins = 0;
                while (__hip_atomic_load(a.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                    __builtin_amdgcn_s_sleep(2);
                    if (++spins > (1 << 24)) { *a.error = 1; break; }
                }
            }
            __syncthreads();
            __threadfence();          // acquire: hbuf written by the other blocks is visible below
            if (*a.error) return;
        }
        for (int b = 0; b < a.B; ++b) {
            if (t > 0) {
                const float* hp = a.hbuf + ((size_t)((t - 1) & 1) * a.B + b) * H;
                for (int k = tid; k < H; k += 256) hs[k] = __hip_atomic_load(hp + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __syncthreads();
                for (int r0 = 0; r0 < R; r0 += rows_per_pass) {
                    const int r = r0 + tid / G, gl = tid % G;
                    float acc = 0.0f;
                    if (r < R)
                        for (int k = gl; k < H; k += G) acc += wsl[(size_t)r * H + k] * hs[k];
                    for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
                    if (r < R && gl == 0) dots[r] = acc;
                }
                __syncthreads();
            }
            if (tid < U) {
                const int j = blk * U + tid;
                const float* xb = a.xp + (size_t)b * 4 * H * a.T + t;
                float gi = xb[(size_t)(0 * H + j) * a.T], gf = xb[(size_t)(1 * H + j) * a.T], gg = xb[(size_t)(2 * H + j) * a.T],
                      go = xb[(size_t)(3 * H + j) * a.T];
                if (t > 0) { gi += dots[0 * U + tid]; gf += dots[1 * U + tid]; gg += dots[2 * U + tid]; go += dots[3 * U + tid]; }
                const float i_ = 1.0f / (1.0f + expf(-gi)), f_ = 1.0f / (1.0f + expf(-gf)), g_ = tanhf(gg), o_ = 1.0f / (1.0f + expf(-go));
                const float c = f_ * cst[b * U + tid] + i_ * g_;
                cst[b * U + tid] = c;
                const float h = o_ * tanhf(c);
                __hip_atomic_store(a.hbuf + ((size_t)(t & 1) * a.B + b) * H + j, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const size_t oi = ((size_t)b * H + j) * a.T + t;
                a.out[oi] = a.resid ? h + a.resid[oi] : h;
            }
            __syncthreads();
        }
        __threadfence();              // release this block's hbuf stores
        if (tid == 0) __hip_atomic_fetch_add(a.counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- encode side
// Loudness of one row (Encodec.swift:227-233): scale = sqrt(mean_t(mono^2)) + 1e-8, mono = mean over channels of the masked input.
// The same two deterministic stages as the GroupNorm: a fixed partition of the time axis, a fixed summation order, sums in double -
// a row's scale does not depend on its neighbours.  x [rows][C][L], mask u8 [rows][L] or null.
#define RMS_BLOCKS 64
__global__ void __launch_bounds__(256) k_encodec_rms_partial(const float* __restrict__ x, const uint8_t* __restrict__ mask, double* __restrict__ part,
                                                             int C, int64_t L) {
    __shared__ double s1[256];
    const int blk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int64_t len = (L + RMS_BLOCKS - 1) / RMS_BLOCKS, lo = (int64_t)blk * len, hi = lo + len < L ? lo + len : L;
    const float* xb = x + (size_t)b * C * L;
    double a = 0.0;
    for (int64_t t = lo + tid; t < hi; t += 256) {
        double m = 0.0;
        if (!mask || mask[(size_t)b * L + t])
            for (int c = 0; c < C; ++c) m += (double)xb[(size_t)c * L + t];
        m /= (double)C;
        a += m * m;
    }
    s1[tid] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s1[tid] += s1[tid + o];
        __syncthreads();
    }
    if (tid == 0) part[(size_t)b * RMS_BLOCKS + blk] = s1[0];
}
__global__ void k_encodec_rms_final(const double* __restrict__ part, float* __restrict__ scale, double L) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    double a = 0.0;
    for (int i = 0; i < RMS_BLOCKS; ++i) a += part[(size_t)b * RMS_BLOCKS + i];
    scale[b] = (float)(sqrt(a / L) + 1e-8);
}
// y = (x * mask) / scale[row]: one float32 multiplication and one division per sample, as the reference
__global__ void k_encodec_norm_apply(const float* __restrict__ x, const uint8_t* __restrict__ mask, const float* __restrict__ scale,
                                     float* __restrict__ y, int C, int64_t L) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (t >= L) return;
    const size_t i = ((size_t)b * C + c) * L + t;
    const float m = (!mask || mask[(size_t)b * L + t]) ? 1.0f : 0.0f;
    y[i] = (x[i] * m) / scale[b];
}

// Input side of a strided EncodecConv1d (kernel 2r, stride r; EncodecLayers.swift:135-211): pad (left, right incl. the extra padding
// of getExtraPaddingForConv1d; the reflect rule of k_encodec_pad_act), ELU, and the phase split y[c*r + p][m] = elu(xpad[c][r*m + p]),
// m in [0, M): the conv is then a two-tap stride-1 contraction over C*r channels.  M*r = left + T + right.
__global__ void k_encodec_pad_act_split(const float* __restrict__ x, float* __restrict__ y, int C, int T, int left, int r, int M, int reflect) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    if (i >= M * r) return;
    const float* xr = x + ((size_t)b * C + c) * T;
    float v;
    if (i < left) v = reflect ? xr[min(left - i, T - 1)] : 0.0f;
    else if (i < left + T) v = xr[i - left];
    else v = reflect ? xr[max(T - 2 - (i - left - T), 0)] : 0.0f;
    v = v > 0.0f ? v : expm1f(v);
    const int m = i / r, p = i - m * r;
    y[(((size_t)b * C + c) * r + p) * M + m] = v;
}

// Residual-VQ search of every quantizer in one launch (EncodecResidualVectorQuantizer.encode, EncodecQuantization.swift:22-32,100-114).
// Block (tile, row) owns RVQ_FT = 32 frames of one row; their residuals R [32][ld] stay in LDS for all quantizers.  Per quantizer:
// score(e, f) = 2 r_f . e - |e|^2 (the reference's -(|r|^2 - 2 r.e + |e|^2) without the per-frame constant |r|^2, which cannot move an
// arg-max) on v_mfma_f32_32x32x2_f32 with the codebook on the M side: wave w takes the 32-entry chunks w, w + 4, ...; a lane's 16
// accumulators are 16 entries (ascending) of frame lane & 31, so the arg-max is in-lane, one exchange between the lane halves and one
// pass over the four waves - every comparison prefers the lower index on equal scores (argMax returns the first maximum).  Then
// r -= E_q[code] in float32, one subtraction per element, a barrier, and the next quantizer.
// The K axis is walked 8 at a time: lane half kh supplies k0 + 4 kh + j at MFMA step j (A and B alike - a permutation of the sum).
// Edges: entries >= CB supply zeros and never compete; k >= D supplies zeros on both sides; frames >= F hold zeros and store nothing.
constexpr int RVQ_FT = 32;
struct RvqArgs {
    const float* emb;      // [rows][D][F]
    const float* tables;   // [nq][CB][D]
    const float* e2;       // [nq][CB]
    int32_t* codes;        // [rows][nq][F]
    float* resid;          // optional [nq + 1][rows][D][F]: the residual before every quantizer and after the last
    int D, CB, F, nq, rows;
};
__global__ void __launch_bounds__(256) k_encodec_rvq(RvqArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, kh = lane >> 5;
    const int row = blockIdx.y, f0 = blockIdx.x * RVQ_FT;
    const int D = a.D, CB = a.CB, F = a.F;
    const int Dp = (D + 7) & ~7, ld = Dp + 4;                 // ld = 4 mod 8 words: the 16-byte reads of 8 frames cover all banks
    float* R = lds;                                           // [32][ld]
    float* bs = R + RVQ_FT * ld;                              // [4][32] best score of a wave
    int* bi = (int*)(bs + 4 * RVQ_FT);                        // [4][32] its entry
    int* code = bi + 4 * RVQ_FT;                              // [32]
    const float* eb = a.emb + (size_t)row * D * F;
    for (int idx = tid; idx < RVQ_FT * Dp; idx += 256) {
        const int f = idx & (RVQ_FT - 1), d = idx >> 5;
        R[f * ld + d] = (d < D && f0 + f < F) ? eb[(size_t)d * F + f0 + f] : 0.0f;
    }
    __syncthreads();
    const bool vec = (D & 7) == 0;
    const int nchunk = (CB + 31) / 32;
    for (int q = 0; q < a.nq; ++q) {
        const float* E = a.tables + (size_t)q * CB * D;
        const float* E2 = a.e2 + (size_t)q * CB;
        if (a.resid) {
            float* ro = a.resid + ((size_t)q * a.rows + row) * D * F;
            for (int idx = tid; idx < RVQ_FT * D; idx += 256) {
                const int f = idx & (RVQ_FT - 1), d = idx >> 5;
                if (f0 + f < F) ro[(size_t)d * F + f0 + f] = R[f * ld + d];
            }
        }
        float best = -INFINITY;
        int besti = 0;
        for (int ch = wave; ch < nchunk; ch += 4) {
            const int er = ch * 32 + col;
            const bool ev = er < CB;
            const float* ep = E + (size_t)(ev ? er : 0) * D;
            f32x16_t acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            for (int k0 = 0; k0 < Dp; k0 += 8) {
                const int k = k0 + 4 * kh;
                float av[4];
                if (vec) {
                    const float4 t = *reinterpret_cast<const float4*>(ep + k);
                    av[0] = t.x; av[1] = t.y; av[2] = t.z; av[3] = t.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) av[j] = (k + j < D) ? ep[k + j] : 0.0f;
                }
                const float4 bv = *reinterpret_cast<const float4*>(R + col * ld + k);
                const float b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ev ? av[j] : 0.0f, b4[j], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int idx = ch * 32 + f32_tile_row(r, kh);
                if (idx < CB) {
                    const float sc = 2.0f * acc[r] - E2[idx];
                    if (sc > best) { best = sc; besti = idx; }
                }
            }
        }
        {   // the other half of the lane pair holds the other 16 entries of every chunk for the same frame
            const float os = __shfl_xor(best, 32, 64);
            const int oi = __shfl_xor(besti, 32, 64);
            if (os > best || (os == best && oi < besti)) { best = os; besti = oi; }
        }
        if (kh == 0) { bs[wave * RVQ_FT + col] = best; bi[wave * RVQ_FT + col] = besti; }
        __syncthreads();
        if (tid < RVQ_FT) {
            float b0 = bs[tid];
            int i0 = bi[tid];
            for (int w = 1; w < 4; ++w) {
                const float os = bs[w * RVQ_FT + tid];
                const int oi = bi[w * RVQ_FT + tid];
                if (os > b0 || (os == b0 && oi < i0)) { b0 = os; i0 = oi; }
            }
            code[tid] = i0;
            if (f0 + tid < F) a.codes[((size_t)row * a.nq + q) * F + f0 + tid] = i0;
        }
        __syncthreads();
        for (int idx = tid; idx < RVQ_FT * D; idx += 256) {
            const int f = idx / D, d = idx - f * D;
            R[f * ld + d] -= E[(size_t)code[f] * D + d];
        }
        __syncthreads();
    }
    if (a.resid) {
        float* ro = a.resid + ((size_t)a.nq * a.rows + row) * D * F;
        for (int idx = tid; idx < RVQ_FT * D; idx += 256) {
            const int f = idx & (RVQ_FT - 1), d = idx >> 5;
            if (f0 + f < F) ro[(size_t)d * F + f0 + f] = R[f * ld + d];
        }
    }
}

// ---------------------------------------------------------------------------- host
extern "C" mis_status mis_encodec_create(const mis_encodec_config* cfg, int device, mis_encodec** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(cfg->n_upsampling_ratios >= 1 && cfg->n_upsampling_ratios <= 8 && cfg->num_filters >= 1 && cfg->hidden_size >= 1 &&
                    cfg->codebook_size >= 1 && cfg->n_quantizers >= 1 && (cfg->audio_channels == 1 || cfg->audio_channels == 2) && cfg->compress >= 1,
                MIS_ERR_INVALID_INPUT, "bad Encodec config (one or two audio channels)");
    MIS_REQUIRE(cfg->kernel_size <= 7 && cfg->last_kernel_size <= 7 && cfg->residual_kernel_size <= 7, MIS_ERR_INVALID_INPUT, "kernel sizes above 7 are not built");
    hipStream_t stream = mis_open_stream(device);
    mis_encodec* c = new mis_encodec();
    c->device = device; c->cfg = *cfg; c->n_q = cfg->n_quantizers; c->stream = stream;
    c->dim0 = cfg->num_filters << cfg->n_upsampling_ratios;
    *out = c;
    MIS_API_END
}
extern "C" void mis_encodec_destroy(mis_encodec* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    delete c;
}
extern "C" int mis_encodec_hop_length(const mis_encodec* c) {
    if (!c) return 0;
    int h = 1;
    for (int i = 0; i < c->cfg.n_upsampling_ratios; ++i) h *= c->cfg.upsampling_ratios[i];
    return h;
}

extern "C" mis_status mis_encodec_set_tensor(mis_encodec* c, const char* name_, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && name_ && data && shape && ndim >= 1 && ndim <= 3, MIS_ERR_INVALID_INPUT, "bad argument");
    MIS_REQUIRE(!c->finalized, MIS_ERR_INVALID_INPUT, "set_tensor after finalize");
    c->raw.put_staged(c->device, name_, data, dtype, shape, ndim);
    MIS_API_END
}
extern "C" int mis_encodec_has_encoder(const mis_encodec* c) { return c && c->finalized && c->has_encoder ? 1 : 0; }
// frames of L samples: every strided conv of the encoder gives ceil(T / r) (EncodecLayers.swift:135-141)
extern "C" int64_t mis_encodec_encode_num_frames(const mis_encodec* c, int64_t L) {
    if (!c || L < 1) return 0;
    for (int i = c->cfg.n_upsampling_ratios - 1; i >= 0; --i) L = (L + c->cfg.upsampling_ratios[i] - 1) / c->cfg.upsampling_ratios[i];
    return L;
}

extern "C" mis_status mis_encodec_finalize(mis_encodec* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const mis_encodec_config& cf = c->cfg;
    F32Arena arena;
    // p.conv.{weight, bias} re-laid-out by `at` (+ p.norm.{weight, bias} of the group_norm models) for co output channels
    auto packed = [&](const std::string& p, const std::vector<float>& at, int64_t co, int64_t K) {
        mis_encodec::Lin L = arena.packed(at, co, K, &c->raw.need(p + ".conv.bias", {co}).v);
        if (cf.group_norm) { L.nw = arena.push(c->raw.need(p + ".norm.weight", {co}).v); L.nb = arena.push(c->raw.need(p + ".norm.bias", {co}).v); }
        return L;
    };
    auto conv = [&](const std::string& p, int64_t co, int64_t k, int64_t ci) {
        return packed(p, conv_taps_t(c->raw.need(p + ".conv.weight", {co, k, ci}).v, co, k, ci), co, k * ci);
    };
    // EncodecResnetBlock j of a stage at width d (decoder and encoder alike)
    auto resnet = [&](const std::string& p, int64_t d, int j) {
        mis_encodec::Res R;
        R.dil = 1;
        for (int e = 0; e < j; ++e) R.dil *= cf.dilation_growth_rate;
        const int64_t hid = d / cf.compress;
        R.c1 = conv(p + ".block.1", hid, cf.residual_kernel_size, d);
        R.c2 = conv(p + ".block.3", d, 1, hid);
        R.has_sc = cf.use_conv_shortcut != 0;
        if (R.has_sc) R.sc = conv(p + ".shortcut", d, 1, d);
        return R;
    };
    {
        const int64_t D = cf.codebook_dim;
        std::vector<float> tables((size_t)c->n_q * cf.codebook_size * D);
        for (int q = 0; q < c->n_q; ++q) {
            const auto& e = c->raw.need("quantizer.layers." + std::to_string(q) + ".codebook.embed", {cf.codebook_size, D}).v;
            memcpy(tables.data() + (size_t)q * cf.codebook_size * D, e.data(), e.size() * 4);
        }
        c->tables = arena.push(tables);
    }
    int64_t dim = c->dim0;
    c->zeros = arena.zeros((size_t)dim);
    c->conv0 = conv("decoder.layers.0", dim, cf.kernel_size, cf.hidden_size);
    c->lstm.clear();
    for (int j = 0; j < cf.num_lstm_layers; ++j) {
        const std::string p = "decoder.layers.1.lstm." + std::to_string(j);
        mis_encodec::Lstm L;
        L.xproj = arena.packed(lin_t(c->raw.need(p + ".Wx", {4 * dim, dim}).v, 4 * dim, dim), 4 * dim, dim, &c->raw.need(p + ".bias", {4 * dim}).v);
        L.wh = arena.push(c->raw.need(p + ".Wh", {4 * dim, dim}).v);
        c->lstm.push_back(L);
    }
    c->ups.clear();
    int li = 2;
    for (int bi = 0; bi < cf.n_upsampling_ratios; ++bi) {
        const int64_t s = cf.upsampling_ratios[bi], k = 2 * s, cin = dim, cout = dim / 2;
        mis_encodec::Up U;
        U.s = (int)s; U.cin = (int)cin; U.cout = (int)cout;
        {   // causal transposed conv: out[s*n + ph] = sum_j sum_c W[co][ph + s*j][c] x[c][n - j]  (full conv, right trim k - s)
            const std::string p = "decoder.layers." + std::to_string(li + 1);
            U.ct = packed(p, convt_phases_t(c->raw.need(p + ".conv.weight", {cout, k, cin}).v, cout, k, cin, s, 0, false), cout, 2 * cin);
        }
        li += 2;
        dim = cout;
        for (int j = 0; j < cf.num_residual_layers; ++j) {
            U.res.push_back(resnet("decoder.layers." + std::to_string(li), dim, j));
            ++li;
        }
        c->ups.push_back(U);
    }
    c->last = conv("decoder.layers." + std::to_string(li + 1), cf.audio_channels, cf.last_kernel_size, dim);
    // encoder (EncodecEncoder, Encodec.swift:17-72): conv, per reversed ratio [resnets, ELU, strided conv], LSTM block, ELU, last conv
    c->has_encoder = c->raw.find("encoder.layers.0.conv.weight") != nullptr;
    c->downs.clear(); c->enc_lstm.clear();
    if (c->has_encoder) {
        const int64_t D = cf.codebook_dim;
        std::vector<float> e2((size_t)c->n_q * cf.codebook_size);
        for (size_t r = 0; r < e2.size(); ++r) {                              // |e|^2 in float32, d ascending
            const float* e = arena.host.data() + c->tables + r * D;
            float acc = 0.0f;
            for (int64_t d = 0; d < D; ++d) acc += e[d] * e[d];
            e2[r] = acc;
        }
        c->e2 = arena.push(e2);
        dim = cf.num_filters;
        c->enc_conv0 = conv("encoder.layers.0", dim, cf.kernel_size, cf.audio_channels);
        li = 1;
        for (int bi = cf.n_upsampling_ratios - 1; bi >= 0; --bi) {
            const int64_t r = cf.upsampling_ratios[bi];
            mis_encodec::Down Dn;
            Dn.r = (int)r; Dn.cin = (int)dim; Dn.cout = (int)(2 * dim);
            for (int j = 0; j < cf.num_residual_layers; ++j) {
                Dn.res.push_back(resnet("encoder.layers." + std::to_string(li), dim, j));
                ++li;
            }
            {   // [co][2r][ci] -> two taps over ci * r phase-split channels: w2[co][j][c r + p] = w[co][j r + p][c]
                const std::string p = "encoder.layers." + std::to_string(li + 1);
                const auto& w = c->raw.need(p + ".conv.weight", {2 * dim, 2 * r, dim}).v;
                std::vector<float> w2(w.size());
                for (int64_t o = 0; o < 2 * dim; ++o) for (int64_t j = 0; j < 2; ++j) for (int64_t ph = 0; ph < r; ++ph) for (int64_t ci = 0; ci < dim; ++ci)
                    w2[(o * 2 + j) * dim * r + ci * r + ph] = w[(o * 2 * r + j * r + ph) * dim + ci];
                Dn.cv = packed(p, conv_taps_t(w2, 2 * dim, 2, dim * r), 2 * dim, 2 * dim * r);
            }
            li += 2;
            dim *= 2;
            c->downs.push_back(Dn);
        }
        MIS_REQUIRE(dim == c->dim0, MIS_ERR_INVALID_INPUT, "internal: encoder width");
        for (int j = 0; j < cf.num_lstm_layers; ++j) {
            const std::string p = "encoder.layers." + std::to_string(li) + ".lstm." + std::to_string(j);
            mis_encodec::Lstm L;
            L.xproj = arena.packed(lin_t(c->raw.need(p + ".Wx", {4 * dim, dim}).v, 4 * dim, dim), 4 * dim, dim, &c->raw.need(p + ".bias", {4 * dim}).v);
            L.wh = arena.push(c->raw.need(p + ".Wh", {4 * dim, dim}).v);
            c->enc_lstm.push_back(L);
        }
        c->enc_last = conv("encoder.layers." + std::to_string(li + 2), cf.hidden_size, cf.last_kernel_size, dim);
    }
    arena.upload(c->arena);
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// What one call's chain - decode or encode - launches through: the layer pieces both directions share.  buf[3] (t2) is the scratch of
// the pad / ELU copy and never holds a layer's result across a conv1d.
struct EncodecChain {
    mis_encodec* c;
    hipStream_t s;
    const float* W;
    int batch;
    bool causal, gn;
    int reflect;
    int elu_mode;      // 1 decode, 2 encode (k_encodec_pad_act); the encode chain also sums its convs in two levels (GemmParams.two_level)
    float* t2;

    EncodecChain(mis_encodec* c_, int batch_, size_t need_elems, int elu_mode_) : c(c_), s(c_->stream), W(c_->arena.p), batch(batch_), elu_mode(elu_mode_) {
        const mis_encodec_config& cf = c->cfg;
        causal = cf.use_causal_conv != 0; gn = cf.group_norm != 0; reflect = cf.pad_reflect;
        for (int i = 0; i < 4; ++i) c->buf[i].alloc((size_t)batch * need_elems);
        t2 = c->buf[3].p;
        if (gn) { c->gn_part.alloc((size_t)batch * GN_BLOCKS * 2); c->gn_stat.alloc((size_t)batch * 2); }
    }
    // GroupNorm over the [C][ldf] block of each sample in xf, applied to the column window [off, off + T) -> y [C][T] (+ R)
    void group_norm(const float* xf, int64_t ldf, int off, float* Y, const mis_encodec::Lin& L, const float* R, int Tn) const {
        const int64_t n = (int64_t)L.M * ldf;
        hipLaunchKernelGGL(k_gn_partial, dim3(GN_BLOCKS, batch), dim3(256), 0, s, xf, c->gn_part.p, n);
        hipLaunchKernelGGL(k_gn_final, dim3(batch), dim3(64), 0, s, c->gn_part.p, c->gn_stat.p, (double)n, 1e-5f);
        hipLaunchKernelGGL(k_gn_apply, dim3(cdiv(Tn, 256), L.M, batch), dim3(256), 0, s, xf, ldf, off, Y, c->gn_stat.p, W + L.nw, W + L.nb, R, L.M, Tn);
    }
    // EncodecConv1d (:84-214), stride 1: pad (left = k - 1 causal / split otherwise; dilation not included: as the reference), conv
    int conv1d(const mis_encodec::Lin& L, int Cin, int k, int dil, const float* X, float* Y, int Tin, int elu, const float* R) const {
        const int keff = (k - 1) * dil + 1, ptotal = k - 1;
        int left = ptotal, right = 0;
        if (!causal) { right = ptotal / 2; left = ptotal - right; }
        const int Tp = left + Tin + right, Tout = Tp - keff + 1;
        MIS_REQUIRE(Tout >= 1, MIS_ERR_INVALID_INPUT, "input too short for the dilated conv");
        const float* src = X;
        if (left + right > 0 || elu) {
            hipLaunchKernelGGL(k_encodec_pad_act, dim3(cdiv(Tp, 256), Cin, batch), dim3(256), 0, s, X, t2, Cin, Tin, left, right, reflect, elu ? elu_mode : 0);
            src = t2;
        }
        GemmParams g{};
        g.AT = W + L.w; g.bias = W + L.b; g.X = src; g.Y = Y; g.R = gn ? nullptr : R; g.M = L.M; g.K = L.K; g.N = Tout; g.Tin = Tp; g.Tout = Tout;
        g.Cin = Cin; g.taps = k; g.dil = dil; g.pad = 0; g.two_level = elu_mode == 2;
        launch_gemm(GEMM_TAPS, false, g, batch, s);
        if (gn) group_norm(Y, Tout, 0, Y, L, R, Tout);          // norm(conv(x)) (+ the residual, which the plain path adds in the GEMM epilogue)
        return Tout;
    }
    // ELU -> strided EncodecConv1d (kernel 2r, stride r; :135-211): ceil(Tin / r) frames.  padding_total = r: all of it on the left when
    // causal, r - r / 2 otherwise; the right side takes the rest of the split plus the extra padding up to a whole number of strides
    int conv_down(const mis_encodec::Down& Dn, const float* X, float* Y, int Tin) const {
        const int r = Dn.r, F = cdiv(Tin, r), M = F + 1, left = causal ? r : r - r / 2;
        hipLaunchKernelGGL(k_encodec_pad_act_split, dim3(cdiv((int64_t)M * r, 256), Dn.cin, batch), dim3(256), 0, s, X, t2, Dn.cin, Tin, left, r, M, reflect);
        GemmParams g{};
        g.AT = W + Dn.cv.w; g.bias = W + Dn.cv.b; g.X = t2; g.Y = Y; g.M = Dn.cv.M; g.K = Dn.cv.K; g.N = F; g.Tin = M; g.Tout = F;
        g.Cin = Dn.cin * r; g.taps = 2; g.dil = 1; g.pad = 0; g.two_level = 1;
        launch_gemm(GEMM_TAPS, false, g, batch, s);
        if (gn) group_norm(Y, F, 0, Y, Dn.cv, nullptr, F);
        return F;
    }
    // EncodecResnetBlock (:266-325): shortcut(x) + conv1(ELU(conv_k(ELU(x)))); the result is left in x (x, y, t1 change roles)
    void resnet(const mis_encodec::Res& R, int dim, float*& x, float*& y, float*& t1, int Tc) const {
        const int hid = R.c1.M;
        int T1 = conv1d(R.c1, dim, c->cfg.residual_kernel_size, R.dil, x, t1, Tc, 1, nullptr);
        MIS_REQUIRE(T1 == Tc, MIS_ERR_INVALID_INPUT, "residual conv changes the length (dilation > 1 is not built)");
        const float* res = x;
        if (R.has_sc) { conv1d(R.sc, dim, 1, 1, x, y, Tc, 0, nullptr); res = y; }
        // second conv (k = 1) on ELU(t1) with the residual epilogue; the ELU copy lands in t2 inside conv1d
        float* outb = (res == y) ? t1 : y;              // t1 is consumed through t2 before outb is written
        conv1d(R.c2, hid, 1, 1, t1, outb, Tc, 1, res);
        if (outb == t1) { std::swap(x, t1); } else { std::swap(x, y); }
    }
    // EncodecLSTMBlock (:66-80): h = lstm_n(...lstm_1(x)) + x, in place in x; reads the time-out flag back (one stream synchronisation)
    void lstm_block(const std::vector<mis_encodec::Lstm>& layers, float* x, float* y, float* t1, int Tc) const {
        if (layers.empty()) return;
        const int H = c->dim0;
        int U = H, NB = 1;
        while ((size_t)4 * U * H * 4 > 48 * 1024 && U > 1) { U = (U + 1) / 2; }
        while (H % U) --U;
        NB = H / U;
        const size_t smem = ((size_t)4 * U * H + H + 4 * U + (size_t)batch * U) * sizeof(float);
        MIS_REQUIRE(smem <= 64 * 1024 && NB <= 256, MIS_ERR_INVALID_INPUT, "LSTM width %d does not fit the persistent kernel", H);
        c->hstate.alloc((size_t)2 * batch * H);
        c->sync.alloc(2);
        const float* in = x;
        float* cur = y;
        for (size_t j = 0; j < layers.size(); ++j) {
            GemmParams g{};
            g.AT = W + layers[j].xproj.w; g.bias = W + layers[j].xproj.b; g.X = in; g.Y = t1; g.M = 4 * H; g.K = H; g.N = Tc; g.Tin = Tc; g.Tout = Tc;
            launch_gemm(GEMM_PLAIN, false, g, batch, s);
            HIP_CHECK(hipMemsetAsync(c->sync.p, 0, 8, s));
            LstmArgs la{};
            la.wh = W + layers[j].wh; la.xp = t1; la.resid = (j + 1 == layers.size()) ? x : nullptr; la.out = cur; la.hbuf = c->hstate.p;
            la.counter = c->sync.p; la.error = c->sync.p + 1; la.H = H; la.T = Tc; la.B = batch; la.U = U; la.NB = NB;
            hipLaunchKernelGGL(k_encodec_lstm, dim3(NB), dim3(256), smem, s, la);
            in = cur;
            cur = (cur == y) ? t2 : y;
        }
        int32_t flags[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(flags, c->sync.p, 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        MIS_REQUIRE(flags[1] == 0, MIS_ERR_AUDIO_DECODE, "LSTM step barrier timed out");
        if (in != x) { HIP_CHECK(hipMemcpyAsync(x, in, (size_t)batch * H * Tc * 4, hipMemcpyDeviceToDevice, s)); }
    }
};

// stage: 0 waveform; 1 conv0; 2 lstm block; 3 + i upsampling block i
static const float* encodec_run(mis_encodec* c, const int32_t* codes_dev, int nq, int batch, int T, float* wav_dev, int stage, int* outC, int64_t* outT) {
    CodecPackScope pack_scope(&c->pack);
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "Encodec model not finalized");
    const mis_encodec_config& cf = c->cfg;
    const int hop = mis_encodec_hop_length(c), H = c->dim0;
    size_t need_elems = (size_t)std::max(4 * H, cf.hidden_size) * (T + 16);
    {
        int64_t Tc = T;
        for (auto& U : c->ups) { Tc *= U.s; need_elems = std::max(need_elems, (size_t)(2 * U.cin) * (Tc + 16)); }
    }
    const EncodecChain ch(c, batch, need_elems, 1);
    hipStream_t s = ch.s;
    const float* W = ch.W;
    const bool causal = ch.causal, gn = ch.gn;
    float *x = c->buf[0].p, *y = c->buf[1].p, *t1 = c->buf[2].p;
    launch_codec_embed(codes_dev, (int64_t)nq * T, T, 1, W + c->tables, x, nq, cf.codebook_size, cf.codebook_dim, T, T, batch, s);
    int Tc = ch.conv1d(c->conv0, cf.hidden_size, cf.kernel_size, 1, x, y, T, 0, nullptr);
    std::swap(x, y);
    if (stage == 1) { *outC = H; *outT = Tc; return x; }
    ch.lstm_block(c->lstm, x, y, t1, Tc);
    if (stage == 2) { *outC = H; *outT = Tc; return x; }
    int bi = 0;
    for (auto& U : c->ups) {
        // ELU -> transposed conv (EncodecConvTranspose1dLayer :218-262), kernel 2s: the full output has s * T + s samples, of which
        // padding_total = s are trimmed - all on the right when causal (trim_right_ratio 1), s / 2 on the right otherwise
        hipLaunchKernelGGL(k_encodec_pad_act, dim3(cdiv(Tc, 256), U.cin, batch), dim3(256), 0, s, x, t1, U.cin, Tc, 0, 0, 0, 1);
        GemmParams g{};
        g.AT = W + U.ct.w; g.bias = W + U.ct.b; g.X = t1; g.Y = y; g.alpha = W + c->zeros; g.ralpha = W + c->zeros;
        g.M = U.cout; g.K = 2 * U.cin; g.N = Tc; g.Tin = Tc; g.Tout = Tc * U.s; g.s = U.s; g.pad = 0; g.Cin = U.cin;
        if (causal && cf.trim_right_ratio == 1.0f && !gn) {
            launch_gemm(GEMM_CONVT, true, g, batch, s);            // the trimmed range is exactly the first s * T samples
            Tc *= U.s;
            std::swap(x, y);
        } else {
            MIS_REQUIRE(!causal || cf.trim_right_ratio == 1.0f, MIS_ERR_INVALID_INPUT, "causal transposed convs need trim_right_ratio 1");
            const int right = causal ? U.s : U.s / 2, left = U.s - right;
            const int Tfull = Tc * U.s + U.s;
            g.N = Tc + 1; g.Tout = Tfull;                          // frame n = T holds the tail of the last input column
            launch_gemm(GEMM_CONVT, true, g, batch, s);
            Tc *= U.s;
            // GroupNorm over the UNTRIMMED output (:244-262), then the trim; without a norm the same kernel only crops
            if (gn) ch.group_norm(y, Tfull, left, t1, U.ct, nullptr, Tc);
            else hipLaunchKernelGGL(k_gn_apply, dim3(cdiv(Tc, 256), U.cout, batch), dim3(256), 0, s, y, (int64_t)Tfull, left, t1, nullptr, nullptr, nullptr, nullptr, U.cout, Tc);
            std::swap(x, t1);
        }
        for (auto& R : U.res) ch.resnet(R, U.cout, x, y, t1, Tc);
        if (stage == 3 + bi) { *outC = U.cout; *outT = Tc; return x; }
        ++bi;
    }
    MIS_REQUIRE(Tc == T * hop, MIS_ERR_AUDIO_DECODE, "internal length mismatch");
    ch.conv1d(c->last, c->ups.back().cout, cf.last_kernel_size, 1, x, wav_dev, Tc, 1, nullptr);
    HIP_CHECK(hipGetLastError());
    *outC = cf.audio_channels; *outT = Tc;
    return wav_dev;
}

// Encode chain: audio_dev [rows][channels][L] (+ mask_dev [rows][L] or null) -> embeddings [rows][hidden][F]; with normalize, scales_dev
// [rows] is filled.  stage: -1 embeddings; 0 normalised input; 1 conv0; 2 + i down block i; 2 + n LSTM block; 3 + n embeddings
static const float* encodec_encode_run(mis_encodec* c, const float* audio_dev, const uint8_t* mask_dev, int rows, int L, float* scales_dev, int stage,
                                       int* outC, int64_t* outT) {
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "Encodec model not finalized");
    MIS_REQUIRE(c->has_encoder, MIS_ERR_AUDIO_ENCODE, "this Encodec handle was loaded without encoder weights");
    const mis_encodec_config& cf = c->cfg;
    MIS_REQUIRE(cf.hidden_size == cf.codebook_dim, MIS_ERR_INVALID_INPUT, "the quantizer needs hidden_size == codebook_dim");
    const int H = c->dim0, ch_in = cf.audio_channels, n_down = (int)c->downs.size();
    size_t need_elems = (size_t)ch_in * (L + 16);
    {
        int64_t Tc = L;
        for (auto& Dn : c->downs) {
            const int64_t F = (Tc + Dn.r - 1) / Dn.r;
            need_elems = std::max(need_elems, std::max((size_t)Dn.cin * (Tc + 16), (size_t)Dn.cin * Dn.r * (F + 1)));
            Tc = F;
        }
        need_elems = std::max(need_elems, (size_t)std::max(4 * H, cf.hidden_size) * (Tc + 16));
    }
    const EncodecChain ch(c, rows, need_elems, 2);
    hipStream_t s = ch.s;
    float *x = c->buf[0].p, *y = c->buf[1].p, *t1 = c->buf[2].p;
    const float* in = audio_dev;
    if (cf.normalize) {
        c->rms_part.alloc((size_t)rows * RMS_BLOCKS);
        hipLaunchKernelGGL(k_encodec_rms_partial, dim3(RMS_BLOCKS, rows), dim3(256), 0, s, audio_dev, mask_dev, c->rms_part.p, ch_in, (int64_t)L);
        hipLaunchKernelGGL(k_encodec_rms_final, dim3(rows), dim3(64), 0, s, c->rms_part.p, scales_dev, (double)L);
        hipLaunchKernelGGL(k_encodec_norm_apply, dim3(cdiv(L, 256), ch_in, rows), dim3(256), 0, s, audio_dev, mask_dev, scales_dev, x, ch_in, (int64_t)L);
        in = x;
    }
    if (stage == 0) { *outC = ch_in; *outT = L; return in; }
    int Tc = ch.conv1d(c->enc_conv0, ch_in, cf.kernel_size, 1, in, y, L, 0, nullptr);
    std::swap(x, y);
    if (stage == 1) { *outC = cf.num_filters; *outT = Tc; return x; }
    int bi = 0;
    for (auto& Dn : c->downs) {
        for (auto& R : Dn.res) ch.resnet(R, Dn.cin, x, y, t1, Tc);
        Tc = ch.conv_down(Dn, x, y, Tc);
        std::swap(x, y);
        if (stage == 2 + bi) { *outC = Dn.cout; *outT = Tc; return x; }
        ++bi;
    }
    ch.lstm_block(c->enc_lstm, x, y, t1, Tc);
    if (stage == 2 + n_down) { *outC = H; *outT = Tc; return x; }
    ch.conv1d(c->enc_last, H, cf.last_kernel_size, 1, x, y, Tc, 1, nullptr);
    HIP_CHECK(hipGetLastError());
    *outC = cf.hidden_size; *outT = Tc;
    return y;
}

static void encodec_rvq(mis_encodec* c, const float* emb_dev, int rows, int F, int nq, int32_t* codes_dev, float* resid_dev) {
    const mis_encodec_config& cf = c->cfg;
    MIS_REQUIRE(cf.codebook_dim <= 256, MIS_ERR_INVALID_INPUT, "codebook_dim above 256 is not built");
    RvqArgs a{};
    a.emb = emb_dev; a.tables = c->arena.p + c->tables; a.e2 = c->arena.p + c->e2; a.codes = codes_dev; a.resid = resid_dev;
    a.D = cf.codebook_dim; a.CB = cf.codebook_size; a.F = F; a.nq = nq; a.rows = rows;
    const int ld = ((cf.codebook_dim + 7) & ~7) + 4;
    const size_t smem = ((size_t)RVQ_FT * ld + 9 * RVQ_FT) * sizeof(float);
    hipLaunchKernelGGL(k_encodec_rvq, dim3(cdiv(F, RVQ_FT), rows), dim3(256), smem, c->stream, a);
    HIP_CHECK(hipGetLastError());
}

// encodeFrame (Encodec.swift:212-238) of rows = chunks x batch independent rows in one pass: audio f32 [rows][channels][L], mask u8
// [rows][L] or NULL (all ones) -> codes i32 [rows][n_q][F], scales f32 [rows] (normalize models; otherwise left untouched)
extern "C" mis_status mis_encodec_encode_frame(mis_encodec* c, const float* audio, const uint8_t* mask, int rows, int64_t L, int n_q, int32_t* codes_out,
                                               float* scales_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && audio && codes_out && rows >= 1 && rows <= 65535 && L >= 1 && L < (1 << 30) && n_q >= 1 && n_q <= c->n_q, MIS_ERR_INVALID_INPUT,
                "bad argument");
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n = (size_t)rows * c->cfg.audio_channels * L;
    c->audio_dev.alloc(n);
    HIP_CHECK(hipMemcpyAsync(c->audio_dev.p, audio, n * 4, hipMemcpyDefault, s));
    if (mask) {
        c->mask_dev.alloc((size_t)rows * L);
        HIP_CHECK(hipMemcpyAsync(c->mask_dev.p, mask, (size_t)rows * L, hipMemcpyDefault, s));
    }
    c->scale_dev.alloc(rows);
    int C; int64_t F;
    const float* emb = encodec_encode_run(c, c->audio_dev.p, mask ? c->mask_dev.p : nullptr, rows, (int)L, c->scale_dev.p, -1, &C, &F);
    c->codes_dev.alloc((size_t)rows * n_q * F);
    encodec_rvq(c, emb, rows, (int)F, n_q, c->codes_dev.p, nullptr);
    HIP_CHECK(hipMemcpyAsync(codes_out, c->codes_dev.p, (size_t)rows * n_q * F * 4, hipMemcpyDefault, s));
    if (scales_out && c->cfg.normalize) HIP_CHECK(hipMemcpyAsync(scales_out, c->scale_dev.p, (size_t)rows * 4, hipMemcpyDefault, s));
    HIP_CHECK(hipStreamSynchronize(s));
    MIS_API_END
}

// Encode-side debug entry.  stage >= 0: `in` is audio [rows][channels][L] (+ mask), out receives that stage's output [rows][C][T']
// (0 normalised input, 1 conv0, 2 + i down block i, 2 + n LSTM block, 3 + n embeddings).  stage == -1: `in` is embeddings [rows][D][L]
// (L frames) for the RVQ launch alone: codes_out i32 [rows][n_q][L], out f32 [n_q + 1][rows][D][L] = the residual before every quantizer
// and after the last.  The input carries a NaN guard behind it, the RVQ outputs sit between 0xFF guards that are checked.
extern "C" mis_status mis_debug_encodec_encode_tap(mis_encodec* c, const float* in, const uint8_t* mask, int rows, int64_t L, int n_q, int stage,
                                                   float* out, int64_t capacity, int32_t* codes_out, int32_t* channels, int64_t* length) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && in && out && channels && length && rows >= 1 && rows <= 65535 && L >= 1 && L < (1 << 30) && stage >= -1, MIS_ERR_INVALID_INPUT,
                "bad argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "Encodec model not finalized");
    MIS_REQUIRE(c->has_encoder, MIS_ERR_AUDIO_ENCODE, "this Encodec handle was loaded without encoder weights");
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevBuf<uint32_t> xin;
    if (stage == -1) {
        const int D = c->cfg.codebook_dim;
        MIS_REQUIRE(codes_out && n_q >= 1 && n_q <= c->n_q, MIS_ERR_INVALID_INPUT, "bad argument");
        const size_t ne = (size_t)rows * D * L, nr = (size_t)(n_q + 1) * ne, nc = (size_t)rows * n_q * L;
        MIS_REQUIRE((int64_t)nr <= capacity, MIS_ERR_INVALID_INPUT, "tap buffer too small");
        alloc32(xin, in, ne, F32_NAN);
        GuardedOut oc, orr;
        oc.alloc(nc * 4, 4096); orr.alloc(nr * 4, 4096);
        HIP_CHECK(hipDeviceSynchronize());                       // the poison fills run on the null stream, the engine's stream does not wait for it
        encodec_rvq(c, reinterpret_cast<const float*>(xin.p), rows, (int)L, n_q, reinterpret_cast<int32_t*>(oc.p()), reinterpret_cast<float*>(orr.p()));
        HIP_CHECK(hipStreamSynchronize(s));
        oc.check_guards(); orr.check_guards();
        HIP_CHECK(hipMemcpy(codes_out, oc.p(), nc * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(out, orr.p(), nr * 4, hipMemcpyDeviceToHost));
        *channels = D; *length = L;
        return MIS_OK;
    }
    alloc32(xin, in, (size_t)rows * c->cfg.audio_channels * L, F32_NAN);
    DevBuf<uint8_t> m;
    if (mask) alloc_bytes(m, mask, (size_t)rows * L);
    c->scale_dev.alloc(rows);
    HIP_CHECK(hipDeviceSynchronize());
    int C = 0; int64_t Tt = 0;
    const float* res = encodec_encode_run(c, reinterpret_cast<const float*>(xin.p), mask ? m.p : nullptr, rows, (int)L, c->scale_dev.p, stage, &C, &Tt);
    MIS_REQUIRE((int64_t)rows * C * Tt <= capacity, MIS_ERR_INVALID_INPUT, "tap buffer too small");
    HIP_CHECK(hipMemcpyAsync(out, res, (size_t)rows * C * Tt * 4, hipMemcpyDefault, s));
    HIP_CHECK(hipStreamSynchronize(s));
    *channels = C; *length = Tt;
    MIS_API_END
}

// decodeFrame (Encodec.swift:295-302): codes int32 [batch, n_q, T] (host or device), scales f32 [batch] or NULL -> wav [batch, channels, T*hop]
extern "C" mis_status mis_encodec_decode_frame(mis_encodec* c, const int32_t* codes, int batch, int n_q, int T, const float* scales, float* wav_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && codes && wav_out && batch >= 1 && T >= 1 && n_q >= 1 && n_q <= c->n_q, MIS_ERR_INVALID_INPUT, "bad argument");
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = (int64_t)T * mis_encodec_hop_length(c) * c->cfg.audio_channels;
    c->codes_dev.alloc((size_t)batch * n_q * T);
    HIP_CHECK(hipMemcpyAsync(c->codes_dev.p, codes, (size_t)batch * n_q * T * 4, hipMemcpyDefault, s));
    DevBuf<float> wav, sc;
    wav.alloc((size_t)batch * n);
    int C; int64_t Tt;
    encodec_run(c, c->codes_dev.p, n_q, batch, T, wav.p, 0, &C, &Tt);
    if (scales) {
        sc.alloc(batch);
        HIP_CHECK(hipMemcpyAsync(sc.p, scales, batch * 4, hipMemcpyDefault, s));
        hipLaunchKernelGGL(k_encodec_scale, dim3(cdiv(n, 256), batch), dim3(256), 0, s, wav.p, sc.p, n);
    }
    HIP_CHECK(hipMemcpyAsync(wav_out, wav.p, (size_t)batch * n * 4, hipMemcpyDefault, s));
    HIP_CHECK(hipStreamSynchronize(s));
    MIS_API_END
}
extern "C" mis_status mis_encodec_debug_tap(mis_encodec* c, const int32_t* codes, int batch, int n_q, int T, int stage, float* out, int64_t capacity,
                                            int32_t* channels, int64_t* length) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && codes && out && channels && length && stage >= 1, MIS_ERR_INVALID_INPUT, "bad argument");
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->codes_dev.alloc((size_t)batch * n_q * T);
    HIP_CHECK(hipMemcpyAsync(c->codes_dev.p, codes, (size_t)batch * n_q * T * 4, hipMemcpyDefault, s));
    DevBuf<float> wav;
    wav.alloc((size_t)batch * T * mis_encodec_hop_length(c) * c->cfg.audio_channels);
    int C = 0; int64_t Tt = 0;
    const float* res = encodec_run(c, c->codes_dev.p, n_q, batch, T, wav.p, stage, &C, &Tt);
    MIS_REQUIRE((int64_t)batch * C * Tt <= capacity, MIS_ERR_INVALID_INPUT, "tap buffer too small");
    HIP_CHECK(hipMemcpyAsync(out, res, (size_t)batch * C * Tt * 4, hipMemcpyDefault, s));
    HIP_CHECK(hipStreamSynchronize(s));
    *channels = C; *length = Tt;
    MIS_API_END
}
