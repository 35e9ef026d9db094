// nemotron_stream.hip - the cache-aware stream session of Nemotron ASR (NemotronASRStreaming.swift streamEncodeChunks / nemoStreamBlock,
// NemotronASRStreamSession.swift step / finish / frozenMelFrames / streamRNNTDecode): 1..64 streams on one finalized mis_nemotron, every
// stream's state on the device, exact f32 from the stem to the tokens.
//
// The yardstick is the offline engine: a stream's encoder frames, prompt output, joint.enc rows, tokens and absolute frame indices are
// those of mis_nemotron_encode / _generate on the whole audio at the same (left, right), bit for bit, for any split into feeds.  With
// C = right + 1 and left % C == 0 offline query q sees the keys [(q / C - L) C, (q / C + 1) C): at most `left` cached frames and the
// query's own chunk, the reference's stream rule.  What makes the bits equal:
//   attention   a (query, key) score is two fixed-order MFMA dot products over the head dimension; a query's online softmax depends only
//               on the partition of its visible keys into ABSOLUTE 32-aligned key tiles walked upwards; a tile or key the rule hides adds
//               exactly nothing (m stays -inf, alpha = 1 or 0, weight 0).  k_nm_attn_stream keeps K and V in a ring addressed by absolute
//               frame index modulo R and walks the same absolute tiles.
//   K, V        projected once (the contraction's order per element does not depend on the rows around it) and put into the ring.
//   conv        the k - 1 frames in front of a pass are the stream's carried GATED frames (zeros at frame 0 = offline's causal pad).
//   stem        the offline kernels on the window [<= 16 cached mel frames ++ new mel frames]; only sub-sampled frames lo .. hi enter the
//               blocks (streamEncodeChunks' base / lo / hi / consumed / emitted); the window's last frame waits for finish.
//   mel         only frozen frames (m hop + n_fft / 2 <= samples seen), each computed ONCE, when its chunk is whole, from the sample tail
//               the host carries (at most n_fft + one chunk + one feed samples a stream).
//   decode      k_nm_rnnt_stream resumes from the carried proposal (h', c' of every LSTM layer and joint.pred of it) and stores it back;
//               newSymbols is 0 at every pass boundary (a pass ends on an advance), so a split never changes a decision.
//
// New kernels (resources off -Rpass-analysis=kernel-resource-usage, gfx950):
//   k_nm_attn_stream   32 queries x head x stream per block, TWO waves: wave dh owns the head dimensions 64 dh .. 64 dh + 63 of all 32
//               queries (k_nm_attn's per-wave code at qh = 0); the two partial scores and band products meet through LDS and are added
//               as (Sx0 + Sx1) + (Bd0 + Bd1), then / sdk; V is the MFMA operand in key order.  A pass has 1..3 C queries, so a block of
//               64 queries and four waves would idle half of itself.  LDS 50560 bytes, 186 VGPRs, 48 AGPRs, scratch 0, 2 waves a SIMD.
//   k_nm_glu_dwconv_ln_stream   k_nm_glu_dwconv_ln with the carried history as the frames in front; block 0 of a stream writes the next
//               history (double-buffered: a stream without frames copies its history through).  LDS 11776 bytes, 48 VGPRs, scratch 0.
//   k_nm_rnnt_stream   k_nm_rnnt's block (a thread owns a unit's four gates, one logit a thread, ties to the lower index), resumed.
//               LDS 45188 bytes, 69 VGPRs, scratch 0.
//   k_nm_mel_stream / k_nm_mel_roll / k_nm_intake_stream / k_nm_ring_put / k_nm_state_reset   the window's mel frames at absolute frame
//               indices, the 16-frame mel cache, frames lo .. hi of the window, K and V rows into the ring, a stream's state to zeros.
//
// Launches of a pass: 9 + 16 L + 2 p = 1 (mel) + 4 (stem) + 1 (intake) + 16 L (the offline block + the ring put) + 2 p (prompt kernel) +
// 1 (joint.enc) + 1 (decode) + 1 (mel cache).  A feed is walked in passes of at most max_pass_frames / C chunks a stream.
//
// bf16 sessions (mis_nemotron_stream_create_dtype with MIS_BF16 on a model finalized in bf16 mode): the 16 L block launches of a pass are
// nemotron_stream_bf16.h's, launch for launch, and the yardstick is the offline bf16 engine; everything around the blocks is the code here.
#include "nemotron_kernels.h"
#include "nemotron_stream_bf16.h"

#include <algorithm>
#include <vector>

#define NMS_MEL_CACHE 16             // nemoPreEncodeMelCache: >= the causal receptive field of the 8 x stem (15 mel frames)
#define NMS_SLOTS 8                  // passes a feed may enqueue before it waits for the device (pinned staging slots)
enum { NMS_WIN = 0, NMS_T1, NMS_T2, NMS_T3, NMS_N, NMS_LO, NMS_POS, NMS_CACHE, NMS_FRAME0, NMS_ORIGIN, NMS_SEEN, NMS_LANG, NMS_TOK0, NMS_SOFF, NMS_FIELDS };

namespace {
// ============================================================================ kernel A: mel frames of the window
// window row i of stream b: i < cache[b]: the carried mel frame i; else the log-mel frame frame0[b] + i - cache[b] of the stream, from
// stage + soff[b] (the pass's samples, packed: streams without work bring none) whose sample 0 is the stream's sample origin[b]
// (k_nemo_log_mel's expressions; samples behind seen[b] do not exist yet).
__global__ void __launch_bounds__(256) k_nm_mel_stream(const float* __restrict__ stage, const int* __restrict__ par, int S,
                                                       const float* __restrict__ cache, size_t sstride, float preemph,
                                                       const float* __restrict__ window, const float* __restrict__ twc, const float* __restrict__ tws,
                                                       const float* __restrict__ fb, const int* __restrict__ fbr, float* __restrict__ out, int Wp, int mels) {
    __shared__ float re[NEMO_NFFT], im[NEMO_NFFT];
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int cl = par[NMS_CACHE * S + b];
    if (i >= par[NMS_WIN * S + b]) return;
    float* o = out + ((size_t)b * Wp + i) * mels;
    if (i < cl) { if (tid < mels) o[tid] = cache[b * sstride + (size_t)i * mels + tid]; return; }
    const int64_t t = (int64_t)par[NMS_FRAME0 * S + b] + (i - cl), n = par[NMS_SEEN * S + b], org = par[NMS_ORIGIN * S + b];
    const float* x = stage + par[NMS_SOFF * S + b];
    for (int j = tid; j < NEMO_NFFT; j += 256) {
        const float w = window[j];
        const int64_t s = t * NEMO_HOP - NEMO_NFFT / 2 + j;
        float v = 0.0f;
        if (w != 0.0f && s >= 0 && s < n) {
            const float cur = x[s - org];
            v = s == 0 ? cur : __fsub_rn(cur, __fmul_rn(preemph, x[s - 1 - org]));
        }
        const int r = (int)(__brev((unsigned)j) >> 23);
        re[r] = __fmul_rn(v, w); im[r] = 0.0f;
    }
    __syncthreads();
    for (int half = 1; half < NEMO_NFFT; half <<= 1) {
        const int k = tid & (half - 1), i0 = ((tid - k) << 1) + k, i1 = i0 + half, ti = k * (NEMO_NFFT / 2 / half);
        const float c = twc[ti], s = tws[ti];
        const float xr = re[i1], xi = im[i1];
        const float pr = xr * c - xi * s, pi = xr * s + xi * c;
        const float ar = re[i0], ai = im[i0];
        re[i0] = ar + pr; im[i0] = ai + pi; re[i1] = ar - pr; im[i1] = ai - pi;
        __syncthreads();
    }
    for (int j = tid; j < NEMO_BINS; j += 256) { const float a = re[j], c = im[j]; re[j] = a * a + c * c; }
    __syncthreads();
    if (tid < mels) {
        float acc = 0.0f;
        for (int k = fbr[2 * tid]; k < fbr[2 * tid + 1]; ++k) acc = fmaf(re[k], fb[(size_t)k * mels + tid], acc);
        o[tid] = logf(acc + 5.9604644775390625e-08f);
    }
}

// the next mel cache: the last min(16, window) frames of the window (a stream without a window keeps its cache)
__global__ void __launch_bounds__(256) k_nm_mel_roll(const float* __restrict__ win, const int* __restrict__ par, int S, float* __restrict__ cache,
                                                     size_t sstride, int Wp, int mels) {
    const int j = blockIdx.x, b = blockIdx.y, wl = par[NMS_WIN * S + b], nc = min(NMS_MEL_CACHE, wl);
    if (j >= nc) return;
    for (int c = threadIdx.x; c < mels; c += 256) cache[b * sstride + (size_t)j * mels + c] = win[((size_t)b * Wp + wl - nc + j) * mels + c];
}

// ============================================================================ kernel B: frames lo .. hi of the window enter the blocks
// k_sf_intake on the pass's frames: y[b][i] = emb[b][lo[b] + i] g for i < n[b], zero behind them
__global__ void __launch_bounds__(256) k_nm_intake_stream(const float* __restrict__ X, float* __restrict__ Y, const int* __restrict__ par, int S, int Twp,
                                                          int Tp, int d, float g, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / d;
    const int b = (int)(row / Tp), t = (int)(row % Tp), c = (int)(i - row * d);
    Y[i] = t < par[NMS_N * S + b] ? X[((size_t)b * Twp + par[NMS_LO * S + b] + t) * d + c] * g : 0.0f;
}

// K and V of the pass's frames -> the ring rows (pos + i) % R of the stream: [k (d) | v (d)]
__global__ void __launch_bounds__(256) k_nm_ring_put(const float* __restrict__ qkv, const int* __restrict__ par, int S, float* __restrict__ ring,
                                                     size_t sstride, int R, int Tp, int d) {
    const int i = blockIdx.x, b = blockIdx.y;
    if (i >= par[NMS_N * S + b]) return;
    const float* src = qkv + ((size_t)b * Tp + i) * 3 * d + d;
    float* dst = ring + b * sstride + (size_t)((par[NMS_POS * S + b] + i) % R) * 2 * d;
    for (int c = threadIdx.x; c < 2 * d; c += 256) dst[c] = src[c];
}

// ============================================================================ kernel C: chunked-limited attention over the ring
struct NmAttnS {
    const float* q; int ldq;                                 // the pass's rows [S][Tp][ldq], q at column h hd
    const float* ring; size_t sstride; int R, ldk, voff;     // ring row (key % R): k at h hd, v at voff + h hd
    float* out; int ldo;
    const int *cnt, *pos; int Tp, hd;                        // the stream's pass frames and the absolute index of the first
    float qscale, sdk;
    const float *u, *v;
    const float* P; int ldp, poff;
    int C, L, dlo, dhi;
};

__global__ void __launch_bounds__(128) k_nm_attn_stream(NmAttnS p) {
    __shared__ float Ks[32][NM_LDP];
    __shared__ float Pb[64 * NM_LDP];                               // the band; between uses: Q tile, exchanged partials, output tile
    __shared__ float Ub[2][128];
    const int tid = threadIdx.x, lane = tid & 63, dh = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 32, n = min(p.cnt[b], p.Tp), hd = p.hd;
    const size_t rowbase = (size_t)b * p.Tp;
    if (q0 >= n) {                                                  // (uniform over the block)
        for (int i = tid; i < 32 * hd; i += 128) {
            const int t = q0 + i / hd;
            if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + i % hd] = 0.0f;
        }
        return;
    }
    const int pos = p.pos[b], kend = pos + n;                       // the ring holds the keys < kend
    const float* ring = p.ring + b * p.sstride;
#pragma unroll 4
    for (int i = tid; i < 32 * 128; i += 128) {
        const int r = i >> 7, c = i & 127, tq = q0 + r;
        Pb[r * NM_LDP + c] = (tq < n && c < hd) ? p.q[(rowbase + tq) * p.ldq + h * hd + c] * p.qscale : 0.0f;
    }
    for (int i = tid; i < 256; i += 128) {
        const int c = i & 127;
        Ub[i >> 7][c] = c < hd ? (i < 128 ? p.u : p.v)[h * hd + c] : 0.0f;
    }
    __syncthreads();
    const int d0 = dh * 64;
    float qf[32];                                                   // the wave's 64 dimensions of query l31; u and v are added at use (LDS)
#pragma unroll
    for (int i = 0; i < 32; ++i) qf[i] = Pb[l31 * NM_LDP + d0 + 2 * i + kh];
    f32x16_t O[2];
#pragma unroll
    for (int dn = 0; dn < 2; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dn][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const float* Bd0 = Pb;                                          // band products [64 band rows][32 queries] of dh 0, dh 1
    const float* Bd1 = Pb + 2048;
    const float* Sx0 = Pb + 4096;                                   // content scores [32 keys][32 queries] of dh 0, dh 1
    const float* Sx1 = Pb + 4096 + 1024;
    // the rule in absolute frames: the lane's query sees the keys [vlo, vhi); the block walks the absolute 32-aligned tiles that the first
    // and the last live query of it see
    const int qc = (pos + q0 + l31) / p.C, vlo = max(qc - p.L, 0) * p.C, vhi = (qc + 1) * p.C;
    const int wlo = (max((pos + q0) / p.C - p.L, 0) * p.C) & ~31, whi = min(kend, ((pos + min(q0 + 31, n - 1)) / p.C + 1) * p.C);
    for (int kb = wlo; kb < whi; kb += 32) {
        __syncthreads();                                            // the previous tile's reads are done (first pass: the Q fragments are taken)
#pragma unroll 4
        for (int i = tid; i < 32 * 128; i += 128) {
            const int r = i >> 7, c = i & 127, key = kb + r;
            Ks[r][c] = (key < kend && c < hd) ? ring[(size_t)(key % p.R) * p.ldk + h * hd + c] : 0.0f;
        }
        const int base = pos + q0 - kb - 31;                        // distance of band row 0
#pragma unroll 4
        for (int i = tid; i < 64 * 128; i += 128) {
            const int r = i >> 7, c = i & 127, dist = base + r;
            Pb[r * NM_LDP + c] = (dist >= p.dlo && dist <= p.dhi && c < hd) ? p.P[(size_t)(dist + p.poff) * p.ldp + h * hd + c] : 0.0f;
        }
        __syncthreads();
        f32x16_t S, G0, G1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = 0.0f; G0[r] = 0.0f; G1[r] = 0.0f; }
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int k = d0 + 2 * i + kh;
            const float qu = qf[i] + Ub[0][k], qv = qf[i] + Ub[1][k];
            S = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[l31][k], qu, S, 0, 0, 0);
            G0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[l31 * NM_LDP + k], qv, G0, 0, 0, 0);
            G1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[(32 + l31) * NM_LDP + k], qv, G1, 0, 0, 0);
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                                            // both waves have read the band: the space becomes the partials'
        {
            float* Bd = Pb + dh * 2048;
            float* Sx = Pb + 4096 + dh * 1024;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int br = f32_tile_row(r, kh);
                Bd[br * 32 + l31] = G0[r];
                Bd[(br + 32) * 32 + l31] = G1[r];
                Sx[br * 32 + l31] = S[r];
            }
        }
        __syncthreads();
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = f32_tile_row(r, kh), at = (l31 - j + 31) * 32 + l31, key = kb + j;
            const float s = (Sx0[j * 32 + l31] + Sx1[j * 32 + l31]) + (Bd0[at] + Bd1[at]);
            S[r] = (key < kend && key >= vlo && key < vhi) ? s / p.sdk : -INFINITY;
            mx = fmaxf(mx, S[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.0f : m_new;      // the query has seen no key yet: every weight below is exp(-inf) = 0
        const float alpha = expf(m_run - m_use);
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = expf(S[r] - m_use); psum += S[r]; }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int dn = 0; dn < 2; ++dn) {
#pragma unroll
            for (int r = 0; r < 16; ++r) O[dn][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {                          // V^T straight from the ring: 32 consecutive floats of key f32_tile_row(r, kh)
                const int key = kb + f32_tile_row(r, kh), d = d0 + dn * 32 + l31;
                const float vv = (key < kend && d < hd) ? ring[(size_t)(key % p.R) * p.ldk + p.voff + h * hd + d] : 0.0f;
                O[dn] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, S[r], O[dn], 0, 0, 0);
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);         // > 0 for a live query: it sees itself
    __syncthreads();
#pragma unroll
    for (int dn = 0; dn < 2; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) Pb[l31 * NM_LDP + d0 + dn * 32 + f32_tile_row(r, kh)] = O[dn][r] / l_tot;
    __syncthreads();
    for (int i = tid; i < 32 * hd; i += 128) {
        const int r = i / hd, c = i - r * hd, t = q0 + r;
        if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + c] = t < n ? Pb[r * NM_LDP + c] : 0.0f;
    }
}

// ============================================================================ kernel D: GLU + causal depthwise conv + LayerNorm statistics, carried
// k_nm_glu_dwconv_ln at padl = k - 1 with hin [S][k - 1][C] (the stream's last gated frames, oldest first) where offline pads zeros; block 0
// of a stream writes hout = the last k - 1 gated frames of [hin ++ the pass's]
__global__ void __launch_bounds__(256) k_nm_glu_dwconv_ln_stream(const float* __restrict__ pw, const float* __restrict__ taps, const float* __restrict__ bias,
                                                                 const int* __restrict__ cnt, float* out, float* __restrict__ stats,
                                                                 const float* __restrict__ hin, float* __restrict__ hout, size_t sstride, int Tp, int C,
                                                                 int k, float eps) {
    __shared__ float g[NM_DW_TT + SF_DW_MAXK - 1][64];
    const int cl = threadIdx.x & 63, tl = threadIdx.x >> 6, b = blockIdx.y, t0 = blockIdx.x * NM_DW_TT, tw = t0 + tl * 4, padl = k - 1;
    const int n = min(cnt[b], Tp);
    const size_t rowbase = (size_t)b * Tp;
    const float* hi_ = hin + b * sstride;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int ch = c0 + cl;
        const bool live = ch < C;
        __syncthreads();
        for (int r = tl; r < NM_DW_TT + k - 1; r += 4) {
            const int t = t0 - padl + r;
            float v = 0.0f;
            if (live && t >= 0 && t < n) {
                const float* row = pw + (rowbase + t) * 2 * C;
                v = row[ch] * (1.0f / (1.0f + expf(-row[C + ch])));
            } else if (live && t < 0) {
                v = hi_[(size_t)(padl + t) * C + ch];
            }
            g[r][cl] = v;
        }
        __syncthreads();
        if (blockIdx.x == 0 && live)                                // the next history: frame n - padl + r, from the tile or from further back
            for (int r = tl; r < padl; r += 4) {
                const int t = n - padl + r;
                float v;
                if (t < 0) v = hi_[(size_t)(padl + t) * C + ch];
                else if (t < NM_DW_TT) v = g[t + padl][cl];
                else { const float* row = pw + (rowbase + t) * 2 * C; v = row[ch] * (1.0f / (1.0f + expf(-row[C + ch]))); }
                hout[b * sstride + (size_t)r * C + ch] = v;
            }
        if (!live) continue;
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
            if (t >= Tp) continue;
            const float v = t < n ? acc[i] : 0.0f;
            out[(rowbase + t) * C + ch] = v;
            s[i] += v;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = tw + i;
        const float mean = wave_sum(s[i]) / (float)C;
        float q = 0.0f;
        if (t < n)
            for (int ch = cl; ch < C; ch += 64) { const float v = out[(rowbase + t) * C + ch] - mean; q = fmaf(v, v, q); }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
        if (cl == 0 && t < Tp) { stats[2 * (rowbase + t)] = t < n ? mean : 0.0f; stats[2 * (rowbase + t) + 1] = t < n ? rstd : 0.0f; }
    }
}

// ============================================================================ kernel E: greedy RNN-T decode of a pass, resumed
// state of stream b: dec + b sstride = h' [2][P], c' [2][P] (the proposal behind the last token from the committed state), joint.pred of it
// [J]; ist + 4 b = started, tokens emitted, flag (the capacity was reached: further frames are ignored), joint evaluations.  Tokens of the
// feed go to r.tokens / r.frames [S][cap] at index (count - tok0[b]); frames are absolute (pos[b] + t).
struct NmRnntS { NmRnnt r; float* dec; size_t sstride; int* ist; const int *pos, *tok0; };

__global__ void __launch_bounds__(NM_NT) k_nm_rnnt_stream(NmRnntS q) {
    __shared__ float xs[NM_MAXW], hs[2][NM_MAXW], cs[2][NM_MAXW], hn[2][NM_MAXW], cn[2][NM_MAXW], pp[NM_MAXW], zs[NM_MAXW];
    __shared__ float rv[NM_NT / 64];
    __shared__ int ri[NM_NT / 64], dec;
    const NmRnnt& p = q.r;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, P = p.P, J = p.J, V = p.V, blank = p.V - 1, top = p.layers - 1;
    const int T = min(p.cnt[b], p.Tp);
    int* ist = q.ist + 4 * b;
    float* sd = q.dec + b * q.sstride;
    int n = ist[1], steps = ist[3], flagged = ist[2];
    const int started = ist[0];
    if (T == 0 || flagged) return;                                  // (uniform) no frames, or the capacity was reached: the state stays
    auto predict = [&](int token) {
        for (int u = tid; u < P; u += NM_NT) xs[u] = token == blank ? 0.0f : p.embed[(size_t)token * P + u];
        __syncthreads();
        nm_lstm_layer(p.wxT[0], p.whT[0], p.bih[0], p.bhh[0], xs, hs[0], cs[0], hn[0], cn[0], P);
        if (top == 1) nm_lstm_layer(p.wxT[1], p.whT[1], p.bih[1], p.bhh[1], hn[0], hs[1], cs[1], hn[1], cn[1], P);
        for (int j = tid; j < J; j += NM_NT) {
            float acc = p.bp[j];
            for (int k = 0; k < P; ++k) acc = fmaf(p.wpT[(size_t)k * J + j], hn[top][k], acc);
            pp[j] = acc;
        }
        __syncthreads();
    };
    for (int u = tid; u < P; u += NM_NT) {                          // (hn[1], cn[1]: one layer never writes them, and they are carried)
        hs[0][u] = 0.0f; hs[1][u] = 0.0f; cs[0][u] = 0.0f; cs[1][u] = 0.0f; hn[1][u] = 0.0f; cn[1][u] = 0.0f;
    }
    if (!started) {
        predict(blank);
    } else {
        for (int u = tid; u < P; u += NM_NT) { hn[0][u] = sd[u]; hn[1][u] = sd[P + u]; cn[0][u] = sd[2 * P + u]; cn[1][u] = sd[3 * P + u]; }
        for (int j = tid; j < J; j += NM_NT) pp[j] = sd[4 * P + j];
        __syncthreads();
    }
    int t = 0, ns = 0;
    const int bound = p.max_symbols > 0 ? T * p.max_symbols + T : T + (p.cap - n) + 1;   // a step emits or advances
    const int tok0 = q.tok0[b], pos = q.pos[b];
    int* otok = p.tokens + (size_t)b * p.cap;
    int* ofrm = p.frames + (size_t)b * p.cap;
    for (int it = 0; it < bound && t < T; ++it) {                   // (every branch below is uniform over the block)
        const float* e = p.encp + ((size_t)b * p.Tp + t) * J;
        for (int j = tid; j < J; j += NM_NT) zs[j] = fmaxf(e[j] + pp[j], 0.0f);
        __syncthreads();
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int v = tid; v < V; v += NM_NT) {
            float acc = p.bo[v];
            for (int j = 0; j < J; ++j) acc = fmaf(p.woT[(size_t)j * V + v], zs[j], acc);
            if (nm_better(acc, v, bv, bi)) { bv = acc; bi = v; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (nm_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < NM_NT / 64; ++w)
                if (nm_better(rv[w], ri[w], bv, bi)) { bv = rv[w]; bi = ri[w]; }
            dec = bi < V ? bi : 0;
        }
        __syncthreads();
        const int tok = dec;
        ++steps;
        // NemoDecodingLogic.rnntStep
        if (tok == blank) { t += 1; ns = 0; continue; }
        if (n >= p.cap) { flagged = 1; break; }
        if (tid == 0) { otok[n - tok0] = tok; ofrm[n - tok0] = pos + t; }
        ++n;
        for (int u = tid; u < P; u += NM_NT) { hs[0][u] = hn[0][u]; hs[1][u] = hn[1][u]; cs[0][u] = cn[0][u]; cs[1][u] = cn[1][u]; }
        __syncthreads();
        predict(tok);
        ++ns;
        if (p.max_symbols > 0 && ns >= p.max_symbols) { t += 1; ns = 0; }
    }
    for (int u = tid; u < P; u += NM_NT) { sd[u] = hn[0][u]; sd[P + u] = hn[1][u]; sd[2 * P + u] = cn[0][u]; sd[3 * P + u] = cn[1][u]; }
    for (int j = tid; j < J; j += NM_NT) sd[4 * P + j] = pp[j];
    if (tid == 0) { ist[0] = 1; ist[1] = n; ist[2] = flagged; ist[3] = steps; }
}

// ============================================================================ kernel F: a stream's state to zeros
// streams first .. first + gridDim.y - 1: rings, conv histories, mel cache, decoder state (floats) and the four counters
__global__ void __launch_bounds__(256) k_nm_state_reset(float* __restrict__ state, size_t sstride, int* __restrict__ ist, int first) {
    const int b = first + blockIdx.y;
    float* s = state + b * sstride;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < sstride; i += (size_t)gridDim.x * 256) s[i] = 0.0f;
    if (blockIdx.x == 0 && threadIdx.x < 4) ist[4 * b + threadIdx.x] = 0;
}

// tests: the pass's frames of a stage appended to the feed's tap rows (not counted as a launch of the engine)
__global__ void __launch_bounds__(256) k_nm_tap_put(const float* __restrict__ X, int ldx, int off, const int* __restrict__ par, int S, const int* __restrict__ fill,
                                                    float* __restrict__ Y, int Tp, int cap, int w) {
    const int i = blockIdx.x, b = blockIdx.y, at = fill[b] + i;
    if (i >= par[NMS_N * S + b] || at >= cap) return;
    for (int c = threadIdx.x; c < w; c += 256) Y[((size_t)b * cap + at) * w + c] = X[((size_t)b * Tp + i + (off ? par[NMS_LO * S + b] : 0)) * ldx + c];
}
__global__ void k_nm_tap_advance(const int* __restrict__ par, int S, int* __restrict__ fill, int reset) {
    const int b = threadIdx.x;
    if (b < S) fill[b] = reset ? 0 : fill[b] + par[NMS_N * S + b];
}
}  // namespace

template <class Ctx>
static void nm_attn_stream(Ctx* c, const NmAttnS& p, int heads, int streams) {
    MIS_LAUNCH(c, k_nm_attn_stream, dim3(cdiv(p.Tp, 32), heads, streams), dim3(128), p);
}

// ============================================================================ the session
struct NmsFrames { int consumed = 0, emitted = 0, cache = 0; };     // mel frames consumed, encoder frames emitted, mel frames cached
struct NmsStream {
    std::vector<float> tail;                                        // the stream's samples from absolute index tail0 on
    int64_t tail0 = 0, seen = 0;
    NmsFrames f;                                                    // the frame bookkeeping (nms_plan)
    int ntok = 0, lang = 0;                                         // tokens the host knows of, the prompt index
    bool fin = false, done = false, flag = false;
};

struct mis_nemotron_stream {
    mis_nemotron* m = nullptr;
    hipStream_t stream = nullptr;                                   // the model's: feeds and offline calls are ordered
    int launches = 0, S = 0, left = 0, right = 0, C = 0, maxchunks = 0, Tq = 0, R = 0, Wp = 0, T1p = 0, T2p = 0, Twp = 0, parity = 0, slot = 0;
    int64_t sstage = 0;                                             // samples a stream stages for a pass
    NmCtx ctx{};
    size_t SS = 0, o_ring = 0, o_hist = 0, o_mel = 0, o_dec = 0;    // a stream's state: floats, and the offsets of its parts
    DevBuf<float> state, stage, win, s0, s1, s2, emb, h, stats, big, qkv, att, prm, encp, tapbuf;
    int bf16 = 0;                                                   // the blocks of nemotron_stream_bf16.h: ring and history hold bf16, as do these
    DevBuf<bf16_t> big16, qkv16, att16;
    DevBuf<int> ist, par, dtok, dfrm, tapfill;
    PinnedBuf<float> hstage;
    PinnedBuf<int> hpar, hist_;
    std::vector<NmsStream> st;
    int tapcap = 0, last_launches = 0;
    HipEvents<4> ev;                                                // a feed's start and end; the last pass's decode launch (split timing)
    bool split = false, split_timed = false;                        // split_timed: the last feed recorded both events
    float last_ms = 0.0f;
};

static size_t nms_hist(const mis_nemotron_stream* s, int parity, int layer) {
    return s->o_hist + ((size_t)parity * s->m->L + layer) * (s->m->ck - 1) * s->m->d;
}

extern "C" mis_status mis_nemotron_stream_create_dtype(mis_nemotron* m, int streams, int left, int right, int max_pass_frames, mis_dtype dtype,
                                                       mis_nemotron_stream** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(m && out, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(m->finalized, MIS_ERR_NOT_INITIALIZED, "model not finalized");
    MIS_REQUIRE(streams >= 1 && streams <= NM_MAX_BATCH, MIS_ERR_INVALID_INPUT, "streams %d outside 1..%d", streams, NM_MAX_BATCH);
    MIS_REQUIRE(dtype == MIS_F32 || dtype == MIS_BF16, MIS_ERR_INVALID_INPUT, "stream session dtype %d: only MIS_F32 and MIS_BF16 are implemented", (int)dtype);
    const bool bf = dtype == MIS_BF16;
    MIS_REQUIRE(bf || !m->enc_bf16, MIS_ERR_INVALID_INPUT,
                "encoder_dtype bfloat16: an f32 stream session runs the f32 block matrices, which are not resident in this mode (ask for a bf16 session)");
    MIS_REQUIRE(!bf || m->enc_bf16, MIS_ERR_INVALID_INPUT,
                "a bf16 stream session runs the bf16 block matrices: finalize the model with encoder_dtype bfloat16 (nothing is rounded for a session)");
    MIS_REQUIRE(m->cfg.normalize == 0, MIS_ERR_INVALID_INPUT,
                "normalize per_feature: a stream session requires NA mel normalization (per-utterance statistics are not frozen incrementally)");
    MIS_REQUIRE(right >= 0 && right < (1 << 20) && left >= 0 && left % (right + 1) == 0, MIS_ERR_INVALID_INPUT,
                "att_context_size (%d, %d): a stream needs right >= 0, left >= 0 and left %% (right + 1) == 0", left, right);
    MIS_REQUIRE(m->cfg.conv_pad_right == 0, MIS_ERR_INVALID_INPUT, "conv_context_size (%d, %d): a stream needs the causal pad (conv_kernel_size - 1, 0)",
                m->cfg.conv_pad_left, m->cfg.conv_pad_right);
    const int C = right + 1, L = left / C;
    NmCtx ctx{C, L, -(C - 1), L * C + C - 1};
    MIS_REQUIRE(ctx.dlo >= m->tab_lo && ctx.dhi <= m->tab_hi, MIS_ERR_INVALID_INPUT,
                "att_context_size (%d, %d) needs the distances %d..%d: the model's listed contexts cover %d..%d", left, right, ctx.dlo, ctx.dhi, m->tab_lo,
                m->tab_hi);
    MIS_REQUIRE(max_pass_frames >= C && max_pass_frames <= 4096, MIS_ERR_INVALID_INPUT, "max_pass_frames %d outside %d (a chunk) .. 4096", max_pass_frames, C);
    HIP_CHECK(hipSetDevice(m->device));
    auto s = std::make_unique<mis_nemotron_stream>();
    s->m = m; s->stream = m->stream; s->S = streams; s->left = left; s->right = right; s->C = C; s->ctx = ctx;
    s->maxchunks = max_pass_frames / C;
    s->Tq = s->maxchunks * C + 2;                                   // the last pass of a stream may bring one frame more (the right pad's)
    s->R = (int)round_up((size_t)left + s->Tq + 32, 32);
    s->Wp = NMS_MEL_CACHE + s->maxchunks * C * 8;
    s->T1p = nm_half(s->Wp); s->T2p = nm_half(s->T1p); s->Twp = nm_half(s->T2p);
    s->sstage = (int64_t)s->maxchunks * C * 8 * NEMO_HOP + NEMO_NFFT + 8;
    const size_t B = streams, d = m->d, Lr = m->L, mels = m->mels, Cc = m->C, M = B * s->Tq;
    s->o_ring = 0;
    s->o_hist = s->o_ring + Lr * s->R * 2 * d / (bf ? 2 : 1);       // (a bf16 session's ring takes half the floats; its history rows are
    s->o_mel = s->o_hist + 2 * Lr * (m->ck - 1) * d;                //  2 d bf16 = d floats, as the f32 gated frames)
    s->o_dec = s->o_mel + NMS_MEL_CACHE * mels;
    s->SS = round_up(s->o_dec + 4 * m->P + m->J, 64);
    s->state.alloc(B * s->SS); s->ist.alloc(4 * B);
    s->stage.alloc(B * s->sstage); s->win.alloc(B * s->Wp * mels);
    s->s0.alloc(B * s->T1p * m->F1 * Cc); s->s1.alloc(B * s->T2p * m->F2 * Cc); s->s2.alloc(B * s->Twp * m->F3 * Cc); s->emb.alloc(B * s->Twp * d);
    s->h.alloc(M * d); s->stats.alloc(M * 2);
    s->bf16 = bf;
    if (bf) {                                                       // ring [R][2 d] and history [ck - 1][2 d] in bf16: the f32 state's byte counts
        s->big16.alloc(M * std::max<size_t>(m->f, 2 * d)); s->qkv16.alloc(M * 3 * d); s->att16.alloc(M * d);
        if (m->PH) s->big.alloc(M * m->PH);
    } else {
        s->big.alloc(M * std::max<size_t>(std::max<size_t>(m->f, 2 * d), m->PH)); s->qkv.alloc(M * 3 * d);
        s->att.alloc(M * d);
    }
    if (m->PH) s->prm.alloc(M * d);
    s->encp.alloc(M * m->J);
    s->par.alloc(NMS_FIELDS * B); s->dtok.alloc(B * m->cap); s->dfrm.alloc(B * m->cap); s->tapfill.alloc(B);
    s->hstage.alloc((size_t)NMS_SLOTS * B * s->sstage); s->hpar.alloc((size_t)NMS_SLOTS * NMS_FIELDS * B); s->hist_.alloc(4 * B);
    s->st.assign(streams, NmsStream{});
    MIS_LAUNCH(s.get(), k_nm_state_reset, dim3(cdiv(std::min<size_t>(s->SS, 1 << 22), 256), streams), dim3(256), s->state.p, s->SS, s->ist.p, 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s->stream));
    s->launches = 0;
    *out = s.release();
    MIS_API_END
}

extern "C" mis_status mis_nemotron_stream_create(mis_nemotron* m, int streams, int left, int right, int max_pass_frames, mis_nemotron_stream** out) {
    return mis_nemotron_stream_create_dtype(m, streams, left, right, max_pass_frames, MIS_F32, out);
}

extern "C" void mis_nemotron_stream_destroy(mis_nemotron_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->m->device);
    (void)hipStreamSynchronize(s->stream);
    delete s;
}

extern "C" mis_status mis_nemotron_stream_reset(mis_nemotron_stream* s, int stream, int lang) {
    MIS_API_BEGIN
    MIS_REQUIRE(s && stream >= -1 && stream < s->S, MIS_ERR_INVALID_INPUT, "stream %d outside -1 (all) .. %d", stream, s ? s->S - 1 : 0);
    MIS_REQUIRE(!s->m->PH || (lang >= 0 && lang < s->m->NP), MIS_ERR_INVALID_INPUT, "prompt index %d outside 0..%d", lang, s->m->NP - 1);
    HIP_CHECK(hipSetDevice(s->m->device));
    const int first = stream < 0 ? 0 : stream, count = stream < 0 ? s->S : 1;
    const int kept = s->launches;
    MIS_LAUNCH(s, k_nm_state_reset, dim3(cdiv(std::min<size_t>(s->SS, 1 << 22), 256), count), dim3(256), s->state.p, s->SS, s->ist.p, first);
    s->launches = kept;
    HIP_CHECK(hipGetLastError());
    for (int b = first; b < first + count; ++b) { s->st[b] = NmsStream{}; s->st[b].lang = s->m->PH ? lang : 0; }
    MIS_API_END
}

extern "C" int mis_nemotron_stream_launches(const mis_nemotron_stream* s) { return s ? s->last_launches : 0; }

extern "C" int64_t mis_nemotron_stream_frames_seen(const mis_nemotron_stream* s, int stream) {
    return s && stream >= 0 && stream < s->S ? s->st[stream].f.emitted : -1;
}

// ---------------------------------------------------------------------------- the frame bookkeeping of a stream: pure, no device
// frozenMelFrames: frame m is frozen once m hop + n_fft / 2 <= samples seen
static int nms_frozen(int64_t seen) {
    if (seen < NEMO_NFFT / 2) return 0;
    return (int)std::min<int64_t>(nm_frames(seen), (seen - NEMO_NFFT / 2) / NEMO_HOP + 1);
}

struct NmsPlan { int take, end, win, t1, t2, t3, lo, n, first; bool last; };

// streamEncodeChunks' next iteration for a stream that has seen `seen` samples (fin: all of it), with up to max_chunks whole chunks of C
// encoder frames taken at once (the flushed tail goes along while the window holds it): the window [cache ++ take mel frames], its
// sub-sampled lengths, the frames lo .. lo + n - 1 of it that enter the blocks as the absolute frames first ..; x is advanced.  false:
// no whole chunk is ready (an empty stream yields nothing, finished or not: advance's guard).
static bool nms_plan(NmsFrames& x, int64_t seen, bool fin, int C, int max_chunks, NmsPlan& p) {
    if (seen == 0) return false;
    const int chunkMel = C * 8, limit = fin ? nm_frames(seen) : nms_frozen(seen), avail = limit - x.consumed;
    p.take = std::min(avail / chunkMel, max_chunks) * chunkMel;
    if (fin && p.take < avail && p.take < max_chunks * chunkMel) p.take = avail;
    if (p.take <= 0) return false;
    p.end = x.consumed + p.take; p.win = x.cache + p.take; p.last = fin && p.end >= limit;
    const int base = (x.consumed - x.cache) / 8;
    p.lo = x.emitted - base; p.t1 = nm_half(p.win); p.t2 = nm_half(p.t1); p.t3 = nm_half(p.t2);
    const int hi = p.last ? p.t3 : p.end / 8 - base;
    p.n = std::max(hi - p.lo, 0); p.first = x.emitted;
    x.consumed = p.end; x.cache = std::min(p.win, NMS_MEL_CACHE); x.emitted = base + std::max(p.lo, hi);
    return true;
}

// the passes a stream runs once it has seen `seen` samples, from state[3] = consumed, emitted, cached (advanced): passes[2 i] = the first
// absolute encoder frame of pass i, passes[2 i + 1] = its frame count; *n_passes = how many there are (the first max_passes are written)
extern "C" mis_status mis_nemotron_stream_plan(int64_t seen, int final, int chunk_frames, int max_chunks, int32_t* state, int32_t* passes, int max_passes,
                                               int32_t* n_passes) {
    MIS_API_BEGIN
    MIS_REQUIRE(state && n_passes && (passes || max_passes == 0) && seen >= 0 && seen < ((int64_t)1 << 30) && chunk_frames >= 1 && chunk_frames <= (1 << 20) &&
                    max_chunks >= 1 && max_chunks <= 4096 && max_passes >= 0, MIS_ERR_INVALID_INPUT, "stream plan: bad argument");
    NmsFrames x{state[0], state[1], state[2]};
    NmsPlan p;
    int k = 0;
    for (; nms_plan(x, seen, final != 0, chunk_frames, max_chunks, p); ++k)
        if (k < max_passes) { passes[2 * k] = p.first; passes[2 * k + 1] = p.n; }
    state[0] = x.consumed; state[1] = x.emitted; state[2] = x.cache; *n_passes = k;
    MIS_API_END
}

// Which contraction a bf16 pass takes: k_nm_gemm_bf16_rows, or k_pk_gemm_bf16 at 64 x 64.  Either gives an element the same bits, so this is
// a matter of time alone.  The short-pass kernel's time follows its 16-row tiles, ceil(live rows / 16); the 64 x 64 rule's follows its 64-row
// tiles, one per ceil(frames / 64) of every stream with frames, however few of the 64 rows are live.  Measured per role and pass shape, one
// chunk and three chunks a stream (profiles/nemotron_stream_bf16/README.md): summed over a block the short-pass kernel wins wherever it
// has no more tiles than the 64 x 64 rule (64 x 1, 16 x 14, 64 x 14 frames) and up to 11 tiles against fewer (4 streams x 44 frames), ties at
// 22 tiles against 8 and loses from 44 against 16 on.  Hence: the short-pass kernel while its tiles are no more than the 64 x 64 rule's, or
// no more than NMS_ROWS_TILES.  Inside it the roles that load a bf16 activation are fastest at 32 columns a block and the roles that stage a
// LayerNorm at 64 (a block's waves share the staging arithmetic).
constexpr int NMS_ROWS_TILES = 16;

// the blocks of a bf16 session's pass on s->h: the f32 loop of nms_pass launch for launch (16 L), on nemotron_stream_bf16.h's kernels;
// live = the pass's frames over all streams, tiles64 = the 64-row tiles they occupy stream by stream
template <class Tap>
static void nms_blocks_bf16(mis_nemotron_stream* s, int live, int tiles64, Tap&& tap) {
    mis_nemotron* m = s->m;
    const int S = s->S, d = m->d, f = m->f, Tp = s->Tq, M = S * Tp;
    const int *cn = s->par.p + NMS_N * S, *cpos = s->par.p + NMS_POS * S;
    bf16_t* st = reinterpret_cast<bf16_t*>(s->state.p);            // a stream's state as bf16 elements: offsets and stride double
    const size_t ss = 2 * s->SS;
    const bool rows = cdiv(live, 16) <= std::max(tiles64, NMS_ROWS_TILES);
    auto stats = [&]() { MIS_LAUNCH(s, k_sf_stats, dim3(cdiv(M, 4)), dim3(256), s->h.p, s->stats.p, d, 1e-5f, M); };
    auto gemm = [&](const PkbRole& r, const bf16_t* W, const float* bias, int N, int K, const float* lnw, const float* lnb, const bf16_t* xb, bf16_t* yb, float ra) {
        PkbGemm p{};
        p.W = W; p.bias = bias; p.cnt = cn; p.Tp = Tp; p.K = K; p.N = N; p.epi = r.epi; p.ldx = K; p.ldy = N;
        if (r.load != PKB_LOAD_BF16) { p.stats = s->stats.p; p.lnw = lnw; p.lnb = lnb; }
        if (r.load == PKB_LOAD_LN) p.Xf = s->h.p;
        else p.Xb = xb;
        if (r.epi == PKB_EPI_RES) { p.Yf = s->h.p; p.R = s->h.p; p.ldr = N; p.ra = ra; }
        else p.Yb = yb;
        nmr_gemm_launch(s, p, r.load, !rows ? PKB_TILE64 : r.load == PKB_LOAD_BF16 ? NMR_ROWS32 : NMR_ROWS64, S, live);
    };
    bf16_t *big = s->big16.p, *qkv = s->qkv16.p, *att = s->att16.p;
    for (int li = 0; li < m->L; ++li) {
        const mis_nemotron::Layer& l = m->fc[li];
        const mis_nemotron::Layer16& w = m->fc16[li];
        stats();
        gemm(PKB_ROLE[PKB_FF1A], w.ff1a, l.ff1a.b, f, d, l.ln1w, l.ln1b, nullptr, big, 0.0f);
        gemm(PKB_ROLE[PKB_FF1B], w.ff1b, l.ff1b.b, d, f, nullptr, nullptr, big, nullptr, 0.5f);
        stats();
        gemm(PKB_ROLE[PKB_QKV], w.qkv, l.qkv.b, 3 * d, d, l.lnaw, l.lnab, nullptr, qkv, 0.0f);
        bf16_t* ring = st + 2 * s->o_ring + (size_t)li * s->R * 2 * d;
        MIS_LAUNCH(s, k_nm_ring_put_bf16, dim3(Tp, S), dim3(256), qkv, cn, cpos, ring, ss, s->R, Tp, d);
        NmbAttnS ap{qkv, 3 * d, ring, ss, s->R, 2 * d, d, att, d, cn, cpos, Tp, m->hd, 1.0f, sqrtf((float)m->hd), l.u, l.v, w.P, d, -m->tab_lo,
                    s->ctx.C, s->ctx.L, s->ctx.dlo, s->ctx.dhi};
        nmb_attn_stream(s, ap, m->H, m->hd, S);
        gemm(PKB_ROLE[PKB_O], w.o, l.o.b, d, d, nullptr, nullptr, att, nullptr, 1.0f);
        stats();
        gemm(PKB_ROLE[PKB_PW1], w.pw1, l.pw1.b, 2 * d, d, l.lncw, l.lncb, nullptr, big, 0.0f);
        nmb_glu_dwconv_ln_stream(s, big, l.dw, l.dwb, cn, att, s->stats.p, st + 2 * nms_hist(s, s->parity, li), st + 2 * nms_hist(s, s->parity ^ 1, li), ss, Tp, d,
                                 m->ck, S);
        gemm(NMB_PW2, w.pw2, l.pw2.b, d, d, l.cnw, l.cnb, att, nullptr, 1.0f);
        stats();
        gemm(PKB_ROLE[PKB_FF2A], w.ff2a, l.ff2a.b, f, d, l.ln2w, l.ln2b, nullptr, big, 0.0f);
        gemm(PKB_ROLE[PKB_FF2B], w.ff2b, l.ff2b.b, d, f, nullptr, nullptr, big, nullptr, 0.5f);
        MIS_LAUNCH(s, k_sf_ln, dim3(cdiv(M, 4)), dim3(256), s->h.p, s->h.p, l.lnow, l.lnob, d, 1e-5f, M, cn, Tp);
        tap(li + 1, s->h.p, d, Tp, 0);
    }
}

// one pass over every stream that has a whole chunk ready (finished streams: whatever is left); false: nobody had work
static bool nms_pass(mis_nemotron_stream* s) {
    mis_nemotron* m = s->m;
    const int S = s->S;
    if (s->slot == NMS_SLOTS) { HIP_CHECK(hipStreamSynchronize(s->stream)); s->slot = 0; }   // the staging slots are in flight: wait once
    int* par = s->hpar.p + (size_t)s->slot * NMS_FIELDS * S;
    float* stage = s->hstage.p + (size_t)s->slot * S * s->sstage;
    std::fill(par, par + NMS_FIELDS * S, 0);
    int maxwin = 0;
    size_t used = 0;                                                // samples staged so far: the streams with work, packed
    for (int b = 0; b < S; ++b) {
        NmsStream& x = s->st[b];
        par[NMS_LANG * S + b] = x.lang; par[NMS_TOK0 * S + b] = x.ntok; par[NMS_POS * S + b] = x.f.emitted;
        const NmsFrames was = x.f;
        NmsPlan p;
        if (x.done || !nms_plan(x.f, x.seen, x.fin, s->C, s->maxchunks, p)) continue;
        const int64_t a0 = std::max<int64_t>(0, (int64_t)was.consumed * NEMO_HOP - NEMO_NFFT / 2 - 1);
        const int64_t a1 = std::min<int64_t>(x.seen, (int64_t)(p.end - 1) * NEMO_HOP + NEMO_NFFT / 2);
        MIS_REQUIRE(a0 >= x.tail0 && a1 - a0 <= s->sstage && p.n <= s->Tq && p.win <= s->Wp && x.seen < ((int64_t)1 << 30), MIS_ERR_GENERATION_FAILED,
                    "stream %d: pass bookkeeping out of range (samples %lld..%lld, %d frames, window %d)", b, (long long)a0, (long long)a1, p.n, p.win);
        std::copy(x.tail.begin() + (a0 - x.tail0), x.tail.begin() + (a1 - x.tail0), stage + used);
        par[NMS_WIN * S + b] = p.win; par[NMS_T1 * S + b] = p.t1; par[NMS_T2 * S + b] = p.t2; par[NMS_T3 * S + b] = p.t3; par[NMS_N * S + b] = p.n;
        par[NMS_LO * S + b] = p.lo; par[NMS_CACHE * S + b] = was.cache; par[NMS_FRAME0 * S + b] = was.consumed; par[NMS_ORIGIN * S + b] = (int)a0;
        par[NMS_SEEN * S + b] = (int)x.seen; par[NMS_SOFF * S + b] = (int)used;
        used += (size_t)(a1 - a0);
        maxwin = std::max(maxwin, p.win);
        x.done = p.last;
        const int64_t keep = std::max<int64_t>(x.tail0, (int64_t)p.end * NEMO_HOP - NEMO_NFFT / 2 - 1);
        x.tail.erase(x.tail.begin(), x.tail.begin() + (keep - x.tail0));
        x.tail0 = keep;
    }
    if (!maxwin) return false;
    int live = 0, tiles64 = 0;                                      // the frames of the pass over all streams; their 64-row tiles, stream by stream
    for (int b = 0; b < S; ++b) { live += par[NMS_N * S + b]; tiles64 += cdiv(par[NMS_N * S + b], 64); }
    hipStream_t q = s->stream;
    HIP_CHECK(hipMemcpyAsync(s->par.p, par, (size_t)NMS_FIELDS * S * 4, hipMemcpyHostToDevice, q));
    if (used) HIP_CHECK(hipMemcpyAsync(s->stage.p, stage, used * 4, hipMemcpyHostToDevice, q));
    s->slot += 1;
    const int* dp = s->par.p;
    const int *cW = dp + NMS_WIN * S, *c1 = dp + NMS_T1 * S, *c2 = dp + NMS_T2 * S, *c3 = dp + NMS_T3 * S, *cn = dp + NMS_N * S, *cpos = dp + NMS_POS * S;
    const int d = m->d, f = m->f, Cc = m->C, F1 = m->F1, F2 = m->F2, F3 = m->F3, Tp = s->Tq, M = S * Tp;
    const int T1p = nm_half(maxwin), T2p = nm_half(T1p), Twp = nm_half(T2p);
    float* st = s->state.p;
    MIS_LAUNCH(s, k_nm_mel_stream, dim3(maxwin, S), dim3(256), s->stage.p, dp, S, st + s->o_mel, s->SS, m->cfg.preemphasis, m->window, m->twc, m->tws,
               m->fb, m->fbr.p, s->win.p, s->Wp, m->mels);
    const size_t n0 = (size_t)S * T1p * F1 * Cc;
    MIS_LAUNCH(s, k_nm_conv0, dim3((unsigned)((n0 + 255) / 256)), dim3(256), s->win.p, cW, c1, m->c0w, m->c0b, s->s0.p, s->Wp, m->mels, T1p, F1, Cc, n0);
    auto dwpw = [&](const float* in, const int* cin, int Tin, int Fin, const float* dww, const float* dwb, const SfLin& pw, float* out, const int* cout,
                    int Tout, int Fout) {
        SfGemm p{};
        p.X = in; p.ldx = Cc; p.W = pw.w; p.bias = pw.b; p.Y = out; p.ldy = Cc; p.cnt = cout; p.Tp = Tout; p.rowmul = Fout; p.K = Cc; p.N = Cc;
        p.load = NM_LOAD_DWC; p.act = SF_ACT_RELU; p.cnt_in = cin; p.Tin = Tin; p.Fin = Fin; p.Fout = Fout; p.dww = dww; p.dwb = dwb;
        nm_gemm(s, p, S);
    };
    dwpw(s->s0.p, c1, T1p, F1, m->dw2w, m->dw2b, m->pw3, s->s1.p, c2, T2p, F2);
    dwpw(s->s1.p, c2, T2p, F2, m->dw5w, m->dw5b, m->pw6, s->s2.p, c3, Twp, F3);
    sf_gemm(s, sf_lin(s->s2.p, F3 * Cc, m->lin, s->emb.p, d, c3, Twp), S);
    const size_t nd = (size_t)M * d;
    MIS_LAUNCH(s, k_nm_intake_stream, dim3((unsigned)((nd + 255) / 256)), dim3(256), s->emb.p, s->h.p, dp, S, Twp, Tp, d,
               m->cfg.scale_input ? sqrtf((float)d) : 1.0f, nd);
    auto tap = [&](int stage, const float* x, int w, int Tx, int off) {
        if (!s->tapcap) return;
        const int kept = s->launches;
        MIS_LAUNCH(s, k_nm_tap_put, dim3(Tp, S), dim3(256), x, w, off, dp, S, s->tapfill.p, s->tapbuf.p + (size_t)stage * S * s->tapcap * std::max(d, m->J), Tx,
                   s->tapcap, w);
        s->launches = kept;
    };
    tap(0, s->emb.p, d, Twp, 1);
    auto stats = [&](const float* x) { MIS_LAUNCH(s, k_sf_stats, dim3(cdiv(M, 4)), dim3(256), x, s->stats.p, d, 1e-5f, M); };
    auto ln_lin = [&](const float* x, const float* w, const float* b, const SfLin& l, float* y, int N, int act) {
        SfGemm p = sf_lin(x, d, l, y, N, cn, Tp, act);
        p.load = SF_LOAD_LN; p.stats = s->stats.p; p.lnw = w; p.lnb = b;
        sf_gemm(s, p, S);
    };
    auto res_lin = [&](const float* x, int K, const SfLin& l, float* hres, int N, float ra) {
        SfGemm p = sf_lin(x, K, l, hres, N, cn, Tp);
        p.R = hres; p.ldr = N; p.ra = ra;
        sf_gemm(s, p, S);
    };
    if (s->bf16) nms_blocks_bf16(s, live, tiles64, tap);
    else for (int li = 0; li < m->L; ++li) {                       // the offline block's 15 launches + the ring put
        const mis_nemotron::Layer& l = m->fc[li];
        stats(s->h.p);
        ln_lin(s->h.p, l.ln1w, l.ln1b, l.ff1a, s->big.p, f, SF_ACT_SILU);
        res_lin(s->big.p, f, l.ff1b, s->h.p, d, 0.5f);
        stats(s->h.p);
        ln_lin(s->h.p, l.lnaw, l.lnab, l.qkv, s->qkv.p, 3 * d, SF_ACT_NONE);
        float* ring = st + s->o_ring + (size_t)li * s->R * 2 * d;
        MIS_LAUNCH(s, k_nm_ring_put, dim3(Tp, S), dim3(256), s->qkv.p, dp, S, ring, s->SS, s->R, Tp, d);
        NmAttnS ap{s->qkv.p, 3 * d, ring, s->SS, s->R, 2 * d, d, s->att.p, d, cn, cpos, Tp, m->hd, 1.0f, sqrtf((float)m->hd), l.u, l.v, l.P, d, -m->tab_lo,
                   s->ctx.C, s->ctx.L, s->ctx.dlo, s->ctx.dhi};
        nm_attn_stream(s, ap, m->H, S);
        res_lin(s->att.p, d, l.o, s->h.p, d, 1.0f);
        stats(s->h.p);
        ln_lin(s->h.p, l.lncw, l.lncb, l.pw1, s->big.p, 2 * d, SF_ACT_NONE);
        MIS_LAUNCH(s, k_nm_glu_dwconv_ln_stream, dim3(cdiv(Tp, NM_DW_TT), S), dim3(256), s->big.p, l.dw, l.dwb, cn, s->att.p, s->stats.p,
                   st + nms_hist(s, s->parity, li), st + nms_hist(s, s->parity ^ 1, li), s->SS, Tp, d, m->ck, 1e-5f);
        {
            SfGemm p = sf_lin(s->att.p, d, l.pw2, s->h.p, d, cn, Tp);
            p.load = NM_LOAD_LN_SILU; p.stats = s->stats.p; p.lnw = l.cnw; p.lnb = l.cnb; p.R = s->h.p; p.ldr = d; p.ra = 1.0f;
            nm_gemm(s, p, S);
        }
        stats(s->h.p);
        ln_lin(s->h.p, l.ln2w, l.ln2b, l.ff2a, s->big.p, f, SF_ACT_SILU);
        res_lin(s->big.p, f, l.ff2b, s->h.p, d, 0.5f);
        MIS_LAUNCH(s, k_sf_ln, dim3(cdiv(M, 4)), dim3(256), s->h.p, s->h.p, l.lnow, l.lnob, d, 1e-5f, M, cn, Tp);
        tap(li + 1, s->h.p, d, Tp, 0);
    }
    s->parity ^= 1;
    const float* x = s->h.p;
    if (m->PH) {
        SfGemm p = sf_lin(s->h.p, d + m->NP, m->pr0, s->big.p, m->PH, cn, Tp, SF_ACT_RELU);
        p.ldx = d; p.load = NM_LOAD_PROMPT; p.Tin = d; p.cnt_in = dp + NMS_LANG * S;
        nm_gemm(s, p, S);
        sf_gemm(s, sf_lin(s->big.p, m->PH, m->pr2, s->prm.p, d, cn, Tp), S);
        x = s->prm.p;
    }
    tap(m->L + 1, x, d, Tp, 0);
    sf_gemm(s, sf_lin(x, d, m->jenc, s->encp.p, m->J, cn, Tp), S);
    tap(m->L + 2, s->encp.p, m->J, Tp, 0);
    NmRnntS rp{m->rnnt, st + s->o_dec, s->SS, s->ist.p, cpos, dp + NMS_TOK0 * S};
    rp.r.encp = s->encp.p; rp.r.cnt = cn; rp.r.Tp = Tp; rp.r.tokens = s->dtok.p; rp.r.frames = s->dfrm.p;
    if (s->split) HIP_CHECK(hipEventRecord(s->ev[2], q));
    MIS_LAUNCH(s, k_nm_rnnt_stream, dim3(S), dim3(NM_NT), rp);
    if (s->split) { HIP_CHECK(hipEventRecord(s->ev[3], q)); s->split_timed = true; }
    MIS_LAUNCH(s, k_nm_mel_roll, dim3(NMS_MEL_CACHE, S), dim3(256), s->win.p, dp, S, st + s->o_mel, s->SS, s->Wp, m->mels);
    if (s->tapcap) { hipLaunchKernelGGL(k_nm_tap_advance, dim3(1), dim3(64), 0, q, dp, S, s->tapfill.p, 0); }
    return true;
}

extern "C" mis_status mis_nemotron_stream_feed(mis_nemotron_stream* s, const float* pcm, const int64_t* n, const int32_t* final, int64_t stride, int32_t* tokens,
                                               int32_t* frames, int64_t out_stride, int32_t* counts, int32_t* flags) {
    MIS_API_BEGIN
    MIS_REQUIRE(s && n && tokens && frames && counts && flags, MIS_ERR_INVALID_INPUT, "null argument");
    mis_nemotron* m = s->m;
    const int S = s->S, cap = m->cap, ms = m->cfg.max_symbols;
    int64_t wmax = 0;
    for (int b = 0; b < S; ++b) {                                   // judged first: nothing of the session is written
        const NmsStream& x = s->st[b];
        MIS_REQUIRE(n[b] >= 0 && n[b] <= stride && (n[b] == 0 || pcm), MIS_ERR_INVALID_INPUT, "stream %d: %lld samples outside 0..%lld (the row stride)", b,
                    (long long)n[b], (long long)stride);
        MIS_REQUIRE(!(x.fin && n[b] > 0), MIS_ERR_INVALID_INPUT, "stream %d is finished: reset it before it is fed again", b);
        MIS_REQUIRE(x.seen + n[b] < ((int64_t)1 << 30), MIS_ERR_INVALID_INPUT, "stream %d: more than 2^30 samples", b);
        const int64_t fb = nm_frames(x.seen + n[b]) / 8 + 2 - x.f.emitted, room = cap - x.ntok;
        wmax = std::max(wmax, ms > 0 ? std::min<int64_t>(room, fb * ms) : room);
    }
    MIS_REQUIRE(out_stride >= wmax, MIS_ERR_INVALID_INPUT, "out_stride %lld: this feed can emit up to %lld tokens a stream", (long long)out_stride, (long long)wmax);
    HIP_CHECK(hipSetDevice(m->device));
    for (int b = 0; b < S; ++b) {
        NmsStream& x = s->st[b];
        if (n[b]) x.tail.insert(x.tail.end(), pcm + (size_t)b * stride, pcm + (size_t)b * stride + n[b]);
        x.seen += n[b];
        if (final && final[b]) x.fin = true;
    }
    hipStream_t q = s->stream;
    s->launches = 0;
    s->split_timed = false;
    HIP_CHECK(hipEventRecord(s->ev[0], q));
    if (s->tapcap) hipLaunchKernelGGL(k_nm_tap_advance, dim3(1), dim3(64), 0, q, s->par.p, S, s->tapfill.p, 1);
    while (nms_pass(s)) {}
    for (int b = 0; b < S; ++b) if (s->st[b].fin && s->st[b].seen == 0) s->st[b].done = true;
    s->last_launches = s->launches;
    if (s->launches && wmax > 0) {
        HIP_CHECK(hipMemcpy2DAsync(tokens, out_stride * 4, s->dtok.p, (size_t)cap * 4, wmax * 4, S, hipMemcpyDeviceToHost, q));
        HIP_CHECK(hipMemcpy2DAsync(frames, out_stride * 4, s->dfrm.p, (size_t)cap * 4, wmax * 4, S, hipMemcpyDeviceToHost, q));
    }
    HIP_CHECK(hipMemcpyAsync(s->hist_.p, s->ist.p, (size_t)4 * S * 4, hipMemcpyDeviceToHost, q));
    HIP_CHECK(hipEventRecord(s->ev[1], q));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(q));                            // the feed's one synchronisation
    s->slot = 0;
    for (int b = 0; b < S; ++b) {
        NmsStream& x = s->st[b];
        counts[b] = s->hist_.p[4 * b + 1] - x.ntok;
        flags[b] = s->hist_.p[4 * b + 2];
        x.ntok = s->hist_.p[4 * b + 1];
    }
    MIS_API_END
}

// the frames the last feed brought, per stage as mis_nemotron_tap's.  Taps are kept from the first call on (out NULL, capacity = frames a
// stream may bring in one feed): that call allocates, a feed never does.
extern "C" mis_status mis_nemotron_stream_tap(mis_nemotron_stream* s, int stage, float* out, int64_t capacity, int64_t* dims, int32_t* counts) {
    MIS_API_BEGIN
    MIS_REQUIRE(s && dims, MIS_ERR_INVALID_INPUT, "null argument");
    mis_nemotron* m = s->m;
    MIS_REQUIRE(stage >= 0 && stage <= m->L + 2, MIS_ERR_INVALID_INPUT, "stage %d outside 0..%d", stage, m->L + 2);
    HIP_CHECK(hipSetDevice(m->device));
    const int wmax = std::max(m->d, m->J), width = stage <= m->L + 1 ? m->d : m->J;
    if (!s->tapcap) {
        MIS_REQUIRE(!out && capacity >= 1 && capacity <= (1 << 20), MIS_ERR_INVALID_INPUT, "the first tap call sets the frames kept a feed (out NULL, capacity 1..2^20)");
        s->tapbuf.alloc((size_t)(m->L + 3) * s->S * capacity * wmax);
        s->tapcap = (int)capacity;
        hipLaunchKernelGGL(k_nm_tap_advance, dim3(1), dim3(64), 0, s->stream, s->par.p, s->S, s->tapfill.p, 1);
        HIP_CHECK(hipStreamSynchronize(s->stream));
    }
    dims[0] = s->S; dims[1] = s->tapcap; dims[2] = width;
    if (!out) return MIS_OK;
    MIS_REQUIRE(capacity >= (int64_t)s->S * s->tapcap * width && counts, MIS_ERR_INVALID_INPUT, "output capacity too small");
    const float* src = s->tapbuf.p + (size_t)stage * s->S * s->tapcap * wmax;
    HIP_CHECK(hipMemcpyAsync(out, src, (size_t)s->S * s->tapcap * width * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipMemcpyAsync(counts, s->tapfill.p, (size_t)s->S * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
    for (int b = 0; b < s->S; ++b) MIS_REQUIRE(counts[b] <= s->tapcap, MIS_ERR_INVALID_INPUT, "stream %d brought %d frames: more than the %d kept", b, counts[b], s->tapcap);
    MIS_API_END
}

// ============================================================================ test and bench scaffolding (include/mi_speech_debug.h)
#include "debug_guard.h"
#include "../../include/mi_speech_debug.h"

// device milliseconds of the last feed, copies included
extern "C" mis_status mis_debug_nemotron_stream_timing(mis_nemotron_stream* s, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(s && ms, MIS_ERR_INVALID_INPUT, "null argument");
    HIP_CHECK(hipEventElapsedTime(ms, s->ev[0], s->ev[1]));
    MIS_API_END
}

// device milliseconds of k_nm_rnnt_stream in the last pass of the last feed; -1 when that feed ran no pass or ran before the first call
// here, which turns the two event records on
extern "C" mis_status mis_debug_nemotron_stream_decode_timing(mis_nemotron_stream* s, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(s && ms, MIS_ERR_INVALID_INPUT, "null argument");
    *ms = -1.0f;
    if (s->split_timed) HIP_CHECK(hipEventElapsedTime(ms, s->ev[2], s->ev[3]));
    s->split = true;
    MIS_API_END
}

namespace {
struct NmsdCtx { hipStream_t stream = nullptr; int launches = 0; };
}

// ONE launch of k_nm_attn_stream: q [streams][Tp][heads hd] (cnt[b] live rows at the absolute frames pos[b] ..), ring [streams][R][2 heads hd]
// (row key % R: k | v), the table as mis_debug_nemotron_attn's -> out [streams][Tp][heads hd].  R % 32 == 0 and R >= left + Tp + 32.
extern "C" mis_status mis_debug_nemotron_attn_stream(int device, const float* q, const float* ring, int R, const int32_t* cnt, const int32_t* pos, int streams,
                                                     int Tp, int heads, int hd, float qscale, float sdk, const float* u, const float* v, const float* P,
                                                     int ldp, int prow, int poff, int left, int right, float* out, int repeat, float* ms_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(q && ring && cnt && pos && u && v && P && out && streams >= 1 && streams <= 65535 && Tp >= 1 && heads >= 1 && heads <= 65535 && hd >= 65 &&
                    hd <= 128 && prow >= 1, MIS_ERR_INVALID_INPUT, "Nemotron stream attention: every pointer, positive sizes and a head size of 65..128 are required");
    MIS_REQUIRE(right >= 0 && right < (1 << 20) && left >= 0 && left % (right + 1) == 0, MIS_ERR_INVALID_INPUT,
                "Nemotron stream attention: right >= 0, left >= 0 and left %% (right + 1) == 0 are required");
    MIS_REQUIRE(R % 32 == 0 && R >= left + Tp + 32 && R <= (1 << 20), MIS_ERR_INVALID_INPUT, "Nemotron stream attention: R %d must be a multiple of 32 >= left + Tp + 32", R);
    const int C = right + 1, L = left / C, w = heads * hd;
    NmCtx x{C, L, -(C - 1), L * C + C - 1};
    MIS_REQUIRE(x.dlo + poff >= 0 && x.dhi + poff < prow && ldp >= w, MIS_ERR_INVALID_INPUT, "Nemotron stream attention: the table rows %d..%d do not cover the distances %d..%d",
                -poff, prow - 1 - poff, x.dlo, x.dhi);
    for (int b = 0; b < streams; ++b)
        MIS_REQUIRE(cnt[b] >= 0 && cnt[b] <= Tp && pos[b] >= 0 && pos[b] < (1 << 30), MIS_ERR_INVALID_INPUT, "Nemotron stream attention: stream %d count / position", b);
    HIP_CHECK(hipSetDevice(device));
    NmsdCtx c;
    const size_t rows = (size_t)streams * Tp, rs = (size_t)R * 2 * w;
    DevBuf<uint32_t> dq, dr, dc, dpos, du, dv, dP;
    alloc32(dq, q, rows * w, F32_NAN); alloc32(dr, ring, streams * rs, F32_NAN); alloc32(dc, cnt, streams, 0x7FFFFFFFu); alloc32(dpos, pos, streams, 0x7FFFFFFFu);
    alloc32(du, u, w, F32_NAN); alloc32(dv, v, w, F32_NAN); alloc32(dP, P, (size_t)prow * ldp, F32_NAN);
    GuardedOut o;
    o.alloc(rows * w * 4, (size_t)32 * w * 4);
    auto fp = [](const DevBuf<uint32_t>& d) { return reinterpret_cast<const float*>(d.p); };
    NmAttnS p{fp(dq), w, fp(dr), rs, R, 2 * w, w, reinterpret_cast<float*>(o.p()), w, reinterpret_cast<const int*>(dc.p), reinterpret_cast<const int*>(dpos.p), Tp, hd,
              qscale, sdk, fp(du), fp(dv), fp(dP), ldp, poff, x.C, x.L, x.dlo, x.dhi};
    nm_attn_stream(&c, p, heads, streams);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    MIS_REQUIRE(c.launches == 1, MIS_ERR_GENERATION_FAILED, "%d launches where one was meant", c.launches);
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
    if (repeat > 1 && ms_out) {
        HipEvents<2> ev;
        HIP_CHECK(hipEventRecord(ev[0], c.stream));
        for (int i = 0; i < repeat; ++i) nm_attn_stream(&c, p, heads, streams);
        HIP_CHECK(hipEventRecord(ev[1], c.stream));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipEventElapsedTime(ms_out, ev[0], ev[1]));
        *ms_out /= (float)repeat;
    }
    MIS_API_END
}

// ONE launch of k_nm_rnnt_stream: a pass of cnt[b] projected frames encp [streams][Tp][J] at the absolute frames pos[b] .., resumed from
// and stored back to state [streams][4 P + J] and ist [streams][4] (started, tokens, flag, steps; zeros: a fresh stream).  The pass's
// tokens / frames go to [streams][cap] at index (count - tok0[b]).
extern "C" mis_status mis_debug_nemotron_rnnt_stream(int device, const float* encp, const int32_t* cnt, const int32_t* pos, const int32_t* tok0, int streams, int Tp,
                                                     int J, int P, int vocab, int layers, int max_symbols, int cap, const float* embed, const float* const* wih,
                                                     const float* const* whh, const float* const* bih, const float* const* bhh, const float* wp, const float* bp,
                                                     const float* wo, const float* bo, float* state, int32_t* ist, int32_t* tokens, int32_t* frames) {
    MIS_API_BEGIN
    MIS_REQUIRE(encp && cnt && pos && tok0 && embed && wih && whh && bih && bhh && wp && bp && wo && bo && state && ist && tokens && frames, MIS_ERR_INVALID_INPUT,
                "Nemotron stream RNN-T: null argument");
    MIS_REQUIRE(streams >= 1 && streams <= 65535 && Tp >= 1 && cap >= 1 && (int64_t)streams * Tp * J <= ((int64_t)1 << 28), MIS_ERR_INVALID_INPUT,
                "Nemotron stream RNN-T: positive streams, Tp, cap are required");
    nm_check_decoder_dims(layers, P, J, vocab, max_symbols);
    for (int b = 0; b < streams; ++b)
        MIS_REQUIRE(cnt[b] >= 0 && cnt[b] <= Tp && tok0[b] >= 0 && tok0[b] <= ist[4 * b + 1] && ist[4 * b + 1] <= cap && pos[b] >= 0, MIS_ERR_INVALID_INPUT,
                    "Nemotron stream RNN-T: stream %d count / position / token counts", b);
    HIP_CHECK(hipSetDevice(device));
    NmsdCtx c;
    NmRnntS q{};
    DevBuf<float> arena;
    NmDecHost s{embed, {wih[0], layers > 1 ? wih[1] : nullptr}, {whh[0], layers > 1 ? whh[1] : nullptr}, {bih[0], layers > 1 ? bih[1] : nullptr},
                {bhh[0], layers > 1 ? bhh[1] : nullptr}, wp, bp, wo, bo};
    nm_pack_decoder(s, layers, P, J, vocab + 1, arena, q.r);
    const size_t ss = (size_t)4 * P + J, n = (size_t)streams * cap;
    DevBuf<uint32_t> de, dc, dpos, dt0, dst, dis;
    alloc32(de, encp, (size_t)streams * Tp * J, F32_NAN); alloc32(dc, cnt, streams, 0x7FFFFFFFu); alloc32(dpos, pos, streams, 0x7FFFFFFFu);
    alloc32(dt0, tok0, streams, 0x7FFFFFFFu); alloc32(dst, state, streams * ss, F32_NAN); alloc32(dis, ist, (size_t)4 * streams, 0x7FFFFFFFu);
    GuardedOut o;
    o.alloc(2 * n * 4, 4096);
    int* ob = reinterpret_cast<int*>(o.p());
    q.r.encp = reinterpret_cast<const float*>(de.p); q.r.cnt = reinterpret_cast<const int*>(dc.p); q.r.Tp = Tp; q.r.max_symbols = max_symbols; q.r.cap = cap;
    q.r.tokens = ob; q.r.frames = ob + n;
    q.dec = reinterpret_cast<float*>(dst.p); q.sstride = ss; q.ist = reinterpret_cast<int*>(dis.p);
    q.pos = reinterpret_cast<const int*>(dpos.p); q.tok0 = reinterpret_cast<const int*>(dt0.p);
    MIS_LAUNCH(&c, k_nm_rnnt_stream, dim3(streams), dim3(NM_NT), q);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    o.check_guards();
    HIP_CHECK(hipMemcpy(tokens, ob, n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(frames, ob + n, n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(state, dst.p, streams * ss * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(ist, dis.p, (size_t)4 * streams * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// ---------------------------------------------------------------------------- the bf16 session's kernels (nemotron_stream_bf16.h)
// ONE launch of k_nm_attn_stream_bf16: mis_debug_nemotron_attn_stream's arguments with bf16 q, ring and table, head sizes 1..128 -> out bf16
extern "C" mis_status mis_debug_nemotron_attn_stream_bf16(int device, const uint16_t* q, const uint16_t* ring, int R, const int32_t* cnt, const int32_t* pos,
                                                          int streams, int Tp, int heads, int hd, float qscale, float sdk, const float* u, const float* v,
                                                          const uint16_t* P, int ldp, int prow, int poff, int left, int right, uint16_t* out, int repeat,
                                                          float* ms_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(q && ring && cnt && pos && u && v && P && out && streams >= 1 && streams <= 65535 && Tp >= 1 && heads >= 1 && heads <= 65535 && hd >= 1 &&
                    hd <= 128 && prow >= 1, MIS_ERR_INVALID_INPUT, "Nemotron bf16 stream attention: every pointer, positive sizes and a head size of 1..128 are required");
    MIS_REQUIRE(right >= 0 && right < (1 << 20) && left >= 0 && left % (right + 1) == 0, MIS_ERR_INVALID_INPUT,
                "Nemotron bf16 stream attention: right >= 0, left >= 0 and left %% (right + 1) == 0 are required");
    MIS_REQUIRE(R % 32 == 0 && R >= left + Tp + 32 && R <= (1 << 20), MIS_ERR_INVALID_INPUT, "Nemotron bf16 stream attention: R %d must be a multiple of 32 >= left + Tp + 32", R);
    const int C = right + 1, L = left / C, w = heads * hd;
    NmCtx x{C, L, -(C - 1), L * C + C - 1};
    MIS_REQUIRE(x.dlo + poff >= 0 && x.dhi + poff < prow && ldp >= w, MIS_ERR_INVALID_INPUT,
                "Nemotron bf16 stream attention: the table rows %d..%d do not cover the distances %d..%d", -poff, prow - 1 - poff, x.dlo, x.dhi);
    for (int b = 0; b < streams; ++b)
        MIS_REQUIRE(cnt[b] >= 0 && cnt[b] <= Tp && pos[b] >= 0 && pos[b] < (1 << 30), MIS_ERR_INVALID_INPUT, "Nemotron bf16 stream attention: stream %d count / position", b);
    HIP_CHECK(hipSetDevice(device));
    NmsdCtx c;
    const size_t rows = (size_t)streams * Tp, rs = (size_t)R * 2 * w;
    DevBuf<uint16_t> dq, dr, dP;
    DevBuf<uint32_t> dc, dpos, du, dv;
    alloc16(dq, q, rows * w, BF16_NAN); alloc16(dr, ring, streams * rs, BF16_NAN); alloc16(dP, P, (size_t)prow * ldp, BF16_NAN);
    alloc32(dc, cnt, streams, 0x7FFFFFFFu); alloc32(dpos, pos, streams, 0x7FFFFFFFu); alloc32(du, u, w, F32_NAN); alloc32(dv, v, w, F32_NAN);
    GuardedOut o;
    o.alloc(rows * w * 2, (size_t)32 * w * 2);
    auto fp = [](const DevBuf<uint32_t>& d) { return reinterpret_cast<const float*>(d.p); };
    NmbAttnS p{dq.p, w, dr.p, rs, R, 2 * w, w, reinterpret_cast<bf16_t*>(o.p()), w, reinterpret_cast<const int*>(dc.p), reinterpret_cast<const int*>(dpos.p), Tp, hd,
               qscale, sdk, fp(du), fp(dv), dP.p, ldp, poff, x.C, x.L, x.dlo, x.dhi};
    nmb_attn_stream(&c, p, heads, hd, streams);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    MIS_REQUIRE(c.launches == 1, MIS_ERR_GENERATION_FAILED, "%d launches where one was meant", c.launches);
    o.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
    if (repeat > 1 && ms_out) {
        HipEvents<2> ev;
        HIP_CHECK(hipEventRecord(ev[0], c.stream));
        for (int i = 0; i < repeat; ++i) nmb_attn_stream(&c, p, heads, hd, streams);
        HIP_CHECK(hipEventRecord(ev[1], c.stream));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipEventElapsedTime(ms_out, ev[0], ev[1]));
        *ms_out /= (float)repeat;
    }
    MIS_API_END
}

// ONE launch of k_nm_glu_dwconv_ln_stream_bf16: mis_debug_nemotron_dwconv_ln_bf16's arguments at the causal pad (padl = k - 1 is required)
// with hist_in / hist_out bf16 [batch][k - 1][2 C], the pointwise_conv1 rows in front of the pass and behind it
extern "C" mis_status mis_debug_nemotron_dwconv_ln_stream_bf16(int device, const uint16_t* pw, const float* taps, const float* bias, const int32_t* cnt, int batch,
                                                               int Tp, int C, int k, int padl, const uint16_t* hist_in, uint16_t* hist_out, uint16_t* out,
                                                               float* stats) {
    MIS_API_BEGIN
    MIS_REQUIRE(pw && taps && cnt && out && stats && hist_in && hist_out && batch >= 1 && batch <= 65535 && Tp >= 1 && C >= 1 && k >= 2 && k <= SF_DW_MAXK &&
                    padl == k - 1 && (int64_t)batch * Tp * 2 * C <= ((int64_t)1 << 28), MIS_ERR_INVALID_INPUT,
                "Nemotron bf16 stream conv module: every pointer, positive batch, Tp, C, 2 <= k <= %d and padl = k - 1 are required", SF_DW_MAXK);
    for (int b = 0; b < batch; ++b) MIS_REQUIRE(cnt[b] >= 0 && cnt[b] <= Tp, MIS_ERR_INVALID_INPUT, "Nemotron bf16 stream conv module: count of row %d", b);
    HIP_CHECK(hipSetDevice(device));
    NmsdCtx c;
    const size_t rows = (size_t)batch * Tp, hs = (size_t)(k - 1) * 2 * C;
    DevBuf<uint16_t> dpw, dh;
    DevBuf<uint32_t> dt, db, dc;
    alloc16(dpw, pw, rows * 2 * C, BF16_NAN); alloc16(dh, hist_in, batch * hs, BF16_NAN);
    alloc32(dt, taps, (size_t)k * C, F32_NAN); alloc32(dc, cnt, batch, 0x7FFFFFFFu);
    if (bias) alloc32(db, bias, C, F32_NAN);
    GuardedOut o, st, ho;
    o.alloc(rows * C * 2, 4096); st.alloc(rows * 2 * 4, 4096); ho.alloc(batch * hs * 2, 4096);
    nmb_glu_dwconv_ln_stream(&c, dpw.p, reinterpret_cast<const float*>(dt.p), bias ? reinterpret_cast<const float*>(db.p) : nullptr,
                             reinterpret_cast<const int*>(dc.p), reinterpret_cast<bf16_t*>(o.p()), reinterpret_cast<float*>(st.p()), dh.p,
                             reinterpret_cast<bf16_t*>(ho.p()), hs, Tp, C, k, batch);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    MIS_REQUIRE(c.launches == 1, MIS_ERR_GENERATION_FAILED, "%d launches where one was meant", c.launches);
    o.check_guards(); st.check_guards(); ho.check_guards();
    HIP_CHECK(hipMemcpy(out, o.p(), o.body, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(stats, st.p(), st.body, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hist_out, ho.p(), ho.body, hipMemcpyDeviceToHost));
    MIS_API_END
}
