// sortformer_kernels.h - the NeMo FastConformer kernels and their launchers, shared by sortformer.hip and parakeet.hip: the stem's first
// conv, the one contraction with its operand loads, the frame statistics, LayerNorm, the intake, flash attention for head sizes up to 64
// (with and without relative positions) and the GLU + depthwise conv.  Each including file gets its own copy (the anonymous namespace):
// a file's kernels live in that file's code object, so neither engine's bits depend on how the other is compiled.
// Include common.h and f32_tile.h first.
#pragma once

#define SF_DW_TT 64
#define SF_DW_MAXK 31

namespace {

enum { SF_LOAD_ACT = 0, SF_LOAD_LN, SF_LOAD_RELU, SF_LOAD_DW };
enum { SF_ACT_NONE = 0, SF_ACT_SILU, SF_ACT_RELU, SF_ACT_SIGMOID };
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

// ============================================================================ launchers
struct SfLin { const float *w = nullptr, *b = nullptr; };
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

template <bool REL, class Ctx>
static void sf_attn(Ctx* c, const SfAttn& p, int heads, int hd, int batch) {
    const dim3 grid(cdiv(p.Tp, 64), heads, batch);
    if (hd <= 32) MIS_LAUNCH(c, (k_sf_attn<1, REL>), grid, dim3(128), p);
    else MIS_LAUNCH(c, (k_sf_attn<2, REL>), grid, dim3(128), p);
}

}  // namespace
