// deepfilternet_kernels.h - the DeepFilterNet kernels and the model handle, shared by the offline engine (deepfilternet.hip) and the
// hop-by-hop streamer (deepfilternet_stream.hip).  Every kernel is a template on S: S = false is the offline form, a row's frames from
// row 0 of its block and zeros behind them; S = true is the stream form, where a block of a buffer is `hist` rows of carried history
// followed by the rows of this feed, nothing is written behind a stream's own rows, and
//   - a frame index below the feed's first row reads the history (below absolute frame 0: zero, as offline),
//   - the look-ahead shift is the per-stream row offset off[b] (the frames have already arrived: nothing is zero-filled),
//   - the normalisation and the recurrence start from the carried state.
// The arithmetic of an output element is the same expression in the same order in both forms, which is what makes a stream bit-equal
// to the offline call.
#pragma once
#include "common.h"
#include "f32_tile.h"
#include "host_weights.h"
#include "step_loop.h"

#include <math.h>
#include <string.h>
#include <memory>

#define DF_MAX_BATCH 64
#define DF_MAX_ERB 128
#define DF_MAX_REC 16             // recurrence launches a call that get their own pair of events

enum { DF_LOAD_LIN = 0, DF_LOAD_FRAME, DF_LOAD_MAGSQ, DF_LOAD_IM2COL, DF_LOAD_GCONV, DF_LOAD_GCONVT };
enum { DF_ACT_NONE = 0, DF_ACT_RELU, DF_ACT_SIGMOID, DF_ACT_TANH, DF_ACT_LOG10, DF_ACT_LSNR };
enum { DF_PH_FRONT = 0, DF_PH_NET, DF_PH_REC, DF_PH_SYNTH };

__device__ __forceinline__ float df_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---------------------------------------------------------------------------- the contraction
struct DfGemm {
    const int32_t* cnt; int nr, Fo, load;                   // a row's frames; positions a frame (m = t Fo + fo); the operand load
    const float* W; int K, N, gws, ghs;                     // [N][gws]: row co holds the gws inputs of its group co / ghs (dense: gws = K)
    const float* X; int ldx;                                // LIN / MAGSQ: [frame][ldx]; convs: [frame][Fin][Cin]
    int Fin, Cin, kT, kF, fs, tshift;                       // conv geometry; tshift: the look-ahead (applied when T > tshift)
    const float* Wm; int ipg, opg;                          // GCONV [K][ipg][kT][kF], GCONVT [Cin][opg][1][kF] (torch layouts)
    const float* pcm; int64_t pcm_stride; const int32_t* lens; int hop; const float* win;   // FRAME
    const float *scale, *bias; int act; float mul, s0, s1;  // epilogue: acc mul scale[co] + bias[co], activation (LSNR: sigmoid s0 + s1)
    const float* cscale; const float* R; int ldr;           // column scale, residual (after the activation)
    float* Y; int ldy;
    // stream form: rows of history in front of a block; the absolute index of a stream's first row (rows below -t0[b] are frames below
    // 0); the feature row its first target reads
    int hist; const int32_t *t0, *off;
};

// what a block knows of its row: where its rows start, how many it has, and (stream form) the lowest row that is a frame, the shift
struct DfRow { size_t row0; int T, tlo, off; };

template <bool S>
__device__ __forceinline__ float df_conv_in(const DfGemm& p, const DfRow& r, int t, int f, int ci) {
    if constexpr (S) {
        if (f < 0 || f >= p.Fin || t < r.tlo) return 0.0f;                // the conv's own zero padding: frames below 0
        if (p.tshift) t += r.off;                                         // the shifted frame has arrived: a row of this feed or of the history
        return p.X[((r.row0 + t) * p.Fin + f) * p.Cin + ci];
    } else {
        if (t < 0 || f < 0 || f >= p.Fin) return 0.0f;                    // the conv's own zero padding
        if (r.T > p.tshift) t += p.tshift;                                // applyLookahead: zero-filled from the row's own last frame
        if (t >= r.T) return 0.0f;
        return p.X[((r.row0 + t) * p.Fin + f) * p.Cin + ci];
    }
}

template <bool S>
__device__ __forceinline__ float df_load(const DfGemm& p, int b, const DfRow& r, int m, int k) {
    const int t = m / p.Fo, fo = m - t * p.Fo;
    const size_t row0 = r.row0;
    switch (p.load) {
        case DF_LOAD_FRAME: {                                             // hop zeros in front of the row, zeros behind it
            const int64_t s = (int64_t)t * p.hop + k - p.hop;
            if constexpr (S)                                              // pcm points behind the carried fft - hop samples
                return s < (int64_t)r.T * p.hop ? __fmul_rn(p.pcm[(int64_t)b * p.pcm_stride + s], p.win[k]) : 0.0f;
            else
                return (s >= 0 && s < p.lens[b]) ? __fmul_rn(p.pcm[(size_t)b * p.pcm_stride + s], p.win[k]) : 0.0f;
        }
        case DF_LOAD_MAGSQ: {
            const float re = p.X[(row0 + t) * p.ldx + k], im = p.X[(row0 + t) * p.ldx + p.K + k];
            return __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
        }
        case DF_LOAD_IM2COL: {                                            // k = (dt kF + df) Cin + ci
            const int tap = k / p.Cin, ci = k - tap * p.Cin, dt = tap / p.kF, df = tap - dt * p.kF;
            return df_conv_in<S>(p, r, t - (p.kT - 1) + dt, fo * p.fs - p.kF / 2 + df, ci);
        }
        case DF_LOAD_GCONV: {                                             // mid channel k of the grouped conv, taps (ci, dt, df) ascending
            const int g = k / p.opg;
            const float* w = p.Wm + (size_t)k * p.ipg * p.kT * p.kF;
            float a = 0.0f;
            for (int ci = 0; ci < p.ipg; ++ci)
                for (int dt = 0; dt < p.kT; ++dt)
                    for (int df = 0; df < p.kF; ++df)
                        a = fmaf(df_conv_in<S>(p, r, t - (p.kT - 1) + dt, fo * p.fs - p.kF / 2 + df, g * p.ipg + ci),
                                 w[(ci * p.kT + dt) * p.kF + df], a);
            return a;
        }
        case DF_LOAD_GCONVT: {                                            // y[fo] = sum over fi fs - kF / 2 + j == fo of x[fi] w[j], j ascending
            const int g = k / p.opg;
            const float* w = p.Wm + (size_t)k * p.kF;
            float a = 0.0f;
            for (int j = 0; j < p.kF; ++j) {
                const int q = fo + p.kF / 2 - j;
                if (q >= 0 && q % p.fs == 0) a = fmaf(df_conv_in<S>(p, r, t, q / p.fs, g), w[j], a);
            }
            return a;
        }
        default: return p.X[(row0 + t) * p.ldx + k];
    }
}

template <bool S>
__global__ void __launch_bounds__(256) k_dfn_gemm(DfGemm p) {
    constexpr int TT = F32_TILE, TC = F32_TILE;
    __shared__ float As[TT][F32_KC + 1];
    __shared__ float Bs[TC][F32_KC + 1];
    const int b = blockIdx.z, m0 = blockIdx.x * TT, c0 = blockIdx.y * TC, nr = p.nr;
    const int T = S ? p.cnt[b] : min(p.cnt[b], nr), M = T * p.Fo, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t row0 = (size_t)b * nr + (S ? p.hist : 0);
    const DfRow rw{row0, T, S ? -p.t0[b] : 0, S ? p.off[b] : 0};
    if (m0 >= M) {
        if constexpr (!S) f32_tile_zero<TT, TC>(p.Y, p.ldy, row0 * p.Fo, m0, c0, nr * p.Fo, p.N);
        return;
    }
    f32x16_t acc[1] = {};
    const int wt = (wave & 1) * 32, wc = (wave >> 1) * 32, kh = lane >> 5, l31 = lane & 31;
    // a grouped linear reads the K range of the groups its 64 columns belong to
    const int klo = (c0 / p.ghs) * p.gws, khi = min(p.K, (min(p.N - 1, c0 + TC - 1) / p.ghs + 1) * p.gws);
    for (int k0 = klo; k0 < khi; k0 += F32_KC) {
#pragma unroll
        for (int n = 0; n < TT * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, k = k0 + (i & 31), m = m0 + r;
            As[r][i & 31] = (k < khi && m < M) ? df_load<S>(p, b, rw, m, k) : 0.0f;
        }
#pragma unroll
        for (int n = 0; n < TC * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, k = k0 + (i & 31), co = c0 + r;
            float v = 0.0f;
            if (co < p.N && k < khi) {
                const int kg = k - (co / p.ghs) * p.gws;
                if (kg >= 0 && kg < p.gws) v = p.W[(size_t)co * p.gws + kg];
            }
            Bs[r][i & 31] = v;
        }
        __syncthreads();
        f32_tile_mfma(As, Bs, wt + l31, wc + l31, kh, acc);
        __syncthreads();
    }
    const int co = c0 + wc + l31;                                   // C/D: column = lane & 31, row = f32_tile_row(r, lane >> 5)
    if (co >= p.N) return;
    const float sc = p.scale ? p.scale[co] : 1.0f, add = p.bias ? p.bias[co] : 0.0f, cs = p.cscale ? p.cscale[co] : 1.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wt + f32_tile_row(r, kh);
        if (m >= (S ? M : nr * p.Fo)) continue;                          // stream form: nothing behind a stream's own rows
        const size_t at = row0 * p.Fo + m;
        float v = 0.0f;
        if (m < M) {
            v = __fadd_rn(__fmul_rn(__fmul_rn(acc[0][r], p.mul), sc), add);
            if (p.act == DF_ACT_RELU) v = fmaxf(v, 0.0f);
            else if (p.act == DF_ACT_SIGMOID) v = df_sigmoid(v);
            else if (p.act == DF_ACT_TANH) v = tanhf(v);
            else if (p.act == DF_ACT_LOG10) v = __fmul_rn(10.0f, log10f(__fadd_rn(v, 1e-10f)));
            else if (p.act == DF_ACT_LSNR) v = __fadd_rn(__fmul_rn(df_sigmoid(v), p.s0), p.s1);
            if (p.cscale) v = __fmul_rn(v, cs);
            if (p.R) v = __fadd_rn(v, p.R[at * p.ldr + co]);
        }
        p.Y[at * p.ldy + co] = v;
    }
}

// ---------------------------------------------------------------------------- features
struct DfNorm {
    const float* spec; int F;                               // [frame][2 F], re | im
    const float* erb;                                       // [frame][E] in dB (erb_fb), or null: band means over widths
    const int32_t* wlo;                                     // [E + 1] first bin of every band
    float *feat_erb, *feat_spec;                            // [frame][E], [frame][D][2]
    const int32_t* cnt; int nr, E, D; float a;
    int hist; float* state; const int32_t* seen;            // stream form: s of every band / bin [stream][E + D]; hops before this feed
};

__device__ __forceinline__ float df_magsq(const float* s, int F, int f) { return __fadd_rn(__fmul_rn(s[f], s[f]), __fmul_rn(s[F + f], s[F + f])); }

template <bool S>
__global__ void __launch_bounds__(256) k_dfn_norm(DfNorm p) {
    const int b = blockIdx.x, T = S ? p.cnt[b] : min(p.cnt[b], p.nr);
    const size_t row0 = (size_t)b * p.nr + (S ? p.hist : 0);
    const float a = p.a, oma = __fsub_rn(1.0f, p.a);
    if (S && T == 0) return;
    for (int item = threadIdx.x; item < p.E + p.D; item += 256) {
        const bool erb = item < p.E;
        const int i = erb ? item : item - p.E, n = erb ? p.E : p.D;
        // linspace(start, end, n): start + i (end - start) / (n - 1)
        const float lo = erb ? -60.0f : 0.001f, hi = erb ? -90.0f : 0.0001f;
        float s = n > 1 ? __fadd_rn(lo, __fmul_rn((float)i, __fdiv_rn(__fsub_rn(hi, lo), (float)(n - 1)))) : lo;
        if constexpr (S) { if (p.seen[b] > 0) s = p.state[(size_t)b * (p.E + p.D) + item]; }
        for (int t0 = 0; t0 < T; t0 += 8) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {                                 // the loads of eight frames, then their serial chain
                const int t = t0 + j;
                x[j] = 0.0f;
                if (t >= T) continue;
                const float* sp = p.spec + (row0 + t) * 2 * p.F;
                if (!erb) x[j] = __fsqrt_rn(df_magsq(sp, p.F, i));
                else if (p.erb) x[j] = p.erb[(row0 + t) * p.E + i];
                else {
                    float acc = 0.0f;
                    for (int f = p.wlo[i]; f < p.wlo[i + 1]; ++f) acc = __fadd_rn(acc, df_magsq(sp, p.F, f));
                    const int w = p.wlo[i + 1] - p.wlo[i];
                    x[j] = __fmul_rn(10.0f, log10f(__fadd_rn(w > 0 ? __fdiv_rn(acc, (float)w) : 0.0f, 1e-10f)));
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int t = t0 + j;
                if (t >= T) continue;
                s = __fadd_rn(__fmul_rn(x[j], oma), __fmul_rn(s, a));
                if (erb) p.feat_erb[(row0 + t) * p.E + i] = __fdiv_rn(__fsub_rn(x[j], s), 40.0f);
                else {
                    const float* sp = p.spec + (row0 + t) * 2 * p.F;
                    const float den = __fsqrt_rn(fmaxf(s, 1e-12f));
                    p.feat_spec[((row0 + t) * p.D + i) * 2] = __fdiv_rn(sp[i], den);
                    p.feat_spec[((row0 + t) * p.D + i) * 2 + 1] = __fdiv_rn(sp[p.F + i], den);
                }
            }
        }
        if constexpr (S) p.state[(size_t)b * (p.E + p.D) + item] = s;
        else
            for (int t = T; t < p.nr; ++t) {
                if (erb) p.feat_erb[(row0 + t) * p.E + i] = 0.0f;
                else { p.feat_spec[((row0 + t) * p.D + i) * 2] = 0.0f; p.feat_spec[((row0 + t) * p.D + i) * 2 + 1] = 0.0f; }
            }
    }
}

// ---------------------------------------------------------------------------- the recurrence
struct DfGruChain {
    const float* gx;                                        // [frame][3 H]: Wx x + b_ih, gates r | z | n
    const float* Wh;                                        // [3 H][H]: thread t's register slice is the head of row t
    const float* WhT;                                       // [H][3 H]: the streamed remainder, column k at WhT + k 3 H
    const float* bhh;                                       // [3 H]
    float* out;                                             // [frame][H]
};
struct DfGru { DfGruChain ch[2]; const int32_t* cnt; int nr; int hist; };

// KR = 0 is the short-chunk form: no register slice to fill, every column of Wh streamed from the transposed copy with 32 loads in
// flight (the registers the slice would take).  The accumulation is the same ascending-column chain for every KR.
template <int H, int KR, bool S>
__global__ void __launch_bounds__(3 * H) k_dfn_gru(DfGru p) {
    static_assert(KR % 4 == 0 && KR <= H && H % 4 == 0, "KR and H are multiples of 4");
    __shared__ __attribute__((aligned(16))) float hs[H];
    __shared__ float gs[3 * H];
    const int b = blockIdx.x, t = threadIdx.x, T = S ? p.cnt[b] : min(p.cnt[b], p.nr);
    if (S && T == 0) return;                                              // block-uniform
    const DfGruChain c = p.ch[blockIdx.y];
    const size_t row0 = (size_t)b * p.nr + (S ? p.hist : 0);
    float w[KR > 0 ? KR : 4];
    if constexpr (KR > 0) {
        const float4* src = reinterpret_cast<const float4*>(c.Wh + (size_t)t * H);
#pragma unroll
        for (int q = 0; q < KR / 4; ++q) { const float4 v = src[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
    }
    const float* wt = c.WhT + t;
    const float bh = c.bhh[t];
    float h = 0.0f;
    if constexpr (S) { if (t < H) h = c.out[(row0 - 1) * H + t]; }         // the carried state: the last row of the feed before
    if (t < H) hs[t] = h;
    __syncthreads();
    const float4* h4 = reinterpret_cast<const float4*>(hs);
    for (int s = 0; s < T; ++s) {                                         // T is the row's own count: every barrier is block-uniform
        float xr = 0.0f, xz = 0.0f, xn = 0.0f;
        if (t < H) { const float* g = c.gx + (row0 + s) * 3 * H + t; xr = g[0]; xz = g[H]; xn = g[2 * H]; }
        float a = 0.0f;                                                   // columns ascending: registers first, then the streamed part
        if constexpr (KR > 0) {
#pragma unroll
            for (int q = 0; q < KR / 4; ++q) {
                const float4 v = h4[q];
                a = fmaf(w[4 * q], v.x, a); a = fmaf(w[4 * q + 1], v.y, a); a = fmaf(w[4 * q + 2], v.z, a); a = fmaf(w[4 * q + 3], v.w, a);
            }
        }
        if constexpr (KR < H) {
            constexpr int SC = KR == 0 ? 32 : KR > 96 ? 4 : 8;             // loads in flight: what the registers beside w[] leave room for
#pragma unroll 1
            for (int k = KR; k < H; k += SC) {
                float u[SC];
#pragma unroll
                for (int j = 0; j < SC; ++j) u[j] = wt[(size_t)(k + j) * 3 * H];
#pragma unroll
                for (int j = 0; j < SC; j += 4) {
                    const float4 v = h4[(k + j) / 4];
                    a = fmaf(u[j], v.x, a); a = fmaf(u[j + 1], v.y, a); a = fmaf(u[j + 2], v.z, a); a = fmaf(u[j + 3], v.w, a);
                }
            }
        }
        gs[t] = __fadd_rn(a, bh);
        __syncthreads();
        if (t < H) {
            const float r = df_sigmoid(__fadd_rn(xr, gs[t])), z = df_sigmoid(__fadd_rn(xz, gs[H + t]));
            const float n = tanhf(__fadd_rn(xn, __fmul_rn(r, gs[2 * H + t])));
            h = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, z), n), __fmul_rn(z, h));
            hs[t] = h;
            c.out[(row0 + s) * H + t] = h;
        }
        __syncthreads();
    }
    if constexpr (!S)
        for (int i = T * H + t; i < p.nr * H; i += 3 * H) c.out[row0 * H + i] = 0.0f;
}

// ---------------------------------------------------------------------------- synthesis
struct DfEnh {
    const float *spec, *mask, *coef, *inv;                  // [frame][2 F], [frame][E], [frame][D][order][2], erb_inv_fb [E][F]
    float* enh;                                             // [frame][2 F]
    const int32_t* cnt; int nr, F, E, D, order, pad_left; float wnorm; size_t total;
    // stream form: rows of the launch a stream (the feed's longest), history rows, the look-ahead; spec is indexed by frame, the rest
    // by target: target row j is spec row j + off[b] - la
    int nrc, hist, la; const int32_t *t0, *off;
};

template <bool S>
__global__ void __launch_bounds__(256) k_dfn_enh(DfEnh p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.total) return;
    const int f = (int)(i % p.F);
    const size_t ri = i / p.F;
    const int nrc = S ? p.nrc : p.nr;
    const int t = (int)(ri % nrc), b = (int)(ri / nrc), T = S ? p.cnt[b] : min(p.cnt[b], p.nr);
    if (S && t >= T) return;
    const size_t row = S ? (size_t)b * p.nr + p.hist + t : ri;
    const int tlo = S ? -p.t0[b] : 0;
    const ptrdiff_t srow = S ? (ptrdiff_t)row + p.off[b] - p.la : (ptrdiff_t)row;      // the spec row of frame t
    float re = 0.0f, im = 0.0f;
    if (t < T) {
        if (f >= p.D) {
            float g = 0.0f;
            for (int e = 0; e < p.E; ++e) g = fmaf(p.mask[row * p.E + e], p.inv[(size_t)e * p.F + f], g);
            re = __fmul_rn(p.spec[srow * 2 * p.F + f], g); im = __fmul_rn(p.spec[srow * 2 * p.F + p.F + f], g);
        } else {
            const float* cf = p.coef + (row * p.D + f) * p.order * 2;
            for (int k = 0; k < p.order; ++k) {
                const int tt = t + k - p.pad_left;
                if (tt < tlo || (!S && tt >= T)) continue;                // (adds of + 0 in the reference); stream form: the frame has arrived
                const float* sp = p.spec + (srow - t + tt) * 2 * p.F;
                const float sr = sp[f], si = sp[p.F + f], cr = cf[2 * k], ci = cf[2 * k + 1];
                re = __fadd_rn(re, __fsub_rn(__fmul_rn(sr, cr), __fmul_rn(si, ci)));
                im = __fadd_rn(im, __fadd_rn(__fmul_rn(sr, ci), __fmul_rn(si, cr)));
            }
        }
        re = __fdiv_rn(re, p.wnorm); im = __fdiv_rn(im, p.wnorm);
    }
    p.enh[row * 2 * p.F + f] = re; p.enh[row * 2 * p.F + p.F + f] = im;
}

// the overlap-add of padded sample q over the frames fa..fb that cover it, in frame order, / max(sum w^2, 1e-8), clipped; frame f is
// row f + fo of fr
__device__ __forceinline__ float df_ola_at(const float* __restrict__ fr, int fo, const float* __restrict__ win, int64_t q, int fa, int fb, int W,
                                           int hop) {
    float acc = 0.0f, ws = 0.0f;
    for (int f = fa; f <= fb; ++f) {
        const int j = (int)(q - (int64_t)f * hop);
        acc = __fadd_rn(acc, fr[(size_t)(f + fo) * W + j]);
        ws = __fadd_rn(ws, __fmul_rn(win[j], win[j]));
    }
    return fminf(fmaxf(__fdiv_rn(acc, fmaxf(ws, 1e-8f)), -1.0f), 1.0f);
}

// ============================================================================ host
struct DfBuf { float* p = nullptr; int F = 1, C = 0; size_t off = 0; };       // [B Tcap][F][C] at work + off
struct DfOp {
    int kind = 0, phase = DF_PH_NET;                                          // 0 gemm, 1 norm, 2 gru, 3 enh, 4 ola
    DfGemm g{}; DfNorm n{}; DfGru r{}; DfEnh e{};
    int H = 0, chains = 1;                                                    // recurrence: hidden size, chains of the launch
    int in = -1, res = -1, out = -1;                                          // buffers, resolved once the workspace exists
    int rgx[2] = {-1, -1}, rout[2] = {-1, -1};                                // recurrence: gx and out of its chains
};
struct DfTap { int stage; int buf; };

struct mis_deepfilternet {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_deepfilternet_config cfg{};
    int F = 0, E = 0, D = 0, N = 0, hop = 0, Tcap = 0, KR = 0;
    float wnorm = 0.0f;
    HostWeights raw{"DeepFilterNet", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<float> farena, work, pcm;
    DevBuf<int32_t> counts, iarena;                          // counts: T[64] | lens[64]
    std::vector<int32_t> h_counts;
    std::vector<DfOp> ops;
    std::vector<DfBuf> bufs;
    std::vector<DfTap> taps;
    const float *win = nullptr, *idft = nullptr;
    const int32_t* wlo = nullptr;
    int b_wave = -1, b_fr = -1, b_lsnr = -1;
    int b_spec = -1, b_ferb = -1, b_fspec = -1, b_enh = -1;  // what the streamer binds by name
    int last_batch = 0, last_nr = 0, last_launches = 0;
    int64_t last_out = 0;
    HipEvents<4 + 2 * DF_MAX_REC> ev;
    float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
};
