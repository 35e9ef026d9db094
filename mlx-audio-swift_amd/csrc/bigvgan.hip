// bigvgan.hip - the BigVGAN vocoder: mel [B][num_mels][T] -> waveform [B][T hop].
//
// Reference being replaced: BigVGAN (Sources/MLXAudioCodecs/BigVGAN/BigVGAN.swift:92-218), BigVGANAMPBlock1 / 2 (:5-90) and the layers of
// BigVGANLayers.swift: the Kaiser-sinc filter (:47-81), the periodic activation (:83-111), the weight-normalised convs (:113-225) and the
// anti-aliased Activation1d = DownSample1d(act(UpSample1d(x))) (:227-352).
//
// Activations are f32 NCT, time contiguous; every tensor of a call has the row stride (the call's stride) x (the up-sampling so far).
// One call serves 1..max_batch ragged rows: row b has frames[b] mel frames, T = frames[b] x mult samples at a stage, and every kernel
// takes the counts, reads nothing beyond a row's own T and writes zeros behind it.  Every output element is one fixed-order sum that
// depends on the row alone, so a row's waveform is the same bit for bit whatever batch or padding it travels in.
//
//   k_bv_aa_act   the fused anti-aliased activation, one read and one write of the tensor.  A block takes 4 channels x 128 columns: the x
//                 tile + 5 columns of halo each side in LDS, then v = snake(2 x up-sampled x) for the tile's 2 x 128 + 10 positions in
//                 LDS, then y.  u[n] = 2 sum_i f[n + 15 - 2 i] x[clamp(i - 5, 0, T - 1)] (six taps, i ascending), v = u + sin^2(alpha u) /
//                 (beta + 1e-9), y[t] = sum_j f[j] v[clamp(2 t + j - 5, 0, 2 T - 1)] (j ascending).  THE TWO CLAMPS: the down-sampler
//                 replicates v[0] / v[2 T - 1]; it never reads a u formed beyond the row from replicated x.
//   k_bv_conv     the one contraction, exact f32 on v_mfma_f32_32x32x2_f32 (f32_tile.h): a 64 (channel) x 64 (time) tile, K = taps x Cin
//                 staged F32_KC at a time in ascending order, k = j Cin + ci; the tap shift is applied in the operand load (zeros beyond
//                 the row's own ends); every dimension guarded.  Dense "same" conv of 1..11 taps, dilation 1..5 (conv_pre, the AMP
//                 blocks), epilogue bias then + R; and the transposed conv of kernel 2 s, stride s, pad s / 2 as s two-tap convs, one a
//                 phase: output s n + ph takes tap (ph + pad) % s + s j from x[n + (ph + pad) / s - j].
//   k_bv_mean     (b_0 + b_1 + ... in block order) / num_kernels
//   k_bv_final    conv_post (C -> 1, 7 taps, optional bias), then tanh or clip(-1, 1)
//
// Weight norm is folded at finalize in double: g v / (|v| + 1e-12), per output channel for a conv and per input channel for a transposed
// conv (exceptDim 2 of the [out, k, in] layout); 1 / (beta + 1e-9) is folded too.  No allocation and one synchronisation per call.
#include "common.h"
#include "codec_kernels.h"
#include "debug_guard.h"
#include "f32_tile.h"
#include "host_weights.h"
#include "step_loop.h"

#include <math.h>
#include <string.h>
#include <memory>

#define BV_MAX_BATCH 64
#define BV_MAX_STAGES 8
#define BV_MAX_KERNELS 8
#define BV_MAX_DIL 8
#define BV_FT 12                  // taps of the Kaiser-sinc filter (ratio 2, kernel size 12: fixed by the reference)
#define BV_AT 128                 // columns of an activation tile
#define BV_AC 4                   // channels of an activation tile

struct BvAct {
    const float* X; float* Y;                               // [B][C][ld]
    const float *alpha, *rbeta, *filt;                      // [C], [C] = 1 / (beta + 1e-9), [12]
    const int32_t* frames; int mult, C, ld;
};

__global__ void __launch_bounds__(256) k_bv_aa_act(BvAct p) {
    constexpr int XW = BV_AT + 10, VW = 2 * BV_AT + 10;
    __shared__ float xs[BV_AC][XW], vs[BV_AC][VW], fs[BV_FT];
    const int b = blockIdx.z, c0 = blockIdx.y * BV_AC, t0 = blockIdx.x * BV_AT, tid = threadIdx.x;
    const int T = p.frames[b] * p.mult;
    if (t0 >= T) {                                                    // nothing of the row here: zeros
        for (int i = tid; i < BV_AC * BV_AT; i += 256) {
            const int c = c0 + i / BV_AT, t = t0 + i % BV_AT;
            if (c < p.C && t < p.ld) p.Y[((size_t)b * p.C + c) * p.ld + t] = 0.0f;
        }
        return;
    }
    if (tid < BV_FT) fs[tid] = p.filt[tid];
    for (int i = tid; i < BV_AC * XW; i += 256) {
        const int cc = i / XW, h = i - cc * XW, c = c0 + cc;
        const int xi = min(max(t0 - 5 + h, 0), T - 1);
        xs[cc][h] = c < p.C ? p.X[((size_t)b * p.C + c) * p.ld + xi] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < BV_AC * VW; i += 256) {
        const int cc = i / VW, m = i - cc * VW, c = min(c0 + cc, p.C - 1);
        const int n = min(max(2 * t0 - 5 + m, 0), 2 * T - 1);         // the down-sampler's clamp: v itself is replicated
        const int i_lo = (n + 5) >> 1;
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < 6; ++q) {                                 // i = i_lo + q ascending, tap n + 15 - 2 i
            const int xi = min(max(i_lo + q - 5, 0), T - 1);          // the up-sampler's clamp
            acc = fmaf(fs[n + 15 - 2 * (i_lo + q)], xs[cc][xi - (t0 - 5)], acc);
        }
        const float u = 2.0f * acc;
        vs[cc][m] = fmaf(p.rbeta[c], mis_sin_sq(p.alpha[c] * u), u);
    }
    __syncthreads();
    for (int i = tid; i < BV_AC * BV_AT; i += 256) {
        const int cc = i / BV_AT, tl = i - cc * BV_AT, c = c0 + cc, t = t0 + tl;
        if (c >= p.C || t >= p.ld) continue;
        float acc = 0.0f;
        if (t < T) {
#pragma unroll
            for (int j = 0; j < BV_FT; ++j) acc = fmaf(fs[j], vs[cc][2 * tl + j], acc);
        }
        p.Y[((size_t)b * p.C + c) * p.ld + t] = acc;
    }
}

// tile position n reads x[n + shift0 + j step] for tap j and writes y[n os + ph]: a "same" conv has shift0 = -((taps - 1) / 2) dil,
// step = dil, os = 1; phase ph = blockIdx.z % os of a transposed conv has two taps, shift0 = (ph + pad) / os, step = -1.
struct BvConvP {
    const float* X; int ldx;                                // [B][Cin][ldx]
    const float* W; const float* bias;                      // [os][Cout][taps Cin], k = j Cin + ci; bias [Cout] or null
    const float* R; float* Y; int ldy;                      // [B][Cout][ldy]; R (same layout) or null
    const int32_t* frames; int mult;                        // the row has frames[b] x mult tile positions
    int Cin, Cout, taps, dil, os, pad, npos;                // npos: tile positions of the row stride
};

__global__ void __launch_bounds__(256) k_bv_conv(BvConvP p) {
    __shared__ float As[F32_TILE][F32_KC + 1];              // weights: rows are output channels
    __shared__ float Bs[F32_TILE][F32_KC + 1];              // activations: rows are tile positions
    const int ph = blockIdx.z % p.os, b = blockIdx.z / p.os, t0 = blockIdx.x * F32_TILE, c0 = blockIdx.y * F32_TILE;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kh = lane >> 5, l31 = lane & 31;
    const int wt = (wave & 1) * 32, wc = (wave >> 1) * 32;
    const int T = p.frames[b] * p.mult, K = p.taps * p.Cin;
    float* Yb = p.Y + (size_t)b * p.Cout * p.ldy;
    if (t0 >= T) {
        for (int i = tid; i < F32_TILE * F32_TILE; i += 256) {
            const int co = c0 + (i >> 6), n = t0 + (i & 63);
            if (co < p.Cout && n < p.npos) Yb[(size_t)co * p.ldy + (size_t)n * p.os + ph] = 0.0f;
        }
        return;
    }
    const bool convt = p.os > 1;
    const int shift0 = convt ? (ph + p.pad) / p.os : -((p.taps - 1) / 2) * p.dil, step = convt ? -1 : p.dil;
    const float* Xb = p.X + (size_t)b * p.Cin * p.ldx;
    const float* Wp = p.W + (size_t)ph * p.Cout * K;
    f32x16_t acc[1] = {};
    for (int k0 = 0; k0 < K; k0 += F32_KC) {
#pragma unroll
        for (int n = 0; n < F32_TILE * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i & 63, kk = i >> 6, k = k0 + kk;
            const int j = k / p.Cin, ci = k - j * p.Cin, src = t0 + r + shift0 + j * step;
            Bs[r][kk] = (k < K && src >= 0 && src < T) ? Xb[(size_t)ci * p.ldx + src] : 0.0f;
        }
#pragma unroll
        for (int n = 0; n < F32_TILE * F32_KC / 256; ++n) {
            const int i = tid + n * 256, r = i >> 5, kk = i & 31, co = c0 + r, k = k0 + kk;
            As[r][kk] = (co < p.Cout && k < K) ? Wp[(size_t)co * K + k] : 0.0f;
        }
        __syncthreads();
        f32_tile_mfma(As, Bs, wt + l31, wc + l31, kh, acc);
        __syncthreads();
    }
    // C/D: column (tile position) = lane & 31, row (output channel) = f32_tile_row(r, lane >> 5)
    const int n = t0 + wc + l31;
    if (n >= p.npos) return;
    const size_t o = (size_t)n * p.os + ph;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = c0 + wt + f32_tile_row(r, kh);
        if (co >= p.Cout) continue;
        float v = acc[0][r];
        if (p.bias) v += p.bias[co];
        if (p.R) v = p.R[((size_t)b * p.Cout + co) * p.ldy + o] + v;
        Yb[(size_t)co * p.ldy + o] = n < T ? v : 0.0f;
    }
}

struct BvMean { const float* in[BV_MAX_KERNELS]; float* Y; int nk; size_t total; };

__global__ void __launch_bounds__(256) k_bv_mean(BvMean p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.total) return;
    float s = p.in[0][i];
#pragma unroll
    for (int k = 1; k < BV_MAX_KERNELS; ++k) if (k < p.nk) s += p.in[k][i];
    p.Y[i] = s / (float)p.nk;
}

struct BvFinal {
    const float* X; int C, ld;                              // [B][C][ld]
    const float* W; const float* bias;                      // [7][C]; bias [1] or null
    float* Y; const int32_t* frames; int mult, use_tanh;    // [B][ld]
};

__global__ void __launch_bounds__(256) k_bv_final(BvFinal p) {
    const int b = blockIdx.y, T = p.frames[b] * p.mult;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.ld) return;
    float v = 0.0f;
    if (t < T) {
        const float* Xb = p.X + (size_t)b * p.C * p.ld;
        // Taps ascending; within a tap channel c goes to chain c % 8 (ascending), the eight chains meet in a fixed tree.  One chain over
        // all 7 C products loses sqrt(7 C) roundings at the size of the whole sum; eight short ones a tap keep that at sqrt(C / 8).
        for (int j = 0; j < 7; ++j) {
            const int64_t src = t + j - 3;
            if (src < 0 || src >= T) continue;
            float a[8] = {};
            for (int c = 0; c < p.C; c += 8) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (c + q < p.C) a[q] = fmaf(p.W[j * p.C + c + q], Xb[(size_t)(c + q) * p.ld + src], a[q]);
            }
            v += ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
        }
        if (p.bias) v += p.bias[0];
        v = p.use_tanh ? tanhf(v) : fminf(fmaxf(v, -1.0f), 1.0f);
    }
    p.Y[(size_t)b * p.ld + t] = v;
}

// ============================================================================ host
struct BvConv { const float* w = nullptr; const float* b = nullptr; int cin = 0, cout = 0, taps = 0, dil = 1; };
struct BvSnake { const float* alpha = nullptr; const float* rbeta = nullptr; };
struct BvBlock { int n = 0; BvConv c1[BV_MAX_DIL], c2[BV_MAX_DIL]; BvSnake a1[BV_MAX_DIL], a2[BV_MAX_DIL]; float* out = nullptr; };
struct BvStage { BvConv up; int rate = 1, C = 0, cum = 1; BvBlock blk[BV_MAX_KERNELS]; float* t_up = nullptr; float* t_mean = nullptr; };

struct mis_bigvgan {
    int device = 0;
    hipStream_t stream = nullptr;
    mis_bigvgan_config cfg{};
    int ns = 0, nk = 0, hop = 1, C0 = 0, Cf = 0;
    bool two = false, has_beta = false;
    HostWeights raw{"BigVGAN", MIS_ERR_INVALID_INPUT};
    bool finalized = false;
    DevBuf<float> farena, work;
    DevBuf<int32_t> counts;
    BvConv pre{}, post{};
    BvSnake post_act{};
    const float* filt = nullptr;
    BvStage st[BV_MAX_STAGES];
    float *mel = nullptr, *t_pre = nullptr, *tmp_a = nullptr, *tmp_b = nullptr, *t_post = nullptr, *wav = nullptr;
    int last_batch = 0, last_launches = 0;
    int64_t last_stride = 0;
    HipEvents<2> ev;
    float ms_device = 0.0f;
};

// bigVGANKaiserSincFilter1d (BigVGANLayers.swift:47-81) in double
static void bv_kaiser_sinc(double cutoff, double half_width, int ks, double* f) {
    const double PI = 3.14159265358979323846;
    auto i0 = [](double x) {
        const double y = x * x / 4.0;
        double term = 1.0, sum = 1.0;
        for (int k = 1; k <= 40; ++k) { term *= y / ((double)k * k); sum += term; if (term < 1e-12 * sum) break; }
        return sum;
    };
    const int half = ks / 2;
    const bool even = ks % 2 == 0;
    const double a = 2.285 * (double)std::max(half - 1, 0) * PI * 4.0 * half_width + 7.95;
    const double beta = a > 50.0 ? 0.1102 * (a - 8.7) : a >= 21.0 ? 0.5842 * pow(a - 21.0, 0.4) + 0.07886 * (a - 21.0) : 0.0;
    const double h = (double)(ks - 1) / 2.0, denom = i0(beta);
    double sum = 0.0;
    for (int i = 0; i < ks; ++i) {
        const double ratio = ((double)i - h) / h, win = i0(beta * sqrt(std::max(0.0, 1.0 - ratio * ratio))) / denom;
        const double t = (double)(i - half) + (even ? 0.5 : 0.0), x = 2.0 * cutoff * t;
        f[i] = 2.0 * cutoff * win * (fabs(x) < 1e-12 ? 1.0 : sin(PI * x) / (PI * x));
        sum += f[i];
    }
    sum = std::max(sum, 1e-12);
    for (int i = 0; i < ks; ++i) f[i] /= sum;
}

extern "C" mis_status mis_bigvgan_create(const mis_bigvgan_config* cfg, int device, mis_bigvgan** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    // the configuration is judged before the device is touched
    MIS_REQUIRE(cfg->num_mels >= 1 && cfg->num_mels <= 1024, MIS_ERR_INVALID_INPUT, "num_mels %d unsupported (1..1024)", cfg->num_mels);
    MIS_REQUIRE(cfg->n_upsamples >= 1 && cfg->n_upsamples <= BV_MAX_STAGES, MIS_ERR_INVALID_INPUT, "%d upsample stages unsupported (1..%d)",
                cfg->n_upsamples, BV_MAX_STAGES);
    MIS_REQUIRE(cfg->n_upsample_kernel_sizes == cfg->n_upsamples, MIS_ERR_INVALID_INPUT, "%d upsample_kernel_sizes for %d upsample_rates",
                cfg->n_upsample_kernel_sizes, cfg->n_upsamples);
    int64_t hop = 1;
    for (int i = 0; i < cfg->n_upsamples; ++i) {
        const int s = cfg->upsample_rates[i], k = cfg->upsample_kernel_sizes[i];
        MIS_REQUIRE(s >= 2 && s <= 16 && s % 2 == 0, MIS_ERR_INVALID_INPUT, "upsample_rates[%d] = %d unsupported (even, 2..16)", i, s);
        MIS_REQUIRE(k == 2 * s, MIS_ERR_INVALID_INPUT,
                    "upsample_kernel_sizes[%d] = %d with upsample_rates[%d] = %d: only transposed convs of kernel 2 x stride are served", i, k, i, s);
        hop *= s;
    }
    MIS_REQUIRE(hop <= 4096, MIS_ERR_INVALID_INPUT, "a hop of %lld samples is unsupported (at most 4096)", (long long)hop);
    MIS_REQUIRE(cfg->upsample_initial_channel >= 1 && cfg->upsample_initial_channel <= 8192 &&
                cfg->upsample_initial_channel % (1 << cfg->n_upsamples) == 0, MIS_ERR_INVALID_INPUT,
                "upsample_initial_channel %d unsupported (a multiple of 2^%d, at most 8192)", cfg->upsample_initial_channel, cfg->n_upsamples);
    MIS_REQUIRE(cfg->resblock == 1 || cfg->resblock == 2, MIS_ERR_INVALID_INPUT, "resblock %d unsupported (1 or 2)", cfg->resblock);
    MIS_REQUIRE(cfg->n_resblock_kernels >= 1 && cfg->n_resblock_kernels <= BV_MAX_KERNELS, MIS_ERR_INVALID_INPUT,
                "%d resblock kernels unsupported (1..%d)", cfg->n_resblock_kernels, BV_MAX_KERNELS);
    for (int i = 0; i < cfg->n_resblock_kernels; ++i) {
        const int k = cfg->resblock_kernel_sizes[i], nd = cfg->n_resblock_dilations[i];
        MIS_REQUIRE(k >= 1 && k <= 11 && k % 2 == 1, MIS_ERR_INVALID_INPUT, "resblock_kernel_sizes[%d] = %d unsupported (odd, 1..11)", i, k);
        MIS_REQUIRE(nd >= 1 && nd <= BV_MAX_DIL, MIS_ERR_INVALID_INPUT, "%d dilations in resblock %d unsupported (1..%d)", nd, i, BV_MAX_DIL);
        for (int j = 0; j < nd; ++j)
            MIS_REQUIRE(cfg->resblock_dilation_sizes[i][j] >= 1 && cfg->resblock_dilation_sizes[i][j] <= 5, MIS_ERR_INVALID_INPUT,
                        "resblock_dilation_sizes[%d][%d] = %d unsupported (1..5)", i, j, cfg->resblock_dilation_sizes[i][j]);
    }
    MIS_REQUIRE(cfg->activation == 0 || cfg->activation == 1, MIS_ERR_INVALID_INPUT, "activation %d unsupported (0 snake, 1 snakebeta)", cfg->activation);
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= BV_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch must be 1..%d", BV_MAX_BATCH);
    MIS_REQUIRE(cfg->max_frames >= 1 && (int64_t)cfg->max_frames * hop < ((int64_t)1 << 30), MIS_ERR_INVALID_INPUT,
                "max_frames %d unsupported (max_frames x hop below 2^30)", cfg->max_frames);
    hipStream_t stream = mis_open_stream(device);
    auto c = std::make_unique<mis_bigvgan>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->ns = cfg->n_upsamples; c->nk = cfg->n_resblock_kernels; c->hop = (int)hop; c->C0 = cfg->upsample_initial_channel;
    c->Cf = c->C0 >> c->ns; c->two = cfg->resblock == 2; c->has_beta = cfg->activation == 1;
    int cum = 1;
    for (int i = 0; i < c->ns; ++i) {
        BvStage& s = c->st[i];
        s.rate = cfg->upsample_rates[i]; cum *= s.rate; s.cum = cum; s.C = c->C0 >> (i + 1);
        for (int k = 0; k < c->nk; ++k) s.blk[k].n = cfg->n_resblock_dilations[k];
    }
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_bigvgan_destroy(mis_bigvgan* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int mis_bigvgan_hop(const mis_bigvgan* c) { return c ? c->hop : 0; }
extern "C" int mis_bigvgan_launches(const mis_bigvgan* c) { return c ? c->last_launches : 0; }

// the reference's key names, MLX layouts: X.weight_g ([out, 1, 1]; a transposed conv [1, 1, in]), X.weight_v [out, k, in], X.bias [out],
// Y.act.alpha / Y.act.beta [channels]; host pointers
extern "C" mis_status mis_bigvgan_set_tensor(mis_bigvgan* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape, int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 3, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

// g v / (|v| + 1e-12) in double, the norm over everything but the output channel -> [cout][k cin]
static void bv_fold_conv(HostArena& a, const std::string& p, int64_t cout, int64_t k, int64_t cin, int dil, bool bias, BvConv& cv) {
    const HostTensor &g = a.w.need(p + ".weight_g", {cout, 1, 1}), &v = a.w.need(p + ".weight_v", {cout, k, cin});
    cv = BvConv{nullptr, nullptr, (int)cin, (int)cout, (int)k, dil};
    const size_t o_w = a.ftake((size_t)cout * k * cin, cv.w);
    for (int64_t o = 0; o < cout; ++o) {
        double ss = 0.0;
        for (int64_t i = 0; i < k * cin; ++i) ss += (double)v.v[o * k * cin + i] * (double)v.v[o * k * cin + i];
        const double scale = (double)g.v[o] / (sqrt(ss) + 1e-12);
        for (int64_t i = 0; i < k * cin; ++i) a.fhost[o_w + o * k * cin + i] = (float)(scale * (double)v.v[o * k * cin + i]);
    }
    if (bias) a.fvec(p + ".bias", {cout}, cout, cv.b);
}

// transposed conv [cout][2 s][cin], the norm per input channel -> [s][cout][2 cin]: phase ph, tap slot j holds tap (ph + pad) % s + s j
static void bv_fold_convt(HostArena& a, const std::string& p, int64_t cout, int64_t s, int64_t cin, BvConv& cv) {
    const int64_t k = 2 * s, pad = s / 2;
    const HostTensor &g = a.w.need(p + ".weight_g", {1, 1, cin}), &v = a.w.need(p + ".weight_v", {cout, k, cin});
    cv = BvConv{nullptr, nullptr, (int)cin, (int)cout, 2, 1};
    const size_t o_w = a.ftake((size_t)cout * k * cin, cv.w);
    std::vector<double> scale(cin);
    for (int64_t ci = 0; ci < cin; ++ci) {
        double ss = 0.0;
        for (int64_t i = 0; i < cout * k; ++i) ss += (double)v.v[i * cin + ci] * (double)v.v[i * cin + ci];
        scale[ci] = (double)g.v[ci] / (sqrt(ss) + 1e-12);
    }
    for (int64_t ph = 0; ph < s; ++ph) for (int64_t o = 0; o < cout; ++o) for (int64_t j = 0; j < 2; ++j) {
        const int64_t tap = (ph + pad) % s + s * j;
        for (int64_t ci = 0; ci < cin; ++ci)
            a.fhost[o_w + ((ph * cout + o) * 2 + j) * cin + ci] = (float)(scale[ci] * (double)v.v[(o * k + tap) * cin + ci]);
    }
    a.fvec(p + ".bias", {cout}, cout, cv.b);
}

// alpha and 1 / (beta + 1e-9), exp() of the parameters under snake_logscale; beta = alpha for activation snake
static void bv_fold_act(const mis_bigvgan* c, HostArena& a, const std::string& p, int64_t C, BvSnake& sn) {
    const HostTensor& al = a.w.need(p + ".act.alpha", {C});
    const HostTensor& be = c->has_beta ? a.w.need(p + ".act.beta", {C}) : al;
    const size_t o_a = a.ftake(C, sn.alpha), o_b = a.ftake(C, sn.rbeta);
    const bool lg = c->cfg.snake_logscale != 0;
    for (int64_t i = 0; i < C; ++i) {
        const double av = lg ? exp((double)al.v[i]) : (double)al.v[i], bv = lg ? exp((double)be.v[i]) : (double)be.v[i];
        a.fhost[o_a + i] = (float)av;
        a.fhost[o_b + i] = (float)(1.0 / (bv + 1e-9));
    }
}

extern "C" mis_status mis_bigvgan_finalize(mis_bigvgan* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    HostArena a(c->raw);
    bv_fold_conv(a, "conv_pre", c->C0, 7, c->cfg.num_mels, 1, true, c->pre);
    for (int i = 0; i < c->ns; ++i) {
        BvStage& s = c->st[i];
        bv_fold_convt(a, "ups." + std::to_string(i) + ".0", s.C, s.rate, 2 * s.C, s.up);
        for (int k = 0; k < c->nk; ++k) {
            BvBlock& bl = s.blk[k];
            const std::string q = "resblocks." + std::to_string(i * c->nk + k);
            const int ks = c->cfg.resblock_kernel_sizes[k];
            for (int d = 0; d < bl.n; ++d) {
                const int dil = c->cfg.resblock_dilation_sizes[k][d];
                if (c->two) {
                    bv_fold_conv(a, q + ".convs." + std::to_string(d), s.C, ks, s.C, dil, true, bl.c1[d]);
                    bv_fold_act(c, a, q + ".activations." + std::to_string(d), s.C, bl.a1[d]);
                } else {
                    bv_fold_conv(a, q + ".convs1." + std::to_string(d), s.C, ks, s.C, dil, true, bl.c1[d]);
                    bv_fold_conv(a, q + ".convs2." + std::to_string(d), s.C, ks, s.C, 1, true, bl.c2[d]);
                    bv_fold_act(c, a, q + ".activations." + std::to_string(2 * d), s.C, bl.a1[d]);
                    bv_fold_act(c, a, q + ".activations." + std::to_string(2 * d + 1), s.C, bl.a2[d]);
                }
            }
        }
    }
    bv_fold_act(c, a, "activation_post", c->Cf, c->post_act);
    {   // conv_post [1][7][Cf]: already [tap][channel]
        bv_fold_conv(a, "conv_post", 1, 7, c->Cf, 1, c->cfg.use_bias_at_final != 0, c->post);
    }
    double f[BV_FT];
    bv_kaiser_sinc(0.25, 0.3, BV_FT, f);
    const size_t o_f = a.ftake(BV_FT, c->filt);
    for (int i = 0; i < BV_FT; ++i) a.fhost[o_f + i] = (float)f[i];
    // ---- the workspace, sized once
    const size_t BF = (size_t)c->cfg.max_batch * (size_t)c->cfg.max_frames;
    size_t total = round_up(BF * c->cfg.num_mels, 64) + round_up(BF * c->C0, 64), widest = 0;
    for (int i = 0; i < c->ns; ++i) {
        const size_t n = round_up(BF * c->st[i].C * c->st[i].cum, 64);
        total += n * (c->nk + 2);
        widest = std::max(widest, n);
    }
    total += 2 * widest + round_up(BF * c->Cf * c->hop, 64) + round_up(BF * c->hop, 64);
    MIS_REQUIRE(total * 4 <= ((size_t)24 << 30), MIS_ERR_INVALID_INPUT, "max_batch x max_frames needs a workspace of %zu MiB (at most 24 GiB)",
                total * 4 >> 20);
    DevBuf<bf16_t> none;
    a.upload(none, c->farena);
    c->work.alloc(total);
    c->counts.alloc(BV_MAX_BATCH);
    float* w = c->work.p;
    auto take = [&](size_t n) { float* p = w; w += round_up(n, 64); return p; };
    c->mel = take(BF * c->cfg.num_mels); c->t_pre = take(BF * c->C0);
    for (int i = 0; i < c->ns; ++i) {
        BvStage& s = c->st[i];
        const size_t n = BF * s.C * s.cum;
        s.t_up = take(n);
        for (int k = 0; k < c->nk; ++k) s.blk[k].out = take(n);
        s.t_mean = take(n);
    }
    c->tmp_a = take(widest); c->tmp_b = take(widest); c->t_post = take(BF * c->Cf * c->hop); c->wav = take(BF * c->hop);
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key of a sanitized checkpoint; the norms keep a stage's variance near its input's
extern "C" mis_status mis_bigvgan_init_synthetic(mis_bigvgan* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    SynthWeights sw{c->raw, seed * 100000ull};
    auto conv = [&](const std::string& p, int64_t cout, int64_t k, int64_t cin, bool bias) {
        sw.put(p + ".weight_g", {cout, 1, 1}, 0.1, 1.0f);
        sw.put(p + ".weight_v", {cout, k, cin}, sqrt(3.0 / (double)(k * cin)), 0.0f);
        if (bias) sw.put(p + ".bias", {cout}, 0.05, 0.0f);
    };
    auto act = [&](const std::string& p, int64_t C) {
        const float mid = c->cfg.snake_logscale ? 0.0f : 1.0f;
        sw.put(p + ".act.alpha", {C}, 0.3, mid);
        if (c->has_beta) sw.put(p + ".act.beta", {C}, 0.3, mid);
    };
    conv("conv_pre", c->C0, 7, c->cfg.num_mels, true);
    for (int i = 0; i < c->ns; ++i) {
        const BvStage& s = c->st[i];
        const std::string u = "ups." + std::to_string(i) + ".0";
        sw.put(u + ".weight_g", {1, 1, 2 * s.C}, 0.05, (float)sqrt((double)s.rate / 2.0));
        sw.put(u + ".weight_v", {s.C, 2 * s.rate, 2 * s.C}, 1.0, 0.0f);
        sw.put(u + ".bias", {s.C}, 0.05, 0.0f);
        for (int k = 0; k < c->nk; ++k) {
            const std::string q = "resblocks." + std::to_string(i * c->nk + k);
            const int ks = c->cfg.resblock_kernel_sizes[k];
            for (int d = 0; d < s.blk[k].n; ++d) {
                if (c->two) { conv(q + ".convs." + std::to_string(d), s.C, ks, s.C, true); act(q + ".activations." + std::to_string(d), s.C); }
                else {
                    conv(q + ".convs1." + std::to_string(d), s.C, ks, s.C, true); conv(q + ".convs2." + std::to_string(d), s.C, ks, s.C, true);
                    act(q + ".activations." + std::to_string(2 * d), s.C); act(q + ".activations." + std::to_string(2 * d + 1), s.C);
                }
            }
        }
    }
    act("activation_post", c->Cf);
    conv("conv_post", 1, 7, c->Cf, c->cfg.use_bias_at_final != 0);
    MIS_API_END
}

// ---------------------------------------------------------------------------- launches
struct BvCall { const int32_t* frames; int B; int64_t stride; hipStream_t s; };

static void bv_launch_act(const BvCall& k, const BvSnake& sn, const float* filt, const float* X, float* Y, int C, int mult) {
    const int ld = (int)(k.stride * mult);
    BvAct p{X, Y, sn.alpha, sn.rbeta, filt, k.frames, mult, C, ld};
    hipLaunchKernelGGL(k_bv_aa_act, dim3(cdiv(ld, BV_AT), cdiv(C, BV_AC), k.B), dim3(256), 0, k.s, p);
}
// a "same" conv at `mult` samples a frame
static void bv_launch_conv(const BvCall& k, const BvConv& cv, const float* X, const float* R, float* Y, int mult) {
    const int ld = (int)(k.stride * mult);
    BvConvP p{X, ld, cv.w, cv.b, R, Y, ld, k.frames, mult, cv.cin, cv.cout, cv.taps, cv.dil, 1, 0, ld};
    hipLaunchKernelGGL(k_bv_conv, dim3(cdiv(ld, F32_TILE), cdiv(cv.cout, F32_TILE), k.B), dim3(256), 0, k.s, p);
}
// the transposed conv of stride s from `mult` samples a frame
static void bv_launch_convt(const BvCall& k, const BvConv& cv, const float* X, float* Y, int mult, int s) {
    const int ld = (int)(k.stride * mult);
    BvConvP p{X, ld, cv.w, cv.b, nullptr, Y, ld * s, k.frames, mult, cv.cin, cv.cout, 2, 1, s, s / 2, ld};
    hipLaunchKernelGGL(k_bv_conv, dim3(cdiv(ld, F32_TILE), cdiv(cv.cout, F32_TILE), k.B * s), dim3(256), 0, k.s, p);
}

// mel f32 [batch][num_mels][stride] (host), frames[batch] (NULL = stride) -> wav f32 [batch][stride hop] (host), zeros behind a row's own
extern "C" mis_status mis_bigvgan_decode(mis_bigvgan* c, const float* mel, const int32_t* frames, int batch, int64_t stride, float* wav_out) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && mel && wav_out, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "BigVGAN model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch must be 1..%d (max_batch)", c->cfg.max_batch);
    MIS_REQUIRE(stride >= 1 && stride <= c->cfg.max_frames, MIS_ERR_INVALID_INPUT, "a row of %lld frames: 1..%d (max_frames) are served",
                (long long)stride, c->cfg.max_frames);
    int32_t h_frames[BV_MAX_BATCH];
    for (int b = 0; b < batch; ++b) {
        const int64_t n = frames ? frames[b] : stride;
        MIS_REQUIRE(n >= 1 && n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld frames, 1..%lld (the row stride) are served", b, (long long)n,
                    (long long)stride);
        h_frames[b] = (int32_t)n;
    }
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t B = batch;
    HIP_CHECK(hipMemcpyAsync(c->counts.p, h_frames, B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->mel, mel, B * c->cfg.num_mels * stride * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(c->ev[0], s));
    const BvCall k{c->counts.p, batch, stride, s};
    int launches = 0;
    bv_launch_conv(k, c->pre, c->mel, nullptr, c->t_pre, 1); ++launches;
    const float* h = c->t_pre;
    int mult = 1;
    for (int i = 0; i < c->ns; ++i) {
        BvStage& st = c->st[i];
        bv_launch_convt(k, st.up, h, st.t_up, mult, st.rate); ++launches;
        mult = st.cum;
        BvMean mp{};
        for (int j = 0; j < c->nk; ++j) {
            BvBlock& bl = st.blk[j];
            const float* cur = st.t_up;                               // out = out + conv(act(out)), the running out in bl.out
            for (int d = 0; d < bl.n; ++d) {
                bv_launch_act(k, bl.a1[d], c->filt, cur, c->tmp_a, st.C, mult); ++launches;
                if (c->two) {
                    bv_launch_conv(k, bl.c1[d], c->tmp_a, cur, bl.out, mult); ++launches;
                } else {
                    bv_launch_conv(k, bl.c1[d], c->tmp_a, nullptr, c->tmp_b, mult);
                    bv_launch_act(k, bl.a2[d], c->filt, c->tmp_b, c->tmp_a, st.C, mult);
                    bv_launch_conv(k, bl.c2[d], c->tmp_a, cur, bl.out, mult);
                    launches += 3;
                }
                cur = bl.out;
            }
            mp.in[j] = bl.out;
        }
        mp.Y = st.t_mean; mp.nk = c->nk; mp.total = B * st.C * (size_t)stride * mult;
        hipLaunchKernelGGL(k_bv_mean, dim3((unsigned)((mp.total + 255) / 256)), dim3(256), 0, s, mp); ++launches;
        h = st.t_mean;
    }
    bv_launch_act(k, c->post_act, c->filt, h, c->t_post, c->Cf, mult); ++launches;
    const int ld = (int)(stride * c->hop);
    BvFinal fp{c->t_post, c->Cf, ld, c->post.w, c->post.b, c->wav, c->counts.p, c->hop, c->cfg.use_tanh_at_final != 0};
    hipLaunchKernelGGL(k_bv_final, dim3(cdiv(ld, 256), batch), dim3(256), 0, s, fp); ++launches;
    HIP_CHECK(hipEventRecord(c->ev[1], s));
    HIP_CHECK(hipMemcpyAsync(wav_out, c->wav, B * ld * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));                               // the one synchronisation of a call
    HIP_CHECK(hipEventElapsedTime(&c->ms_device, c->ev[0], c->ev[1]));
    c->last_batch = batch; c->last_stride = stride; c->last_launches = launches;
    MIS_API_END
}

// tensors of the last call, f32 [B, C, stride x up-sampling], zeros behind a row's own samples.  stage 0 conv_pre; 1 + i (nk + 2) + 0 stage
// i's transposed conv, + 1 + j AMP block j's output, + nk + 1 the stage mean; 1 + ns (nk + 2) activation_post.
extern "C" mis_status mis_bigvgan_tap(mis_bigvgan* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && stage >= 0 && stage <= 1 + c->ns * (c->nk + 2), MIS_ERR_INVALID_INPUT, "bad argument");
    MIS_REQUIRE(c->last_batch > 0, MIS_ERR_INVALID_INPUT, "no call to tap");
    HIP_CHECK(hipSetDevice(c->device));
    const float* src; size_t C, mult;
    if (stage == 0) { src = c->t_pre; C = c->C0; mult = 1; }
    else if (stage == 1 + c->ns * (c->nk + 2)) { src = c->t_post; C = c->Cf; mult = c->hop; }
    else {
        const int i = (stage - 1) / (c->nk + 2), r = (stage - 1) % (c->nk + 2);
        const BvStage& st = c->st[i];
        src = r == 0 ? st.t_up : r == c->nk + 1 ? st.t_mean : st.blk[r - 1].out; C = st.C; mult = st.cum;
    }
    const size_t B = c->last_batch, n = (size_t)c->last_stride * mult;
    if (dims) { dims[0] = (int64_t)B; dims[1] = (int64_t)C; dims[2] = (int64_t)n; }
    if (!out) return MIS_OK;
    MIS_REQUIRE((int64_t)(B * C * n) <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    HIP_CHECK(hipMemcpy(out, src, B * C * n * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// measurements: device milliseconds of the last call's kernels (events behind the copy in and before the copy out)
extern "C" mis_status mis_debug_bigvgan_timing(const mis_bigvgan* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && ms, MIS_ERR_INVALID_INPUT, "null argument");
    ms[0] = c->ms_device;
    MIS_API_END
}

// tests: ONE launch of k_bv_aa_act on host data.  x f32 [batch][channels][stride], counts[batch] columns of each row (1..stride), alpha /
// beta [channels] as the kernel uses them (after any exp()); out f32 [batch][channels][stride], zeros behind a row's own columns.  The
// inputs are followed by NaN and the output lies between guard bands, as for the other operator entry points.
extern "C" mis_status mis_debug_bigvgan_aa_act(int device, const float* x, const int32_t* counts, int batch, int channels, int64_t stride,
                                               const float* alpha, const float* beta, float* out) {
    MIS_API_BEGIN
    MIS_REQUIRE(x && counts && alpha && beta && out, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(batch >= 1 && batch <= BV_MAX_BATCH && channels >= 1 && channels <= 8192 && stride >= 1 && stride < (1 << 24), MIS_ERR_INVALID_INPUT,
                "bad shape");
    for (int b = 0; b < batch; ++b) MIS_REQUIRE(counts[b] >= 1 && counts[b] <= stride, MIS_ERR_INVALID_INPUT, "row %d: bad count", b);
    hipStream_t s = mis_open_stream(device);
    struct Close { hipStream_t s; ~Close() { (void)hipStreamDestroy(s); } } close{s};
    const size_t n = (size_t)batch * channels * stride;
    std::vector<float> rb(channels);
    for (int i = 0; i < channels; ++i) rb[i] = (float)(1.0 / ((double)beta[i] + 1e-9));
    double f[BV_FT]; float ff[BV_FT];
    bv_kaiser_sinc(0.25, 0.3, BV_FT, f);
    for (int i = 0; i < BV_FT; ++i) ff[i] = (float)f[i];
    DevBuf<uint32_t> dx, da, db, df, dc;
    alloc32(dx, x, n, F32_NAN); alloc32(da, alpha, channels, F32_NAN); alloc32(db, rb.data(), channels, F32_NAN);
    alloc32(df, ff, BV_FT, F32_NAN); alloc32(dc, counts, batch, 0);
    GuardedOut go;
    go.alloc(n * 4, 1 << 16);
    const BvCall k{(const int32_t*)dc.p, batch, stride, s};
    const BvSnake sn{(const float*)da.p, (const float*)db.p};
    bv_launch_act(k, sn, (const float*)df.p, (const float*)dx.p, (float*)go.p(), channels, 1);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    go.check_guards();
    HIP_CHECK(hipMemcpy(out, go.p(), n * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}
