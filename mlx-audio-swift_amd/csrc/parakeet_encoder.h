// parakeet_encoder.h - the Parakeet FastConformer encoder as parakeet.hip and canary.hip run it: the head-128 relative-position attention
// kernel, the encoder's weight and workspace members, the checks of its configuration, its part of finalize and of init_synthetic, and the
// two halves of the chain (front end + stem, Conformer blocks).  Cut out of parakeet.hip the way sortformer_kernels.h was cut out of
// sortformer.hip: each including file gets its own copy (the anonymous namespace), the functions take the owning handle as a template
// parameter.  The handle derives from PkEncoder and supplies: device, stream, cfg (the encoder fields of mis_parakeet_config by name, and
// max_batch / max_seconds / preemphasis / normalize / scale_input / attention_bias), raw (HostWeights), finalized, timed, timed_done, ev.
// Include common.h, audio_front.h (AUDIO_FRONT_NEMO_KERNELS), f32_tile.h, host_weights.h, step_loop.h and sortformer_kernels.h first, and
// parakeet_encoder_bf16.h behind it: the opt-in bf16 form of the block chain (enc_bf16; its precision contract stands there).  With
// enc_bf16 the eight block matrices go to the bf16 arena instead of the f32 one, each layer's table is projected by pk_bf16_tables, big /
// qkv / att are bf16 buffers and pk_encoder hands over to pk_encoder_bf16; everything else here is shared by both modes.
#pragma once

#include <math.h>
#include <string>

#define PK_MAX_BATCH 64
#define PK_MAX_SECONDS 120

namespace {

// ============================================================================ kernel A: attention, head sizes 65..128
// SfAttn as k_sf_attn<.., true> takes it.  LDP: an odd row stride, so the 32 rows a half-wave reads fall into 32 banks.
#define PK_LDP 129
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) k_pk_attn(SfAttn p) {
    __shared__ float Ks[32][PK_LDP];
    __shared__ float Pb[96 * PK_LDP];                               // the band; between uses: Q tile, exchanged partials, output tile
    __shared__ float Ub[2][128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5, qh = wave & 1, dh = wave >> 1;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 64, n = min(p.cnt[b], p.Tp), hd = p.hd;
    const size_t rowbase = (size_t)b * p.Tp;
    if (q0 >= n) {                                                  // (uniform over the block)
        for (int i = tid; i < 64 * hd; i += 256) {
            const int t = q0 + i / hd;
            if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + i % hd] = 0.0f;
        }
        return;
    }
#pragma unroll 4
    for (int i = tid; i < 64 * 128; i += 256) {
        const int r = i >> 7, c = i & 127, tq = q0 + r;
        Pb[r * PK_LDP + c] = (tq < n && c < hd) ? p.qkv[(rowbase + tq) * p.ld + h * hd + c] * p.qscale : 0.0f;
    }
    {
        const int c = tid & 127;
        Ub[tid >> 7][c] = c < hd ? (tid < 128 ? p.u : p.v)[h * hd + c] : 0.0f;
    }
    __syncthreads();
    const int wq = qh * 32, d0 = dh * 64;
    float qf[32];                                                   // the wave's 64 dimensions of query wq + l31; u and v are added at use (LDS), as registers are short
#pragma unroll
    for (int i = 0; i < 32; ++i) qf[i] = Pb[(wq + l31) * PK_LDP + d0 + 2 * i + kh];
    f32x16_t O[2];
#pragma unroll
    for (int dn = 0; dn < 2; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) O[dn][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const float* Bd0 = Pb + qh * 2048;                              // band products [64 band rows][32 queries] of dh 0, dh 1
    const float* Bd1 = Pb + (qh + 2) * 2048;
    const float* Sx0 = Pb + 8192 + qh * 1024;                       // content scores [32 keys][32 queries] of dh 0, dh 1
    const float* Sx1 = Pb + 8192 + (qh + 2) * 1024;
    for (int kb = 0; kb < n; kb += 32) {
        __syncthreads();                                            // the previous tile's reads are done (first pass: the Q fragments are taken)
#pragma unroll 4
        for (int i = tid; i < 32 * 128; i += 256) {
            const int r = i >> 7, c = i & 127, key = kb + r;
            Ks[r][c] = (key < n && c < hd) ? p.qkv[(rowbase + key) * p.ld + p.koff + h * hd + c] : 0.0f;
        }
        const int base = q0 - kb - 31 + p.Tcap - 1;                 // table row of band row 0
#pragma unroll 4
        for (int i = tid; i < 96 * 128; i += 256) {
            const int r = i >> 7, c = i & 127, idx = base + r;
            Pb[r * PK_LDP + c] = (idx >= 0 && idx < 2 * p.Tcap - 1 && c < hd) ? p.P[(size_t)idx * p.ldp + h * hd + c] : 0.0f;
        }
        __syncthreads();
        // partial S^T[key][query] and partial band products over the wave's 64 dimensions
        f32x16_t S, G0, G1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = 0.0f; G0[r] = 0.0f; G1[r] = 0.0f; }
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int k = d0 + 2 * i + kh;
            const float qu = qf[i] + Ub[0][k], qv = qf[i] + Ub[1][k];
            S = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[l31][k], qu, S, 0, 0, 0);
            G0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[(wq + l31) * PK_LDP + k], qv, G0, 0, 0, 0);
            G1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[(wq + 32 + l31) * PK_LDP + k], qv, G1, 0, 0, 0);
            if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);    // keep the operand loads of at most four steps in flight (registers)
        }
        __syncthreads();                                            // every wave has read its band rows: the space becomes the partials'
        {
            float* Bd = Pb + wave * 2048;
            float* Sx = Pb + 8192 + wave * 1024;
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
            const int j = f32_tile_row(r, kh), at = (l31 - j + 31) * 32 + l31;   // distance i - j, the literal rel-shift's entry
            const float s = (Sx0[j * 32 + l31] + Sx1[j * 32 + l31]) + (Bd0[at] + Bd1[at]);
            S[r] = (kb + j < n) ? s / p.sdk : -INFINITY;
            mx = fmaxf(mx, S[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);                       // finite: every tile holds a key < n
        const float alpha = expf(m_run - m_new);
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { S[r] = expf(S[r] - m_new); psum += S[r]; }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int dn = 0; dn < 2; ++dn) {
#pragma unroll
            for (int r = 0; r < 16; ++r) O[dn][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {                          // V^T straight from memory: 32 consecutive floats of key f32_tile_row(r, kh)
                const int key = kb + f32_tile_row(r, kh), d = d0 + dn * 32 + l31;
                const float vv = (key < n && d < hd) ? p.qkv[(rowbase + key) * p.ld + p.voff + h * hd + d] : 0.0f;
                O[dn] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, S[r], O[dn], 0, 0, 0);
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    __syncthreads();                                                // the band space is free: the outputs go through it for coalesced stores
#pragma unroll
    for (int dn = 0; dn < 2; ++dn)
#pragma unroll
        for (int r = 0; r < 16; ++r) Pb[(wq + l31) * PK_LDP + d0 + dn * 32 + f32_tile_row(r, kh)] = O[dn][r] / l_tot;
    __syncthreads();
    for (int i = tid; i < 64 * hd; i += 256) {
        const int r = i / hd, c = i - r * hd, t = q0 + r;
        if (t < p.Tp) p.out[(rowbase + t) * p.ldo + h * hd + c] = t < n ? Pb[r * PK_LDP + c] : 0.0f;
    }
}

template <class Ctx>
static void pk_attn(Ctx* c, const SfAttn& p, int heads, int hd, int batch) {
    if (hd <= 64) { sf_attn<true>(c, p, heads, hd, batch); return; }
    MIS_LAUNCH(c, k_pk_attn, dim3(cdiv(p.Tp, 64), heads, batch), dim3(256), p);
}

// ============================================================================ the encoder's members
struct PkEncoder {
    int mels = 0, C = 0, d = 0, H = 0, hd = 0, f = 0, L = 0, ck = 0, F1 = 0, F2 = 0, F3 = 0;
    DevBuf<float> farena, ptab;
    DevBuf<int> fbr;
    const float *window = nullptr, *twc = nullptr, *tws = nullptr, *fb = nullptr, *c0w = nullptr, *c0b = nullptr, *dw2w = nullptr, *dw2b = nullptr,
                *dw5w = nullptr, *dw5b = nullptr, *postab = nullptr;
    SfLin pw3, pw6, lin;
    struct Layer {
        const float *ln1w, *ln1b, *lnaw, *lnab, *lncw, *lncb, *ln2w, *ln2b, *lnow, *lnob, *u, *v, *P, *dw, *dwshift;
        SfLin ff1a, ff1b, qkv, o, pw1, pw2, ff2a, ff2b;
    };
    std::vector<Layer> fc;
    std::vector<SfLin> rk;                                           // relative_k_proj of every block: used once, at finalize
    std::vector<int> fb_ranges;
    // workspace (sized at finalize)
    int64_t maxN = 0;
    int Fcap = 0, T1cap = 0, T2cap = 0, Tcap = 0;
    DevBuf<float> pcm, melraw, feats, s0, s1, s2, emb, h, stats, big, qkv, att;
    DevBuf<int> cntN, cntF, cnt1, cnt2, cnt3;
    // state of the last call
    int batch = 0, Fp = 0, T1p = 0, T2p = 0, Tp = 0, launches = 0;
    std::vector<int> hN, hF, hT1, hT2, hT3;
    bool has_emb = false;
    // bf16 mode (parakeet_encoder_bf16.h): the block matrices [N][K] and the rounded tables [2 Tcap - 1][d]; Layer keeps the f32 members
    int enc_bf16 = 0;
    struct Layer16 { bf16_t *ff1a, *ff1b, *qkv, *o, *pw1, *pw2, *ff2a, *ff2b, *P; };
    std::vector<Layer16> fc16;
    DevBuf<bf16_t> warena, ptab16, big16, qkv16, att16;
};

template <class Ctx> static void pk_bf16_tables(Ctx* c);
template <class Ctx> static void pk_encoder_bf16(Ctx* c, int stop);

static inline int pk_half(int t) { return t >= 1 ? (t - 1) / 2 + 1 : 0; }
static inline int pk_frames(int64_t n) { return (int)(1 + n / NEMO_HOP); }

// the sinusoid table by distance [2 Tc - 1][d]: row dist + Tc - 1, columns interleaved sin, cos; formed in double, rounded once
static void pk_postab(float* tab, int Tc, int64_t d) {
    for (int r = 0; r < 2 * Tc - 1; ++r) {
        const double dist = (double)(r - (Tc - 1));
        for (int64_t k = 0; 2 * k < d; ++k) {
            const double ang = dist * exp(-(double)(2 * k) * log(10000.0) / (double)d);
            tab[(size_t)r * d + 2 * k] = (float)sin(ang);
            if (2 * k + 1 < d) tab[(size_t)r * d + 2 * k + 1] = (float)cos(ang);
        }
    }
}

// what create asks of the encoder's fields
template <class Cfg>
static void pk_encoder_check(const Cfg* cfg) {
    const int d = cfg->hidden_size, H = cfg->num_attention_heads;
    MIS_REQUIRE(cfg->sampling_rate == 16000 && cfg->n_fft == NEMO_NFFT && cfg->hop_length == NEMO_HOP && cfg->win_length == NEMO_WIN, MIS_ERR_INVALID_INPUT,
                "sampling_rate / n_fft / hop_length / win_length: only 16000 / 512 / 160 / 400 are implemented");
    MIS_REQUIRE(cfg->preemphasis >= 0.0f && cfg->preemphasis <= 1.0f, MIS_ERR_INVALID_INPUT, "preemphasis outside 0..1");
    MIS_REQUIRE(cfg->num_mel_bins >= 8 && cfg->num_mel_bins <= 256, MIS_ERR_INVALID_INPUT, "num_mel_bins %d outside 8..256", cfg->num_mel_bins);
    MIS_REQUIRE(cfg->subsampling_factor == 8, MIS_ERR_INVALID_INPUT, "subsampling_factor %d: only 8 is implemented", cfg->subsampling_factor);
    MIS_REQUIRE(cfg->subsampling_conv_channels >= 1 && cfg->subsampling_conv_channels <= 1024, MIS_ERR_INVALID_INPUT,
                "subsampling_conv_channels %d outside 1..1024", cfg->subsampling_conv_channels);
    MIS_REQUIRE(d >= 8 && d <= 4096, MIS_ERR_INVALID_INPUT, "hidden_size %d outside 8..4096", d);
    MIS_REQUIRE(H >= 1 && d % H == 0 && d / H <= 128, MIS_ERR_INVALID_INPUT,
                "num_attention_heads %d: head size hidden_size / num_attention_heads must be a whole number up to 128", H);
    MIS_REQUIRE(cfg->intermediate_size >= 1 && cfg->intermediate_size <= 16384, MIS_ERR_INVALID_INPUT, "intermediate_size %d outside 1..16384",
                cfg->intermediate_size);
    MIS_REQUIRE(cfg->num_hidden_layers >= 1 && cfg->num_hidden_layers <= 64, MIS_ERR_INVALID_INPUT, "num_hidden_layers %d outside 1..64", cfg->num_hidden_layers);
    MIS_REQUIRE(cfg->conv_kernel_size >= 3 && cfg->conv_kernel_size <= SF_DW_MAXK && cfg->conv_kernel_size % 2 == 1, MIS_ERR_INVALID_INPUT,
                "conv_kernel_size %d unsupported (odd, 3..%d)", cfg->conv_kernel_size, SF_DW_MAXK);
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= PK_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch %d outside 1..%d", cfg->max_batch, PK_MAX_BATCH);
    MIS_REQUIRE(cfg->max_seconds >= 1 && cfg->max_seconds <= PK_MAX_SECONDS, MIS_ERR_INVALID_INPUT, "max_seconds %d outside 1..%d", cfg->max_seconds,
                PK_MAX_SECONDS);
}

template <class Ctx>
static void pk_encoder_dims(Ctx* c) {
    const auto& cfg = c->cfg;
    c->mels = cfg.num_mel_bins; c->C = cfg.subsampling_conv_channels; c->d = cfg.hidden_size; c->H = cfg.num_attention_heads; c->hd = c->d / c->H;
    c->f = cfg.intermediate_size; c->L = cfg.num_hidden_layers; c->ck = cfg.conv_kernel_size;
    c->F1 = pk_half(c->mels); c->F2 = pk_half(c->F1); c->F3 = pk_half(c->F2);
}

// finalize, first half: the front end's tables and every encoder tensor into the arena (nothing is uploaded yet)
template <class Ctx>
static void pk_encoder_weights(Ctx* c, HostArena& a) {
    const int64_t mels = c->mels, C = c->C, d = c->d, f = c->f, ck = c->ck, F3 = c->F3, H = c->H, hd = c->hd;
    const bool ab = c->cfg.attention_bias != 0;
    std::vector<float>& fh = a.fhost;
    const size_t o_win = a.ftake(NEMO_NFFT, c->window), o_twc = a.ftake(NEMO_NFFT / 2, c->twc), o_tws = a.ftake(NEMO_NFFT / 2, c->tws);
    hann_padded(&fh[o_win], NEMO_WIN, NEMO_NFFT);
    fft512_twiddles(&fh[o_twc], &fh[o_tws]);
    const size_t o_fb = a.ftake((size_t)NEMO_BINS * mels, c->fb);
    c->fb_ranges.assign(2 * mels, 0);
    slaney_filterbank(&fh[o_fb], c->fb_ranges.data(), NEMO_BINS, (int)mels, 16000.0, NEMO_NFFT);
    c->maxN = (int64_t)c->cfg.max_seconds * 16000;
    c->Fcap = pk_frames(c->maxN); c->T1cap = pk_half(c->Fcap); c->T2cap = pk_half(c->T1cap); c->Tcap = pk_half(c->T2cap);
    const int Tc = c->Tcap, NP = 2 * Tc - 1;
    const bool b16 = c->enc_bf16 != 0;
    // a block matrix: the f32 arena, or rounded once into the bf16 arena
    auto mat = [&](const std::string& name, std::initializer_list<int64_t> shape, int64_t N, int64_t K, const float*& wf, bf16_t*& wb) {
        if (!b16) { a.fvec(name, shape, N * K, wf); return; }
        const HostTensor& t = c->raw.need(name, shape);
        const size_t off = a.btake((size_t)N * K, wb);
        for (int64_t i = 0; i < N * K; ++i) a.host[off + i] = f32_to_bf16(t.v[i]);
    };
    auto lin = [&](const std::string& p, int64_t N, int64_t K, bool bias, SfLin& l, bf16_t*& wb) {
        l = SfLin{};
        mat(p + ".weight", {N, K}, N, K, l.w, wb);
        if (bias) a.fvec(p + ".bias", {N}, N, l.b);
    };
    auto norm = [&](const std::string& p, int64_t n, const float*& w, const float*& b) { a.fvec(p + ".weight", {n}, n, w); a.fvec(p + ".bias", {n}, n, b); };
    const std::string SUB = "encoder.subsampling.";
    auto taps9 = [&](const std::string& name, const float*& dst) {    // conv taps [C][3][3][1] -> [9][C]
        const HostTensor& t = c->raw.need(name, {C, 3, 3, 1});
        const size_t off = a.ftake(9 * C, dst);
        for (int64_t ch = 0; ch < C; ++ch) for (int k = 0; k < 9; ++k) fh[off + k * C + ch] = t.v[ch * 9 + k];
    };
    taps9(SUB + "layers_0.weight", c->c0w); a.fvec(SUB + "layers_0.bias", {C}, C, c->c0b);
    taps9(SUB + "layers_2.weight", c->dw2w); a.fvec(SUB + "layers_2.bias", {C}, C, c->dw2b);
    a.fvec(SUB + "layers_3.weight", {C, 1, 1, C}, C * C, c->pw3.w); a.fvec(SUB + "layers_3.bias", {C}, C, c->pw3.b);
    taps9(SUB + "layers_5.weight", c->dw5w); a.fvec(SUB + "layers_5.bias", {C}, C, c->dw5b);
    a.fvec(SUB + "layers_6.weight", {C, 1, 1, C}, C * C, c->pw6.w); a.fvec(SUB + "layers_6.bias", {C}, C, c->pw6.b);
    {   // linear [d][C F3] reads the flattening (c, f); the stem keeps channels last: columns re-ordered to (f, c)
        const size_t ow = a.ftake((size_t)d * C * F3, c->lin.w);
        a.fvec(SUB + "linear.bias", {d}, d, c->lin.b);
        const HostTensor& w = c->raw.need(SUB + "linear.weight", {d, C * F3});
        for (int64_t n = 0; n < d; ++n) for (int64_t ch = 0; ch < C; ++ch) for (int64_t fq = 0; fq < F3; ++fq)
            fh[ow + (n * F3 + fq) * C + ch] = w.v[n * C * F3 + ch * F3 + fq];
    }
    c->fc.assign(c->L, PkEncoder::Layer{});
    c->fc16.assign(c->L, PkEncoder::Layer16{});
    c->rk.assign(c->L, SfLin{});
    for (int li = 0; li < c->L; ++li) {
        const std::string q = "encoder.layers." + std::to_string(li) + ".";
        PkEncoder::Layer& l = c->fc[li];
        PkEncoder::Layer16& l16 = c->fc16[li];
        norm(q + "norm_feed_forward1", d, l.ln1w, l.ln1b);
        lin(q + "feed_forward1.linear1", f, d, ab, l.ff1a, l16.ff1a); lin(q + "feed_forward1.linear2", d, f, ab, l.ff1b, l16.ff1b);
        norm(q + "norm_self_att", d, l.lnaw, l.lnab);
        {   // q, k, v over the same input as one [3 d][d]; an absent bias is zero
            const size_t ow = b16 ? a.btake((size_t)3 * d * d, l16.qkv) : a.ftake((size_t)3 * d * d, l.qkv.w), ob = a.ftake(3 * d, l.qkv.b);
            const char* names[3] = {"q_proj", "k_proj", "v_proj"};
            for (int i = 0; i < 3; ++i) {
                const HostTensor& w = c->raw.need(q + "self_attn." + names[i] + ".weight", {d, d});
                if (b16) for (int64_t j = 0; j < d * d; ++j) a.host[ow + (size_t)i * d * d + j] = f32_to_bf16(w.v[j]);
                else std::copy(w.v.begin(), w.v.end(), fh.begin() + ow + (size_t)i * d * d);
                if (ab) { const HostTensor& bb = c->raw.need(q + "self_attn." + names[i] + ".bias", {d}); std::copy(bb.v.begin(), bb.v.end(), fh.begin() + ob + (size_t)i * d); }
            }
        }
        lin(q + "self_attn.o_proj", d, d, ab, l.o, l16.o);
        if (b16) c->raw.need(q + "self_attn.relative_k_proj.weight", {d, d});       // uploaded by pk_bf16_tables, for the projection only
        else a.fvec(q + "self_attn.relative_k_proj.weight", {d, d}, d * d, c->rk[li].w);
        a.fvec(q + "self_attn.bias_u", {H, hd}, d, l.u); a.fvec(q + "self_attn.bias_v", {H, hd}, d, l.v);
        norm(q + "norm_conv", d, l.lncw, l.lncb);
        mat(q + "conv.pointwise_conv1.weight", {2 * d, 1, d}, 2 * d, d, l.pw1.w, l16.pw1);
        mat(q + "conv.pointwise_conv2.weight", {d, 1, d}, d, d, l.pw2.w, l16.pw2);
        if (ab) { a.fvec(q + "conv.pointwise_conv1.bias", {2 * d}, 2 * d, l.pw1.b); a.fvec(q + "conv.pointwise_conv2.bias", {d}, d, l.pw2.b); }
        const HostTensor& dw = c->raw.need(q + "conv.depthwise_conv.weight", {d, ck, 1});
        const HostTensor* dwb = ab ? &c->raw.need(q + "conv.depthwise_conv.bias", {d}) : nullptr;
        const HostTensor& bw = c->raw.need(q + "conv.norm.weight", {d}); const HostTensor& bb = c->raw.need(q + "conv.norm.bias", {d});
        const HostTensor& bm = c->raw.need(q + "conv.norm.running_mean", {d}); const HostTensor& bv = c->raw.need(q + "conv.norm.running_var", {d});
        const size_t o_dw = a.ftake((size_t)ck * d, l.dw), o_sh = a.ftake(d, l.dwshift);
        fold_bn_dwconv(&fh[o_dw], &fh[o_sh], dw.v.data(), dwb ? dwb->v.data() : nullptr, bw.v.data(), bb.v.data(), bm.v.data(), bv.v.data(), d, ck);
        norm(q + "norm_feed_forward2", d, l.ln2w, l.ln2b);
        lin(q + "feed_forward2.linear1", f, d, ab, l.ff2a, l16.ff2a); lin(q + "feed_forward2.linear2", d, f, ab, l.ff2b, l16.ff2b);
        norm(q + "norm_out", d, l.lnow, l.lnob);
    }
    if (b16) return;                                                // the table is pk_bf16_tables' in bf16 mode
    const size_t o_tab = a.ftake((size_t)NP * d, c->postab);
    pk_postab(&fh[o_tab], Tc, d);
}

// finalize, second half (the arena is uploaded): each layer's relative_k_proj of the table, one GEMM each, once; the workspace
template <class Ctx>
static void pk_encoder_workspace(Ctx* c) {
    const int64_t mels = c->mels, C = c->C, d = c->d, f = c->f, F3 = c->F3;
    const int Tc = c->Tcap, NP = 2 * Tc - 1;
    c->fbr.alloc(2 * mels);
    HIP_CHECK(hipMemcpy(c->fbr.p, c->fb_ranges.data(), 2 * mels * sizeof(int), hipMemcpyHostToDevice));
    if (c->enc_bf16) pk_bf16_tables(c);
    else {
        c->ptab.alloc((size_t)c->L * NP * d);
        for (int li = 0; li < c->L; ++li) {
            float* dst = c->ptab.p + (size_t)li * NP * d;
            sf_gemm(c, sf_lin(c->postab, (int)d, c->rk[li], dst, (int)d, nullptr, NP), 1);
            c->fc[li].P = dst;
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    c->launches = 0;
    const size_t B = c->cfg.max_batch, M = B * Tc;
    c->pcm.alloc(B * c->maxN); c->melraw.alloc(B * c->Fcap * mels); c->feats.alloc(B * c->Fcap * mels);
    c->s0.alloc(B * c->T1cap * c->F1 * C); c->s1.alloc(B * c->T2cap * c->F2 * C); c->s2.alloc(M * F3 * C); c->emb.alloc(M * d);
    c->h.alloc(M * d); c->stats.alloc(M * 2);
    if (c->enc_bf16) { c->big16.alloc(M * std::max<size_t>(f, 2 * d)); c->qkv16.alloc(M * 3 * d); c->att16.alloc(M * d); }
    else { c->big.alloc(M * std::max<size_t>(f, 2 * d)); c->qkv.alloc(M * 3 * d); c->att.alloc(M * d); }
    c->cntN.alloc(B); c->cntF.alloc(B); c->cnt1.alloc(B); c->cnt2.alloc(B); c->cnt3.alloc(B);
}

// mis-synth-v1 weights: every encoder key, in this order
template <class Ctx>
static void pk_encoder_synthetic(Ctx* c, SynthWeights& sw) {
    const int64_t C = c->C, d = c->d, f = c->f, ck = c->ck;
    const bool ab = c->cfg.attention_bias != 0;
    const std::string SUB = "encoder.subsampling.";
    for (const char* n : {"layers_0", "layers_2", "layers_5"}) { sw.put(SUB + n + ".weight", {C, 3, 3, 1}, sqrt(3.0 / 9.0), 0.0f); sw.put(SUB + n + ".bias", {C}, 0.05, 0.0f); }
    for (const char* n : {"layers_3", "layers_6"}) { sw.put(SUB + n + ".weight", {C, 1, 1, C}, sqrt(3.0 / (double)C), 0.0f); sw.put(SUB + n + ".bias", {C}, 0.05, 0.0f); }
    sw.lin(SUB + "linear", d, C * c->F3, true, 1.0);
    for (int li = 0; li < c->L; ++li) {
        const std::string q = "encoder.layers." + std::to_string(li) + ".";
        for (const char* n : {"norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"}) sw.norm(q + n, d);
        for (const char* n : {"feed_forward1", "feed_forward2"}) { sw.lin(q + n + ".linear1", f, d, ab, 1.0); sw.lin(q + n + ".linear2", d, f, ab, 0.5); }
        for (const char* n : {"q_proj", "k_proj", "v_proj"}) sw.lin(q + "self_attn." + n, d, d, ab, 1.0);
        sw.lin(q + "self_attn.o_proj", d, d, ab, 0.5);
        sw.lin(q + "self_attn.relative_k_proj", d, d, false, 1.0);
        sw.put(q + "self_attn.bias_u", {c->H, c->hd}, 0.1, 0.0f); sw.put(q + "self_attn.bias_v", {c->H, c->hd}, 0.1, 0.0f);
        sw.put(q + "conv.pointwise_conv1.weight", {2 * d, 1, d}, sqrt(3.0 / (double)d), 0.0f);
        sw.put(q + "conv.pointwise_conv2.weight", {d, 1, d}, 0.5 * sqrt(3.0 / (double)d), 0.0f);
        sw.put(q + "conv.depthwise_conv.weight", {d, ck, 1}, sqrt(3.0 / (double)ck), 0.0f);
        if (ab) {
            sw.put(q + "conv.pointwise_conv1.bias", {2 * d}, 0.05, 0.0f); sw.put(q + "conv.pointwise_conv2.bias", {d}, 0.05, 0.0f);
            sw.put(q + "conv.depthwise_conv.bias", {d}, 0.05, 0.0f);
        }
        sw.put(q + "conv.norm.weight", {d}, 0.1, 1.0f); sw.put(q + "conv.norm.bias", {d}, 0.05, 0.0f);
        sw.put(q + "conv.norm.running_mean", {d}, 0.05, 0.0f); sw.put(q + "conv.norm.running_var", {d}, 0.1, 1.0f);
    }
}

// ============================================================================ the chain
// judged first (nothing of the handle is written), then taken: counts uploaded, pcm copied, the front end and the stem launched (6 launches)
template <class Ctx>
static void pk_front_stem(Ctx* c, const float* pcm, const int64_t* lens, int batch, int64_t stride) {
    MIS_REQUIRE(c->finalized, MIS_ERR_NOT_INITIALIZED, "model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch %d outside 1..%d (max_batch)", batch, c->cfg.max_batch);
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    std::vector<int> N(batch), F(batch), t1(batch), t2(batch), t3(batch);
    int Fp = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 0 && n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the row stride %lld", b, (long long)n, (long long)stride);
        MIS_REQUIRE(n <= c->maxN, MIS_ERR_INVALID_INPUT, "row %d: %lld samples exceed the workspace of %d seconds (max_seconds)", b, (long long)n,
                    c->cfg.max_seconds);
        N[b] = (int)n; F[b] = pk_frames(n); t1[b] = pk_half(F[b]); t2[b] = pk_half(t1[b]); t3[b] = pk_half(t2[b]);
        Fp = std::max(Fp, F[b]);
    }
    c->hN = N; c->hF = F; c->hT1 = t1; c->hT2 = t2; c->hT3 = t3;
    c->batch = batch; c->Fp = Fp; c->T1p = pk_half(Fp); c->T2p = pk_half(c->T1p); c->Tp = pk_half(c->T2p);
    c->launches = 0; c->has_emb = false; c->timed_done = false;
    hipStream_t s = c->stream;
    HIP_CHECK(hipMemcpyAsync(c->cntN.p, c->hN.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cntF.p, c->hF.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt1.p, c->hT1.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt2.p, c->hT2.data(), batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c->cnt3.p, c->hT3.data(), batch * 4, hipMemcpyHostToDevice, s));
    const int64_t ws = std::min<int64_t>(stride, c->maxN);
    HIP_CHECK(hipMemcpy2DAsync(c->pcm.p, ws * 4, pcm, stride * 4, ws * 4, batch, hipMemcpyDefault, s));
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[0], s));
    MIS_LAUNCH(c, k_nemo_log_mel<false>, dim3(Fp, batch), dim3(256), c->pcm.p, ws, c->cntN.p, c->cntF.p, (const float*)nullptr, c->cfg.preemphasis, c->window,
               c->twc, c->tws, c->fb, c->fbr.p, c->melraw.p, Fp, c->mels);
    MIS_LAUNCH(c, k_nemo_norm, dim3(cdiv(c->mels, 64), batch), dim3(256), c->melraw.p, c->cntF.p, c->feats.p, Fp, c->mels, c->cfg.normalize);
    if (c->timed) HIP_CHECK(hipEventRecord(c->ev[1], s));
    const int B = batch, C = c->C, F1 = c->F1, F2 = c->F2, F3 = c->F3;
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

// c->emb -> the Conformer blocks -> c->h (1 + 15 L launches); stop: -1 all, 1 .. L behind that block
template <class Ctx>
static void pk_encoder(Ctx* c, int stop) {
    if (c->enc_bf16) { pk_encoder_bf16(c, stop); return; }
    const int B = c->batch, Tp = c->Tp, d = c->d, f = c->f, M = B * Tp;
    const int* cnt = c->cnt3.p;
    const size_t nd = (size_t)M * d;
    MIS_LAUNCH(c, k_sf_intake, dim3((unsigned)((nd + 255) / 256)), dim3(256), c->emb.p, c->h.p, cnt, Tp, d, c->cfg.scale_input ? sqrtf((float)d) : 1.0f, nd);
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
    for (int li = 0; li < c->L; ++li) {                            // 15 launches a block
        const PkEncoder::Layer& l = c->fc[li];
        stats(c->h.p);
        ln_lin(c->h.p, l.ln1w, l.ln1b, l.ff1a, c->big.p, f, SF_ACT_SILU);
        res_lin(c->big.p, f, l.ff1b, c->h.p, d, 0.5f);
        stats(c->h.p);
        ln_lin(c->h.p, l.lnaw, l.lnab, l.qkv, c->qkv.p, 3 * d, SF_ACT_NONE);
        SfAttn ap{c->qkv.p, 3 * d, d, 2 * d, c->att.p, d, cnt, Tp, c->hd, 1.0f, sqrtf((float)c->hd), l.u, l.v, l.P, d, c->Tcap};
        pk_attn(c, ap, c->H, c->hd, B);
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
}

}  // namespace
