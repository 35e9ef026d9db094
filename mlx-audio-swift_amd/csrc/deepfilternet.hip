// deepfilternet.hip - DeepFilterNet V2 / V3 speech enhancement, offline: waveform -> STFT -> ERB + complex features -> encoder ->
// three squeezed GRUs -> ERB mask + deep-filter coefficients -> filtered spectrum -> inverse STFT and overlap-add.  Exact f32.
//
// Reference being replaced: DeepFilterNetModel.enhance (Sources/MLXAudioSTS/Models/DeepFilterNet/DeepFilterNetModel.swift:323-418),
// forward / encode / decodeErb / decodeDf / applyMask / deepFilter (DeepFilterNetForward.swift:9-198), the layers of
// DeepFilterNetLayers.swift and the features of DeepFilterNetDSP.swift.
//
// One call serves 1..max_batch ragged rows.  Row b of n_b samples has T_b = 1 + (hop + n_b) / hop frames (hop zeros in front, fft zeros
// behind, both formed in the operand load) and n_b output samples.  Every activation is f32 [B][nr][F][C] (frame, frequency, channel;
// F = 1 for the GRU chains), nr the call's longest row, a row's own frames first and zeros behind them.  Every output element is one
// fixed-order sum over data of its own row: a row's result is bit for bit the same whatever batch it travels in.
//
//   k_dfn_gemm   the one contraction, exact f32 on v_mfma_f32_32x32x2_f32 (f32_tile.h), 64 x 64 tile, every edge guarded.  Operand
//                loads: activations (grouped linears read their own K range only), windowed frames of the zero-padded waveform, |spec|^2,
//                im2col of a causal conv, and a grouped / depthwise conv or a grouped transposed conv computed on the fly in front of
//                its pointwise conv (no intermediate tensor).  Epilogue: folded BatchNorm or bias, ReLU / sigmoid / tanh / 10 log10 /
//                lsnr, column scale, residual.
//   k_dfn_norm   one block a row, one thread a band / bin: band means (without erb_fb) and the two exponential normalisations as the
//                serial recurrence s_t = a s_(t-1) + (1 - a) x_t
//   k_dfn_gru    the recurrence of one GRU layer for all frames of all rows in one launch, block = (row, chain): thread t owns gate row
//                t of Wh, its first KR columns in registers for the whole launch, the other H - KR re-read every step from a
//                transposed copy ([column][3H]: a wave reads consecutive addresses); h in LDS, read as broadcasts; two barriers a step
//   k_dfn_enh    bins >= nb_df: spec x (mask @ erb_inv_fb); bins < nb_df: the deep filter of the unmasked spec; / wnorm
//   k_dfn_ola    overlap-add as a gather, / max(sum w^2, 1e-8), the first fft - hop samples dropped, clip to [-1, 1]
//
// Launches of a call: 26 + [erb_fb] + [df_skip] + [enc linear_out] + [erb_dec linear_out] + 2 L_enc + L_erb + L_df
// + (H_emb == H_df ? max(L_erb, L_df) : L_erb + L_df).
//
// The kernels and the handle live in deepfilternet_kernels.h, shared with the hop-by-hop streamer (deepfilternet_stream.hip); this file
// instantiates their offline form (S = false).
#include "deepfilternet_kernels.h"

// out[b][s] = sum over the frames f covering padded sample s + fft - hop, in frame order, / max(sum w^2, 1e-8), clipped; 0 from lens[b] on
__global__ void __launch_bounds__(256) k_dfn_ola(const float* __restrict__ fr, const float* __restrict__ win, float* __restrict__ out,
                                                 const int32_t* cnt, const int32_t* lens, int nr, int W, int hop, int64_t out_stride) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y, T = min(cnt[b], nr);
    if (s >= out_stride) return;
    float v = 0.0f;
    if (s < lens[b]) {
        const int64_t q = s + W - hop, lo = q - W + 1;
        const int fa = lo <= 0 ? 0 : (int)((lo + hop - 1) / hop), fb = q / hop > T - 1 ? T - 1 : (int)(q / hop);
        v = df_ola_at(fr + (size_t)b * nr * W, 0, win, q, fa, fb, W, hop);
    }
    out[(size_t)b * out_stride + s] = v;
}

static int64_t df_frames_of(const mis_deepfilternet* c, int64_t n) { return 1 + (c->hop + n) / c->hop; }
static bool df_gru_served(int H) { return H == 32 || H == 64 || H == 128 || H == 256; }

extern "C" mis_status mis_deepfilternet_create(const mis_deepfilternet_config* cfg, int device, mis_deepfilternet** out) {
    MIS_API_BEGIN
    MIS_REQUIRE(cfg && out, MIS_ERR_INVALID_INPUT, "null argument");
    // the configuration is judged before the device is touched
    MIS_REQUIRE(cfg->sample_rate >= 1000 && cfg->sample_rate <= 192000, MIS_ERR_INVALID_INPUT, "sample_rate %d unsupported", cfg->sample_rate);
    MIS_REQUIRE(cfg->fft_size >= 4 && cfg->fft_size <= 4096 && cfg->fft_size % 2 == 0, MIS_ERR_INVALID_INPUT,
                "fft_size %d unsupported (even, 4..4096)", cfg->fft_size);
    MIS_REQUIRE(cfg->hop_size >= 1 && cfg->hop_size <= cfg->fft_size, MIS_ERR_INVALID_INPUT, "hop_size %d unsupported (1..fft_size)", cfg->hop_size);
    const int F = cfg->fft_size / 2 + 1;
    MIS_REQUIRE(cfg->nb_erb >= 4 && cfg->nb_erb <= DF_MAX_ERB && cfg->nb_erb % 4 == 0, MIS_ERR_INVALID_INPUT,
                "nb_erb %d unsupported (a multiple of 4, 4..%d)", cfg->nb_erb, DF_MAX_ERB);
    MIS_REQUIRE(cfg->nb_df >= 2 && cfg->nb_df <= F && cfg->nb_df % 2 == 0, MIS_ERR_INVALID_INPUT, "nb_df %d unsupported (even, 2..freq_bins)",
                cfg->nb_df);
    MIS_REQUIRE(cfg->df_order >= 1 && cfg->df_order <= 16 && cfg->df_lookahead >= 0 && cfg->df_lookahead < cfg->df_order, MIS_ERR_INVALID_INPUT,
                "df_order %d / df_lookahead %d unsupported (1..16, 0..df_order - 1)", cfg->df_order, cfg->df_lookahead);
    MIS_REQUIRE(cfg->conv_lookahead >= 0 && cfg->conv_lookahead <= 16, MIS_ERR_INVALID_INPUT, "conv_lookahead %d unsupported (0..16)",
                cfg->conv_lookahead);
    MIS_REQUIRE(cfg->conv_ch >= 1 && cfg->conv_ch <= 512, MIS_ERR_INVALID_INPUT, "conv_ch %d unsupported (1..512)", cfg->conv_ch);
    MIS_REQUIRE(df_gru_served(cfg->emb_hidden_dim) && df_gru_served(cfg->df_hidden_dim), MIS_ERR_INVALID_INPUT,
                "emb_hidden_dim %d / df_hidden_dim %d: the recurrence kernel is instantiated for hidden sizes 32, 64, 128 and 256 only",
                cfg->emb_hidden_dim, cfg->df_hidden_dim);
    MIS_REQUIRE(cfg->gru_kr == 0 || cfg->gru_kr == 64 || cfg->gru_kr == 96 || cfg->gru_kr == 128, MIS_ERR_INVALID_INPUT,
                "gru_kr %d: the register columns of Wh at hidden size 256 are 64, 96 or 128 (0: the default)", cfg->gru_kr);
    MIS_REQUIRE(cfg->norm_alpha > 0.0f && cfg->norm_alpha < 1.0f, MIS_ERR_INVALID_INPUT, "norm_alpha outside (0, 1)");
    MIS_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= DF_MAX_BATCH, MIS_ERR_INVALID_INPUT, "max_batch must be 1..%d", DF_MAX_BATCH);
    MIS_REQUIRE(cfg->max_samples >= 1 && cfg->max_samples <= ((int64_t)1 << 28), MIS_ERR_INVALID_INPUT, "max_samples must be 1..2^28");
    int64_t wsum = 0;
    for (int i = 0; i < cfg->nb_erb; ++i) { MIS_REQUIRE(cfg->erb_widths[i] >= 0, MIS_ERR_INVALID_INPUT, "erb_widths[%d] negative", i); wsum += cfg->erb_widths[i]; }
    MIS_REQUIRE(wsum == F, MIS_ERR_INVALID_INPUT, "erb_widths sum to %lld, freq_bins is %d", (long long)wsum, F);
    hipStream_t stream = mis_open_stream(device);
    auto c = std::make_unique<mis_deepfilternet>();
    c->device = device; c->cfg = *cfg; c->stream = stream;
    c->F = F; c->E = cfg->nb_erb; c->D = cfg->nb_df; c->N = cfg->fft_size; c->hop = cfg->hop_size;
    c->KR = cfg->gru_kr ? cfg->gru_kr : 96;                               // measured: 4.6 us a step against 5.2 (64) and 5.3 (128)
    c->wnorm = 1.0f / (float)(cfg->fft_size * cfg->fft_size) * (float)(2 * cfg->hop_size);
    c->Tcap = (int)df_frames_of(c.get(), cfg->max_samples);
    *out = c.release();
    MIS_API_END
}

extern "C" void mis_deepfilternet_destroy(mis_deepfilternet* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// names of the checkpoint as the reference reads them (enc.erb_conv0.1.weight, erb_dec.emb_gru.gru.weight_hh_l0, mask.erb_inv_fb, ...)
extern "C" mis_status mis_deepfilternet_set_tensor(mis_deepfilternet* c, const char* name, const void* data, mis_dtype dtype, const int64_t* shape,
                                                   int ndim) {
    MIS_API_BEGIN
    set_tensor_check(c, name, data, shape, ndim, 4, c && c->finalized, dtype);
    c->raw.put(name, data, dtype, shape, ndim);
    MIS_API_END
}

// ---------------------------------------------------------------------------- finalize: the chain as a list of launches
namespace {
struct DfBuilder {
    mis_deepfilternet* c;
    HostArena& a;
    size_t work_floats = 0;
    int new_buf(int F, int C) {
        DfBuf b; b.F = F; b.C = C; b.off = work_floats;
        work_floats += round_up((size_t)c->cfg.max_batch * c->Tcap * F * C, 64);
        c->bufs.push_back(b);
        return (int)c->bufs.size() - 1;
    }
    DfOp& new_op(int kind, int phase) {
        MIS_REQUIRE(c->ops.size() < c->ops.capacity(), MIS_ERR_GENERATION_FAILED, "DeepFilterNet: more launches than the list holds");
        c->ops.emplace_back();
        c->ops.back().kind = kind; c->ops.back().phase = phase;
        return c->ops.back();
    }
    void tap(int stage, int buf) { c->taps.push_back({stage, buf}); }
    const HostTensor& t4(const std::string& name) {
        const HostTensor& t = c->raw.need(name);
        MIS_REQUIRE(t.shape.size() == 4, MIS_ERR_INVALID_INPUT, "DeepFilterNet weight %s has the wrong shape (4 dimensions expected)", name.c_str());
        return t;
    }
    // inference BatchNorm (eps 1e-5) as scale + shift, formed in double
    void bn(const std::string& p, int64_t n, DfGemm& g) {
        const HostTensor &w = c->raw.need(p + ".weight", {n}), &b = c->raw.need(p + ".bias", {n}), &m = c->raw.need(p + ".running_mean", {n}),
                         &v = c->raw.need(p + ".running_var", {n});
        const size_t os = a.ftake(n, g.scale), ob = a.ftake(n, g.bias);
        for (int64_t i = 0; i < n; ++i) {
            const double s = (double)w.v[i] / sqrt((double)v.v[i] + 1e-5);
            a.fhost[os + i] = (float)s; a.fhost[ob + i] = (float)((double)b.v[i] - (double)m.v[i] * s);
        }
    }
    DfGemm base(int in, int out, int Fo) {
        DfGemm g{};
        g.Fo = Fo; g.mul = 1.0f; g.X = nullptr; g.ldx = c->bufs[in].F * c->bufs[in].C; g.ldy = c->bufs[out].C; g.N = c->bufs[out].C; g.ghs = g.N;
        g.Fin = c->bufs[in].F; g.Cin = c->bufs[in].C; g.kT = 1; g.kF = 1; g.fs = 1; g.ipg = 1; g.opg = 1;
        return g;
    }
    // conv block: main conv (grouped / depthwise / dense, or grouped transposed) [+ pointwise] + BatchNorm + activation [+ residual]
    int conv(const std::string& prefix, int main, int pw, int bnidx, int fs, bool transposed, int act, int in, int tshift, int res, int stage) {
        const DfBuf bi = c->bufs[in];
        const std::string mk = prefix + "." + std::to_string(main) + ".weight";
        const HostTensor& wm = t4(mk);
        const int64_t kT = wm.shape[2], kF = wm.shape[3];
        MIS_REQUIRE(kT >= 1 && kT <= 5 && (kF == 1 || kF == 3), MIS_ERR_INVALID_INPUT, "DeepFilterNet weight %s: a %lld x %lld kernel (time 1..5, "
                    "frequency 1 or 3 are served)", mk.c_str(), (long long)kT, (long long)kF);
        int64_t Cmid, ipg, opg, Fo;
        if (transposed) {
            MIS_REQUIRE(wm.shape[0] == bi.C && kT == 1, MIS_ERR_INVALID_INPUT, "DeepFilterNet weight %s: a transposed conv with one input "
                        "channel a group and a time kernel of 1 is served", mk.c_str());
            ipg = 1; opg = wm.shape[1]; Cmid = bi.C * opg;
            Fo = (bi.F - 1) * fs - 2 * (kF / 2) + (kF - 1) + kF / 2 + 1;
        } else {
            Cmid = wm.shape[0]; ipg = wm.shape[1];
            MIS_REQUIRE(ipg >= 1 && bi.C % ipg == 0 && Cmid % (bi.C / ipg) == 0, MIS_ERR_INVALID_INPUT,
                        "DeepFilterNet weight %s: %lld inputs a group do not divide %d channels", mk.c_str(), (long long)ipg, bi.C);
            opg = Cmid / (bi.C / ipg);
            Fo = (bi.F + 2 * (kF / 2) - kF) / fs + 1;
        }
        int64_t Cout = Cmid;
        const HostTensor* wp = nullptr;
        if (pw >= 0) {
            const std::string pk = prefix + "." + std::to_string(pw) + ".weight";
            wp = &t4(pk);
            MIS_REQUIRE(wp->shape[1] == Cmid && wp->shape[2] == 1 && wp->shape[3] == 1, MIS_ERR_INVALID_INPUT,
                        "DeepFilterNet weight %s has the wrong shape", pk.c_str());
            Cout = wp->shape[0];
        }
        MIS_REQUIRE(pw >= 0 || !transposed, MIS_ERR_INVALID_INPUT, "DeepFilterNet: %s has no pointwise conv", prefix.c_str());
        const int out = new_buf((int)Fo, (int)Cout);
        DfOp& op = new_op(0, DF_PH_NET);
        DfGemm& g = op.g;
        g = base(in, out, (int)Fo);
        g.kT = (int)kT; g.kF = (int)kF; g.fs = fs; g.tshift = tshift; g.act = act; g.ipg = (int)ipg; g.opg = (int)opg;
        if (wp) {
            g.load = transposed ? DF_LOAD_GCONVT : DF_LOAD_GCONV;
            g.K = (int)Cmid; g.gws = g.K;
            const size_t om = a.ftake(wm.v.size(), g.Wm), ow = a.ftake(wp->v.size(), g.W);
            std::copy(wm.v.begin(), wm.v.end(), a.fhost.begin() + om);
            std::copy(wp->v.begin(), wp->v.end(), a.fhost.begin() + ow);
        } else {                                                          // im2col: the groups as zeros of a dense [Cout][(dt kF + df) Cin + ci]
            g.load = DF_LOAD_IM2COL;
            g.K = (int)(kT * kF * bi.C); g.gws = g.K;
            const size_t ow = a.ftake((size_t)Cout * g.K, g.W);
            for (int64_t co = 0; co < Cout; ++co)
                for (int64_t ci = 0; ci < ipg; ++ci)
                    for (int64_t dt = 0; dt < kT; ++dt)
                        for (int64_t df = 0; df < kF; ++df)
                            a.fhost[ow + co * g.K + (dt * kF + df) * bi.C + (co / opg) * ipg + ci] = wm.v[((co * ipg + ci) * kT + dt) * kF + df];
        }
        bn(prefix + "." + std::to_string(bnidx), Cout, g);
        if (res >= 0) {
            MIS_REQUIRE(c->bufs[res].F == Fo && c->bufs[res].C == Cout, MIS_ERR_INVALID_INPUT,
                        "DeepFilterNet: the output of %s is [%lld, %lld] a frame, the tensor added to it [%d, %d]", prefix.c_str(), (long long)Fo,
                        (long long)Cout, c->bufs[res].F, c->bufs[res].C);
            g.ldr = (int)Cout;
        }
        op.in = in; op.res = res; op.out = out;
        if (stage >= 0) tap(stage, out);
        return out;
    }
    // grouped linear [G][in / G][out / G] (GroupedLinearEinsum) or dense [out][in] (+ bias)
    int linear(const std::string& name, bool grouped, const char* bias, int act, int in, int res, int stage, int phase = DF_PH_NET) {
        const DfBuf bi = c->bufs[in];
        const int64_t K = (int64_t)bi.F * bi.C;
        const HostTensor& w = c->raw.need(name);
        int64_t G, ws, hs;
        if (grouped) {
            MIS_REQUIRE(w.shape.size() == 3 && w.shape[0] * w.shape[1] == K, MIS_ERR_INVALID_INPUT,
                        "DeepFilterNet weight %s has the wrong shape ([groups, %lld / groups, out / groups] expected)", name.c_str(), (long long)K);
            G = w.shape[0]; ws = w.shape[1]; hs = w.shape[2];
        } else {
            MIS_REQUIRE(w.shape.size() == 2 && w.shape[1] == K, MIS_ERR_INVALID_INPUT, "DeepFilterNet weight %s has the wrong shape ([out, %lld] expected)",
                        name.c_str(), (long long)K);
            G = 1; ws = K; hs = w.shape[0];
        }
        const int64_t N = G * hs;
        const int out = new_buf(1, (int)N);
        DfOp& op = new_op(0, phase);
        DfGemm& g = op.g;
        g = base(in, out, 1);
        g.load = DF_LOAD_LIN; g.K = (int)K; g.gws = (int)ws; g.ghs = (int)hs; g.act = act;
        const size_t ow = a.ftake((size_t)N * ws, g.W);
        if (grouped) {
            for (int64_t gg = 0; gg < G; ++gg)
                for (int64_t i = 0; i < ws; ++i)
                    for (int64_t o = 0; o < hs; ++o) a.fhost[ow + (gg * hs + o) * ws + i] = w.v[(gg * ws + i) * hs + o];
        } else std::copy(w.v.begin(), w.v.end(), a.fhost.begin() + ow);
        if (bias) a.fvec(bias, {N}, N, g.bias);
        if (res >= 0) {
            MIS_REQUIRE((int64_t)c->bufs[res].F * c->bufs[res].C == N, MIS_ERR_INVALID_INPUT,
                        "DeepFilterNet: %s gives %lld values a frame, the tensor added to it has %d", name.c_str(), (long long)N,
                        c->bufs[res].F * c->bufs[res].C);
            g.ldr = (int)N;
        }
        op.in = in; op.res = res; op.out = out;
        if (stage >= 0) tap(stage, out);
        return out;
    }
};
}  // namespace

static int df_gru_layers(const mis_deepfilternet* c, const std::string& p) {
    int n = 0;
    while (c->raw.count(p + ".gru.weight_ih_l" + std::to_string(n))) ++n;
    return n;
}

extern "C" mis_status mis_deepfilternet_finalize(mis_deepfilternet* c) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    HIP_CHECK(hipSetDevice(c->device));
    const auto& cfg = c->cfg;
    const int64_t F = c->F, E = c->E, D = c->D, N = c->N, O = cfg.df_order;
    const double PI = 3.14159265358979323846;
    c->ops.clear(); c->bufs.clear(); c->taps.clear();
    c->ops.reserve(160);
    HostArena a(c->raw);
    std::vector<float>& fh = a.fhost;
    DfBuilder B{c, a};
    // the reference's initialiser asks for mask.erb_inv_fb first
    const float* inv = nullptr;
    a.fvec("mask.erb_inv_fb", {E, F}, E * F, inv);
    const HostTensor* efb = c->raw.find("erb_fb");
    const bool has_fb = efb && efb->shape == std::vector<int64_t>{F, E};
    // ---- tables: Vorbis window (the reference's f32 arithmetic), the transform pair formed in double
    const size_t o_win = a.ftake(N, c->win);
    for (int64_t i = 0; i < N; ++i) {
        const float inner = sinf(0.5f * (float)M_PI * ((float)i + 0.5f) / (float)std::max<int64_t>(1, N / 2));
        fh[o_win + i] = sinf(0.5f * (float)M_PI * inner * inner);
    }
    const float* dft = nullptr;
    const size_t o_dft = a.ftake((size_t)2 * F * N, dft), o_idft = a.ftake((size_t)N * 2 * F, c->idft);
    for (int64_t k = 0; k < F; ++k)
        for (int64_t n = 0; n < N; ++n) {
            const double ang = 2.0 * PI * (double)((k * n) % N) / (double)N;
            fh[o_dft + k * N + n] = (float)cos(ang); fh[o_dft + (F + k) * N + n] = (float)-sin(ang);
            const bool edge = k == 0 || k == N / 2;                    // irfft ignores the imaginary parts of DC and Nyquist
            fh[o_idft + n * 2 * F + k] = (float)((edge ? 1.0 : 2.0) * cos(ang) / (double)N);
            fh[o_idft + n * 2 * F + F + k] = edge ? 0.0f : (float)(-2.0 * sin(ang) / (double)N);
        }
    std::vector<int32_t> ih((size_t)round_up(E + 1, 64), 0);
    for (int i = 0; i < E; ++i) ih[i + 1] = ih[i] + cfg.erb_widths[i];
    // ---- 1. analysis
    const int b_spec = B.new_buf(1, (int)(2 * F));
    {
        DfOp& op = B.new_op(0, DF_PH_FRONT);
        DfGemm& g = op.g;
        g.Fo = 1; g.load = DF_LOAD_FRAME; g.K = (int)N; g.N = (int)(2 * F); g.gws = g.K; g.ghs = g.N; g.mul = c->wnorm; g.hop = c->hop; g.ldy = g.N;
        g.Fin = 1; g.Cin = 1; g.kT = 1; g.kF = 1; g.fs = 1; g.ipg = 1; g.opg = 1;
        a.bind(g.W, o_dft); a.bind(g.win, o_win);
        op.out = b_spec;
        B.tap(0, b_spec);
    }
    // ---- 2. features
    int b_erb = -1;
    if (has_fb) {
        b_erb = B.new_buf(1, (int)E);
        DfOp& op = B.new_op(0, DF_PH_FRONT);
        DfGemm& g = op.g;
        g = B.base(b_spec, b_erb, 1);
        g.load = DF_LOAD_MAGSQ; g.K = (int)F; g.gws = g.K; g.act = DF_ACT_LOG10;
        const size_t ow = a.ftake((size_t)E * F, g.W);
        for (int64_t e = 0; e < E; ++e) for (int64_t f = 0; f < F; ++f) fh[ow + e * F + f] = efb->v[f * E + e];
        op.in = b_spec; op.out = b_erb;
        B.tap(26, b_erb);
    }
    const int b_ferb = B.new_buf((int)E, 1), b_fspec = B.new_buf((int)D, 2);
    {
        DfOp& op = B.new_op(1, DF_PH_FRONT);
        op.n.F = (int)F; op.n.E = (int)E; op.n.D = (int)D; op.n.a = cfg.norm_alpha;
        op.in = b_spec; op.res = b_erb;
        c->b_spec = b_spec; c->b_ferb = b_ferb; c->b_fspec = b_fspec;
        B.tap(1, b_ferb); B.tap(2, b_fspec);
    }
    // ---- 3. encoder
    const int la = cfg.conv_lookahead;
    const int e0 = B.conv("enc.erb_conv0", 1, -1, 2, 1, false, DF_ACT_RELU, b_ferb, la, -1, 3);
    const int e1 = B.conv("enc.erb_conv1", 0, 1, 2, 2, false, DF_ACT_RELU, e0, 0, -1, 4);
    const int e2 = B.conv("enc.erb_conv2", 0, 1, 2, 2, false, DF_ACT_RELU, e1, 0, -1, 5);
    const int e3 = B.conv("enc.erb_conv3", 0, 1, 2, 1, false, DF_ACT_RELU, e2, 0, -1, 6);
    const int c0 = B.conv("enc.df_conv0", 1, 2, 3, 1, false, DF_ACT_RELU, b_fspec, la, -1, 7);
    const int c1 = B.conv("enc.df_conv1", 0, 1, 2, 2, false, DF_ACT_RELU, c0, 0, -1, 8);
    const int emb0 = B.linear("enc.df_fc_emb.0.weight", true, nullptr, DF_ACT_RELU, c1, e3, 9);
    // ---- 4. the three squeezed GRUs
    struct Chain { std::string prefix; int H, layers, x; };
    Chain ch[3] = {{"enc.emb_gru", cfg.emb_hidden_dim, 0, -1}, {"erb_dec.emb_gru", cfg.emb_hidden_dim, 0, -1}, {"df_dec.df_gru", cfg.df_hidden_dim, 0, -1}};
    struct GruW { const float *Wh, *WhT, *bhh; };
    std::vector<GruW> gw; gw.reserve(64);
    struct RecFix { int op, slot, gw, gx, out; };
    std::vector<RecFix> fix;
    auto open_chain = [&](int i, int in) {                                // grouped linear_in + ReLU; the layer count is the checkpoint's
        Chain& q = ch[i];
        q.layers = df_gru_layers(c, q.prefix);
        MIS_REQUIRE(q.layers >= 1 && q.layers <= 15, MIS_ERR_INVALID_INPUT, "DeepFilterNet: %s has %d GRU layers (1..15 are served)", q.prefix.c_str(), q.layers);
        q.x = B.linear(q.prefix + ".linear_in.0.weight", true, nullptr, DF_ACT_RELU, in, -1, 32 + 16 * i);
    };
    // layer l of the chains in `which` (one hidden size): Wx x + b_ih for all (row, frame) pairs, a contraction each; then ONE launch of
    // the recurrence, block = (row, chain)
    auto layer = [&](int l, std::initializer_list<int> which) {
        const std::string sl = std::to_string(l);
        int gx[2] = {-1, -1}, n = 0;
        for (int i : which) {
            Chain& q = ch[i];
            const int64_t H = q.H, in = (int64_t)c->bufs[q.x].F * c->bufs[q.x].C;
            c->raw.need(q.prefix + ".gru.weight_ih_l" + sl, {3 * H, in});
            const std::string bias = q.prefix + ".gru.bias_ih_l" + sl;
            gx[n++] = B.linear(q.prefix + ".gru.weight_ih_l" + sl, false, bias.c_str(), DF_ACT_NONE, q.x, -1, -1);
        }
        DfOp& op = B.new_op(2, DF_PH_REC);
        op.chains = n;
        n = 0;
        for (int i : which) {
            Chain& q = ch[i];
            const int64_t H = q.H;
            op.H = q.H;
            const HostTensor& wh = c->raw.need(q.prefix + ".gru.weight_hh_l" + sl, {3 * H, H});
            gw.emplace_back();
            GruW& w = gw.back();
            const size_t o1 = a.ftake((size_t)3 * H * H, w.Wh), o2 = a.ftake((size_t)3 * H * H, w.WhT);
            for (int64_t r = 0; r < 3 * H; ++r) for (int64_t k = 0; k < H; ++k) { fh[o1 + r * H + k] = wh.v[r * H + k]; fh[o2 + k * 3 * H + r] = wh.v[r * H + k]; }
            a.fvec(q.prefix + ".gru.bias_hh_l" + sl, {3 * H}, 3 * H, w.bhh);
            const int out = B.new_buf(1, q.H);
            fix.push_back({(int)c->ops.size() - 1, n, (int)gw.size() - 1, gx[n], out});
            ++n;
            B.tap(32 + 16 * i + 1 + l, out);
            q.x = out;
        }
    };
    open_chain(0, emb0);
    for (int l = 0; l < ch[0].layers; ++l) layer(l, {0});
    int emb = ch[0].x;
    if (c->raw.count("enc.emb_gru.linear_out.0.weight")) emb = B.linear("enc.emb_gru.linear_out.0.weight", true, nullptr, DF_ACT_RELU, emb, -1, -1);
    B.tap(10, emb);
    {
        const int lsnr = B.linear("enc.lsnr_fc.0.weight", false, "enc.lsnr_fc.0.bias", DF_ACT_LSNR, emb, -1, 11);
        c->ops.back().g.s0 = (float)(cfg.lsnr_max - cfg.lsnr_min); c->ops.back().g.s1 = (float)cfg.lsnr_min;
        MIS_REQUIRE(c->bufs[lsnr].C == 1, MIS_ERR_INVALID_INPUT, "DeepFilterNet weight enc.lsnr_fc.0.weight has the wrong shape");
        c->b_lsnr = lsnr;
    }
    open_chain(1, emb);
    open_chain(2, emb);
    for (int l = 0; l < std::max(ch[1].layers, ch[2].layers); ++l) {     // both decoder chains depend on emb alone
        const bool h1 = l < ch[1].layers, h2 = l < ch[2].layers;
        if (h1 && h2 && ch[1].H == ch[2].H) layer(l, {1, 2});
        else { if (h1) layer(l, {1}); if (h2) layer(l, {2}); }
    }
    // ---- 5. decoders
    int embd = ch[1].x;
    if (c->raw.count("erb_dec.emb_gru.linear_out.0.weight"))
        embd = B.linear("erb_dec.emb_gru.linear_out.0.weight", true, nullptr, DF_ACT_RELU, embd, -1, -1);
    B.tap(12, embd);
    {
        const DfBuf be3 = c->bufs[e3];
        MIS_REQUIRE(c->bufs[embd].C == be3.F * be3.C, MIS_ERR_INVALID_INPUT,
                    "DeepFilterNet: erb_dec.emb_gru gives %d values a frame, e3 holds %d x %d", c->bufs[embd].C, be3.F, be3.C);
        c->bufs[embd].F = be3.F; c->bufs[embd].C = be3.C;                // reshaped [f8, C]: the same memory
    }
    const int d3i = B.conv("erb_dec.conv3p", 0, -1, 1, 1, false, DF_ACT_RELU, e3, 0, embd, 13);
    const int d3 = B.conv("erb_dec.convt3", 0, 1, 2, 1, false, DF_ACT_RELU, d3i, 0, -1, 14);
    const int d2i = B.conv("erb_dec.conv2p", 0, -1, 1, 1, false, DF_ACT_RELU, e2, 0, d3, 15);
    const int d2 = B.conv("erb_dec.convt2", 0, 1, 2, 2, true, DF_ACT_RELU, d2i, 0, -1, 16);
    const int d1i = B.conv("erb_dec.conv1p", 0, -1, 1, 1, false, DF_ACT_RELU, e1, 0, d2, 17);
    const int d1 = B.conv("erb_dec.convt1", 0, 1, 2, 2, true, DF_ACT_RELU, d1i, 0, -1, 18);
    const int d0 = B.conv("erb_dec.conv0p", 0, -1, 1, 1, false, DF_ACT_RELU, e0, 0, d1, 19);
    const int mask = B.conv("erb_dec.conv0_out", 0, -1, 1, 1, false, DF_ACT_SIGMOID, d0, 0, -1, 20);
    MIS_REQUIRE(c->bufs[mask].F == E && c->bufs[mask].C == 1, MIS_ERR_INVALID_INPUT, "DeepFilterNet: the mask is [%d, %d] a frame, [%lld, 1] expected",
                c->bufs[mask].F, c->bufs[mask].C, (long long)E);
    int cdf = ch[2].x;
    if (c->raw.count("df_dec.df_skip.weight")) cdf = B.linear("df_dec.df_skip.weight", true, nullptr, DF_ACT_NONE, emb, cdf, -1);
    B.tap(21, cdf);
    const int c0p = B.conv("df_dec.df_convp", 1, 2, 3, 1, false, DF_ACT_RELU, c0, 0, -1, 22);
    MIS_REQUIRE(c->bufs[c0p].F == D && c->bufs[c0p].C == 2 * O, MIS_ERR_INVALID_INPUT, "DeepFilterNet: df_convp gives [%d, %d] a frame, [%lld, %lld] expected",
                c->bufs[c0p].F, c->bufs[c0p].C, (long long)D, (long long)(2 * O));
    const int coef = B.linear("df_dec.df_out.0.weight", true, nullptr, DF_ACT_TANH, cdf, c0p, 23);
    // ---- 6. synthesis
    const int b_enh = B.new_buf(1, (int)(2 * F));
    c->b_enh = b_enh;
    {
        DfOp& op = B.new_op(3, DF_PH_SYNTH);
        op.e.F = (int)F; op.e.E = (int)E; op.e.D = (int)D; op.e.order = (int)O; op.e.pad_left = (int)O - 1 - cfg.df_lookahead; op.e.wnorm = c->wnorm;
        op.in = mask; op.res = coef;
        B.tap(24, b_enh);
    }
    c->b_fr = B.new_buf(1, (int)N);
    {
        DfOp& op = B.new_op(0, DF_PH_SYNTH);
        DfGemm& g = op.g;
        g = B.base(b_enh, c->b_fr, 1);
        g.load = DF_LOAD_LIN; g.K = (int)(2 * F); g.gws = g.K;
        a.bind(g.W, o_idft); a.bind(g.cscale, o_win);
        op.in = b_enh; op.out = c->b_fr;
    }
    B.new_op(4, DF_PH_SYNTH);
    int nrec = 0;
    for (const DfOp& op : c->ops) nrec += op.kind == 2;
    MIS_REQUIRE(nrec <= DF_MAX_REC, MIS_ERR_INVALID_INPUT, "DeepFilterNet: %d recurrence launches a call, %d are served", nrec, DF_MAX_REC);
    // ---- the workspace, sized once.  No call reads the handle before finalized is set: a rejected finalize can be repeated.
    const size_t Bm = cfg.max_batch, wave_floats = round_up(Bm * (size_t)cfg.max_samples, 64);
    const size_t total = B.work_floats + wave_floats;
    MIS_REQUIRE((total + Bm * (size_t)cfg.max_samples) * 4 <= ((size_t)96 << 30), MIS_ERR_INVALID_INPUT,
                "max_batch x max_samples needs a workspace of %zu MiB (at most 96 GiB)", (total + Bm * (size_t)cfg.max_samples) * 4 >> 20);
    DevBuf<bf16_t> none;
    a.upload(none, c->farena);
    c->iarena.alloc(ih.size());
    HIP_CHECK(hipMemcpy(c->iarena.p, ih.data(), ih.size() * 4, hipMemcpyHostToDevice));
    c->wlo = c->iarena.p;
    c->work.alloc(total);
    c->pcm.alloc(Bm * (size_t)cfg.max_samples);
    c->counts.alloc(2 * DF_MAX_BATCH);
    c->h_counts.assign(2 * DF_MAX_BATCH, 0);
    for (DfBuf& b : c->bufs) b.p = c->work.p + b.off;
    DfBuf wv; wv.F = 1; wv.C = 1; wv.p = c->work.p + B.work_floats;
    c->bufs.push_back(wv);
    c->b_wave = (int)c->bufs.size() - 1;
    c->taps.push_back({25, c->b_wave});
    const int32_t *cnt = c->counts.p, *lens = c->counts.p + DF_MAX_BATCH;
    for (DfOp& op : c->ops) {
        if (op.kind == 0) {
            DfGemm& g = op.g;
            g.cnt = cnt; g.lens = lens; g.pcm = c->pcm.p;
            g.Y = c->bufs[op.out].p;
            if (op.in >= 0) g.X = c->bufs[op.in].p;
            if (op.res >= 0) g.R = c->bufs[op.res].p;
        } else if (op.kind == 1) {
            DfNorm& n = op.n;
            n.spec = c->bufs[op.in].p; n.erb = op.res >= 0 ? c->bufs[op.res].p : nullptr; n.wlo = c->wlo;
            n.feat_erb = c->bufs[b_ferb].p; n.feat_spec = c->bufs[b_fspec].p; n.cnt = cnt;
        } else if (op.kind == 2) {
            op.r.cnt = cnt;
        } else if (op.kind == 3) {
            DfEnh& e = op.e;
            e.spec = c->bufs[b_spec].p; e.mask = c->bufs[op.in].p; e.coef = c->bufs[op.res].p; e.inv = inv; e.enh = c->bufs[b_enh].p; e.cnt = cnt;
        }
    }
    for (const RecFix& f : fix) {
        DfGruChain& q = c->ops[f.op].r.ch[f.slot];
        c->ops[f.op].rgx[f.slot] = f.gx; c->ops[f.op].rout[f.slot] = f.out;
        q.gx = c->bufs[f.gx].p; q.Wh = gw[f.gw].Wh; q.WhT = gw[f.gw].WhT; q.bhh = gw[f.gw].bhh; q.out = c->bufs[f.out].p;
    }
    c->raw.clear();
    c->finalized = true;
    MIS_API_END
}

// mis-synth-v1 weights (benches): every key the chain reads at the shapes the configuration implies (DeepFilterNet3's layout: one
// encoder GRU layer, emb_num_layers - 1 in the ERB decoder, df_num_layers in the DF decoder; erb_fb and df_skip present)
extern "C" mis_status mis_deepfilternet_init_synthetic(mis_deepfilternet* c, uint64_t seed) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && !c->finalized, MIS_ERR_INVALID_INPUT, "bad handle");
    const auto& cfg = c->cfg;
    const int64_t C = cfg.conv_ch, E = c->E, D = c->D, F = c->F, O = cfg.df_order, H = cfg.emb_hidden_dim, Hd = cfg.df_hidden_dim;
    const int64_t G = std::max(1, cfg.linear_groups), Ge = std::max(1, cfg.enc_linear_groups), emb = C * E / 4;
    MIS_REQUIRE(emb % G == 0 && H % G == 0 && Hd % G == 0 && (C * D / 2) % Ge == 0 && emb % Ge == 0 && (D * O * 2) % G == 0, MIS_ERR_INVALID_INPUT,
                "synthetic weights: the group counts do not divide the widths");
    c->raw.clear();
    SynthWeights sw{c->raw, seed * 100000ull};
    auto bn = [&](const std::string& p, int64_t n) {
        sw.put(p + ".weight", {n}, 0.1, 1.0f); sw.put(p + ".bias", {n}, 0.05, 0.0f);
        sw.put(p + ".running_mean", {n}, 0.05, 0.0f); sw.put(p + ".running_var", {n}, 0.1, 1.0f);
    };
    auto conv = [&](const std::string& name, int64_t o, int64_t i, int64_t kt, int64_t kf, double gain) {
        sw.put(name, {o, i, kt, kf}, gain * sqrt(3.0 / (double)(i * kt * kf)), 0.0f);
    };
    auto glin = [&](const std::string& name, int64_t g, int64_t in, int64_t out) { sw.put(name, {g, in / g, out / g}, sqrt(3.0 / (double)(in / g)), 0.0f); };
    auto sgru = [&](const std::string& p, int64_t in, int64_t h, int layers, int64_t out) {
        glin(p + ".linear_in.0.weight", G, in, h);
        for (int l = 0; l < layers; ++l) {
            const std::string s = std::to_string(l);
            sw.put(p + ".gru.weight_ih_l" + s, {3 * h, h}, sqrt(3.0 / (double)h), 0.0f); sw.put(p + ".gru.weight_hh_l" + s, {3 * h, h}, sqrt(3.0 / (double)h), 0.0f);
            sw.put(p + ".gru.bias_ih_l" + s, {3 * h}, 0.05, 0.0f); sw.put(p + ".gru.bias_hh_l" + s, {3 * h}, 0.05, 0.0f);
        }
        if (out) glin(p + ".linear_out.0.weight", G, h, out);
    };
    const int64_t ki0 = cfg.conv_kernel_inp[0], ki1 = cfg.conv_kernel_inp[1], k0 = cfg.conv_kernel[0], k1 = cfg.conv_kernel[1];
    conv("enc.erb_conv0.1.weight", C, 1, ki0, ki1, 1.0); bn("enc.erb_conv0.2", C);
    for (int i = 1; i <= 3; ++i) {
        const std::string p = "enc.erb_conv" + std::to_string(i);
        conv(p + ".0.weight", C, 1, k0, k1, 1.0); conv(p + ".1.weight", C, C, 1, 1, 1.4); bn(p + ".2", C);
    }
    conv("enc.df_conv0.1.weight", C, 1, ki0, ki1, 1.0); conv("enc.df_conv0.2.weight", C, C, 1, 1, 1.4); bn("enc.df_conv0.3", C);
    conv("enc.df_conv1.0.weight", C, 1, k0, k1, 1.0); conv("enc.df_conv1.1.weight", C, C, 1, 1, 1.4); bn("enc.df_conv1.2", C);
    glin("enc.df_fc_emb.0.weight", Ge, C * D / 2, emb);
    sgru("enc.emb_gru", emb, H, 1, emb);
    sw.put("enc.lsnr_fc.0.weight", {1, emb}, sqrt(3.0 / (double)emb), 0.0f); sw.put("enc.lsnr_fc.0.bias", {1}, 0.05, 0.0f);
    sgru("erb_dec.emb_gru", emb, H, std::max(1, cfg.emb_num_layers - 1), emb);
    for (int i = 0; i <= 3; ++i) {
        const std::string p = "erb_dec.conv" + std::to_string(i) + "p";
        conv(p + ".0.weight", C, 1, 1, 1, 1.0); bn(p + ".1", C);
    }
    conv("erb_dec.convt3.0.weight", C, 1, k0, k1, 1.0); conv("erb_dec.convt3.1.weight", C, C, 1, 1, 1.4); bn("erb_dec.convt3.2", C);
    for (int i = 1; i <= 2; ++i) {
        const std::string p = "erb_dec.convt" + std::to_string(i);
        conv(p + ".0.weight", C, 1, cfg.convt_kernel[0], cfg.convt_kernel[1], 1.0); conv(p + ".1.weight", C, C, 1, 1, 1.4); bn(p + ".2", C);
    }
    conv("erb_dec.conv0_out.0.weight", 1, C, k0, k1, 1.0); bn("erb_dec.conv0_out.1", 1);
    sgru("df_dec.df_gru", emb, Hd, std::max(1, cfg.df_num_layers), 0);
    glin("df_dec.df_skip.weight", G, emb, Hd);
    int64_t gc = C, o2 = 2 * O;
    while (o2) { const int64_t r = gc % o2; gc = o2; o2 = r; }              // gcd(conv_ch, 2 df_order) groups
    conv("df_dec.df_convp.1.weight", 2 * O, C / gc, cfg.df_pathway_kernel_size_t, 1, 1.0); conv("df_dec.df_convp.2.weight", 2 * O, 2 * O, 1, 1, 1.4);
    bn("df_dec.df_convp.3", 2 * O);
    glin("df_dec.df_out.0.weight", G, Hd, D * O * 2);
    // the rectangular ERB filterbank of the widths and its inverse
    HostTensor fb, ifb;
    fb.shape = {F, E}; fb.v.assign((size_t)F * E, 0.0f); ifb.shape = {E, F}; ifb.v.assign((size_t)E * F, 0.0f);
    for (int64_t e = 0, f = 0; e < E; ++e)
        for (int w = 0; w < cfg.erb_widths[e]; ++w, ++f) { fb.v[f * E + e] = 1.0f / (float)cfg.erb_widths[e]; ifb.v[e * F + f] = 1.0f; }
    c->raw.put("erb_fb", std::move(fb)); c->raw.put("mask.erb_inv_fb", std::move(ifb));
    MIS_API_END
}

extern "C" int mis_deepfilternet_launches(const mis_deepfilternet* c) { return c ? c->last_launches : 0; }

extern "C" mis_status mis_deepfilternet_frames(const mis_deepfilternet* c, const int64_t* lens, int batch, int32_t* frames, int64_t* out_lens) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && lens && batch >= 0, MIS_ERR_INVALID_INPUT, "bad argument");
    for (int b = 0; b < batch; ++b) {
        MIS_REQUIRE(lens[b] >= 0 && lens[b] < ((int64_t)1 << 40), MIS_ERR_INVALID_INPUT, "row %d: bad length", b);
        const int64_t T = df_frames_of(c, lens[b]);
        MIS_REQUIRE(T < (1 << 30), MIS_ERR_INVALID_INPUT, "row %d: too many frames", b);
        if (frames) frames[b] = (int32_t)T;
        if (out_lens) out_lens[b] = lens[b];
    }
    MIS_API_END
}

// ---------------------------------------------------------------------------- a call
template <int H, int KR>
static void df_launch_gru(mis_deepfilternet* c, const DfOp& op, int B) {
    hipLaunchKernelGGL((k_dfn_gru<H, KR, false>), dim3(B, op.chains), dim3(3 * H), 0, c->stream, op.r);
}

static void df_run(mis_deepfilternet* c, const float* pcm, int64_t stride, int B, int nr, int64_t nmax, float* out, int64_t out_stride, float* lsnr,
                   int lsnr_rows) {
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->last_launches = 0; c->last_batch = 0;
    for (float& m : c->ms) m = 0.0f;
    MIS_REQUIRE(nr <= c->Tcap, MIS_ERR_INVALID_INPUT, "%d frames, the workspace holds %d (max_samples)", nr, c->Tcap);
    HIP_CHECK(hipMemcpyAsync(c->counts.p, c->h_counts.data(), c->h_counts.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(c->ev[0], s));
    const int64_t ns = std::max<int64_t>(nmax, 1);
    HIP_CHECK(hipMemcpy2DAsync(c->pcm.p, (size_t)ns * 4, pcm, (size_t)stride * 4, (size_t)ns * 4, B, hipMemcpyHostToDevice, s));
    int launches = 0, phase = DF_PH_FRONT, nrec = 0;
    for (DfOp& op : c->ops) {
        if (op.phase != DF_PH_REC && op.phase != phase) {                 // front -> net -> synth: events 1 and 2
            HIP_CHECK(hipEventRecord(c->ev[phase == DF_PH_FRONT ? 1 : 2], s));
            phase = op.phase;
        }
        if (op.kind == 0) {
            op.g.nr = nr; op.g.pcm_stride = ns;
            hipLaunchKernelGGL(k_dfn_gemm<false>, dim3(cdiv((int64_t)nr * op.g.Fo, 64), cdiv(op.g.N, 64), B), dim3(256), 0, s, op.g);
        } else if (op.kind == 1) {
            op.n.nr = nr;
            hipLaunchKernelGGL(k_dfn_norm<false>, dim3(B), dim3(256), 0, s, op.n);
        } else if (op.kind == 2) {
            op.r.nr = nr;
            HIP_CHECK(hipEventRecord(c->ev[4 + 2 * nrec], s));
            if (op.H == 32) df_launch_gru<32, 32>(c, op, B);
            else if (op.H == 64) df_launch_gru<64, 64>(c, op, B);
            else if (op.H == 128) df_launch_gru<128, 128>(c, op, B);
            else if (c->KR == 64) df_launch_gru<256, 64>(c, op, B);
            else if (c->KR == 96) df_launch_gru<256, 96>(c, op, B);
            else df_launch_gru<256, 128>(c, op, B);
            HIP_CHECK(hipEventRecord(c->ev[5 + 2 * nrec], s));
            ++nrec;
        } else if (op.kind == 3) {
            op.e.nr = nr; op.e.total = (size_t)B * nr * c->F;
            hipLaunchKernelGGL(k_dfn_enh<false>, dim3((unsigned)((op.e.total + 255) / 256)), dim3(256), 0, s, op.e);
        } else {
            hipLaunchKernelGGL(k_dfn_ola, dim3((unsigned)((ns + 255) / 256), B), dim3(256), 0, s, c->bufs[c->b_fr].p, c->win, c->bufs[c->b_wave].p,
                               c->counts.p, c->counts.p + DF_MAX_BATCH, nr, c->N, c->hop, ns);
        }
        ++launches;
    }
    HIP_CHECK(hipMemcpy2DAsync(out, (size_t)out_stride * 4, c->bufs[c->b_wave].p, (size_t)ns * 4, (size_t)std::min(ns, out_stride) * 4, B,
                               hipMemcpyDeviceToHost, s));
    if (lsnr) HIP_CHECK(hipMemcpy2DAsync(lsnr, (size_t)lsnr_rows * 4, c->bufs[c->b_lsnr].p, (size_t)nr * 4, (size_t)nr * 4, B, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(c->ev[3], s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));                               // the one synchronisation of a call
    float front = 0.0f, net = 0.0f, synth = 0.0f, rec = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&front, c->ev[0], c->ev[1]));
    HIP_CHECK(hipEventElapsedTime(&net, c->ev[1], c->ev[2]));
    HIP_CHECK(hipEventElapsedTime(&synth, c->ev[2], c->ev[3]));
    for (int i = 0; i < nrec; ++i) { float m = 0.0f; HIP_CHECK(hipEventElapsedTime(&m, c->ev[4 + 2 * i], c->ev[5 + 2 * i])); rec += m; }
    c->ms[0] = front; c->ms[1] = net - rec; c->ms[2] = rec; c->ms[3] = synth;
    c->last_batch = B; c->last_nr = nr; c->last_launches = launches; c->last_out = ns;
}

// pcm f32 [batch, stride], lens[batch] (NULL = stride) -> out f32 [batch, out_stride] (row b: lens[b] samples, zeros behind them),
// lsnr f32 [batch, lsnr_rows] (may be NULL)
extern "C" mis_status mis_deepfilternet_enhance(mis_deepfilternet* c, const float* pcm, const int64_t* lens, int batch, int64_t stride, float* out,
                                                int64_t out_stride, int64_t* out_lens, float* lsnr, int lsnr_rows) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && pcm && out, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->finalized, MIS_ERR_INVALID_INPUT, "DeepFilterNet model not finalized");
    MIS_REQUIRE(batch >= 1 && batch <= c->cfg.max_batch, MIS_ERR_INVALID_INPUT, "batch must be 1..%d (max_batch)", c->cfg.max_batch);
    MIS_REQUIRE(stride >= 1, MIS_ERR_INVALID_INPUT, "bad stride");
    int Tmax = 0;
    int64_t nmax = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = lens ? lens[b] : stride;
        MIS_REQUIRE(n >= 0 && n <= stride, MIS_ERR_INVALID_INPUT, "row %d: %lld samples, the row stride is %lld", b, (long long)n, (long long)stride);
        MIS_REQUIRE(n <= c->cfg.max_samples, MIS_ERR_INVALID_INPUT, "row %d: %lld samples, the workspace holds %lld (max_samples)", b, (long long)n,
                    (long long)c->cfg.max_samples);
        c->h_counts[b] = (int32_t)df_frames_of(c, n); c->h_counts[DF_MAX_BATCH + b] = (int32_t)n;
        Tmax = std::max(Tmax, c->h_counts[b]); nmax = std::max(nmax, n);
        if (out_lens) out_lens[b] = n;
    }
    MIS_REQUIRE(out_stride >= std::max<int64_t>(nmax, 1), MIS_ERR_INVALID_INPUT, "out: room for %lld samples a row, %lld are needed", (long long)out_stride,
                (long long)nmax);
    MIS_REQUIRE(!lsnr || lsnr_rows >= Tmax, MIS_ERR_INVALID_INPUT, "lsnr: room for %d frames, %d are needed", lsnr_rows, Tmax);
    df_run(c, pcm, stride, batch, Tmax, nmax, out, out_stride, lsnr, lsnr_rows);
    MIS_API_END
}

// tensors of the last call (include/mi_speech.h lists the stages)
extern "C" mis_status mis_deepfilternet_tap(mis_deepfilternet* c, int stage, float* out, int64_t capacity, int64_t* dims) {
    MIS_API_BEGIN
    MIS_REQUIRE(c, MIS_ERR_INVALID_INPUT, "null argument");
    MIS_REQUIRE(c->last_batch > 0, MIS_ERR_INVALID_INPUT, "no call to tap");
    const DfBuf* buf = nullptr;
    for (const DfTap& t : c->taps) if (t.stage == stage) buf = &c->bufs[t.buf];
    MIS_REQUIRE(buf, MIS_ERR_INVALID_INPUT, "bad stage %d (this model does not compute it)", stage);
    HIP_CHECK(hipSetDevice(c->device));
    const size_t B = c->last_batch, n = stage == 25 ? (size_t)c->last_out : (size_t)c->last_nr, width = (size_t)buf->F * buf->C;
    if (dims) { dims[0] = (int64_t)B; dims[1] = (int64_t)n; dims[2] = (int64_t)width; }
    if (!out) return MIS_OK;
    MIS_REQUIRE((int64_t)(B * n * width) <= capacity, MIS_ERR_INVALID_INPUT, "output capacity too small");
    HIP_CHECK(hipMemcpy(out, buf->p, B * n * width * 4, hipMemcpyDeviceToHost));
    MIS_API_END
}

// measurements: device milliseconds of the last call, ms[4] = front end (copy in + STFT + features), network without the recurrences,
// the recurrences, synthesis (+ copy out)
extern "C" mis_status mis_debug_deepfilternet_timing(const mis_deepfilternet* c, float* ms) {
    MIS_API_BEGIN
    MIS_REQUIRE(c && ms, MIS_ERR_INVALID_INPUT, "null argument");
    for (int i = 0; i < 4; ++i) ms[i] = c->ms[i];
    MIS_API_END
}
