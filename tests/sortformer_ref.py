"""CPU reference of Sortformer (csrc/sortformer.hip, mlx-audio-swift_amd/sortformer.py), written from the model's definition in torch,
float32 or float64 by `dtype`: the NeMo log-mel front end, the depthwise-striding Conv2d stem, the FastConformer block with the
LITERAL pad / reshape / slice rel-shift, the distance-indexed band form the device uses, the post-LN BART layer, the head, and the
streaming chain: streamingStep with its state update, generateStream's chunking and right context, and line-by-line transliterations
of maybeCompressState, the silence profile and both compressions.  Every function takes ONE row (the reference runs batch 1,
unmasked)."""
import math

import numpy as np
import torch
import torch.nn.functional as Fn


def synthetic_weights(cfg, seed, head_gain=1.0):
    """Sanitized names -> float32 numpy arrays, every key of the model; head_gain scales the speaker head so that the sigmoids move."""
    e, t, m = cfg.fc_encoder_config, cfg.tf_encoder_config, cfg.modules_config
    rng = np.random.default_rng(seed)
    W = {}
    C, d, f, k, dt, ft, S = e.subsampling_conv_channels, e.hidden_size, e.intermediate_size, e.conv_kernel_size, t.d_model, t.encoder_ffn_dim, m.num_speakers
    H, hd = e.num_attention_heads, e.hidden_size // e.num_attention_heads
    F3 = -(-e.num_mel_bins // 8)

    def put(name, shape, amp, plus=0.0):
        W[name] = (plus + rng.uniform(-amp, amp, shape)).astype(np.float32)

    def lin(p, o, i, bias=True, gain=1.0):
        put(p + ".weight", (o, i), gain * math.sqrt(3.0 / i))
        if bias:
            put(p + ".bias", (o,), 0.05)

    def norm(p, n):
        put(p + ".weight", (n,), 0.1, 1.0)
        put(p + ".bias", (n,), 0.05)

    SUB = "fc_encoder.subsampling."
    for n in ("layers_0", "layers_2", "layers_5"):
        put(SUB + n + ".weight", (C, 3, 3, 1), math.sqrt(3.0 / 9)); put(SUB + n + ".bias", (C,), 0.05)
    for n in ("layers_3", "layers_6"):
        put(SUB + n + ".weight", (C, 1, 1, C), math.sqrt(3.0 / C)); put(SUB + n + ".bias", (C,), 0.05)
    lin(SUB + "linear", d, C * F3)
    for i in range(e.num_hidden_layers):
        q = f"fc_encoder.layers.{i}."
        for n in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"):
            norm(q + n, d)
        for n in ("feed_forward1", "feed_forward2"):
            lin(q + n + ".linear1", f, d); lin(q + n + ".linear2", d, f, gain=0.5)
        for n in ("q_proj", "k_proj", "v_proj"):
            lin(q + "self_attn." + n, d, d, e.attention_bias)
        lin(q + "self_attn.o_proj", d, d, e.attention_bias, 0.5)
        lin(q + "self_attn.relative_k_proj", d, d, False)
        put(q + "self_attn.bias_u", (H, hd), 0.1); put(q + "self_attn.bias_v", (H, hd), 0.1)
        put(q + "conv.pointwise_conv1.weight", (2 * d, 1, d), math.sqrt(3.0 / d)); put(q + "conv.pointwise_conv1.bias", (2 * d,), 0.05)
        put(q + "conv.pointwise_conv2.weight", (d, 1, d), 0.5 * math.sqrt(3.0 / d)); put(q + "conv.pointwise_conv2.bias", (d,), 0.05)
        put(q + "conv.depthwise_conv.weight", (d, k, 1), math.sqrt(3.0 / k)); put(q + "conv.depthwise_conv.bias", (d,), 0.05)
        put(q + "conv.norm.weight", (d,), 0.1, 1.0); put(q + "conv.norm.bias", (d,), 0.05)
        put(q + "conv.norm.running_mean", (d,), 0.05); put(q + "conv.norm.running_var", (d,), 0.1, 1.0)
    put("tf_encoder.embed_positions.weight", (t.max_source_positions, dt), 0.1)
    for i in range(t.encoder_layers):
        q = f"tf_encoder.layers.{i}."
        lin(q + "self_attn.q_proj", dt, dt); lin(q + "self_attn.k_proj", dt, dt, t.k_proj_bias); lin(q + "self_attn.v_proj", dt, dt)
        lin(q + "self_attn.out_proj", dt, dt, gain=0.5)
        norm(q + "self_attn_layer_norm", dt); norm(q + "final_layer_norm", dt)
        lin(q + "fc1", ft, dt); lin(q + "fc2", dt, ft, gain=0.5)
    SM = "sortformer_modules."
    lin(SM + "encoder_proj", dt, d); lin(SM + "first_hidden_to_hidden", dt, dt)
    lin(SM + "single_hidden_to_spks", S, dt, gain=head_gain); lin(SM + "hidden_to_spks", S, 2 * dt)
    return W


# ---------------------------------------------------------------------------------------------------- front end
def hz_to_mel(f):
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def mel_to_hz(m):
    return (200.0 / 3.0) * m if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def mel_filters(n_mels, n_fft=512, sr=16000):
    """slaney scale, slaney norm: [n_fft / 2 + 1, n_mels], float64"""
    pts = [mel_to_hz(i * hz_to_mel(sr / 2) / (n_mels + 1)) for i in range(n_mels + 2)]
    fr = np.arange(n_fft // 2 + 1) * sr / n_fft
    fb = np.zeros((n_fft // 2 + 1, n_mels))
    for j in range(n_mels):
        lo, ce, hi = pts[j], pts[j + 1], pts[j + 2]
        up, down = (fr - lo) / (ce - lo), (hi - fr) / (hi - ce)
        fb[:, j] = np.maximum(0.0, np.minimum(up, down)) * 2.0 / (hi - lo)
    return fb


def features(wave, n_mels, dtype, peak_normalize=True, normalize=True, pad_to=16, preemph=0.97):
    """extractMelFeatures (+ generate's peak normalisation) of one row -> [F, n_mels] (time major)."""
    x = torch.as_tensor(np.asarray(wave, np.float32)).to(dtype)
    if peak_normalize:
        x = (1.0 / (x.abs().max() + 1e-3)) * x
    x = torch.cat([x[:1], x[1:] - preemph * x[:-1]])
    n = torch.arange(400, dtype=torch.float64)
    win = torch.zeros(512, dtype=torch.float64)
    win[56:456] = 0.5 * (1.0 - torch.cos(2.0 * math.pi * n / 399.0))
    xp = Fn.pad(x, (256, 256))
    F = 1 + x.numel() // 160
    frames = xp.unfold(0, 512, 160)[:F] * win.to(dtype)
    power = torch.fft.rfft(frames, dim=-1).abs() ** 2
    mel = torch.log(power @ torch.as_tensor(mel_filters(n_mels)).to(dtype) + 2.0 ** -24)
    if normalize:
        mean = mel.mean(dim=0, keepdim=True)
        var = ((mel - mean) ** 2).sum(dim=0, keepdim=True) / max(F - 1, 1)
        mel = (mel - mean) / (var.sqrt() + 1e-5)
    if pad_to > 0 and F % pad_to:
        mel = Fn.pad(mel, (0, 0, 0, pad_to - F % pad_to))
    return mel


# ---------------------------------------------------------------------------------------------------- model
class Ref:
    def __init__(self, cfg, weights, dtype):
        self.cfg, self.dtype = cfg, dtype
        self.W = {k: torch.as_tensor(np.asarray(v, np.float32)).to(dtype) for k, v in weights.items()}

    def lin(self, p, x):
        return Fn.linear(x, self.W[p + ".weight"], self.W.get(p + ".bias"))

    def ln(self, p, x, eps=1e-5):
        return Fn.layer_norm(x, x.shape[-1:], self.W[p + ".weight"], self.W[p + ".bias"], eps)

    # ConvSubsampling (:16-87): feats [F, mels] -> [T, hidden]
    def pre_encode(self, feats):
        W, S = self.W, "fc_encoder.subsampling."
        conv = lambda n, x, groups=1, stride=2, pad=1: Fn.conv2d(x, W[S + n + ".weight"].permute(0, 3, 1, 2), W[S + n + ".bias"], stride=stride,
                                                                 padding=pad, groups=groups)
        C = self.cfg.fc_encoder_config.subsampling_conv_channels
        h = feats[None, None]                                           # NCHW: H time, W mel
        h = torch.relu(conv("layers_0", h))
        h = torch.relu(conv("layers_3", conv("layers_2", h, C), 1, 1, 0))
        h = torch.relu(conv("layers_6", conv("layers_5", h, C), 1, 1, 0))
        h = h[0].permute(1, 0, 2).reshape(h.shape[2], -1)               # (t, c, f) -> (t, c f)
        return self.lin(S + "linear", h)

    def pos_emb(self, T):
        """RelPositionalEncoding (:90-116): [2 T - 1, d], positions T - 1 .. -(T - 1), interleaved sin / cos; angles in float64"""
        d = self.cfg.fc_encoder_config.hidden_size
        pos = torch.arange(T - 1, -T, -1, dtype=torch.float64)[:, None]
        div = torch.exp(torch.arange(0, d, 2, dtype=torch.float64) * (-math.log(10000.0) / d))[None]
        return torch.stack([torch.sin(pos * div), torch.cos(pos * div)], dim=-1).reshape(2 * T - 1, d).to(self.dtype)

    @staticmethod
    def rel_shift(x):
        """relShift (:150-157), literally: pad left, reshape, drop the first row, reshape.  x [H, T, 2 T - 1]"""
        H, q, p = x.shape
        x = Fn.pad(x, (1, 0)).reshape(H, p + 1, q)
        return x[:, 1:].reshape(H, q, p)

    def rel_scores(self, q, k, p, u, v, band=False):
        """q, k [H, T, hd], p [H, 2 T - 1, hd] -> scores [H, T, T] before the softmax"""
        T, hd = q.shape[1], q.shape[2]
        ac = (q + u[:, None]) @ k.transpose(1, 2)
        raw = (q + v[:, None]) @ p.transpose(1, 2)
        if band:                                                        # the device's form: the entry of distance i - j
            i = torch.arange(T)[:, None]
            j = torch.arange(T)[None]
            bd = torch.gather(raw, 2, ((T - 1) - (i - j))[None].expand(raw.shape[0], T, T))
        else:
            bd = self.rel_shift(raw)[:, :, :T]
        return (ac + bd) / math.sqrt(hd)

    def fc_attn(self, q_, x, band=False):
        e = self.cfg.fc_encoder_config
        T, H = x.shape[0], e.num_attention_heads
        hd = e.hidden_size // H
        sp = lambda y: y.reshape(-1, H, hd).transpose(0, 1)
        q, k, v = (sp(self.lin(q_ + n, x)) for n in ("q_proj", "k_proj", "v_proj"))
        p = sp(Fn.linear(self.pos_emb(T), self.W[q_ + "relative_k_proj.weight"]))
        s = self.rel_scores(q, k, p, self.W[q_ + "bias_u"], self.W[q_ + "bias_v"], band)
        o = (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(T, H * hd)
        return self.lin(q_ + "o_proj", o)

    def conv_module(self, q_, x):
        W = self.W
        k = self.cfg.fc_encoder_config.conv_kernel_size
        h = Fn.linear(x, W[q_ + "pointwise_conv1.weight"][:, 0], W[q_ + "pointwise_conv1.bias"])
        a, b = h.chunk(2, dim=-1)
        h = a * torch.sigmoid(b)
        h = Fn.conv1d(h.t()[None], W[q_ + "depthwise_conv.weight"].permute(0, 2, 1), W[q_ + "depthwise_conv.bias"], padding=(k - 1) // 2,
                      groups=h.shape[1])[0].t()
        h = (h - W[q_ + "norm.running_mean"]) / torch.sqrt(W[q_ + "norm.running_var"] + 1e-5) * W[q_ + "norm.weight"] + W[q_ + "norm.bias"]
        h = Fn.silu(h)
        return Fn.linear(h, W[q_ + "pointwise_conv2.weight"][:, 0], W[q_ + "pointwise_conv2.bias"])

    def fc_layer(self, i, x, band=False):
        q = f"fc_encoder.layers.{i}."
        ff = lambda n, y: self.lin(q + n + ".linear2", Fn.silu(self.lin(q + n + ".linear1", y)))
        r = x + 0.5 * ff("feed_forward1", self.ln(q + "norm_feed_forward1", x))
        r = r + self.fc_attn(q + "self_attn.", self.ln(q + "norm_self_att", r), band)
        r = r + self.conv_module(q + "conv.", self.ln(q + "norm_conv", r))
        r = r + 0.5 * ff("feed_forward2", self.ln(q + "norm_feed_forward2", r))
        return self.ln(q + "norm_out", r)

    def intake(self, emb):
        e = self.cfg.fc_encoder_config
        return emb * math.sqrt(e.hidden_size) if e.scale_input else emb

    def project(self, x):
        return self.lin("sortformer_modules.encoder_proj", x) + self.W["tf_encoder.embed_positions.weight"][: x.shape[0]]

    def tf_layer(self, i, x):
        t = self.cfg.tf_encoder_config
        q = f"tf_encoder.layers.{i}."
        T, H = x.shape[0], t.encoder_attention_heads
        hd = t.d_model // H
        sp = lambda y: y.reshape(T, H, hd).transpose(0, 1)
        qq, k, v = (sp(self.lin(q + "self_attn." + n, x)) for n in ("q_proj", "k_proj", "v_proj"))
        a = torch.softmax((qq * hd ** -0.5) @ k.transpose(1, 2), dim=-1) @ v
        h = self.ln(q + "self_attn_layer_norm", x + self.lin(q + "self_attn.out_proj", a.transpose(0, 1).reshape(T, H * hd)), t.layer_norm_eps)
        return self.ln(q + "final_layer_norm", h + self.lin(q + "fc2", torch.relu(self.lin(q + "fc1", h))), t.layer_norm_eps)

    def head(self, x):
        h = torch.relu(self.lin("sortformer_modules.first_hidden_to_hidden", torch.relu(x)))
        return torch.sigmoid(self.lin("sortformer_modules.single_hidden_to_spks", h))

    def stages_from_embeddings(self, emb):
        """[the Conformer blocks ..., the projection, the BART layers ..., the probabilities], each from the one before"""
        out, x = [], self.intake(emb)
        for i in range(self.cfg.fc_encoder_config.num_hidden_layers):
            x = self.fc_layer(i, x)
            out.append(x)
        x = self.project(x)
        out.append(x)
        for i in range(self.cfg.tf_encoder_config.encoder_layers):
            x = self.tf_layer(i, x)
            out.append(x)
        out.append(self.head(x))
        return out

    def encode(self, emb):
        return self.stages_from_embeddings(emb)[-1]

    def forward_features(self, feats):
        return self.encode(self.pre_encode(feats))

    def stage_after(self, stage, prev):
        """device stage `stage` (mis_sortformer_tap numbering, >= 1) computed from the DEVICE's stage - 1 tensor of one row"""
        L, Lt = self.cfg.fc_encoder_config.num_hidden_layers, self.cfg.tf_encoder_config.encoder_layers
        x = torch.as_tensor(np.asarray(prev, np.float32)).to(self.dtype)
        if stage == 1:
            return self.fc_layer(0, self.intake(x))
        if stage <= L:
            return self.fc_layer(stage - 1, x)
        if stage == L + 1:
            return self.project(x)
        if stage <= L + 1 + Lt:
            return self.tf_layer(stage - L - 2, x)
        return self.head(x)


# ---------------------------------------------------------------------------------------------------- compression, transliterated
def literal_compress_aosc(embs, preds, mean_sil, m):
    """compressSpkcacheAosc (:1216-1264) one statement at a time, with plain loops; ties of the top-k go to the lower flat index."""
    f32 = np.float32
    embs, preds = np.asarray(embs, f32)[0], np.asarray(preds, f32)[0]
    n, S = preds.shape
    L, sil = m.spkcache_len, m.spkcache_sil_frames_per_spk
    per = L // S - sil
    strong, weak, min_pos = (int(math.floor(f32(per) * f32(r))) for r in (m.strong_boost_rate, m.weak_boost_rate, m.min_pos_scores_rate))
    thr = f32(m.pred_score_threshold)
    scores = np.zeros((n, S), f32)
    for t in range(n):
        l1 = [np.log(max(f32(1.0) - preds[t, s], thr)) for s in range(S)]
        tot = f32(0)
        for v in l1:
            tot = f32(tot + v)
        for s in range(S):
            scores[t, s] = np.log(max(preds[t, s], thr)) - l1[s] + tot - f32(math.log(0.5))
    for s in range(S):
        for t in range(n):
            if not preds[t, s] > f32(0.5):
                scores[t, s] = -np.inf
        npos = sum(1 for t in range(n) if scores[t, s] > 0)
        if npos >= min_pos:
            for t in range(n):
                if preds[t, s] > f32(0.5) and not scores[t, s] > 0:
                    scores[t, s] = -np.inf
    if m.scores_boost_latest > 0 and n > L:
        for t in range(L, n):
            scores[t] = scores[t] + f32(m.scores_boost_latest)
    for nb, scale in ((strong, 2.0), (weak, 1.0)):
        if nb <= 0:
            continue
        k = min(nb, n)
        for s in range(S):
            order = sorted(range(n), key=lambda t: (-scores[t, s], t))[:k]
            for t in order:
                if scores[t, s] > -np.inf:
                    scores[t, s] = scores[t, s] + f32(-f32(scale) * f32(math.log(0.5)))
    if sil > 0:
        scores = np.concatenate([scores, np.full((sil, S), np.inf, f32)])
    nf = scores.shape[0]
    flat = [scores[t, s] for s in range(S) for t in range(nf)]
    k = min(L, len(flat))
    top = sorted(range(len(flat)), key=lambda i: (-flat[i], i))[:k]
    top = sorted(i if flat[i] > -np.inf else m.max_index for i in top)
    out_e, out_p = np.zeros((k, embs.shape[1]), f32), np.zeros((k, S), f32)
    for r, i in enumerate(top):
        t = i % nf
        if i == m.max_index or t >= nf - sil:
            out_e[r] = np.asarray(mean_sil, f32)[0]
        else:
            out_e[r], out_p[r] = embs[t], preds[t]
    return out_e[None], out_p[None]


def diar_frames(F):
    for _ in range(3):
        F = (F - 1) // 2 + 1
    return F


def test_wave(seed, n):
    """A row that is neither silent nor stationary: a few amplitude-modulated tones over noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    w = 0.02 * rng.standard_normal(n)
    for _ in range(4):
        f, fm, ph = rng.uniform(100, 3000), rng.uniform(0.5, 4.0), rng.uniform(0, 6.28)
        w += rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * f * t + ph) * (0.5 + 0.5 * np.sin(2 * np.pi * fm * t + ph))
    return w.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the tests' shapes
def case_config(name, max_batch=9, max_seconds=10, **modules):
    """A: stem 32 channels, 128 / 2 heads / 256 / 2 layers / 9 taps, then 48 / 2 heads (head 24) / 96 / 2 layers, 4 speakers.
    B: other widths: head size 32, 5 taps, k_proj_bias on, scale_input off, 20 mels (20 / 8 is no whole number).
    P: the published widths at 2 + 2 layers."""
    import mlx_audio_swift_amd as mas
    fc = dict(A=dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, intermediate_size=256, num_mel_bins=32,
                     conv_kernel_size=9, subsampling_conv_channels=32),
              B=dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, intermediate_size=96, num_mel_bins=20,
                     conv_kernel_size=5, subsampling_conv_channels=24, scale_input=False),
              P=dict(num_hidden_layers=2))[name]
    tf = dict(A=dict(d_model=48, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=96),
              B=dict(d_model=64, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=80, k_proj_bias=True, max_source_positions=200),
              P=dict(encoder_layers=2))[name]
    e, t = mas.FCEncoderConfig(**fc), mas.TFEncoderConfig(**tf)
    m = mas.ModulesConfig(fc_d_model=e.hidden_size, tf_d_model=t.d_model, **modules)
    return mas.SortformerConfig(fc_encoder_config=e, tf_encoder_config=t, modules_config=m,
                                processor_config=mas.ProcessorConfig(feature_size=e.num_mel_bins), max_batch=max_batch, max_seconds=max_seconds)


HEAD_GAIN = 6.0                    # synthetic speaker-head gain at which the sigmoids of DECISION_SEEDS cross the thresholds (test_sortformer_cpu)
DECISION_SEEDS = (11, 12, 13, 14, 15, 16, 17, 18)
DECISION_THRESHOLDS = (0.25, 0.5, 0.75)


def decision_row(seed):
    return test_wave(seed, 16000 * 2 + 137 * (seed % 5))


def exempt_mask(p64, p32, threshold):
    """entries whose float64 probability lies within ten times the row's largest float32-vs-float64 gap of the threshold"""
    m = 10.0 * float(np.abs(np.asarray(p32, np.float64) - np.asarray(p64, np.float64)).max())
    return np.abs(np.asarray(p64, np.float64) - threshold) <= m


# ---------------------------------------------------------------------------------------------------- the streaming chain
class State:
    """StreamingState as plain numpy arrays [1, n, width]; the functions below read attributes only, so they take the host's too."""

    def __init__(self, spkcache, spkcache_preds, fifo, fifo_preds, frames_processed, mean_sil_emb, n_sil_frames):
        self.spkcache, self.spkcache_preds, self.fifo, self.fifo_preds = spkcache, spkcache_preds, fifo, fifo_preds
        self.frames_processed, self.mean_sil_emb, self.n_sil_frames = frames_processed, mean_sil_emb, n_sil_frames


def init_state(d, n_spk):
    z = lambda *s: np.zeros(s, np.float32)
    return State(z(1, 0, d), z(1, 0, n_spk), z(1, 0, d), z(1, 0, n_spk), 0, z(1, d), z(1))


def literal_trim_silence(w, sr=16000, frame_ms=30, ratio=0.01, min_sec=0.5):
    fl = int(sr * frame_ms / 1000)
    need = max(3, int(min_sec * 1000 / frame_ms))
    n = len(w) // fl
    if n < 2 * need:
        return w, 0
    en = [float(np.sqrt(np.mean(np.square(w[i * fl:(i + 1) * fl], dtype=np.float32), dtype=np.float32))) for i in range(n)]
    thr = float(np.float32(max(en)) * np.float32(ratio))
    sp = [e > thr for e in en]
    start = next((i for i in range(n - need + 1) if all(sp[i:i + need])), 0)
    end = next((i + 1 for i in range(n - 1, need - 2, -1) if all(sp[i - need + 1:i + 1])), n)
    a, b = start * fl, min(end * fl, len(w))
    return (w, 0) if (a == 0 and b == len(w)) else (w[a:b], a)


def streaming_step(ref, chunk_feats, state, right=None):
    """streamingStep + updateStreamingState (:672-743, :992-1016) with the model in `ref`: chunk features [F, mels], a state of
    float32 arrays, right-context embeddings [1, r, d] or None -> (chunk probabilities [T, speakers], the new State), float32 arrays
    holding the reference's values."""
    m = ref.cfg.modules_config
    lc = m.chunk_left_context if m.use_aosc else 0
    rc = m.chunk_right_context if m.use_aosc else 0
    to = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(ref.dtype)
    chunk = ref.pre_encode(to(chunk_feats))
    n = chunk.shape[0]
    a, f = state.spkcache.shape[1], state.fifo.shape[1]
    parts = []
    if a > 0:
        parts.append(to(state.spkcache[0]))
    if f > 0:
        parts.append(to(state.fifo[0]))
    left = 0
    if lc > 0 and f > 0:
        left = min(lc, f)
        parts.append(to(state.fifo[0, f - left:]))
    parts.append(chunk)
    if right is not None and rc > 0 and right.shape[1] > 0:
        parts.append(to(right[0]))
    preds = ref.encode(torch.cat(parts)).numpy()
    c0 = a + f + left
    chunk_preds = preds[c0:c0 + n]
    cache_preds = preds[None, :a] if a > 0 else np.asarray(state.spkcache_preds)
    fifo_preds = preds[None, a:a + f] if f > 0 else np.asarray(state.fifo_preds)
    new = State(state.spkcache, cache_preds, np.concatenate([state.fifo, chunk.numpy()[None]], axis=1),
                np.concatenate([fifo_preds, chunk_preds[None]], axis=1), state.frames_processed + n, state.mean_sil_emb, state.n_sil_frames)
    return chunk_preds, new


def literal_compress_simple(embs, preds, target):
    """compressSpkcacheSimple (:1266-1280) with plain loops: frames sorted by the sum of log(clip(p, 1e-7, 1)) descending (ties: the
    earlier frame), the first `target` kept in time order."""
    f32 = np.float32
    p = np.asarray(preds, f32)[0]
    score = []
    for t in range(p.shape[0]):
        tot = f32(0)
        for s in range(p.shape[1]):
            tot = f32(tot + np.log(min(max(p[t, s], f32(1e-7)), f32(1.0))))
        score.append(tot)
    keep = sorted(sorted(range(len(score)), key=lambda t: (-score[t], t))[:target])
    return np.asarray(embs, f32)[:, keep], np.asarray(preds, f32)[:, keep]


def literal_maybe_compress_state(state, spkcache_max, fifo_max, m):
    """maybeCompressState (:1018-1084) with getSilenceProfile (:1088-1106), one statement at a time."""
    f32 = np.float32
    fifo_len = state.fifo.shape[1]
    if fifo_len <= fifo_max:
        return state
    pop = fifo_len - fifo_max
    if m.use_aosc:
        pop = min(pop, m.spkcache_update_period)
    p_embs, p_preds = np.asarray(state.fifo, f32)[:, :pop], np.asarray(state.fifo_preds, f32)[:, :pop]
    mean_sil, n_sil = np.asarray(state.mean_sil_emb, f32), np.asarray(state.n_sil_frames, f32)
    if m.use_aosc:
        count, total = f32(0), np.zeros(mean_sil.shape[1], f32)
        for t in range(pop):
            tot = f32(0)
            for s in range(p_preds.shape[2]):
                tot = f32(tot + p_preds[0, t, s])
            if tot < f32(m.sil_threshold):
                count = f32(count + 1)
                total = total + p_embs[0, t]
        upd = f32(n_sil[0] + count)
        mean_sil = ((mean_sil[0] * n_sil[0] + total) / max(upd, f32(1)))[None].astype(f32)
        n_sil = np.asarray([upd], f32)
    cache = np.concatenate([np.asarray(state.spkcache, f32), p_embs], axis=1)
    cache_preds = np.concatenate([np.asarray(state.spkcache_preds, f32), p_preds], axis=1)
    if cache.shape[1] > spkcache_max:
        if m.use_aosc:
            cache, cache_preds = literal_compress_aosc(cache, cache_preds, mean_sil, m)
        else:
            cache, cache_preds = literal_compress_simple(cache, cache_preds, spkcache_max)
    return State(cache, cache_preds, np.asarray(state.fifo)[:, pop:], np.asarray(state.fifo_preds)[:, pop:], state.frames_processed, mean_sil, n_sil)


def expected_lengths(cache_len, fifo_len, spkcache_max, fifo_max, m):
    """(cache length, FIFO length) behind maybeCompressState, from its definition"""
    if fifo_len <= fifo_max:
        return cache_len, fifo_len
    pop = fifo_len - fifo_max
    if m.use_aosc:
        pop = min(pop, m.spkcache_update_period)
    grown = cache_len + pop
    if grown > spkcache_max:
        grown = m.spkcache_len if m.use_aosc else spkcache_max
    return grown, fifo_len - pop


def stream_features(ref, wave):
    """the features generateStream cuts its chunks from (:854-879) and the trim offset in samples"""
    m, mels = ref.cfg.modules_config, ref.cfg.fc_encoder_config.num_mel_bins
    w, off = np.asarray(wave, np.float32), 0
    if not m.use_aosc:
        w, off = literal_trim_silence(w)
    return features(w, mels, ref.dtype, not m.use_aosc, not m.use_aosc, 0 if m.use_aosc else 16).numpy().astype(np.float32), off


def generate_stream(ref, wave, chunk_duration, spkcache_max, fifo_max, states=None, feats=None):
    """generateStream (:834-988): yields (chunk index, features slice, right context, state before the step, chunk probabilities, state
    behind the step, state behind the compression).  states: an iterator of the states to run each step FROM (a device run's); None:
    the reference's own chain.  feats: the features to cut the chunks from (a device run's); None: the reference's own."""
    m = ref.cfg.modules_config
    if feats is None:
        feats, _ = stream_features(ref, wave)
    total = feats.shape[0]
    chunk_mel = max(int(round(chunk_duration * 16000 / 160 / 8)) * 8, 8)
    rc = m.chunk_right_context
    all_pre = ref.pre_encode(torch.as_tensor(feats).to(ref.dtype)).numpy().astype(np.float32)[None] if (m.use_aosc and rc > 0) else None
    state = init_state(ref.cfg.fc_encoder_config.hidden_size, m.num_speakers)
    off, emb_off, idx = 0, 0, 0
    while off < total:
        end = min(off + chunk_mel, total)
        right = None
        if all_pre is not None:
            n_emb = diar_frames(end - off)
            a, b = emb_off + n_emb, min(emb_off + n_emb + rc, all_pre.shape[1])
            right = all_pre[:, a:b] if b > a else None
            emb_off += n_emb
        before = state if states is None else next(states)
        preds, new = streaming_step(ref, feats[off:end], before, right)
        after = literal_maybe_compress_state(new, spkcache_max, fifo_max, m)
        yield idx, (off, end), right, before, preds, new, after
        state, off, idx = after, end, idx + 1
