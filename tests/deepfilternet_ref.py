"""numpy reference of DeepFilterNet V2 / V3 offline enhancement (Sources/MLXAudioSTS/Models/DeepFilterNet of the reference), float64 by
default and float32 on request.  Every stage is a function of the previous stage's output, so a test can run it on the device's own
taps.  Layouts follow the engine: activations [T, F, C] (frame, frequency, channel), spec [T, 2 F] = re | im.

Where the engine uses another form than the reference, the reference's literal form is here as well: the closed-form normalisation
(ema_closed; band_mean_norm / band_unit_norm with closed=True), pad / conv / crop (conv2d), the per-group loop (conv_transpose2d) and the
at[].add overlap-add (istft)."""
import numpy as np


# ---------------------------------------------------------------------------------------------- the three cases
def case(name, **kw):
    import mlx_audio_swift_amd as mas
    if name == "S":      # tiny everywhere; no erb_fb, no df_skip; one df_gru layer fewer than erb_dec
        d = dict(fft_size=192, hop_size=96, nb_erb=16, nb_df=24, conv_ch=16, emb_hidden_dim=32, df_hidden_dim=32, linear_groups=4,
                 enc_linear_groups=4, df_order=5, df_lookahead=2, conv_lookahead=2, max_batch=8, max_seconds=0.7)
        layers, fb, skip = (1, 2, 1), False, False
    elif name == "W":    # the published GRU and group widths on small convs
        d = dict(fft_size=192, hop_size=96, nb_erb=32, nb_df=24, conv_ch=16, emb_hidden_dim=256, df_hidden_dim=256, gru_groups=8,
                 linear_groups=16, enc_linear_groups=16, max_batch=8, max_seconds=0.7)
        layers, fb, skip = (1, 2, 2), True, True
    else:                # P: the published DeepFilterNet3 shape
        d = dict(max_batch=1, max_seconds=0.1)
        layers, fb, skip = (1, 2, 2), True, True
    d.update(kw)
    cfg = mas.DeepFilterNetConfig(**d)
    return cfg, mas.deepfilternet_synthetic_weights(cfg, seed=sum(map(ord, name)), layers=layers, erb_fb=fb, df_skip=skip)


def rows(cfg, long_frames=300, seed=5):
    """Eight ragged rows: 0, 1, hop - 1, hop, hop + 1 samples, noise bursts on a noise floor, an all-zero row, a medium row."""
    rng = np.random.default_rng(seed)
    hop = cfg.hop_size

    def bursts(n):
        x = 0.01 * rng.standard_normal(n)
        for s in range(0, n, 7 * hop):
            m = min(3 * hop, n - s)
            x[s: s + m] += 0.3 * rng.standard_normal(m) * np.hanning(m) if m > 2 else 0
        return x.astype(np.float32)

    return [np.zeros(0, np.float32), bursts(1), bursts(hop - 1), bursts(hop), bursts(hop + 1), bursts(long_frames * hop + 17),
            np.zeros(9 * hop + 5, np.float32), bursts(40 * hop + 3)]


# ---------------------------------------------------------------------------------------------- layers
def vorbis_window(n, dtype=np.float64):
    i = np.arange(n, dtype=dtype)
    inner = np.sin(dtype(0.5) * dtype(np.pi) * (i + dtype(0.5)) / dtype(max(1, n // 2)))
    return np.sin(dtype(0.5) * dtype(np.pi) * inner * inner).astype(dtype)


def conv2d(x, w, fstride=1, lookahead=0):
    """conv2dLayer, literally: x [T, F, Cin], w torch [Cout, Cin / groups, kT, kF]; pad kT - 1 - lookahead rows in front (crop when
    negative), lookahead behind, kF / 2 in frequency; stride (1, fstride); groups = Cin / w.shape[1]."""
    T, F, Cin = x.shape
    Cout, ipg, kT, kF = w.shape
    groups = max(1, Cin // max(1, ipg))
    raw_left = kT - 1 - lookahead
    crop, left, right, fp = max(0, -raw_left), max(0, raw_left), max(0, lookahead), kF // 2
    if crop > 0 and T > crop:
        x = x[crop:]
    xp = np.pad(x, ((left, right), (fp, fp), (0, 0)))
    To, Fo = xp.shape[0] - kT + 1, (xp.shape[1] - kF) // fstride + 1
    opg = Cout // groups
    y = np.zeros((To, Fo, Cout), x.dtype)
    for g in range(groups):
        xg, wg = xp[:, :, g * ipg: (g + 1) * ipg], w[g * opg: (g + 1) * opg].astype(x.dtype)
        for dt in range(kT):
            for df in range(kF):
                patch = xg[dt: dt + To, df: df + (Fo - 1) * fstride + 1: fstride]          # [To, Fo, ipg]
                y[:, :, g * opg: (g + 1) * opg] += patch @ wg[:, :, dt, df].T
    return y


def conv_transpose2d(x, w, fstride, groups):
    """convTranspose2dLayer, the per-group loop: x [T, F, Cin], w torch [Cin, Cout / groups, kT, kF]; stride (1, fstride), padding
    (kT - 1, kF / 2), output_padding (0, kF / 2).  Time kernel 1 (what the engine serves)."""
    T, F, Cin = x.shape
    _, opg, kT, kF = w.shape
    assert kT == 1
    ipg, pad = Cin // groups, kF // 2
    Fo = (F - 1) * fstride - 2 * pad + (kF - 1) + pad + 1
    ys = []
    for g in range(groups):
        xg, wg = x[:, :, g * ipg: (g + 1) * ipg], w[g * ipg: (g + 1) * ipg].astype(x.dtype)
        full = np.zeros((T, (F - 1) * fstride + kF + pad, opg), x.dtype)
        for j in range(kF):
            full[:, j: j + (F - 1) * fstride + 1: fstride] += xg @ wg[:, :, 0, j]
        ys.append(full[:, pad: pad + Fo])
    return np.concatenate(ys, axis=2)


def batch_norm(x, W, p):
    d = x.dtype
    scale = W[p + ".weight"].astype(d) / np.sqrt(W[p + ".running_var"].astype(d) + d.type(1e-5))
    shift = W[p + ".bias"].astype(d) - W[p + ".running_mean"].astype(d) * scale
    return x * scale + shift


def grouped_linear(x, w):
    """groupedLinear: x [T, G ws], w [G, ws, hs] -> [T, G hs]."""
    G, ws, hs = w.shape
    out = np.zeros((x.shape[0], G, hs), x.dtype)
    xr = x.reshape(x.shape[0], G, ws)
    for g in range(G):
        out[:, g] = xr[:, g] @ w[g].astype(x.dtype)
    return out.reshape(x.shape[0], G * hs)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gru_layer(x, W, p, l):
    """pytorchGRULayer: gates r | z | n, n = tanh(xn + r (Wh_n h + b_hn)), h = (1 - z) n + z h, from the zero state."""
    d = x.dtype
    wih, whh = W[f"{p}.weight_ih_l{l}"].astype(d), W[f"{p}.weight_hh_l{l}"].astype(d)
    bih, bhh = W[f"{p}.bias_ih_l{l}"].astype(d), W[f"{p}.bias_hh_l{l}"].astype(d)
    H = whh.shape[1]
    gx = x @ wih.T + bih
    h, out = np.zeros(H, d), np.zeros((x.shape[0], H), d)
    for t in range(x.shape[0]):
        gh = h @ whh.T + bhh
        r, z = sigmoid(gx[t, :H] + gh[:H]), sigmoid(gx[t, H: 2 * H] + gh[H: 2 * H])
        n = np.tanh(gx[t, 2 * H:] + r * gh[2 * H:])
        h = (d.type(1) - z) * n + z * h
        out[t] = h
    return out


def n_layers(W, p):
    n = 0
    while f"{p}.gru.weight_ih_l{n}" in W:
        n += 1
    return n


# ---------------------------------------------------------------------------------------------- normalisation
def linspace(a, b, n, dtype):
    return np.array([a]) .astype(dtype) if n <= 1 else (dtype(a) + np.arange(n).astype(dtype) * ((dtype(b) - dtype(a)) / dtype(n - 1))).astype(dtype)


def ema(x, alpha, init):
    """s_t = a s_(t-1) + (1 - a) x_t, the state of frame t includes x_t."""
    d = x.dtype
    a, oma = d.type(alpha), d.type(1) - d.type(alpha)
    s, out = init.astype(d).copy(), np.zeros_like(x)
    for t in range(x.shape[0]):
        s = x[t] * oma + s * a
        out[t] = s
    return out


def ema_closed(x, alpha, init):
    """The reference's V2 / V3 closed form: a^t (init + (1 - a) cumsum(x / a^t))."""
    d = x.dtype
    a = d.type(alpha)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        powers = np.power(a, np.arange(x.shape[0]).astype(d)).astype(d)
        inv = (d.type(1) / powers).astype(d)
        accum = np.cumsum(x * inv[:, None], axis=0, dtype=d)
        return powers[:, None] * (init.astype(d)[None] + (d.type(1) - a) * accum)


def band_mean_norm(x, alpha, closed=False):
    d = x.dtype
    state = (ema_closed if closed else ema)(x, alpha, linspace(-60.0, -90.0, x.shape[1], d.type))
    return (x - state) / d.type(40)


def band_unit_norm(re, im, alpha, closed=False):
    d = re.dtype
    state = (ema_closed if closed else ema)(np.sqrt(re * re + im * im), alpha, linspace(0.001, 0.0001, re.shape[1], d.type))
    den = np.sqrt(np.maximum(state, d.type(1e-12)))
    return re / den, im / den


# ---------------------------------------------------------------------------------------------- the chain
class DeepFilterNetRef:
    def __init__(self, cfg, W, dtype=np.float64):
        self.cfg, self.d = cfg, np.dtype(dtype)
        self.W = {k: np.asarray(v, np.float32) for k, v in W.items()}
        self.win = vorbis_window(cfg.fft_size, np.float32).astype(dtype)       # the engine's table: the reference's float32 window
        self.wnorm = self.d.type(np.float32(cfg.wnorm))
        self.alpha = np.float32(cfg.norm_alpha)
        self.widths = cfg.erb_band_widths
        self.L = tuple(n_layers(self.W, p) for p in ("enc.emb_gru", "erb_dec.emb_gru", "df_dec.df_gru"))

    def w(self, k):
        return self.W[k].astype(self.d)

    def frames(self, n):
        return 1 + (self.cfg.hop_size + n) // self.cfg.hop_size

    # -- 1. analysis
    def stft(self, x):
        c = self.cfg
        T = self.frames(len(x))
        p = np.concatenate([np.zeros(c.hop_size, self.d), np.asarray(x, self.d), np.zeros(c.fft_size, self.d)])
        p = np.concatenate([p, np.zeros(max(0, (T - 1) * c.hop_size + c.fft_size - len(p)), self.d)])
        fr = np.stack([p[t * c.hop_size: t * c.hop_size + c.fft_size] for t in range(T)]) * self.win
        s = self._rfft32(fr) if self.d == np.float32 else np.fft.rfft(fr, axis=1)
        s = s * self.wnorm
        return np.concatenate([s.real, s.imag], axis=1).astype(self.d)

    def _rfft32(self, fr):
        N, F = self.cfg.fft_size, self.cfg.freq_bins
        ang = 2.0 * np.pi * ((np.arange(F)[:, None] * np.arange(N)[None]) % N) / N
        c, s = np.cos(ang).astype(np.float32), (-np.sin(ang)).astype(np.float32)
        return (fr @ c.T).astype(np.float32) + 1j * (fr @ s.T).astype(np.float32)

    def _irfft32(self, enh):
        N, F = self.cfg.fft_size, self.cfg.freq_bins
        ang = 2.0 * np.pi * ((np.arange(N)[:, None] * np.arange(F)[None]) % N) / N
        edge = (np.arange(F) == 0) | (np.arange(F) == N // 2)
        cr = (np.where(edge, 1.0, 2.0) * np.cos(ang) / N).astype(np.float32)
        ci = (np.where(edge, 0.0, -2.0) * np.sin(ang) / N).astype(np.float32)
        return (enh[:, :F] @ cr.T + enh[:, F:] @ ci.T).astype(np.float32)

    # -- 2. features
    def erb_db(self, spec):
        F = self.cfg.freq_bins
        mag = spec[:, :F] ** 2 + spec[:, F:] ** 2
        fb = self.W.get("erb_fb")
        if fb is not None and fb.shape == (F, self.cfg.nb_erb):
            e = mag @ fb.astype(self.d)
        else:
            cols, s = [], 0
            for wd in self.widths:
                cols.append(mag[:, s: s + wd].mean(axis=1, dtype=self.d) if wd > 0 else np.zeros(len(mag), self.d))
                s += wd
            e = np.stack(cols, axis=1)
        return (self.d.type(10) * np.log10(e + self.d.type(1e-10))).astype(self.d)

    def features(self, spec, erb_db=None, closed=False):
        F, D = self.cfg.freq_bins, self.cfg.nb_df
        fe = band_mean_norm(self.erb_db(spec) if erb_db is None else erb_db.astype(self.d), self.alpha, closed)
        re, im = band_unit_norm(spec[:, :D], spec[:, F: F + D], self.alpha, closed)
        return fe[:, :, None].astype(self.d), np.stack([re, im], axis=-1).astype(self.d)

    def lookahead(self, x):
        la = self.cfg.conv_lookahead
        if la <= 0 or x.shape[0] <= la:
            return x
        return np.concatenate([x[la:], np.zeros((la,) + x.shape[1:], x.dtype)])

    # -- 3. conv blocks
    def block(self, x, p, main, pw, bn, fstride=1, transposed=False, act="relu"):
        if transposed:
            y = conv_transpose2d(x, self.w(f"{p}.{main}.weight"), fstride, self.cfg.conv_ch)
        else:
            y = conv2d(x, self.w(f"{p}.{main}.weight"), fstride)
        if pw is not None:
            y = conv2d(y, self.w(f"{p}.{pw}.weight"))
        y = batch_norm(y, self.W, f"{p}.{bn}")
        return np.maximum(y, 0) if act == "relu" else sigmoid(y) if act == "sigmoid" else y

    def e0(self, feat_erb): return self.block(self.lookahead(feat_erb), "enc.erb_conv0", 1, None, 2)
    def e1(self, e0): return self.block(e0, "enc.erb_conv1", 0, 1, 2, 2)
    def e2(self, e1): return self.block(e1, "enc.erb_conv2", 0, 1, 2, 2)
    def e3(self, e2): return self.block(e2, "enc.erb_conv3", 0, 1, 2, 1)
    def c0(self, feat_spec): return self.block(self.lookahead(feat_spec), "enc.df_conv0", 1, 2, 3)
    def c1(self, c0): return self.block(c0, "enc.df_conv1", 0, 1, 2, 2)

    def emb0(self, e3, c1):
        T = e3.shape[0]
        return e3.reshape(T, -1) + np.maximum(grouped_linear(c1.reshape(T, -1), self.w("enc.df_fc_emb.0.weight")), 0)

    # -- 4. squeezed GRUs, one step at a time
    def linear_in(self, x, p): return np.maximum(grouped_linear(x, self.w(p + ".linear_in.0.weight")), 0)
    def gru(self, x, p, l): return gru_layer(x, {k: v.astype(self.d) for k, v in self.W.items() if k.startswith(p + ".gru.")}, p + ".gru", l)

    def linear_out(self, x, p):
        k = p + ".linear_out.0.weight"
        return np.maximum(grouped_linear(x, self.w(k)), 0) if k in self.W else x

    def squeezed(self, x, p, out=True):
        y = self.linear_in(x, p)
        for l in range(n_layers(self.W, p)):
            y = self.gru(y, p, l)
        return self.linear_out(y, p) if out else y

    def lsnr(self, emb):
        c = self.cfg
        v = emb @ self.w("enc.lsnr_fc.0.weight").T + self.w("enc.lsnr_fc.0.bias")
        return sigmoid(v) * self.d.type(c.lsnr_max - c.lsnr_min) + self.d.type(c.lsnr_min)

    # -- 5. decoders
    def pathway(self, e, i, up): return self.block(e, f"erb_dec.conv{i}p", 0, None, 1) + up
    def d3(self, d3i): return self.block(d3i, "erb_dec.convt3", 0, 1, 2)
    def d2(self, d2i): return np.maximum(self.block(d2i, "erb_dec.convt2", 0, 1, 2, 2, True, act=None), 0)
    def d1(self, d1i): return np.maximum(self.block(d1i, "erb_dec.convt1", 0, 1, 2, 2, True, act=None), 0)
    def mask(self, d0): return self.block(d0, "erb_dec.conv0_out", 0, None, 1, act="sigmoid")

    def df_skip(self, c, emb):
        k = "df_dec.df_skip.weight"
        return c + grouped_linear(emb, self.w(k)) if k in self.W else c

    def c0p(self, c0): return self.block(c0, "df_dec.df_convp", 1, 2, 3)

    def coefs(self, c, c0p):
        T = c.shape[0]
        return np.tanh(grouped_linear(c, self.w("df_dec.df_out.0.weight"))).reshape(T, self.cfg.nb_df, self.cfg.df_order * 2) + c0p

    # -- 6. synthesis
    def enhanced(self, spec, mask, coefs):
        """specEnhanced / wnorm: bins >= nb_df masked, bins < nb_df the deep filter of the unmasked spec (padded copy, as deepFilter)."""
        c, F, D, O = self.cfg, self.cfg.freq_bins, self.cfg.nb_df, self.cfg.df_order
        T = spec.shape[0]
        gains = mask.reshape(T, -1) @ self.w("mask.erb_inv_fb")
        re, im = spec[:, :F] * gains, spec[:, F:] * gains
        pl = O - 1 - c.df_lookahead
        pr_ = np.pad(spec[:, :D], ((pl, c.df_lookahead), (0, 0)))
        pi_ = np.pad(spec[:, F: F + D], ((pl, c.df_lookahead), (0, 0)))
        cf = coefs.reshape(T, D, O, 2)
        outr, outi = np.zeros((T, D), self.d), np.zeros((T, D), self.d)
        for k in range(O):
            sr, si, cr, ci = pr_[k: k + T], pi_[k: k + T], cf[:, :, k, 0], cf[:, :, k, 1]
            outr, outi = outr + (sr * cr - si * ci), outi + (sr * ci + si * cr)
        re[:, :D], im[:, :D] = outr, outi
        return (np.concatenate([re, im], axis=1) / self.wnorm).astype(self.d)

    def istft(self, enh, n):
        """MossFormer2DSP.istft with center = false and the at[].add overlap-add, then enhance's crop and clip."""
        c, F = self.cfg, self.cfg.freq_bins
        T = enh.shape[0]
        if self.d == np.float32:
            fr = self._irfft32(enh) * self.win
        else:
            fr = np.fft.irfft(enh[:, :F] + 1j * enh[:, F:], n=c.fft_size, axis=1) * self.win
        full = (T - 1) * c.hop_size + c.fft_size
        idx = (np.arange(T)[:, None] * c.hop_size + np.arange(c.fft_size)[None]).reshape(-1)
        out, ws = np.zeros(full, self.d), np.zeros(full, self.d)
        np.add.at(out, idx, fr.reshape(-1))
        np.add.at(ws, idx, np.tile(self.win * self.win, T))
        res = out / np.maximum(ws, self.d.type(1e-8))
        res = res[: n + c.hop_size + c.fft_size]
        delay = c.fft_size - c.hop_size
        return np.clip(res[delay: min(delay + n, len(res))], -1.0, 1.0).astype(self.d)

    # -- the whole chain; returns every stage by the engine's tap number
    def forward(self, x):
        t = {}
        t[0] = self.stft(x)
        t[1], t[2] = self.features(t[0])
        t[3] = self.e0(t[1]); t[4] = self.e1(t[3]); t[5] = self.e2(t[4]); t[6] = self.e3(t[5])
        t[7] = self.c0(t[2]); t[8] = self.c1(t[7])
        t[9] = self.emb0(t[6], t[8])
        t[10] = self.squeezed(t[9], "enc.emb_gru")
        t[11] = self.lsnr(t[10])
        T = t[9].shape[0]
        t[12] = self.squeezed(t[10], "erb_dec.emb_gru")
        t[13] = self.pathway(t[6], 3, t[12].reshape(t[6].shape)); t[14] = self.d3(t[13])
        t[15] = self.pathway(t[5], 2, t[14]); t[16] = self.d2(t[15])
        t[17] = self.pathway(t[4], 1, t[16]); t[18] = self.d1(t[17])
        t[19] = self.pathway(t[3], 0, t[18]); t[20] = self.mask(t[19])
        t[21] = self.df_skip(self.squeezed(t[10], "df_dec.df_gru", out=False), t[10])
        t[22] = self.c0p(t[7]); t[23] = self.coefs(t[21], t[22])
        t[24] = self.enhanced(t[0], t[20], t[23])
        t[25] = self.istft(t[24], len(x))
        return t
