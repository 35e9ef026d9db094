"""BigVGAN reference for the tests: a numpy model written from the reference's Swift (Sources/MLXAudioCodecs/BigVGAN), float64 by
default and float32 on request (`dtype`).  UpSample1d is the literal edge pad -> transposed depthwise conv -> crop, LowPassFilter1d the
literal edge pad -> strided depthwise conv (BigVGANLayers.swift:227-306); `aa_gather` is the closed gather form the device kernel
computes, and `aa_gather(..., mutate=True)` the wrong form that up-samples beyond the row instead of replicating the activated signal.
Weights are in the reference's layouts: conv weight_v [out, k, in] / weight_g [out, 1, 1], transposed conv weight_v [out, k, in] /
weight_g [1, 1, in].  Activations are [C, T] (one row)."""
import numpy as np


# ---------------------------------------------------------------------------------------------- filter
def _bessel_i0(x):
    y, term, total = x * x / 4.0, 1.0, 1.0
    for k in range(1, 41):
        term *= y / (k * k)
        total += term
        if term < 1e-12 * total:
            break
    return total


def kaiser_sinc_filter(cutoff=0.25, half_width=0.3, kernel_size=12):
    """bigVGANKaiserSincFilter1d (BigVGANLayers.swift:47-81) in float64."""
    half = kernel_size // 2
    a = 2.285 * max(half - 1, 0) * np.pi * 4.0 * half_width + 7.95
    beta = 0.1102 * (a - 8.7) if a > 50.0 else (0.5842 * (a - 21.0) ** 0.4 + 0.07886 * (a - 21.0) if a >= 21.0 else 0.0)
    h = (kernel_size - 1) / 2.0
    f = np.zeros(kernel_size)
    for i in range(kernel_size):
        ratio = (i - h) / h
        win = _bessel_i0(beta * np.sqrt(max(0.0, 1.0 - ratio * ratio))) / _bessel_i0(beta)
        t = (i - half) + (0.5 if kernel_size % 2 == 0 else 0.0)
        x = 2.0 * cutoff * t
        f[i] = 2.0 * cutoff * win * (1.0 if abs(x) < 1e-12 else np.sin(np.pi * x) / (np.pi * x))
    return f / max(f.sum(), 1e-12)


FILTER = kaiser_sinc_filter()


# ---------------------------------------------------------------------------------------------- Activation1d
def upsample1d(x, f):
    """BigVGANUpSample1d (:267-306), ratio 2, kernel 12: pad 5 / 5 (edge), transposed conv stride 2, x 2, crop 15 / 15."""
    C, T = x.shape
    xp = np.pad(x, ((0, 0), (5, 5)), mode="edge")
    w = np.zeros((C, 2 * (T + 10 - 1) + 12), x.dtype)
    for i in range(T + 10):
        w[:, 2 * i: 2 * i + 12] += xp[:, i: i + 1] * f[None, :]
    w = x.dtype.type(2.0) * w
    return w[:, 15: w.shape[1] - 15]


def downsample1d(v, f):
    """BigVGANLowPassFilter1d (:227-265), stride 2, kernel 12: pad 5 / 6 (edge), strided depthwise conv."""
    C, n = v.shape
    vp = np.pad(v, ((0, 0), (5, 6)), mode="edge")
    T = (n + 11 - 12) // 2 + 1
    y = np.zeros((C, T), v.dtype)
    for j in range(12):
        y += f[j] * vp[:, j: j + 2 * T: 2]
    return y


def snake(u, alpha, beta):
    """BigVGANPeriodicActivation (:83-111) on the values the activation uses (after any exp())."""
    dt = u.dtype.type
    s = np.sin(u * alpha[:, None])
    return u + (dt(1.0) / (beta[:, None] + dt(1e-9))) * (s * s)


def activation1d(x, alpha, beta, f=None):
    f = FILTER.astype(x.dtype) if f is None else f
    return downsample1d(snake(upsample1d(x, f), alpha, beta), f)


def aa_gather(x, alpha, beta, f=None, mutate=False):
    """The closed form: u[n] = 2 sum_i f[n + 15 - 2 i] x[clamp(i - 5, 0, T - 1)], v = snake(u), y[t] = sum_j f[j] v[clamp(2 t + j - 5, 0,
    2 T - 1)].  mutate: v is NOT clamped - u is formed beyond the row from the replicated x (the mistake the two-clamp rule names)."""
    f = FILTER.astype(x.dtype) if f is None else f
    C, T = x.shape

    def u_at(n):                                                         # the six i with 0 <= n + 15 - 2 i <= 11, ascending
        acc = np.zeros(C, x.dtype)
        for tap in range(11, -1, -1):
            if (n + 15 - tap) % 2 == 0:
                i = (n + 15 - tap) // 2
                acc = acc + f[tap] * x[:, min(max(i - 5, 0), T - 1)]
        return x.dtype.type(2.0) * acc

    lo, hi = (-5, 2 * T + 6) if mutate else (0, 2 * T)
    v = {n: snake(u_at(n)[:, None], alpha, beta)[:, 0] for n in range(lo, hi)}
    y = np.zeros((C, T), x.dtype)
    for t in range(T):
        acc = np.zeros(C, x.dtype)
        for j in range(12):
            n = 2 * t + j - 5
            acc = acc + f[j] * v[n if mutate else min(max(n, 0), 2 * T - 1)]
        y[:, t] = acc
    return y


# ---------------------------------------------------------------------------------------------- convs
def wn_conv_weight(g, v):
    """g v / (|v| + 1e-12), the norm over everything but the output channel (BigVGANWNConv1d, :151-152); float64."""
    v = np.asarray(v, np.float64)
    n = np.sqrt((v * v).sum(axis=(1, 2), keepdims=True))
    return np.asarray(g, np.float64).reshape(-1, 1, 1) * v / (n + 1e-12)


def wn_convt_weight(g, v):
    """the norm per input channel (exceptDim 2, :210)."""
    v = np.asarray(v, np.float64)
    n = np.sqrt((v * v).sum(axis=(0, 1), keepdims=True))
    return np.asarray(g, np.float64).reshape(1, 1, -1) * v / (n + 1e-12)


def conv1d_same(x, w, bias, dil=1):
    """x [Cin, T], w [out, k, in], zero padding ((k - 1) dil) / 2 each side."""
    out, k, cin = w.shape
    T, pad = x.shape[1], (k - 1) * dil // 2
    xp = np.pad(x, ((0, 0), (pad, pad)))
    y = np.zeros((out, T), x.dtype)
    for j in range(k):
        y += w[:, j, :] @ xp[:, j * dil: j * dil + T]
    return y if bias is None else y + bias[:, None]


def conv_transpose1d(x, w, bias, stride):
    """x [Cin, T], w [out, k, in], padding (k - stride) / 2: y[i stride - pad + j] += w[:, j, :] x[:, i]."""
    out, k, cin = w.shape
    T, pad = x.shape[1], (k - stride) // 2
    full = np.zeros((out, (T - 1) * stride + k), x.dtype)
    for j in range(k):
        full[:, j: j + (T - 1) * stride + 1: stride] += w[:, j, :] @ x
    y = full[:, pad: full.shape[1] - pad]
    return y + bias[:, None]


# ---------------------------------------------------------------------------------------------- the model
class BigVGANRef:
    """cfg: an object with BigVGANConfig's fields; weights: name -> array in the reference's layouts.  Every method takes and returns one
    row [C, T] in `dtype`; forward returns (taps in the engine's order, waveform [T hop])."""

    def __init__(self, cfg, weights, dtype=np.float64):
        self.cfg, self.dt = cfg, np.dtype(dtype)
        self.w, self._fold = weights, {}
        self.f = FILTER.astype(self.dt)
        self.nk, self.ns = len(cfg.resblock_kernel_sizes), len(cfg.upsample_rates)

    def _folded(self, p, fold):
        if p not in self._fold:
            self._fold[p] = fold(self.w[p + ".weight_g"], self.w[p + ".weight_v"]).astype(self.dt)
        return self._fold[p]

    def _conv(self, p, x, dil=1, bias=True):
        return conv1d_same(x, self._folded(p, wn_conv_weight), self.w[p + ".bias"].astype(self.dt) if bias else None, dil)

    def _act(self, p, x):
        a = np.asarray(self.w[p + ".act.alpha"], np.float64)
        b = np.asarray(self.w[p + ".act.beta"], np.float64) if self.cfg.activation == "snakebeta" else a
        if self.cfg.snake_logscale:
            a, b = np.exp(a), np.exp(b)
        return activation1d(x, a.astype(self.dt), b.astype(self.dt), self.f)

    def max_rbeta(self, prefixes):
        """max 1 / beta over the activations under the given key prefixes (the Snake term of the gates)."""
        m = 0.0
        for k, v in self.w.items():
            if k.startswith(tuple(prefixes)) and k.endswith(".act.alpha"):
                b = np.asarray(self.w[k[:-5] + "beta"] if self.cfg.activation == "snakebeta" else v, np.float64)
                b = np.exp(b) if self.cfg.snake_logscale else b
                m = max(m, float((1.0 / (b + 1e-9)).max()))
        return m

    def conv_pre(self, mel):
        return self._conv("conv_pre", mel.astype(self.dt))

    def up(self, i, x):
        p = f"ups.{i}.0"
        return conv_transpose1d(x.astype(self.dt), self._folded(p, wn_convt_weight), self.w[p + ".bias"].astype(self.dt), self.cfg.upsample_rates[i])

    def block(self, i, j, x):
        q = f"resblocks.{i * self.nk + j}"
        out = x.astype(self.dt)
        for d, dil in enumerate(self.cfg.resblock_dilation_sizes[j]):
            if str(self.cfg.resblock) == "1":
                h = self._conv(f"{q}.convs1.{d}", self._act(f"{q}.activations.{2 * d}", out), dil)
                out = out + self._conv(f"{q}.convs2.{d}", self._act(f"{q}.activations.{2 * d + 1}", h))
            else:
                out = out + self._conv(f"{q}.convs.{d}", self._act(f"{q}.activations.{d}", out), dil)
        return out

    def mean(self, blocks):
        s = blocks[0].astype(self.dt)
        for b in blocks[1:]:
            s = s + b.astype(self.dt)
        return s / self.dt.type(len(blocks))

    def act_post(self, x):
        return self._act("activation_post", x.astype(self.dt))

    def final(self, x):
        y = self._conv("conv_post", x.astype(self.dt), bias=bool(self.cfg.use_bias_at_final))[0]
        return np.tanh(y) if self.cfg.use_tanh_at_final else np.clip(y, -1.0, 1.0).astype(self.dt)

    def forward(self, mel):
        taps = [self.conv_pre(mel)]
        h = taps[0]
        for i in range(self.ns):
            u = self.up(i, h)
            blocks = [self.block(i, j, u) for j in range(self.nk)]
            h = self.mean(blocks)
            taps += [u] + blocks + [h]
        taps.append(self.act_post(h))
        return taps, self.final(taps[-1])

    def step(self, stage, taps, mel):
        """The engine's tap `stage` recomputed from the given previous taps (the device's own): what one stage of the chain computes."""
        n = self.nk + 2
        if stage == 0:
            return self.conv_pre(mel)
        if stage == 1 + self.ns * n:
            return self.act_post(taps[stage - 1])
        i, r = divmod(stage - 1, n)
        base = 1 + i * n
        if r == 0:
            return self.up(i, taps[base - 1])
        if r == self.nk + 1:
            return self.mean(taps[base + 1: base + 1 + self.nk])
        return self.block(i, r - 1, taps[base])
