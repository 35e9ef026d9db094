"""Operator-level reference of the private kernels of csrc/moonshine.hip (k_ms_conv1_tanh, k_ms_gn_partial<0|1> / k_ms_gn_final / k_ms_gn_apply,
k_ms_rope_rows, k_ms_attn_enc / _self / _cross, k_ms_gemv<LN, EPI>, k_ms_embed, k_ms_argmax_embed), inputs whose result is known exactly, the
case tables of tests/test_gpu_moonshine_ops.py and thin wrappers of the mis_debug_moonshine_* entry points (include/mi_speech_debug.h).  Pure
numpy, float64, written from the kernel header comments and MoonshineModel.swift; nothing here calls a kernel to build its data.
tests/test_moonshine_ops_ref_cpu.py proves every claim below that the GPU test leans on.

Specification, T() = round to bf16 (gemm_ref.T), u = 2^-24:
  conv1      out[b][t][c] = tanh(sum_k w[c][k] pcm[b][64 t + k]) for t < T1[b], 0 for T1[b] <= t < T1pad (float32, weights as [127][d])
  GroupNorm  chunks of 32768 elements of the row's own T1[b] d values, nch = ceil(max T1 d / 32768): part0[b][ch] = sum of the chunk,
             mean = (sum_ch part0) / n, part1[b][ch] = sum (x - mean)^2, stats = (mean, 1 / sqrt(sum_ch part1 / n + 1e-5f)), chunks behind the
             row: 0;  y = T((x - mean) rstd gw[c] + gb[c]) for t < T1[b], 0 behind, in the tail of 8 d elements and for the tail's rows >= B
  RoPE       heads 0 .. nheads - 1 of 64 columns, position p = m % Tpad, i < rot / 2: y[2i] = T(x[2i] c[p][i] - x[2i+1] s[p][i]),
             y[2i+1] = T(x[2i+1] c[p][i] + x[2i] s[p][i]); every other column (>= rot, v heads, padding) untouched
  attention  out = T(sum_j p_j v_j), p = softmax over the keys j < n of scale q . k_j, kv head h // (H / Hkv), one wave a query
             encoder: rows [B Tpad][ld] = q | k | v heads, n = T3[b], queries t >= n: zero;  cross: q [B][H 64], kv [B Tpad][2 Hkv 64];
             self: q, k = RoPE at `pos` of the new token's q, k; k, v written to row `pos` of the caches [B][Hkv][Smax][64] (once per kv
             head), keys 0 .. pos
  gemv       xs = X, or LN: T((x - mean) rstd lnw) with two-pass float32 statistics, eps 1e-5; acc[b][n] = sum_k xs[b][k] W[n][k];
             MS_BF16 T(acc + bias);  MS_RESID h = T(T(acc + bias) + h);  MS_GATE T(T(silu(g)) a), a = T(acc[n] + bias[n]),
             g = T(acc[n + F] + bias[n + F]), output [B][F];  MS_F32 acc, float32, no bias
  embed      h[b] = E[ids[b]], an id outside 0 .. vocab - 1 reads row 0
  arg-max    id = lowest index of the row's maximum (NaN never compares; no comparable value: 0); an ACTIVE row: id == eos ends it (active 0,
             done_count + 1, nothing kept), else tokens[b][n_gen] = id where n_gen < stride and n_gen + 1 in any case; h[b] = E[id] always

Tiers.  The exact tiers are compared bit for bit, and every one of their float32 sums is exact in any order (integers, or one non-zero term):
  conv1 exact: one +-1 tap per channel (taps 0, 63, 64, 126 among them), samples in {0, +-16}: the sum is 0 or +-16 and float32 tanh(16) == 1
    (it saturates above about 9.01: 1 - tanh(16) = 2.5e-14, a millionth of half a float32 ulp); samples behind the row's own extent (T1 - 1) 64 + 127 hold 3e4.
  conv1 Gaussian: |out - tanh64(a)| <= SAFETY gamma_127 sum |w x| (1 - tanh^2(|a| - that)) + TANH_ULP ulp_f32(tanh a).  TANH_ULP: the ROCm
    math-function accuracy table is not installed with the toolchain this was written against, so the figure is MEASURED as the issue
    prescribes: the largest distance of torch's float32 CPU tanh to float64 over tanh_probe() is 0.5690 ulp (TANH_CPU_ULP = 0.569 bounds it;
    the CPU test re-measures), and another correct float32 realisation is allowed 4 x that: TANH_ULP = 2.276.
  GroupNorm exact: x in {+-1, +-2}, each value as often as its negative: partials are integers, the mean is 0, stats[0] == 0 exactly.  rstd
    is not exact; y is held to the boundary rule of lasr_ops_ref.rule_holds against y64 = x rstd64 gw + gb with the float32 evaluation error
    |y32 - y64| <= SAFETY u (10 |x rstd gw| + |y64|) (q / n, + eps, sqrt, the reciprocal <= 2.5 ulp: 8 u on rstd; two products and an
    addition, fused or not), at most SILU_SHARE = 1 % of the live elements exempt.
  RoPE exact: tables in {0, +-1, +-0.5}, x integers in [-8, 8]: x c +- x' s is a multiple of 1/2 up to 16, a bf16 value.
  attention: the three tiers of attn_ref.  locator: q is the designed key of one target, which beats all others by 4096 scale >= 512 > 110:
    out == V[target]; uniform: q = 0, integer V: out == T(float32(sum) / float32(n)), stale +-1e4 / NaN behind n; Gaussian: for this kernel -
    a fmaf chain of 64 and one rounding of the product with scale (es = gamma_64 max a_j + u max |s_j|, a_j = scale sum |q k_j|), one maximum,
    one __expf per key (relative (1 + 1.45) X u + 2 u, X = max |s_j - max|; attn_ref), so p_j is off by D = 2 es + 2.45 X u + 2 u; a serial
    fmaf value sum over n (+ 1) keys, gamma_(n + 1); the sum of probabilities per lane and through the wave, gamma_(ceil(n / 64) + 7), and
    one division, 4 u:    E = 2 D + gamma_(n + 1) + gamma_(ceil(n / 64) + 7) + 4 u,   |out - ref| <= ulp_bf16 / 2 + SAFETY E sum p |v|
    (no MFMA factor; attn_ref.SAFETY; not tuned on the device).  Self-attention: q, k after RoPE are known bit for bit (dyadic tables).
  gemv exact: integer x in [-1, 1], w in [-4, 4] (LN: xs = +-lnw, lnw in {1, 2}, w in [-2, 2]): |sums| <= 2048 < 2^12.  LN rows are
    +-m 2^k, half of each sign, (m, k) different for every row (m = 1 for rows < 52, k = row; then m = 3): the mean is 0 and the variance
    m^2 4^k exactly, x rstd = +-(1 - delta), delta <= 5.1e-6 far inside half a bf16 ulp (2^-9), so T(x rstd lnw) == +-lnw; statistics of
    another row give +-lnw times another power of two (or 3).  MS_GATE: W is scaled by a power of two until |g| <= 8; T(silu(g)) is held to
    the SiLU rule of lasr_ops_ref (exempt elements may take either bf16 neighbour), the product with a is exact in float32.
  gemv Gaussian: x, w, bias with full bf16 mantissas, x of mean 0.5; LN rows go through the float64 LayerNorm (ln_reference derives the
    float32 error of xn and which elements may round to the other bf16 neighbour).  |acc - ref64| <= gamma_K sum |xs w| (a float32 sum of K
    products in any order) + |w| ulp for every such element; each later rounding is exact unless its argument lies within the error so far
    of a rounding boundary, the last one adds HALF a bf16 ulp (gemv_gauss_reference), MS_GATE included."""
import ctypes as C
import math

import numpy as np

import attn_ref as ar
import gemm_ref as gr
import lasr_ops_ref as lo

OK, GENERATION_FAILED, INVALID_INPUT = 0, 2, 3
MS_BF16, MS_RESID, MS_GATE, MS_F32 = range(4)
SAFETY, U, T, ulp_bf16 = ar.SAFETY, ar.U, gr.T, ar.ulp_bf16
SILU_SHARE = lo.SILU_SHARE
HD, MAX_KEYS, MAX_POS, MAX_BATCH, GN_CHUNK = 64, 1280, 2048, 64, 32768
NAN16 = 0x7FC0
EPS32 = float(np.float32(1e-5))
TANH_CPU_ULP = 0.569
TANH_ULP = 4 * TANH_CPU_ULP
STALE_PCM = 3e4


def gam(k):
    return k * U / (1.0 - k * U)


def ulp_f32(v):
    a = np.abs(np.asarray(v, np.float64))
    return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - 23)


def tanh_probe():
    """the arguments TANH_CPU_ULP is measured on (float32): a fine grid over the unsaturated range and the Gaussian tier's own sums"""
    rng = np.random.default_rng(77)
    return np.concatenate([np.linspace(-10, 10, 2000001), 2.0 * rng.standard_normal(2000000), 0.01 * rng.standard_normal(1000000)]).astype(np.float32)


def boundary(s, m_abs):
    """(T(s), True where the float64 value s lies within m_abs of a bf16 rounding boundary)"""
    s = np.asarray(s, np.float64)
    r = T(s)
    dn, up = lo._neighbours(r)
    return r, np.minimum(np.abs(s - (r + dn) / 2), np.abs(s - (r + up) / 2)) <= m_abs


def bits(v):
    return gr.exact_bits(v)


def val(b):
    return gr.bf16_value(b).astype(np.float64)


def tbits(v):
    """payload of T(v)"""
    return gr.bf16_bits(np.asarray(T(v), np.float64).astype(np.float32))


# ------------------------------------------------------------------------------------------------ conv1 + tanh
CONV1_D, CONV1_T1, CONV1_T1PAD = [288, 416], [0, 1, 15, 16, 17, 33], 35
CONV1_STRIDE = (max(CONV1_T1) - 1) * 64 + 127 + 101
CONV1_TAPS = [0, 63, 64, 126]


def conv1_cases():
    return [dict(tier=t, d=d, seed=41000 + 10 * i + j) for i, d in enumerate(CONV1_D) for j, t in enumerate(("exact", "gauss"))]


def conv1_case(c):
    d, B = c["d"], len(CONV1_T1)
    rng = np.random.default_rng(c["seed"])
    T1 = np.array(CONV1_T1, np.int32)
    w = np.zeros((d, 127))
    if c["tier"] == "exact":
        tap = np.concatenate([CONV1_TAPS, rng.integers(0, 127, d - 4)])
        w[np.arange(d), tap] = rng.choice([-1.0, 1.0], d)
        pcm = rng.choice([0.0, 16.0, -16.0], (B, CONV1_STRIDE))
    else:
        tap = None
        w = (rng.standard_normal((d, 127)) * math.sqrt(1.0 / 127)).astype(np.float32).astype(np.float64)
        pcm = (1.5 * rng.standard_normal((B, CONV1_STRIDE))).astype(np.float32).astype(np.float64)
    ext = np.where(T1 > 0, (T1 - 1) * 64 + 127, 0)
    pcm = np.where(np.arange(CONV1_STRIDE)[None] >= ext[:, None], STALE_PCM, pcm)
    return dict(c, B=B, T1=T1, T1pad=CONV1_T1PAD, stride=CONV1_STRIDE, w=w, tap=tap, pcm=pcm)


def conv1_windows(c, shift=0):
    """[B][T1pad][127] sample windows (zeros behind the buffer); shift: a kernel that starts its windows late (CPU sensitivity)"""
    p = np.pad(c["pcm"], ((0, 0), (0, 64 * c["T1pad"] + 256)))
    idx = 64 * np.arange(c["T1pad"])[:, None] + np.arange(127)[None] + shift
    return p[:, idx]


def conv1_reference(c, shift=0, order=None, dtype=np.float64):
    """(out [B][T1pad][d] float64, bound or None).  order / dtype: the sum over the taps in a given order and precision (CPU proofs)"""
    win = conv1_windows(c, shift)
    live = (np.arange(c["T1pad"])[None] < c["T1"][:, None])[:, :, None]
    win = np.where(live, win, 0.0)
    if order is None and dtype == np.float64:
        a = win @ c["w"].T
    else:
        a = np.zeros(win.shape[:2] + (c["d"],), dtype)
        for k in (range(127) if order is None else order):
            a = (a + (win[:, :, k, None].astype(dtype) * c["w"][None, None, :, k].astype(dtype)).astype(dtype)).astype(dtype)
        a = a.astype(np.float64)
    out = np.where(live, np.tanh(a), 0.0)
    if c["tier"] != "gauss":
        return out, None
    delta = SAFETY * gam(127) * (np.abs(win) @ np.abs(c["w"]).T)
    slope = 1.0 - np.tanh(np.maximum(np.abs(a) - delta, 0.0)) ** 2
    return out, np.where(live, delta * slope + TANH_ULP * ulp_f32(out), 0.0)


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_D, GN_T1 = 288, [1, 113, 114, 115, 228]
GN_T1PAD = 228


def gn_case(seed=42000):
    d, B, Tp = GN_D, len(GN_T1), GN_T1PAD
    rng = np.random.default_rng(seed)
    T1 = np.array(GN_T1, np.int32)
    x = np.zeros((B, Tp * d))
    for b in range(B):
        n = int(T1[b]) * d
        half = rng.choice([1.0, 2.0], n // 2) * rng.choice([-1.0, 1.0], n // 2)
        x[b, :n] = rng.permutation(np.concatenate([half, -half]))
    gw = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32).astype(np.float64)
    gb = (0.05 * rng.standard_normal(d)).astype(np.float32).astype(np.float64)
    return dict(B=B, d=d, T1=T1, T1pad=Tp, x=x.reshape(B, Tp, d), gw=gw, gb=gb, nch=-(-int(T1.max()) * d // GN_CHUNK))


def gn_reference(c, order=None, dtype=np.float64, mean_of=None):
    """part0, part1 [B][nch], stats [B][2] (float64), y [B T1pad d + 8 d] bf16 values, exempt, live.  order / dtype: the chunk sums in a given
    element order and precision; mean_of: a kernel that takes the statistics of another row (CPU sensitivity)"""
    B, d, Tp, nch = c["B"], c["d"], c["T1pad"], c["nch"]
    p0, p1, st = np.zeros((B, nch)), np.zeros((B, nch)), np.zeros((B, 2))
    flat = c["x"].reshape(B, -1)
    n1 = B * Tp * d
    y, ex, live = np.zeros(n1 + 8 * d), np.zeros(n1 + 8 * d, bool), np.zeros(n1 + 8 * d, bool)

    def total(v):
        if order is None and dtype == np.float64:
            return v.sum()
        v = (v if order is None else v[order(len(v))]).astype(dtype)
        return float(np.cumsum(v, dtype=dtype)[-1])                  # a serial sum in that precision
    for b in range(B):
        n = int(c["T1"][b]) * d
        row = flat[b, :n]
        for ch in range(-(-n // GN_CHUNK)):
            p0[b, ch] = total(row[ch * GN_CHUNK:(ch + 1) * GN_CHUNK])
        mean = p0[b].sum() / n
        for ch in range(-(-n // GN_CHUNK)):
            p1[b, ch] = total((row[ch * GN_CHUNK:(ch + 1) * GN_CHUNK] - mean) ** 2)
        st[b] = mean, 1.0 / math.sqrt(p1[b].sum() / n + EPS32)
    for b in range(B):
        n = int(c["T1"][b]) * d
        mean, rstd = st[b if mean_of is None else mean_of(b)]
        p = (flat[b, :n] - mean) * rstd * np.tile(c["gw"], n // d)
        y64 = p + np.tile(c["gb"], n // d)
        sl = slice(b * Tp * d, b * Tp * d + n)
        y[sl], ex[sl] = boundary(y64, SAFETY * U * (10 * np.abs(p) + np.abs(y64)))
        live[sl] = True
    return dict(part0=p0, part1=p1, stats=st, y=y, exempt=ex, live=live)


# ------------------------------------------------------------------------------------------------ RoPE
ROPE_ROT, ROPE_TPAD, ROPE_M, ROPE_NHEADS, ROPE_LD = [32, 46, 56, 64], [1, 5], 7, 3, 5 * HD + 8
DYADIC = (0.0, 1.0, -1.0, 0.5, -0.5)


def rope_cases():
    return [dict(rot=r, Tpad=tp, seed=43000 + 10 * i + j) for i, r in enumerate(ROPE_ROT) for j, tp in enumerate(ROPE_TPAD)]


def rope_case(c):
    """rows [M][ld]: three rotated heads, two v heads, eight padding columns (NaN payloads); tables of M rows and rot / 2 + 1 columns of which the
    launch gets [:Tpad, :rot / 2] - the rest is what a kernel that takes position m, or rotates at column rot, would meet"""
    rng = np.random.default_rng(c["seed"])
    x = rng.integers(-8, 9, (ROPE_M, ROPE_LD)).astype(np.float64)
    x[:, :ROPE_NHEADS * HD][x[:, :ROPE_NHEADS * HD] == 0] = 3.0
    img = bits(x)
    img[:, 5 * HD:] = 0x7FC1
    cs, sn = rng.choice(DYADIC, (ROPE_M, c["rot"] // 2 + 1)), rng.choice(DYADIC[1:], (ROPE_M, c["rot"] // 2 + 1))
    return dict(c, M=ROPE_M, ld=ROPE_LD, nheads=ROPE_NHEADS, x=x, img=img, cs=cs, sn=sn)


def rope_pairs(x, c, s, rot, mut=None):
    """x [..., 64], c, s [..., >= rot / 2] broadcastable -> before the rounding; columns >= rot unchanged"""
    y = x.copy()
    r = rot + 2 if mut == "at_rot" and rot < HD else rot
    c, s = c[..., :r // 2], s[..., :r // 2]
    if mut == "half_split":
        a, b = x[..., :r // 2], x[..., r // 2:r]
        y[..., :r // 2], y[..., r // 2:r] = a * c - b * s, b * c + a * s
    else:
        a, b = x[..., 0:r:2], x[..., 1:r:2]
        y[..., 0:r:2], y[..., 1:r:2] = a * c - b * s, b * c + a * s
    return y


def rope_reference(c, mut=None):
    """the rows' payloads after the launch"""
    M, nh = c["M"], c["nheads"]
    pos = np.arange(M) if mut == "pos" else np.arange(M) % c["Tpad"]
    x = c["x"][:, :nh * HD].reshape(M, nh, HD)
    y = rope_pairs(x, c["cs"][pos][:, None], c["sn"][pos][:, None], c["rot"], mut)
    out = c["img"].copy()
    out[:, :nh * HD] = tbits(y.reshape(M, nh * HD))
    return out


# ------------------------------------------------------------------------------------------------ attention
ATTN_HEADS, ATTN_SCALE, ATTN_TIERS = [(8, 8), (8, 4), (8, 2)], [36.0 ** -0.5, 0.125], ["locator", "uniform", "gaussian"]
ENC_T3, CROSS_T3, ATTN_PAD = [0, 1, 63, 64, 65, 129], [1, 63, 64, 65, 129], 8
SELF_POS, SELF_SMAX, SELF_B = [0, 1, 63, 64, 65, 127, 128, 200], 201, 3


def attn_launches(kind):
    """kind 0 / 2: every tier with every head arrangement, Tpad 130 / 131 and the two scales alternating, and the MS_MAX_KEYS case (one head,
    one row); kind 1: every position with every tier, the arrangements cycling, and position MS_MAX_POS - 1"""
    out = []
    if kind == 1:
        for ip, pos in enumerate(SELF_POS):
            for it, tier in enumerate(ATTN_TIERS):
                out.append(dict(kind=1, tier=tier, heads=ATTN_HEADS[(ip + it) % 3], B=SELF_B, pos=pos, Smax=SELF_SMAX, rot=(32, 46, 56, 64)[(ip + it) % 4],
                                scale=ATTN_SCALE[(ip + it) % 2], seed=45000 + 10 * ip + it))
        out += [dict(kind=1, tier=t, heads=(1, 1), B=1, pos=MAX_POS - 1, Smax=MAX_POS, rot=56, scale=0.125, seed=45900 + i) for i, t in enumerate(ATTN_TIERS[:2])]
        return out
    for it, tier in enumerate(ATTN_TIERS):
        for ih, heads in enumerate(ATTN_HEADS):
            out.append(dict(kind=kind, tier=tier, heads=heads, T3=ENC_T3 if kind == 0 else CROSS_T3, Tpad=130 + (it + ih) % 2, scale=ATTN_SCALE[(it + ih) % 2],
                            seed=44000 + 1000 * kind + 10 * it + ih))
    if kind == 0:
        out.append(dict(kind=0, tier="locator", heads=(1, 1), T3=[MAX_KEYS], Tpad=MAX_KEYS, scale=0.125, seed=44900))
    return out


def _tier_qkv(tier, rng, B, H, Hkv, nq, nk):
    """logical q [B][H][nq][64], K, V [B][Hkv][nk][64] and the locator targets [B][H][nq] (over all nk keys; the caller reduces them)"""
    QS, KS = (B, H, nq, HD), (B, Hkv, nk, HD)
    tg = None
    if tier == "locator":
        K = np.broadcast_to(ar.locator_key(np.arange(nk), HD)[None, None], KS).copy()
        b_, h_, j_, d_ = np.meshgrid(np.arange(B), np.arange(Hkv), np.arange(nk), np.arange(HD), indexing="ij")
        V = ar.locator_v(b_, h_, j_, d_)
        tg = rng.integers(0, 1 << 30, (B, H, nq))
        q = None
    elif tier == "uniform":
        K, V, q = rng.integers(-4, 5, KS).astype(np.float64), rng.integers(-8, 9, KS).astype(np.float64), np.zeros(QS)
    else:
        K, V, q = ar.grid_bf16(0.5 * rng.standard_normal(KS)), ar.grid_bf16(rng.standard_normal(KS)), ar.grid_bf16(rng.standard_normal(QS))
    return q, K, V, tg


def _dead_fill(rng, a, dead, tier):
    """payloads of `a`, with NaN (uniform tier: stale +-1e4 in one half, NaN in the other) where dead"""
    out = lo.bits_nan(a, dead)
    if tier == "uniform":
        st = bits(ar.stale(rng, a.shape))
        pick = np.broadcast_to(dead, a.shape) & (rng.integers(0, 2, a.shape) > 0)
        out[pick] = st[pick]
    return out


def attn_case(c):
    """kinds 0 / 2.  n = T3[b]; keys and (kind 0) queries behind n hold NaN / stale values; locator targets: every query its own, the first
    query the last key and the last query key 0"""
    (H, Hkv), T3, Tp, tier, kind = c["heads"], np.asarray(c["T3"]), c["Tpad"], c["tier"], c["kind"]
    B = len(T3)
    rng = np.random.default_rng(c["seed"])
    nq = Tp if kind == 0 else 1
    q, K, V, tg = _tier_qkv(tier, rng, B, H, Hkv, nq, Tp)
    if tier == "locator":
        tg = (tg + 13 * np.arange(nq)[None, None]) % np.maximum(T3, 1)[:, None, None]
        if kind == 0:
            tg[:, :, 0] = np.maximum(T3, 1)[:, None] - 1
            for b in range(B):
                tg[b, :, max(T3[b], 1) - 1] = 0
        q = ar.locator_key(tg, HD)
    kdead = np.broadcast_to((np.arange(Tp)[None] >= T3[:, None])[:, None, :, None], K.shape)
    Kb, Vb = _dead_fill(rng, K, kdead, tier), _dead_fill(rng, V, kdead, tier)
    flat = lambda a, n: a.transpose(0, 2, 1, 3).reshape(B, -1, n * HD)
    d = dict(c, H=H, Hkv=Hkv, B=B, T3=T3.astype(np.int32), q=q, K=K, V=V, Kb=Kb, Vb=Vb, targets=tg)
    if kind == 0:
        ld, ldo = (H + 2 * Hkv) * HD + ATTN_PAD, H * HD + ATTN_PAD
        rows = np.full((B, Tp, ld), NAN16, np.uint16)
        qdead = np.broadcast_to((np.arange(Tp)[None] >= T3[:, None])[:, None, :, None], q.shape)
        rows[:, :, :H * HD] = flat(lo.bits_nan(q, qdead), H)
        rows[:, :, H * HD:(H + Hkv) * HD], rows[:, :, (H + Hkv) * HD:(H + 2 * Hkv) * HD] = flat(Kb, Hkv), flat(Vb, Hkv)
        return dict(d, ld=ld, ldo=ldo, rows=rows.reshape(B * Tp, ld))
    return dict(d, qrows=flat(bits(q), H).reshape(B, H * HD), kv=np.concatenate([flat(Kb, Hkv), flat(Vb, Hkv)], -1).reshape(B * Tp, 2 * Hkv * HD))


def attend(q, K, V, scale):
    """q [nq][64], K, V [n][64] float64 -> (out before the rounding [nq][64], the Gaussian tier's bound)"""
    n = K.shape[0]
    s = scale * (q @ K.T)
    mx = s.max(-1, keepdims=True)
    p = np.exp(s - mx)
    p /= p.sum(-1, keepdims=True)
    o, mag = p @ V, p @ np.abs(V)
    es = gam(HD) * (scale * (np.abs(q) @ np.abs(K).T)).max(-1) + U * np.abs(s).max(-1)
    D = 2 * es + 2.45 * np.abs(s - mx).max(-1) * U + 2 * U
    E = (2 * D + gam(n + 1) + gam(-(-n // 64) + 7) + 4 * U)[:, None]
    pre = SAFETY * E * mag
    return o, pre + ulp_bf16(np.abs(o) + pre) / 2


def attn_reference(c, extra_keys=0):
    """kinds 0 / 2: (out float64 before the rounding - [B Tpad][H 64], zero rows behind T3, or [B][H 64] -, bound).  extra_keys: a mask that
    lets that many keys too many through, read as the launch holds them (NaN, stale values; CPU sensitivity)"""
    B, H, Hkv, Tp, kind = c["B"], c["H"], c["Hkv"], c["Tpad"], c["kind"]
    nq = Tp if kind == 0 else 1
    out, bound = np.zeros((B, nq, H, HD)), np.zeros((B, nq, H, HD))
    Kv, Vv = val(c["Kb"]), val(c["Vb"])
    with np.errstate(invalid="ignore"):
        for b in range(B):
            n = int(c["T3"][b])
            nk, m = min(n + extra_keys, Tp), (n if kind == 0 else 1)
            for h in range(H if n else 0):
                hk = h // (H // Hkv)
                Kb = np.concatenate([c["K"][b, hk, :n], Kv[b, hk, n:nk]])
                Vb = np.concatenate([c["V"][b, hk, :n], Vv[b, hk, n:nk]])
                out[b, :m, h], bound[b, :m, h] = attend(c["q"][b, h, :m], Kb, Vb, c["scale"])
    return out.reshape(B * nq, H * HD), bound.reshape(B * nq, H * HD)


def attn_exact_expected(c):
    """the locator and the uniform tier's stated outputs"""
    B, H, Hkv, kind = c["B"], c["H"], c["Hkv"], c["kind"]
    nq = c["Tpad"] if kind == 0 else 1
    out = np.zeros((B, nq, H, HD))
    for b in range(B):
        n = int(c["T3"][b])
        m = n if kind == 0 else 1
        for h in range(H if n else 0):
            hk = h // (H // Hkv)
            if c["tier"] == "locator":
                out[b, :m, h] = c["V"][b, hk][c["targets"][b, h, :m]]
            else:
                out[b, :m, h] = lo.b16(c["V"][b, hk, :n].sum(0).astype(np.float32) / np.float32(n)).astype(np.float64)[None]
    return out.reshape(B * nq, H * HD)


def quarter_turns(rng, shape):
    """RoPE table entries (c, s) that are rotations by a multiple of 90 degrees: exactly invertible, dyadic"""
    k = rng.integers(0, 4, shape)
    return np.array([1.0, 0.0, -1.0, 0.0])[k], np.array([0.0, 1.0, 0.0, -1.0])[k]


def self_case(c):
    """the new token's q | k | v row of every batch row, the caches before the launch (positions < pos live, pos stale, > pos NaN), tables
    [Smax][rot / 2].  locator: the row of `pos` holds quarter turns and the raw q, k are the designed keys turned back; the target of head h is
    key (h + b) % (pos + 1) - the new key among them; uniform / gaussian: dyadic tables (attn_ref.dyadic_tables: exact on the 2^-8 grid)"""
    (H, Hkv), B, pos, Smax, rot, tier = c["heads"], c["B"], c["pos"], c["Smax"], c["rot"], c["tier"]
    rng = np.random.default_rng(c["seed"])
    q, K, V, tg = _tier_qkv(tier, rng, B, H, Hkv, 1, pos + 1)
    cs, sn = ar.dyadic_tables(rng, Smax, rot)
    if tier == "locator":
        cs[pos], sn[pos] = quarter_turns(rng, rot // 2)
        tg = ((np.arange(H)[None, :, None] * 7 + np.arange(B)[:, None, None] + tg % 2) % (pos + 1))
        tg[:, H - 1] = 0
        tg[:, 0] = pos if H > 1 else (3 * pos) // 4
        inv = lambda w: rope_pairs(w, cs[pos], -sn[pos], rot)                # the inverse of a quarter turn
        q_raw, k_raw = inv(ar.locator_key(tg, HD)), inv(K[:, :, pos:pos + 1])
    else:
        q_raw, k_raw = q, K[:, :, pos:pos + 1]
    v_new = V[:, :, pos:pos + 1]
    qr, kr = T(rope_pairs(q_raw, cs[pos], sn[pos], rot)), T(rope_pairs(k_raw, cs[pos], sn[pos], rot))
    Kall, Vall = np.concatenate([K[:, :, :pos], kr], 2), np.concatenate([V[:, :, :pos], v_new], 2)
    shape = (B, Hkv, Smax, HD)
    dead = np.broadcast_to((np.arange(Smax) > pos)[None, None, :, None], shape)
    full = lambda a: np.concatenate([a, np.zeros((B, Hkv, Smax - pos - 1, HD))], 2)
    before = lambda a: np.concatenate([a[:, :, :pos], ar.stale(rng, (B, Hkv, 1, HD))], 2)
    kc, vc = lo.bits_nan(full(before(Kall)), dead), lo.bits_nan(full(before(Vall)), dead)
    flat = lambda a: a.transpose(0, 2, 1, 3).reshape(B, -1)
    qkv = np.concatenate([flat(bits(q_raw)), flat(bits(k_raw)), flat(bits(v_new))], -1)
    return dict(c, H=H, Hkv=Hkv, qkv=qkv, kc=kc, vc=vc, cs=cs, sn=sn, qr=qr, Kall=Kall, Vall=Vall, targets=tg, dead=dead, full=full)


def self_reference(c, wrong_head=False):
    """(out [B][H 64] float64 - before the rounding for the Gaussian tier, the stated value else -, bound, kc, vc payloads after the launch).
    wrong_head: the row appended for kv head hk is that of head (hk + 1) % Hkv (CPU sensitivity)"""
    B, H, Hkv, pos = c["B"], c["H"], c["Hkv"], c["pos"]
    out, bound = np.zeros((B, H, HD)), np.zeros((B, H, HD))
    for b in range(B):
        for h in range(H):
            hk = h // (H // Hkv)
            if c["tier"] == "locator":
                out[b, h] = c["Vall"][b, hk, c["targets"][b, h, 0]]
            elif c["tier"] == "uniform":
                out[b, h] = lo.b16(c["Vall"][b, hk].sum(0).astype(np.float32) / np.float32(pos + 1)).astype(np.float64)
            else:
                out[b, h], bound[b, h] = (v[0] for v in attend(c["qr"][b, h], c["Kall"][b, hk], c["Vall"][b, hk], c["scale"]))
    src = (np.arange(Hkv) + 1) % Hkv if wrong_head else np.arange(Hkv)
    kc, vc = c["kc"].copy(), c["vc"].copy()
    kc[:, :, pos], vc[:, :, pos] = bits(c["Kall"][:, src, pos]), bits(c["Vall"][:, src, pos])
    return out.reshape(B, H * HD), bound.reshape(B, H * HD), kc, vc


# ------------------------------------------------------------------------------------------------ decode-step GEMM
GEMV_INST = [(1, MS_BF16), (0, MS_RESID), (1, MS_GATE), (1, MS_F32)]
GEMV_B, GEMV_K, GEMV_N = [1, 7, 8, 9, 33, 64], [4, 252, 256, 260, 288, 416, 512], [1, 4, 5, 131]


def gemv_cases(ln, epi):
    """every (B, K); N (MS_GATE: F) and the bias cycle along both so that every N meets every B and every K"""
    ii = GEMV_INST.index((ln, epi))
    return [dict(ln=ln, epi=epi, B=B, K=K, N=GEMV_N[(i + j + ii) % 4], bias=epi != MS_F32 and (i + j // 4) % 2 == 0, seed=46000 + 1000 * ii + 10 * i + j)
            for i, B in enumerate(GEMV_B) for j, K in enumerate(GEMV_K)]


def ln_exact_rows(rng, B, K):
    """rows +-m 2^k, half of each sign: (m, k) = (1, r) for r < 52, (3, r - 52) behind"""
    r = np.arange(B)
    amp = np.where(r < 52, 1.0, 3.0) * 2.0 ** np.where(r < 52, r, r - 52)
    sign = np.stack([rng.permutation(np.repeat([1.0, -1.0], K // 2)) for _ in range(B)])
    return sign * amp[:, None], sign


def gemv_case(c, gauss=False):
    """X [B][K], lnw, W [rows][K] (rows = N, MS_GATE 2 N), bias, h (MS_RESID) in float64, all bf16 values; xs = what the contraction sees"""
    B, K, ln, epi = c["B"], c["K"], c["ln"], c["epi"]
    rows = 2 * c["N"] if epi == MS_GATE else c["N"]
    rng = np.random.default_rng(c["seed"])
    lnw = h = None
    slack = None
    if gauss:                                                        # full bf16 mantissas: the float32 sums are not exact
        X, W = T(0.5 + rng.standard_normal((B, K))), T(rng.standard_normal((rows, K)) / math.sqrt(K))
        bias = T(rng.standard_normal(rows)) if c["bias"] else None
        xs, slack = X, np.zeros((B, K))
        if ln:                                                       # rows of non-zero mean through the float64 LayerNorm
            lnw = T(1.0 + 0.1 * rng.standard_normal(K))
            xs, amb = ln_reference(X, lnw)
            slack = np.where(amb, ulp_bf16(xs), 0.0)
    elif ln:
        X, sign = ln_exact_rows(rng, B, K)
        lnw = rng.choice([1.0, 2.0], K)
        xs = sign * lnw
        W = rng.integers(-2, 3, (rows, K)).astype(np.float64)
    else:
        X = xs = rng.integers(-1, 2, (B, K)).astype(np.float64)
        W = rng.integers(-4, 5, (rows, K)).astype(np.float64)
    if not gauss:
        W[:, 0] = np.where(W[:, 0] == 0, 1.0, W[:, 0])
        bias = rng.integers(-3, 4, rows).astype(np.float64) if c["bias"] else None
        if bias is not None and rows > 1:
            bias[1] = bias[0] + 1.0                                    # a shifted bias is another bias
        if not ln:
            X[0, 0] = 1.0
        for r in [0] + ([c["N"]] if epi == MS_GATE else []):         # row 0 of the output is not zero (a case of one element compares something)
            if xs[0] @ W[r] + (0.0 if bias is None else bias[r]) == 0:
                W[r, 0] += 1.0 if W[r, 0] != -1.0 else -1.0
        if epi == MS_GATE:                                           # |g| <= 8: the gate rows (and their bias) times a power of two
            e = 0
            g = xs @ W[c["N"]:].T + (0.0 if bias is None else bias[c["N"]:])
            while np.abs(g * 2.0 ** e).max() > lo.SILU_VMAX:
                e -= 1
            W[c["N"]:] *= 2.0 ** e
            if bias is not None:
                bias[c["N"]:] *= 2.0 ** e
    if not gauss and B > 1 and np.array_equal(xs[0] @ W.T, xs[B - 1] @ W.T):       # (K = 4, N = 1: few patterns) the last row repeated into row 0 must show
        return gemv_case(dict(c, seed=c["seed"] + 100000))
    if epi == MS_RESID:
        h = rng.integers(-64, 65, (B, c["N"])).astype(np.float64) if not gauss else ar.grid_bf16(rng.standard_normal((B, c["N"])))
    return dict(c, X=X, xs=xs, lnw=lnw, W=W, b=bias, h=h, rows=rows, gauss=gauss, slack=slack)


def ln_reference(X, lnw, no_mean=False):
    """float64 LayerNorm (weight only, eps 1e-5f) of rows X -> (xs = T(xn), True where the float32 kernel may round xn to the other neighbour).
    Float32 error of xn = t rstd lnw, t = x - mean.  A wave is a row: a lane adds its ceil(K / 64) elements, the wave sum adds six more
    levels, so a sum is n = ceil(K / 64) + 6 additions deep:
      mean     dm = gamma_(n + 1) mean |x|                     (the sum and the division)
      t        dm + u |t|
      var      relative rv = gamma_(n + 3) + 2 dm sum |t| / sum t^2   (squares, the sum, the error of t to first order)
      rstd     relative rr = rv / 2 + 4 u                     (/ K, + eps, sqrt, the reciprocal)
      xn       |lnw rstd| (dm + u |t|) + |xn| (rr + 2 u),  times SAFETY (first-order terms)
    no_mean: a kernel that forgets the mean (variance about 0; CPU sensitivity)"""
    K = X.shape[1]
    m = np.zeros((X.shape[0], 1)) if no_mean else X.mean(-1, keepdims=True)
    t = X - m
    rstd = 1.0 / np.sqrt((t ** 2).mean(-1, keepdims=True) + EPS32)
    xn = t * rstd * lnw
    n = -(-K // 64) + 6
    dm = gam(n + 1) * np.abs(X).mean(-1, keepdims=True)
    rr = (gam(n + 3) + 2 * dm * np.abs(t).sum(-1, keepdims=True) / (t ** 2).sum(-1, keepdims=True)) / 2 + 4 * U
    return boundary(xn, SAFETY * (np.abs(lnw * rstd) * (dm + U * np.abs(t)) + np.abs(xn) * (rr + 2 * U)))


def _round_amb(v, err):
    """(T(v), the distance the device's rounding of its own v may be off: one bf16 ulp where v lies within err of a boundary, else 0)"""
    r, amb = boundary(v, err)
    return r, np.where(amb, ulp_bf16(r), 0.0)


def gemv_gauss_reference(c):
    """Gaussian tier: (out before its LAST rounding, bound).  acc is off by e = gamma_K sum |xs w| (a float32 sum of K products in any order)
    plus |w| ulp for every xs element that may round either way; every later T() is exact unless its argument lies within the error so far
    of a rounding boundary (then one ulp); the last rounding adds half a bf16 ulp.  MS_GATE: silu of a gate off by dg moves by at most
    1.1 dg (|silu'| <= 1.1), T(silu) by one more ulp where the SiLU rule exempts it."""
    N, epi, xs, W, K = c["N"], c["epi"], c["xs"], c["W"], c["K"]
    acc = xs @ W.T
    e = gam(K) * (np.abs(xs) @ np.abs(W).T) + c["slack"] @ np.abs(W).T
    if epi == MS_F32:
        return acc, e
    half = lambda v, d: d + ulp_bf16(np.abs(v) + d) / 2
    if c["b"] is not None:
        acc, e = acc + c["b"][None], e + U * np.abs(acc + c["b"][None])
    if epi == MS_BF16:
        return acc, half(acc, e)
    if epi == MS_RESID:
        v, dv = _round_amb(acc, e)
        return v + c["h"], half(v + c["h"], dv)
    a, da = _round_amb(acc[:, :N], e[:, :N])
    g, dg = _round_amb(acc[:, N:], e[:, N:])
    sg, ex = lo.silu_reference(g)
    dsg = np.where(dg > 0, 1.1 * dg + ulp_bf16(np.abs(sg) + 1.1 * dg), 0.0) + np.where(ex, ulp_bf16(sg), 0.0)
    return sg * a, half(sg * a, np.abs(sg) * da + np.abs(a) * dsg + da * dsg)


def gemv_reference(c, mut=None, order=None, dtype=np.float64):
    """exact tier: (out float64: bf16 values - MS_F32: the sums -, SiLU exempt with its two alternatives or None, None).  mut: a wrong kernel; order / dtype: the K sum in another order and precision (CPU proofs)"""
    B, N, epi, xs, W = c["B"], c["N"], c["epi"], c["xs"], c["W"]
    if mut == "repeat_last" and B > 1:
        xs = xs.copy()
        xs[0] = xs[B - 1]
    if order is None and dtype == np.float64:
        acc = xs @ W.T
    else:
        acc = np.zeros((B, c["rows"]), dtype)
        for k in (range(c["K"]) if order is None else order):
            acc = (acc + np.outer(xs[:, k].astype(dtype), W[:, k].astype(dtype)).astype(dtype)).astype(dtype)
        acc = acc.astype(np.float64)
    if epi == MS_F32:
        return acc, None, None
    bias = np.zeros(c["rows"]) if c["b"] is None else (np.roll(c["b"], 1) if mut == "bias_shift" else c["b"])
    pre = acc + bias[None]
    if epi == MS_BF16:
        return T(pre), None, None
    if epi == MS_RESID:
        h = np.roll(c["h"], 1, 0) if mut == "resid_row" and B > 1 else c["h"]
        return T(T(pre) + h), None, None
    g = pre[:, N:] if mut != "gate_row" else np.concatenate([pre[:, N - 1:N], pre[:, N:-1]], 1)       # the gate read from row n + F - 1
    a, (sg, ex) = T(pre[:, :N]), lo.silu_reference(T(g))
    dn, up = lo._neighbours(sg)
    return T(sg * a), (ex, T(dn * a), T(up * a)), None


# ------------------------------------------------------------------------------------------------ embed, arg-max + embed
EMBED_D, EMBED_VOCAB = 288, 37
ARGMAX_V, ARGMAX_D, ARGMAX_STRIDE, EOS = [255, 256, 257, 2049], 288, 4, 2


def embed_case(seed=47000):
    rng = np.random.default_rng(seed)
    emb = rng.integers(0, 1 << 16, (EMBED_VOCAB, EMBED_D)).astype(np.uint16)
    ids = np.array([-1, EMBED_VOCAB, 0, EMBED_VOCAB - 1, 5, 1 << 30, -(1 << 31), 17], np.int32)
    return emb, ids


def embed_reference(emb, ids):
    return emb[np.where((ids < 0) | (ids >= emb.shape[0]), 0, ids)]


ARGMAX_ROWS = ["max0", "maxlast", "wave0", "wave1", "wave2", "wave3", "tie", "nan", "neginf", "eos", "inactive", "full", "eos_inactive", "eos2",
               "nan_front"]


def argmax_case(V, seed=48000):
    """one launch, a row per rule.  wave w of the block reads ids i with (i % 256) // 64 == w"""
    rng = np.random.default_rng(seed + V)
    B = len(ARGMAX_ROWS)
    x = rng.standard_normal((B, V)).astype(np.float32)
    x[:, EOS] = -5.0
    want = np.zeros(B, np.int64)
    for b, name in enumerate(ARGMAX_ROWS):
        if name in ("max0", "maxlast", "wave0", "wave1", "wave2", "wave3", "inactive", "full"):
            i = {"max0": 0, "maxlast": V - 1, "wave0": 10, "wave1": 70, "wave2": 130, "wave3": 200, "inactive": 77, "full": 141}[name]
            x[b, i], want[b] = 9.0, i
        elif name == "tie":                                          # waves 3, 1 and 2 (a second trip of the stride where V allows): the lowest id
            ids = [200, 70, 130 + 256 if V > 400 else 130]
            x[b, ids], want[b] = 9.0, 70
        elif name == "nan":
            x[b] = np.nan
        elif name == "neginf":
            x[b] = -np.inf
        elif name == "nan_front":                                    # NaN never compares: the maximum behind it
            x[b, :V // 2], x[b, V // 2 + 3], want[b] = np.nan, 9.0, V // 2 + 3
        else:
            x[b, EOS], want[b] = 9.0, EOS
    active = np.array([n not in ("inactive", "eos_inactive") for n in ARGMAX_ROWS], np.uint8)
    n_gen = (np.arange(B) % ARGMAX_STRIDE).astype(np.int32)
    n_gen[ARGMAX_ROWS.index("full")] = ARGMAX_STRIDE
    tokens = (-7 - np.arange(B * ARGMAX_STRIDE)).astype(np.int32).reshape(B, ARGMAX_STRIDE)
    emb = rng.integers(0, 1 << 16, (V, ARGMAX_D)).astype(np.uint16)
    return dict(V=V, B=B, x=x, want=want, active=active, n_gen=n_gen, tokens=tokens, done=np.array([5], np.int32), emb=emb, stride=ARGMAX_STRIDE, eos=EOS,
                d=ARGMAX_D)


def argmax_reference(c, highest=False):
    """(active, n_gen, tokens, done_count, h) after the launch.  highest: a kernel whose ties go to the highest id (CPU sensitivity)"""
    x = np.where(np.isnan(c["x"]), -np.inf, c["x"])
    ids = (c["V"] - 1 - np.argmax(x[:, ::-1], 1)) if highest else np.argmax(x, 1)
    ids = np.where(np.isnan(c["x"]).all(1), 0, ids)
    active, n_gen, tokens, done = c["active"].copy(), c["n_gen"].copy(), c["tokens"].copy(), c["done"].copy()
    for b in range(c["B"]):
        if not active[b]:
            continue
        if ids[b] == c["eos"]:
            active[b] = 0
            done[0] += 1
        else:
            if n_gen[b] < c["stride"]:
                tokens[b, n_gen[b]] = ids[b]
            n_gen[b] += 1
    return active, n_gen, tokens, done, c["emb"][ids], ids


# ------------------------------------------------------------------------------------------------ the operators on values (the model's chain)
def op_conv1(pcm, w):
    """pcm [n], w [d][127] -> float32 values [T1][d]"""
    t1 = (len(pcm) - 127) // 64 + 1
    win = pcm[64 * np.arange(t1)[:, None] + np.arange(127)[None]]
    return np.tanh(win @ w.T).astype(np.float32).astype(np.float64)


def op_groupnorm(x, gw, gb):
    m = x.mean()
    return T((x - m) / np.sqrt(((x - m) ** 2).mean() + EPS32) * gw[None] + gb[None])


def op_ln(x, w):
    m = x.mean(-1, keepdims=True)
    return T((x - m) / np.sqrt(((x - m) ** 2).mean(-1, keepdims=True) + EPS32) * w)


def op_gemv(x, lnw, W, bias, epi, h=None):
    c = dict(B=x.shape[0], N=W.shape[0] // (2 if epi == MS_GATE else 1), K=x.shape[1], epi=epi, xs=x if lnw is None else op_ln(x, lnw), W=W, b=bias, h=h,
             rows=W.shape[0], gauss=False, slack=None)
    return gemv_reference(c)[0]


def op_rope_row(x, nheads, cs, sn, rot):
    """x [nheads 64 + ...]: heads 0 .. nheads - 1 rotated with one table row"""
    out = x.copy()
    out[:nheads * HD] = T(rope_pairs(x[:nheads * HD].reshape(nheads, HD), cs[None], sn[None], rot)).reshape(-1)
    return out


def op_attend(q, K, V, H, Hkv, scale):
    """q [H 64], K, V [n][Hkv 64] -> [H 64]"""
    n = K.shape[0]
    return np.concatenate([T(attend(q[None, h * HD:(h + 1) * HD], K.reshape(n, Hkv, HD)[:, h // (H // Hkv)], V.reshape(n, Hkv, HD)[:, h // (H // Hkv)], scale)[0][0])
                           for h in range(H)])


# ------------------------------------------------------------------------------------------------ the entry points
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _L():
    from mlx_audio_swift_amd import _lib as L
    return L.lib()


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def _u16(a):
    return None if a is None else np.ascontiguousarray(a, np.uint16)


def run_conv1(c, T1=None, stride=None):
    pcm, wT, T1 = _f32(c["pcm"]), _f32(c["w"].T), _i32(c["T1"] if T1 is None else T1)
    out = np.full((c["B"], c["T1pad"], c["d"]), np.nan, np.float32)
    st = _L().mis_debug_moonshine_conv1(0, _ptr(pcm), c["stride"] if stride is None else stride, _ptr(T1), c["B"], c["T1pad"], c["d"], _ptr(wT), _ptr(out))
    return st, out


def run_groupnorm(c, stage=2, T1=None):
    B, d, Tp = c["B"], c["d"], c["T1pad"]
    room = -(-Tp * d // GN_CHUNK)
    x, T1, gw, gb = _f32(c["x"]), _i32(c["T1"] if T1 is None else T1), _f32(c["gw"]), _f32(c["gb"])
    p0, p1, stats = np.full((B, room), np.nan, np.float32), np.full((B, room), np.nan, np.float32), np.full((B, 2), np.nan, np.float32)
    y, nch = np.full(B * Tp * d + 8 * d, 0xFFFF, np.uint16), np.full(1, -7, np.int32)
    st = _L().mis_debug_moonshine_groupnorm(0, _ptr(x), _ptr(T1), B, Tp, d, _ptr(gw), _ptr(gb), stage, _ptr(p0), _ptr(p1), _ptr(stats), _ptr(y), _ptr(nch))
    n = max(int(nch[0]), 0)
    return st, p0.reshape(-1)[:B * n].reshape(B, n), p1.reshape(-1)[:B * n].reshape(B, n), stats, y, int(nch[0])


def run_rope(c, rot=None):
    rot = c["rot"] if rot is None else rot
    img = _u16(c["img"]).copy()
    cs, sn = _f32(c["cs"][:c["Tpad"], :rot // 2]), _f32(c["sn"][:c["Tpad"], :rot // 2])
    st = _L().mis_debug_moonshine_rope(0, _ptr(img), c["M"], c["ld"], c["nheads"], c["Tpad"], rot, _ptr(cs), _ptr(sn))
    return st, img


def run_attn(c, T3=None, Hkv=None):
    """kinds 0 / 2 -> (status, out payloads)"""
    T3, Hkv = _i32(c["T3"] if T3 is None else T3), c["Hkv"] if Hkv is None else Hkv
    if c["kind"] == 0:
        out, rows = np.zeros((c["B"] * c["Tpad"], c["H"] * HD), np.uint16), _u16(c["rows"])
        st = _L().mis_debug_moonshine_attn(0, 0, _ptr(rows), None, c["ld"], c["H"], Hkv, _ptr(T3), c["B"], c["Tpad"], c["scale"], c["ldo"], None, None, 0, 0, 0,
                                           None, None, _ptr(out))
        return st, out
    out, q, kv = np.zeros((c["B"], c["H"] * HD), np.uint16), _u16(c["qrows"]), _u16(c["kv"])
    st = _L().mis_debug_moonshine_attn(0, 2, _ptr(q), _ptr(kv), 0, c["H"], Hkv, _ptr(T3), c["B"], c["Tpad"], c["scale"], 0, None, None, 0, 0, 0, None, None, _ptr(out))
    return st, out


def run_self(c, pos=None, Smax=None):
    out, qkv, kc, vc = np.zeros((c["B"], c["H"] * HD), np.uint16), _u16(c["qkv"]), _u16(c["kc"]).copy(), _u16(c["vc"]).copy()
    cs, sn = _f32(c["cs"]), _f32(c["sn"])
    st = _L().mis_debug_moonshine_attn(0, 1, _ptr(qkv), None, 0, c["H"], c["Hkv"], None, c["B"], 0, c["scale"], 0, _ptr(kc), _ptr(vc), c["Smax"] if Smax is None else Smax,
                                       c["pos"] if pos is None else pos, c["rot"], _ptr(cs), _ptr(sn), _ptr(out))
    return st, out, kc, vc


def run_gemv(c, ln=None, epi=None, B=None, K=None):
    ln, epi = c["ln"] if ln is None else ln, c["epi"] if epi is None else epi
    cols = c["N"]
    X, W = bits(c["X"]), bits(c["W"])
    lnw, bias = None if c["lnw"] is None else bits(c["lnw"]), None if c["b"] is None else bits(c["b"])
    out = np.full((c["B"], cols), np.nan, np.float32) if epi == MS_F32 else (bits(c["h"]).copy() if c["h"] is not None else np.zeros((c["B"], cols), np.uint16))
    rep = np.full(2, -7, np.int32)
    st = _L().mis_debug_moonshine_gemv(0, ln, epi, _ptr(X), _ptr(lnw), _ptr(W), _ptr(bias), c["B"] if B is None else B, c["K"] if K is None else K, c["rows"],
                                       c["N"] if epi == MS_GATE else 0, _ptr(out), _ptr(rep))
    return st, out, tuple(int(v) for v in rep)


def run_embed(emb, ids):
    emb, ids = _u16(emb), _i32(ids)
    h = np.full((len(ids), emb.shape[1]), 0xFFFF, np.uint16)
    st = _L().mis_debug_moonshine_embed(0, _ptr(emb), _ptr(ids), len(ids), emb.shape[1], emb.shape[0], _ptr(h))
    return st, h


def run_argmax_embed(c):
    x, emb = _f32(c["x"]), _u16(c["emb"])
    active, n_gen, tokens, done = c["active"].copy(), c["n_gen"].copy(), c["tokens"].copy(), c["done"].copy()
    h = np.full((c["B"], c["d"]), 0xFFFF, np.uint16)
    st = _L().mis_debug_moonshine_argmax_embed(0, _ptr(x), c["B"], c["V"], c["eos"], _ptr(active), _ptr(n_gen), _ptr(tokens), c["stride"], _ptr(done),
                                               _ptr(emb), c["d"], _ptr(h))
    return st, active, n_gen, tokens, done, h
