"""Operator-level reference of the decode-attention kernels (csrc/lm_kernels.hip: k_attn_decode<D, NIT, XS, QP>, k_attn_decode2<NS>), the
cache layouts, input generators whose result is known exactly, the case table that mirrors launch_attn_decode, and a thin wrapper of
mis_debug_attn_decode (include/mi_speech_debug.h).  Pure numpy, float64; nothing here calls a kernel to build its data.

Specification of one launch (from the kernel headers), T() = round to bf16:
  x = T(sum of the S slabs, in slab order)                               q heads | k | v of the row's kv head
  optional q/k RMSNorm per head:  n = T(x / sqrt(mean x^2 + eps)),  x = T(w n)
  RoPE with the table row of the row's position, pairs (i, i + D/2):     r1 = T(x1 c - x2 s), r2 = T(x1 s + x2 c)
      rope_in_dtype:  c = T(c), s = T(s), r1 = T(T(x1 c) + T(-x2 s)), r2 = T(T(x2 c) + T(x1 s));   no tables: r = x
  append k (after RoPE) and v at position pos of the row's cache, kv_len = pos + 1 (cross-attention: nothing appended, kv_len = cross_len)
  out = T(sum_j p_j v_j), p = softmax over keys j < kv_len of scale q . k_j
  QP prologue (cross-attention): h_new = T(h + T(sum slabs)), x = T(LayerNorm two-pass(h_new) w + b), q = T(W_q x + bias)

Cache layouts (32-key tiles, 8-element fragments of the MFMA operands):
  K   [S/32][2][D/32][64][8]: element e of lane l = 16 g + i of (tile t, half hf, chunk c) is K[32 t + 8 (i >> 2) + (i & 3) + 4 hf][32 c + 8 g + e]
  V^T [S/32][D/16][64][8]:    element e of lane l = 16 g + i of (tile t, dt)           is V[32 t + 8 g + e][16 dt + i]

Three tiers of input.
  locator (exact): every head of every row has ONE key whose score exceeds all others by more than 110, so in float32 every other
    probability is exactly 0 and out == V[target] bit for bit; V encodes (cache row, kv head, key, d).
  uniform (exact): q = 0, every probability 1, V small integers: out == bf16(float32(sum) / float32(kv_len)); K and V hold stale +-1e4
    behind kv_len, so one key too many or too few, or a leaking mask, shows.
  gaussian (bounded): q, k, v known bit for bit (exact slab sums, dyadic RoPE tables); the output is held to

      |out - ref| <= ulp_bf16(ref) / 2 + eps sum_j p_j |v_jd|,        eps = 2 SAFETY E,   u = 2^-24,

    E = 2 gamma_D max_j a_j + u max_j |s_j|        the score: D products accumulated in float32 (gamma_n = n u / (1 - n u), a_j = scale
                                                   sum_i |q_i k_ji|; the factor 2: the MFMA's internal order and rounding are not
                                                   documented as IEEE per add), one rounding of the multiplication by scale
      + (1.45 + 1) X u                             __expf(x) = exp2(x log2 e): one rounding of the product and the rounded constant, relative
                                                   <= 1.45 |x| u in the result; the subtraction s - m itself, |x| u.  The online softmax
                                                   factors exp(s - M) into exp(s - m_tile) exp(m_old - m_new) ... exp(m_wave - M): all
                                                   exponents are <= 0 and add up to s - M, so X = max_j |s_j - M| bounds their sum
                                                   (X over ALL keys, which is conservative; the generators keep X <= 32, far from
                                                   the 87 at which a float32 exp underflows)
      + 2 F u                                      the hardware exp2, 1 ulp (2 u relative) per factor, F = tiles per wave + 1 factors
      + 2^-17                                      P = hi + lo in bf16: |p - hi| <= 2^-9 p, the rounding of lo <= 2^-9 of that
      + 2 gamma_(kv_len + F + 8)                   float32 accumulation of P V over the keys of a wave (factor 2 as above), one rescale by
                                                   alpha per tile, the eight-way combine
      + gamma_(kv_len) + 4 u                       the denominator: sum of p, its combine, the division
    The leading 2 of eps: the numerator's error scales sum p |v|, the denominator's scales |ref| <= sum p |v|.  SAFETY = 2 on top (a
    stated factor for what the derivation treats to first order only); it is not tuned on the device.
  Launches whose q is NOT known exactly (real cos / sin tables, q/k-norm, the QP projection) gain the first-order term
      2 ds sum_j p_j |v_jd - ref_d|,    ds = scale max_j sum_i ulp_bf16(q_i) |k_ji|:
    every q element off by one bf16 ulp."""
import ctypes as C
import math

import numpy as np

import gemm_ref as gr

OK, GENERATION_FAILED, INVALID_INPUT = 0, 2, 3
ATT_WAVES, ATT2_MAX_J, XS_MIN_J, XS_MAX_J, QP_KW = 8, 4, 5, 6, 5
SAFETY = 2.0
U = 2.0 ** -24
T = gr.T


def ulp_bf16(v):
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 7)


def bits_of(v):
    """bf16 payload of representable values"""
    return gr.exact_bits(v)


# ------------------------------------------------------------------------------------------------ layouts
def _k_map(S, D):
    """flat image index of K[s][d], from the READER's side: which (key, dim) element e of lane l of fragment (t, hf, c) holds"""
    t, hf, c, l, e = np.meshgrid(np.arange(S // 32), np.arange(2), np.arange(D // 32), np.arange(64), np.arange(8), indexing="ij")
    g, i = l >> 4, l & 15
    key = 32 * t + 8 * (i >> 2) + (i & 3) + 4 * hf
    dim = 32 * c + 8 * g + e
    m = np.empty((S, D), np.int64)
    m[key.ravel(), dim.ravel()] = np.arange(S * D)
    return m


def _v_map(S, D):
    t, dt, l, e = np.meshgrid(np.arange(S // 32), np.arange(D // 16), np.arange(64), np.arange(8), indexing="ij")
    key = 32 * t + 8 * (l >> 4) + e
    dim = 16 * dt + (l & 15)
    m = np.empty((S, D), np.int64)
    m[key.ravel(), dim.ravel()] = np.arange(S * D)
    return m


_maps = {}


def _map(kind, S, D):
    k = (kind, S, D)
    if k not in _maps:
        _maps[k] = (_k_map if kind == "k" else _v_map)(S, D)
    return _maps[k]


def k_to_image(K):
    """logical [..., S, D] -> image [..., S * D] (any dtype)"""
    S, D = K.shape[-2:]
    img = np.empty(K.shape[:-2] + (S * D,), K.dtype)
    img[..., _map("k", S, D).ravel()] = K.reshape(K.shape[:-2] + (S * D,))
    return img


def k_from_image(img, S, D):
    return img[..., _map("k", S, D).ravel()].reshape(img.shape[:-1] + (S, D))


def v_to_image(V):
    S, D = V.shape[-2:]
    img = np.empty(V.shape[:-2] + (S * D,), V.dtype)
    img[..., _map("v", S, D).ravel()] = V.reshape(V.shape[:-2] + (S * D,))
    return img


def v_from_image(img, S, D):
    return img[..., _map("v", S, D).ravel()].reshape(img.shape[:-1] + (S, D))


def append_k_index(pos, d, D):
    """the index expression of the kernels' append (k_attn_decode prologue), transcribed: an independent second formula of the K layout"""
    ptile, pr = pos >> 5, pos & 31
    prow, phalf = ((pr >> 3) << 2) | (pr & 3), (pr >> 2) & 1
    return ((((ptile * 2 + phalf) * (D // 32) + (d >> 5)) * 64 + (((d & 31) >> 3) << 4) + prow) * 8) + (d & 7)


def append_v_index(pos, d, D):
    ptile, pr = pos >> 5, pos & 31
    return (((ptile * (D // 16) + (d >> 4)) * 64 + ((pr >> 3) << 4) + (d & 15)) * 8) + (pr & 7)


def xpk_index(m, k, MT):
    return ((((k >> 5) * MT + (m >> 4)) * 64) + (((k & 31) >> 3) << 4) + (m & 15)) * 8 + (k & 7)


# ------------------------------------------------------------------------------------------------ the launcher's rule
def nit(G, D):
    return 2 if (G + 2) * D <= 1024 else (5 if D == 128 else 3)


def expected(c, xs_on=True):
    """what launch_attn_decode does with a case: ("err", status) or the report (kernel, D, NIT, XS, QP, NS)"""
    H, Hkv, D, Smax = c["H"], c["Hkv"], c["D"], c["Smax"]
    G = H // Hkv
    qp = c.get("qp")
    if G < 1 or G > 16 or H % Hkv:
        return ("err", INVALID_INPUT)
    smem = nit(G, D) * 512 * 4 + 16 * D * 2 + D * 2 + 2 * ATT_WAVES * 16 * 4 + ATT_WAVES * G * D * 4
    if smem > 64 * 1024:
        return ("err", INVALID_INPUT)
    if not qp and not 1 <= c["S"] <= 8:
        return ("err", GENERATION_FAILED)
    tiles = (c["cross_len"] + 31) // 32
    xs_range = ATT_WAVES * XS_MIN_J <= tiles <= ATT_WAVES * XS_MAX_J
    if qp:
        KT = qp["KT"]
        ok = (xs_on and c["cross"] and D == 64 and H == Hkv and not c["append_only"] and not c["cache_rows"] and c["rope"] is None and
              c["qnorm_w"] is None and xs_range and KT >= 1 and (KT + ATT_WAVES - 1) // ATT_WAVES <= QP_KW and KT * 32 == H * D and 1 <= qp["S"] <= 8)
        if not ok:
            return ("err", GENERATION_FAILED)
    if Smax < 32 or Smax % 32:
        return ("err", INVALID_INPUT)
    if (not c["first_schedule"] and not c["cache_rows"] and not c["append_only"] and D == 128 and not c["cross"] and c["rope"] is not None and
            not c["rope_in_dtype"] and c["qnorm_w"] is None and c["S"] <= 4 and G <= 4 and Smax <= 32 * ATT_WAVES * ATT2_MAX_J):
        return (1, 128, 0, 0, 0, c["S"])
    if D == 128:
        return (0, 128, nit(G, D), 0, 0, 0)
    if (G + 2) * D <= 1024 and c["cross"] and not c["append_only"] and not c["cache_rows"] and xs_on and xs_range:
        return (0, 64, 2, 1, (4 if qp["S"] <= 4 else 8) if qp else 0, 0)
    return (0, 64, nit(G, D), 0, 0, 0)


# the eleven instantiations launch_attn_decode can reach; tests/test_gpu_attn_ops.py asserts that its cases reported every one
INSTANTIATIONS = {(0, 128, 2, 0, 0, 0), (0, 128, 5, 0, 0, 0), (0, 64, 2, 0, 0, 0), (0, 64, 3, 0, 0, 0), (0, 64, 2, 1, 0, 0), (0, 64, 2, 1, 4, 0),
                  (0, 64, 2, 1, 8, 0), (1, 128, 0, 0, 0, 1), (1, 128, 0, 0, 0, 2), (1, 128, 0, 0, 0, 3), (1, 128, 0, 0, 0, 4)}


# ------------------------------------------------------------------------------------------------ generators
def split_exact(x, S, rng):
    """S slabs [S, ...] whose sum is x in float32 whatever the order: every slab is an integer multiple of x's bf16 ulp (2^-20 where x
    is 0), |multiples| < 2^10"""
    g = np.where(x == 0, 2.0 ** -20, ulp_bf16(x))
    parts = [rng.integers(-8, 9, x.shape).astype(np.float64) * g for _ in range(S - 1)]
    first = x - sum(parts) if parts else x.copy()
    out = np.stack([first] + parts)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out


def grid_bf16(v, step=2.0 ** -8):
    """nearest multiple of step, then nearest bf16 (still a multiple of step)"""
    return T(np.round(np.asarray(v, np.float64) / step) * step)


def stale(rng, shape):
    """large finite left-overs, mixed signs, exact in bf16"""
    return (8192.0 + 64.0 * rng.integers(0, 64, shape)) * rng.choice([-1.0, 1.0], shape)


def dyadic_tables(rng, Smax, D, values=(0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.0, -1.0)):
    """cos / sin with at most two significant bits: x c, and x1 c - x2 s for x on the 2^-8 grid below 2^4, are exact in float32 with or without
    fusing.  Not a rotation - the kernel only multiplies by the table."""
    return rng.choice(values, (Smax, D // 2)), rng.choice(values, (Smax, D // 2))


def locator_tables(rng, Smax, D):
    """per entry either (c, 0) or (0, s), c / s in +-{0.5, 1, 2}: exactly invertible, and a wrong row or sign moves q to other components"""
    mag = rng.choice([0.5, 1.0, 2.0], (Smax, D // 2)) * rng.choice([-1.0, 1.0], (Smax, D // 2))
    which = rng.integers(0, 2, (Smax, D // 2)).astype(bool)
    return np.where(which, mag, 0.0), np.where(which, 0.0, mag)


def rope_tables(Smax, D, theta):
    inv = theta ** (-np.arange(D // 2, dtype=np.float64) * 2.0 / D)
    ang = np.arange(Smax, dtype=np.float64)[:, None] * inv[None, :]
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return f32(np.cos(ang)), f32(np.sin(ang))


def unrope_locator(w, c, s):
    """x with rope(x) == w for locator tables"""
    h = w.shape[-1] // 2
    w1, w2 = w[..., :h], w[..., h:]
    cz = np.where(c == 0, 1.0, c)
    sz = np.where(s == 0, 1.0, s)
    x1 = np.where(s == 0, w1 / cz, w2 / sz)
    x2 = np.where(s == 0, w2 / cz, -w1 / sz)
    return np.concatenate([x1, x2], -1)


def locator_key(j, D):
    """designed key j: 64 on components j mod D and (j mod D + 1 + j div D) mod D: q = key(target) scores 2 * 4096 on its target and at
    most 4096 on any other key (they share at most one component)"""
    k = np.zeros(np.shape(j) + (D,))
    idx = np.indices(np.shape(j))
    k[tuple(idx) + (np.asarray(j) % D,)] = 64.0
    k[tuple(idx) + ((np.asarray(j) % D + 1 + np.asarray(j) // D) % D,)] = 64.0
    return k


def locator_v(row, kvh, j, d):
    """bf16 value that encodes (cache row, kv head, key, d): payload 0x3000 + a 12-bit mix (normal numbers around 2^-31 .. 2^-15); two keys
    of one cache agree in no d unless they are 4096 apart"""
    return gr.bf16_value((0x3000 + ((row * 1009 + kvh * 2003 + j * 37 + d * 101) % 4096)).astype(np.uint16)).astype(np.float64)


def build(name, tier, D, G, pos, S=1, Hkv=2, Mpad=None, Smax=None, out_ld=0, rope="dyadic", theta=1e4, rope_in_dtype=0, qknorm=False, cross_len=0,
          cache_rows=0, first_schedule=0, active=None, targets=None, seed=0, append_only=0, scale=None, kamp=0.5, neg_zero=False):
    """one launch as a dict: shapes, logical inputs in float64 (all exactly representable), the cache images before the launch"""
    rng = np.random.default_rng(seed)
    pos = np.asarray(pos, np.int64)
    batch, H, cross = len(pos), G * Hkv, cross_len > 0
    Mpad = Mpad or (batch + 15) // 16 * 16
    rows = cache_rows or batch
    Nqkv = H * D if cross else (H + 2 * Hkv) * D
    act = np.ones(batch, np.uint8) if active is None else np.asarray(active, np.uint8)
    cb = np.arange(batch) % rows
    kv_len = np.full(batch, cross_len) if cross else pos + 1
    if rope == "dyadic":
        tab = dyadic_tables(rng, Smax, D)
    elif rope == "locator":
        tab = locator_tables(rng, Smax, D)
    elif rope == "real":
        tab = rope_tables(Smax, D, theta)
    else:
        tab = None
    prow = np.zeros(batch, np.int64) if cross else pos                     # the table row a launch reads
    KV = (rows, Hkv, Smax, D)
    valid = np.zeros((rows, Smax), bool)                                    # keys the cache holds BEFORE the launch
    for b in range(batch):
        valid[cb[b], :cross_len if cross else pos[b]] = True
    vm = valid[:, None, :, None]
    tg = None
    if tier == "locator":
        jj = np.arange(Smax)
        K = np.where(vm, np.broadcast_to(locator_key(jj, D), KV), stale(rng, KV))
        r_, h_, j_, d_ = np.meshgrid(np.arange(rows), np.arange(Hkv), jj, np.arange(D), indexing="ij")
        vfun = lambda r, h, j, d: locator_v(r, h, j, d)
        V = np.where(vm, vfun(r_, h_, j_, d_), stale(rng, KV))
        base = np.asarray(targets if targets is not None else rng.integers(0, 1 << 30, batch), np.int64)
        tg = (base[:, None] + 7 * np.arange(H)[None, :]) % kv_len[:, None]                 # [batch][H]
        tg[:, 0] = base % kv_len
        qw = locator_key(tg, D)                                                            # post-RoPE q wanted
        kw = np.broadcast_to(locator_key(pos, D)[:, None], (batch, Hkv, D))
        vw = vfun(cb[:, None, None], np.arange(Hkv)[None, :, None], pos[:, None, None], np.arange(D)[None, None, :])
        if tab is not None:
            c_, s_ = tab[0][prow], tab[1][prow]
            qx, kx = unrope_locator(qw, c_[:, None], s_[:, None]), unrope_locator(kw, c_[:, None], s_[:, None])
        else:
            qx, kx = qw, kw
        vx = vw
    elif tier == "uniform":
        K = np.where(vm, rng.integers(-4, 5, KV).astype(np.float64), stale(rng, KV))
        V = np.where(vm, rng.integers(-8, 9, KV).astype(np.float64), stale(rng, KV))
        qx = np.zeros((batch, H, D))
        kx = rng.integers(-4, 5, (batch, Hkv, D)).astype(np.float64)
        vx = rng.integers(-8, 9, (batch, Hkv, D)).astype(np.float64)
    else:
        K = np.where(vm, grid_bf16(kamp * rng.standard_normal(KV)), stale(rng, KV))
        V = np.where(vm, grid_bf16(rng.standard_normal(KV)), stale(rng, KV))
        qx = grid_bf16(rng.standard_normal((batch, H, D)))
        kx = grid_bf16(kamp * rng.standard_normal((batch, Hkv, D)))
        vx = grid_bf16(rng.standard_normal((batch, Hkv, D)))
    x = np.zeros((Mpad, Nqkv))
    x[:batch, :H * D] = qx.reshape(batch, H * D)
    if not cross:
        x[:batch, H * D:(H + Hkv) * D] = kx.reshape(batch, Hkv * D)
        x[:batch, (H + Hkv) * D:] = vx.reshape(batch, Hkv * D)
    if neg_zero:         # (tests/test_gpu_attn_ops.py::test_negative_zero_slab: every fifth k and v element a -0.0)
        x[:batch, H * D + 3::5] = -0.0
    else:
        x = x + 0.0      # no -0.0 in a slab: with ONE slab k_attn_decode computes 0.0f + x (+0) and k_attn_decode2 keeps x (-0) - the one place where the
                         # schedules' bits differ (the sign of a zero in the appended key / value; test_negative_zero_slab holds that case)
    qn = kn = None
    if qknorm:
        qn, kn = T(1.0 + 0.5 * rng.standard_normal(D)), T(1.0 + 0.5 * rng.standard_normal(D))
    return dict(name=name, tier=tier, D=D, H=H, Hkv=Hkv, S=S, Mpad=Mpad, batch=batch, Smax=Smax, Nqkv=Nqkv, pos=pos, active=act, out_ld=out_ld,
                scale=float(scale if scale is not None else 1.0 / math.sqrt(D)), rope=tab, rope_kind=rope, rope_in_dtype=rope_in_dtype, qnorm_w=qn, knorm_w=kn,
                qk_eps=1e-6, cross=int(cross), cross_len=cross_len, cache_rows=cache_rows, append_only=append_only, first_schedule=first_schedule,
                slabs=split_exact(x, S, rng), kimg=bits_of(k_to_image(K)), vimg=bits_of(v_to_image(V)), qp=None, targets=tg,
                exact=rope in ("dyadic", "locator", None) and not qknorm and not rope_in_dtype)


def add_qp(c, qp_S, bias, seed, KT=None):
    """turns a cross-attention case (H = Hkv, D = 64) into a QP launch: slabs with exact sums, h on the 2^-5 grid (h + T(sum) exact in float32,
    so h_new is known bit for bit), Gaussian LayerNorm weights and W_q"""
    rng = np.random.default_rng(seed)
    N, Mpad = c["H"] * c["D"], c["Mpad"]
    o = rng.integers(-64, 65, (Mpad, N)).astype(np.float64) * 2.0 ** -5
    h = rng.integers(-64, 65, (Mpad, N)).astype(np.float64) * 2.0 ** -5
    c["qp"] = dict(S=qp_S, KT=N // 32 if KT is None else KT, slabs=split_exact(o, qp_S, rng), h_in=h, lnw=T(1.0 + 0.5 * rng.standard_normal(N)),
                   lnb=T(0.5 * rng.standard_normal(N)), eps=1e-5, W=T(rng.standard_normal((N, N)) / math.sqrt(N)),
                   bias=T(0.5 * rng.standard_normal(N)) if bias else None)
    c["slabs"], c["S"], c["Nqkv"], c["exact"] = None, 0, 0, False
    return c


# ------------------------------------------------------------------------------------------------ the specification
def _rope(x, c, s, in_dtype, mut=None):
    h = x.shape[-1] // 2
    if mut == "adjacent_pairs":
        x1, x2 = x[..., 0::2], x[..., 1::2]
    else:
        x1, x2 = x[..., :h], x[..., h:]
    if mut == "sin_sign":
        s = -s
    if in_dtype:
        c, s = T(c), T(s)
        r1, r2 = T(T(x1 * c) + T(-x2 * s)), T(T(x2 * c) + T(x1 * s))
    else:
        r1, r2 = T(x1 * c - x2 * s), T(x1 * s + x2 * c)
    if mut == "adjacent_pairs":
        r = np.empty_like(x)
        r[..., 0::2], r[..., 1::2] = r1, r2
        return r
    return np.concatenate([r1, r2], -1)


def _norm(x, w, eps):
    return T(w * T(x / np.sqrt(np.mean(x * x, -1, keepdims=True) + eps)))


def prologue(c, mut=None):
    """(q [batch][H][D], knew [batch][Hkv][D] or None, vnew, h_new or None) of every row, active or not"""
    B, H, Hkv, D = c["batch"], c["H"], c["Hkv"], c["D"]
    h_new = None
    if c["qp"]:
        q_ = c["qp"]
        acc = np.zeros_like(q_["slabs"][0])
        for s in range(q_["S"]):
            acc = acc + q_["slabs"][s]
        h_new = T(q_["h_in"] + T(acc))[:B]
        mean = h_new.mean(-1, keepdims=True)
        var = ((h_new - mean) ** 2).mean(-1, keepdims=True)
        lnw, lnb, W, bias = q_["lnw"], q_["lnb"], q_["W"], q_["bias"]
        if mut == "qp_no_ln_affine":
            lnw, lnb = np.ones_like(lnw), np.zeros_like(lnb)
        if mut == "qp_drop_ktile":                       # the last k-tile of W_q never multiplied
            W = W.copy()
            W[:, -32:] = 0.0
        if mut == "qp_swap_ntiles":                      # n-tiles 0 and 1 of every head exchanged
            W = W.reshape(H, D // 16, 16, -1)[:, [1, 0] + list(range(2, D // 16))].reshape(W.shape)
        if mut == "qp_drop_bias":
            bias = None
        xn = T((h_new - mean) / np.sqrt(var + q_["eps"]) * lnw + lnb)
        q = T(xn @ W.T + (0.0 if bias is None else bias)).reshape(B, H, D)
        return q, None, None, h_new
    acc = np.zeros_like(c["slabs"][0])
    for s in range(c["S"]):
        acc = acc + c["slabs"][s]
    x = T(acc)[:B]
    q = x[:, :H * D].reshape(B, H, D)
    k = v = None
    if not c["cross"]:
        k, v = x[:, H * D:(H + Hkv) * D].reshape(B, Hkv, D), x[:, (H + Hkv) * D:].reshape(B, Hkv, D)
    if c["qnorm_w"] is not None and mut != "norm_after_rope":
        q = _norm(q, c["qnorm_w"], c["qk_eps"])
        k = k if k is None else _norm(k, c["knorm_w"], c["qk_eps"])
    if c["rope"] is not None:
        row = np.zeros(B, np.int64) if c["cross"] else c["pos"] + (1 if mut == "row_plus_one" else 0)
        row = np.minimum(row, c["Smax"] - 1)
        cs, sn = c["rope"][0][row][:, None], c["rope"][1][row][:, None]
        q = _rope(q, cs, sn, c["rope_in_dtype"], mut)
        k = k if k is None else _rope(k, cs, sn, c["rope_in_dtype"], mut)
    if c["qnorm_w"] is not None and mut == "norm_after_rope":
        q = _norm(q, c["qnorm_w"], c["qk_eps"])
        k = k if k is None else _norm(k, c["knorm_w"], c["qk_eps"])
    return q, k, v, h_new


def reference(c, mut=None):
    """the launch in float64: out [batch][H D] BEFORE the final rounding (NaN on rows the launch does not write), the logical caches after
    it, the appended key / value, h_new, and per element the bound of the module docstring (exact launches: `bound`; others: `wide`)"""
    B, H, Hkv, D, Smax = c["batch"], c["H"], c["Hkv"], c["D"], c["Smax"]
    G, rows = H // Hkv, c["cache_rows"] or c["batch"]
    q, knew, vnew, h_new = prologue(c, mut)
    K = gr.bf16_value(k_from_image(c["kimg"].reshape(rows, Hkv, Smax * D), Smax, D)).astype(np.float64)
    V = gr.bf16_value(v_from_image(c["vimg"].reshape(rows, Hkv, Smax * D), Smax, D)).astype(np.float64)
    act = c["active"].astype(bool)
    if not c["cross"]:
        for b in np.nonzero(act)[0]:
            K[b % rows, :, c["pos"][b]] = knew[b]
            V[b % rows, :, c["pos"][b]] = vnew[b]
    out = np.full((B, H * D), np.nan)
    bound, wide, ratio_x = np.full((B, H * D), np.nan), np.full((B, H * D), np.nan), 0.0
    if not c["append_only"]:
        for b in np.nonzero(act)[0]:
            n = int(c["cross_len"] if c["cross"] else c["pos"][b] + 1) + (1 if mut == "kv_len_plus_one" else 0)
            n = min(n, Smax)
            tpw = ((n + 31) // 32 + ATT_WAVES - 1) // ATT_WAVES
            for kvh in range(Hkv):
                Kb, Vb = K[b % rows, kvh, :n], V[b % rows, kvh, :n]
                qh = q[b, kvh * G:(kvh + 1) * G]
                s = c["scale"] * (qh @ Kb.T)
                M = s.max(-1, keepdims=True)
                p = np.exp(s - M)
                p /= p.sum(-1, keepdims=True)
                o = p @ Vb
                mag = p @ np.abs(Vb)
                a = c["scale"] * (np.abs(qh) @ np.abs(Kb).T)
                X = float(np.abs(s - M).max())
                ratio_x = max(ratio_x, X)
                gam = lambda k: k * U / (1.0 - k * U)
                F = tpw + 1
                E = (2 * gam(D) * a.max(-1) + U * np.abs(s).max(-1) + 2.45 * X * U + 2 * F * U + 2.0 ** -17 + 2 * gam(n + F + 8) + gam(n) + 4 * U)[:, None]
                pre = 2 * SAFETY * E * mag
                spread = np.einsum("gj,gjd->gd", p, np.abs(Vb[None] - o[:, None]))
                ds = c["scale"] * (ulp_bf16(qh) @ np.abs(Kb).T).max(-1)
                prew = pre + 2 * ds[:, None] * spread
                sl = slice(kvh * G * D, (kvh + 1) * G * D)
                out[b, sl] = o.reshape(-1)
                bound[b, sl] = (pre + ulp_bf16(np.abs(o) + pre) / 2).reshape(-1)
                wide[b, sl] = (prew + ulp_bf16(np.abs(o) + prew) / 2).reshape(-1)
    return dict(out=out, K=K, V=V, knew=knew, vnew=vnew, h_new=h_new, bound=bound, wide=wide, q=q, xmax=ratio_x)


def uniform_expected(c, r):
    """the uniform tier's exact output: bf16(float32(sum v) / float32(kv_len)), one float32 division as the kernel's combine does"""
    B, H, Hkv, D = c["batch"], c["H"], c["Hkv"], c["D"]
    G, rows = H // Hkv, c["cache_rows"] or B
    out = np.full((B, H * D), np.nan)
    for b in np.nonzero(c["active"])[0]:
        n = int(c["cross_len"] if c["cross"] else c["pos"][b] + 1)
        sv = r["V"][b % rows, :, :n].sum(1)                                               # [Hkv][D], exact integers
        val = gr.bf16_value(gr.bf16_bits(sv.astype(np.float32) / np.float32(n))).astype(np.float64)
        out[b] = np.repeat(val[:, None, :], G, 1).reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------ a float32 realisation (CPU tests)
def realise_f32(c, fused=False):
    """the specification as the kernels compute it, in float32: 32-key tiles, tiles w, w + 8, ... per wave, online softmax, P = hi + lo in bf16,
    float32 accumulation, eight-way log-sum-exp combine; np.exp in float32 stands in for __expf.  The prologue is the float64 one (exact
    launches) - this function is about the main loop.  Returns out [batch][H D] (bf16 values, NaN where not written)."""
    f = np.float32
    B, H, Hkv, D = c["batch"], c["H"], c["Hkv"], c["D"]
    G, rows = H // Hkv, c["cache_rows"] or B
    r = reference(c)
    b16 = lambda v: gr.bf16_value(gr.bf16_bits(np.asarray(v, f)))
    out = np.full((B, H * D), np.nan)
    if c["append_only"]:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        for b in np.nonzero(c["active"])[0]:
            n = int(c["cross_len"] if c["cross"] else c["pos"][b] + 1)
            nt = (n + 31) // 32
            for kvh in range(Hkv):
                Kb, Vb = r["K"][b % rows, kvh].astype(f), r["V"][b % rows, kvh].astype(f)
                qh = r["q"][b, kvh * G:(kvh + 1) * G].astype(f)
                ms, ls, Os = [], [], []
                for w in range(ATT_WAVES):
                    m, l, O = np.full(G, -np.inf, f), np.zeros(G, f), np.zeros((G, D), f)
                    for t in range(w, nt, ATT_WAVES):
                        sc = (qh @ Kb[32 * t:32 * t + 32].T) * f(c["scale"])
                        sc = np.where(np.arange(32 * t, 32 * t + 32)[None] < n, sc, f(-np.inf)).astype(f)
                        mn = np.maximum(m, sc.max(-1))
                        alpha = np.exp(m - mn).astype(f)
                        pe = np.exp(sc - mn[:, None]).astype(f)
                        hi = b16(pe)
                        lo = b16(pe - hi)
                        l = (l * alpha + pe.sum(-1, dtype=f)).astype(f)
                        O = ((O * alpha[:, None]).astype(f) + hi @ Vb[32 * t:32 * t + 32] + lo @ Vb[32 * t:32 * t + 32]).astype(f)
                        m = mn
                    ms.append(m); ls.append(l); Os.append(O)
                ms, ls, Os = np.stack(ms), np.stack(ls), np.stack(Os)
                Mx = ms.max(0)
                fw = np.exp(ms - Mx[None]).astype(f)
                num, den = np.zeros((G, D), f), np.zeros(G, f)
                for w in range(ATT_WAVES):
                    num = (num + fw[w][:, None] * Os[w]).astype(f)
                    den = (den + fw[w] * ls[w]).astype(f)
                out[b, kvh * G * D:(kvh + 1) * G * D] = b16(num / den[:, None]).astype(np.float64).reshape(-1)
    return out


def rope_f32(x, c, s, fused):
    """the RoPE step in float32, plain or with the second product fused into the add (what a compiler may do): [r1 | r2] before the rounding to bf16"""
    f = np.float32
    h = x.shape[-1] // 2
    x1, x2, c, s = x[..., :h].astype(f), x[..., h:].astype(f), np.asarray(c, f), np.asarray(s, f)
    if fused:      # fma(x1, c, -(x2 s)) with the inner product rounded, the outer exact: float64 holds a float32 product exactly
        r1 = (x1.astype(np.float64) * c - (x2 * s).astype(f)).astype(f)
        r2 = (x1.astype(np.float64) * s + (x2 * c).astype(f)).astype(f)
    else:
        r1, r2 = ((x1 * c).astype(f) - (x2 * s).astype(f)).astype(f), ((x1 * s).astype(f) + (x2 * c).astype(f)).astype(f)
    return np.concatenate([r1, r2], -1)


# ------------------------------------------------------------------------------------------------ the entry point
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run(c):
    """mis_debug_attn_decode -> (status, out float32 [Mpad][H D], kimg, vimg after the launch, qp_h_out bf16 values or None, report)"""
    from mlx_audio_swift_amd import _lib as L
    a = L.AttnDebugArgsC()
    keep = []

    def put(v, dt):
        if v is None:
            return None
        arr = np.ascontiguousarray(v, dt)
        keep.append(arr)
        return _ptr(arr)

    f32x = lambda v: None if v is None else np.asarray(v, np.float64).astype(np.float32)
    for k in ("batch", "Mpad", "S", "Nqkv", "H", "Hkv", "D", "Smax", "cache_rows", "append_only", "first_schedule", "cross", "cross_len", "out_ld", "rope_in_dtype"):
        setattr(a, k, int(c[k]))
    a.scale, a.qk_eps = c["scale"], c["qk_eps"]
    Mpad, HD = c["Mpad"], c["H"] * c["D"]
    pos = np.zeros(Mpad, np.int32); pos[:c["batch"]] = c["pos"]
    act = np.zeros(Mpad, np.uint8); act[:c["batch"]] = c["active"]
    a.qkv_part, a.pos, a.active = put(f32x(c["slabs"]), np.float32), put(pos, np.int32), put(act, np.uint8)
    if c["rope"] is not None:
        a.rope_cos, a.rope_sin = put(f32x(c["rope"][0]), np.float32), put(f32x(c["rope"][1]), np.float32)
    if c["qnorm_w"] is not None:
        a.qnorm_w, a.knorm_w = put(bits_of(c["qnorm_w"]), np.uint16), put(bits_of(c["knorm_w"]), np.uint16)
    hout = None
    if c["qp"]:
        q = c["qp"]
        a.qp_S, a.qp_KT, a.qp_eps = q["S"], q["KT"], q["eps"]
        a.qp_w, a.qp_slabs, a.qp_h_in = put(bits_of(q["W"]), np.uint16), put(f32x(q["slabs"]), np.float32), put(bits_of(q["h_in"]), np.uint16)
        a.qp_lnw, a.qp_lnb = put(bits_of(q["lnw"]), np.uint16), put(bits_of(q["lnb"]), np.uint16)
        a.qp_bias = put(None if q["bias"] is None else bits_of(q["bias"]), np.uint16)
        hout = np.zeros((c["batch"], HD), np.uint16)
        a.qp_h_out = _ptr(hout)
    kin, vin = np.ascontiguousarray(c["kimg"], np.uint16), np.ascontiguousarray(c["vimg"], np.uint16)
    kout, vout = np.zeros_like(kin), np.zeros_like(vin)
    out = np.zeros((Mpad, HD), np.float32)
    rep = np.full(6, -7, np.int32)
    a.kcache, a.vtcache, a.kcache_out, a.vtcache_out, a.out, a.report = _ptr(kin), _ptr(vin), _ptr(kout), _ptr(vout), _ptr(out), _ptr(rep)
    st = L.lib().mis_debug_attn_decode(0, C.byref(a))
    return st, out, kout, vout, (None if hout is None else gr.bf16_value(hout).astype(np.float64)), tuple(int(v) for v in rep)


# ------------------------------------------------------------------------------------------------ case lists (tests/test_gpu_attn_ops.py)
POS14 = [0, 1, 30, 31, 32, 33, 255, 256, 257, 511, 512, 543, 544]


def _slots(Smax, seed):
    """32 positions covering every slot pos & 31 once, spread over the tiles of the cache, the last one at Smax - 1"""
    rng = np.random.default_rng(seed)
    return [int(32 * rng.integers(0, Smax // 32) + s) for s in range(31)] + [Smax - 1]


def first_schedule_cases():
    cs = []
    for i, G in enumerate([1, 3, 4, 6, 7, 12]):                 # D = 128: <128, 2> up to G = 6, <128, 5> above
        Smax = 576
        pos = POS14 + [Smax - 1]
        S = [1, 2, 5, 8][i % 4]
        cs.append(build(f"d128_g{G}_gauss", "gauss", 128, G, pos, S=S, Smax=Smax, first_schedule=1, out_ld=0 if i % 2 else G * 2 * 128 + 64, seed=100 + i))
        cs.append(build(f"d128_g{G}_uniform", "uniform", 128, G, pos, S=[8, 5, 2, 1][i % 4], Smax=Smax, first_schedule=1, seed=120 + i))
    for i, G in enumerate([1, 2, 14, 15, 16]):                  # D = 64: <64, 2> up to G = 14, <64, 3> above
        Smax = 576
        pos = POS14 + [Smax - 1]
        cs.append(build(f"d64_g{G}_gauss", "gauss", 64, G, pos, S=[2, 8, 1, 5, 3][i], Smax=Smax, out_ld=0 if i % 2 == 0 else G * 2 * 64, seed=140 + i))
        cs.append(build(f"d64_g{G}_uniform", "uniform", 64, G, pos, S=[1, 2, 5, 8, 4][i], Smax=Smax, rope=None, seed=160 + i))
    # locator: every slot pos & 31 once, the first key, the last key and the new key itself as targets, a tile of every wave; Mpad 32 and 48
    for D, G, Mpad in ((128, 3, 32), (64, 2, 48), (128, 7, 32), (64, 16, 48)):
        Smax = 576
        pos = _slots(Smax, D + G) + ([0] if Mpad == 48 else [])
        rng = np.random.default_rng(D * G)
        tg = [0 if b % 3 == 0 else (pos[b] if b % 3 == 1 else int(rng.integers(0, pos[b] + 1))) for b in range(len(pos))]
        tg[31] = Smax - 2
        cs.append(build(f"d{D}_g{G}_locator", "locator", D, G, pos, S=3, Smax=Smax, Mpad=Mpad, rope="locator", first_schedule=1, targets=tg, seed=180 + G))
    return cs


def second_schedule_cases():
    """pos so that waves hold 0 .. 4 tiles, the new key's tile owned by wave 0, wave 7 and waves between, pos = Smax - 1 at Smax = 1024"""
    cs = []
    pos = [0, 31, 32, 100, 255, 256, 300, 511, 543, 700, 767, 770, 800, 1000, 1023, 5]   # new-key tiles 0, 0, 1, 3, 7, 8, 9, 15, 16, 21, 23, 24, 25, 31, 31, 0
    for i, (NS, G) in enumerate([(1, 1), (2, 3), (3, 4), (4, 1), (1, 4), (2, 1), (3, 3), (4, 4)]):
        tier = ["gauss", "uniform", "locator"][i % 3]
        rope = "locator" if tier == "locator" else "dyadic"
        tg = [0 if b % 3 == 0 else (pos[b] if b % 3 == 1 else pos[b] // 2) for b in range(len(pos))]
        cs.append(build(f"s2_ns{NS}_g{G}_{tier}", tier, 128, G, pos, S=NS, Smax=1024, rope=rope, targets=tg, out_ld=0 if i % 2 else G * 2 * 128, seed=200 + i))
    return cs


def flavour_cases():
    """real-valued prologues.  Keys of amplitude 2 (scores of standard deviation about 2: a handful of keys carry each softmax) - with flat
    softmaxes the widened bound would not tell a wrong q from a right one (tests/test_attn_ref_cpu.py, sensitivity)"""
    pos = [0, 5, 31, 32, 100, 255, 256, 300]
    kw = dict(Smax=320, kamp=2.0)
    return [build("qknorm_d128", "gauss", 128, 2, pos, S=2, rope="real", theta=1e6, qknorm=True, seed=300, **kw),
            build("qknorm_d64", "gauss", 64, 2, pos, S=2, rope="real", theta=1e4, qknorm=True, seed=301, **kw),
            build("rope_in_dtype", "gauss", 128, 2, pos, S=1, rope="real", theta=1e6, rope_in_dtype=1, seed=302, **kw),
            build("real_theta1e4", "gauss", 128, 4, pos, S=3, rope="real", theta=1e4, first_schedule=1, seed=303, **kw),
            build("real_theta1e6", "gauss", 64, 4, pos, S=3, rope="real", theta=1e6, seed=304, **kw),
            build("whisper_self_d64", "gauss", 64, 1, pos, S=4, rope=None, seed=305, **kw)]


def cross_cases():
    cs = []
    for i, L in enumerate([1, 31, 33, 200]):
        tier = ["uniform", "gauss", "locator", "uniform"][i]
        cs.append(build(f"cross_{L}_{tier}", tier, 64, [1, 2, 3, 1][i], [0] * 5, S=[1, 2, 3, 8][i], Smax=256, rope=None, cross_len=L, seed=400 + i))
    return cs


def xs_cases():
    return [build(f"xs_{L}_{tier}", tier, 64, G, [0] * 3, S=S, Smax=1536, rope=None, cross_len=L, seed=420 + L)
            for (L, tier, G, S) in ((1280, "uniform", 1, 1), (1500, "gauss", 2, 4), (1536, "locator", 1, 2), (1500, "uniform", 1, 3), (1290, "locator", 14, 1))]


QP_KAMP = 2.0      # keys of amplitude 2: peaked softmaxes, so that the output depends on q (tests/test_attn_ref_cpu.py: a wrong projection leaves the widened bound)


def qp_cases():
    cs = []
    for i, (H, qS, bias) in enumerate([(2, 1, True), (2, 5, False), (6, 4, False), (6, 8, True), (20, 4, True), (20, 5, False)]):
        c = build(f"qp_h{H}_s{qS}_{'bias' if bias else 'nobias'}", "gauss", 64, 1, [0] * 3, Hkv=H, Smax=1536, rope=None, cross_len=[1500, 1280, 1536][i % 3], seed=440 + i,
                  kamp=QP_KAMP)
        cs.append(add_qp(c, qS, bias, 460 + i))
    return cs


def prefill_pair():
    """cache_rows = 3 with 3 x 5 (position, sequence) rows: the append-only launch; the test repeats it as an attending launch on the cache
    images the first one returned (which it has just held to the reference)"""
    pos = [t for t in (30, 31, 32, 33, 34) for _ in range(3)]
    return build("prefill_append", "gauss", 128, 2, pos, S=2, Smax=64, cache_rows=3, append_only=1, out_ld=4 * 128, seed=500)


def contract_cases():
    """inactive rows interleaved with active ones at rows 0 .. 7 (the `active` word at b >> 2, byte b & 3), both schedules and cross-attention"""
    act = [1, 0, 1, 1, 0, 0, 1, 0, 0, 1, 1]
    pos = [40, 3, 0, 31, 7, 90, 64, 12, 33, 95, 32]
    return [build("inactive_s1", "locator", 128, 2, pos, S=2, Smax=96, rope="locator", first_schedule=1, active=act, seed=600),
            build("inactive_s2", "uniform", 128, 2, pos, S=2, Smax=96, active=act, seed=601),
            build("inactive_d64", "gauss", 64, 3, pos, S=1, Smax=96, active=act, out_ld=6 * 64, seed=602),
            build("inactive_cross", "locator", 64, 1, [0] * 11, S=1, Smax=96, rope=None, cross_len=77, active=act, seed=603)]


_cases = {}


def gpu_cases():
    """every launch of tests/test_gpu_attn_ops.py's sweep, built once per process"""
    if not _cases:
        for c in first_schedule_cases() + second_schedule_cases() + flavour_cases() + cross_cases() + xs_cases() + qp_cases() + contract_cases():
            assert c["name"] not in _cases
            _cases[c["name"]] = c
    return list(_cases.values())


KEY_SHARE_CAP = 0.01      # share of appended-key elements that may differ (by one bf16 ulp) from T(float64) under real tables / q/k-norm:
                          # tests/test_attn_ref_cpu.py measures 0 for a float32 prologue, fused or not, on the cases above


def new_key_f32(c, fused):
    """the appended key of every row with the prologue in float32 (the slab sum is exact): q/k-norm and RoPE as the kernel orders them"""
    f = np.float32
    B, H, Hkv, D = c["batch"], c["H"], c["Hkv"], c["D"]
    b16 = lambda v: gr.bf16_value(gr.bf16_bits(np.asarray(v, f)))
    x = T(c["slabs"].sum(0))[:B, H * D:(H + Hkv) * D].reshape(B, Hkv, D).astype(f)
    if c["knorm_w"] is not None:
        ss = (x * x).sum(-1, keepdims=True, dtype=f)
        inv = (f(1.0) / np.sqrt(ss / f(D) + f(c["qk_eps"]), dtype=f)).astype(f)
        x = b16(c["knorm_w"].astype(f) * b16(x * inv))
    if c["rope"] is None:
        return x.astype(np.float64)
    cs, sn = c["rope"][0][c["pos"]][:, None].astype(f), c["rope"][1][c["pos"]][:, None].astype(f)
    if c["rope_in_dtype"]:
        h = D // 2
        cs, sn, x1, x2 = b16(cs), b16(sn), x[..., :h], x[..., h:]
        return np.concatenate([b16(b16(x1 * cs) + b16(-x2 * sn)), b16(b16(x2 * cs) + b16(x1 * sn))], -1).astype(np.float64)
    return b16(rope_f32(x, cs, sn, fused)).astype(np.float64)
