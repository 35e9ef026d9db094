"""Operator-level reference of the encoder kernels of csrc/whisper_kernels.hip (k_gemm_big / k_gemm_big2 / k_gemm_big3, k_layernorm /
k_layernorm8, k_im2col3, k_scatter_kv, k_attn_prefill / k_attn_prefill2, k_whisper_embed_ln, k_whisper_suppress), inputs whose result is
known exactly, the case tables of tests/test_gpu_enc_ops.py, the launchers' rules restated, and thin wrappers of the mis_debug_* entry
points of csrc/enc_debug.hip (include/mi_speech_debug.h).  Pure numpy, float64, written from the kernel headers; nothing here calls a
kernel to build its data.  tests/test_enc_ref_cpu.py proves every claim below that the GPU test leans on.

Specification, T() = round to bf16:
  GEMM       v = T(sum_k x[m][k] w[n][k] + b[n]);  GELU, GELU_POS: v = T(gelu(v));  RESID: v = T(v + R[m][n]);
             GELU_POS: v = T(v + R[m % pos_rows][n]).  x[m][k] = X[m ldx + k]: rows overlap when ldx < K.
  LayerNorm  y = T((x - mean) rstd w + b), mean and variance two-pass in float32, rstd = 1 / sqrt(var + eps)
  im2col     out[b Tout + t][k C + c] = T(in[b][t stride + k - 1][c]), zero outside 0 .. Tin - 1, k = 0 .. 2
  scatter    the K / V^T image layouts of tests/attn_ref.py per (b, h), tiles of 32 keys; keys T .. tile end are zero, tiles behind untouched
  attention  out = T(sum_j p_j v_j), p = softmax over j < T of q . k_j / sqrt(D)
  embed_ln   h = T(E[id] + P[min(pos, max_pos - 1)]), id outside 0 .. vocab - 1 -> 0; x = LayerNorm(h) (eps 1e-5) in the xpk layout;
             pos_cur = pos_next, pos_next += 1 on active rows; rows batch .. Mpad - 1: id 0 at position 0
  suppress   l[id] = T(l[id] + -1e9) once per listed id of an active row; the begin list only where n_gen == 0

GEMM grid inputs (exact in every summation order up to K = 4096): x in {-1, 0, 1} 2^e, w integers in [-4, 4], so every partial sum is an
integer multiple of 2^e of magnitude <= 4 K <= 2^14 such units - below 2^24, hence exact in float32 in any order and grouping.  The bias
(integers) and the residual / positional rows (multiples of 2^-5 up to 2) keep acc + b and v + R exact too, so each T() is ONE rounding
of an exactly known number and the linear epilogues are compared bit for bit.  GELU: pre-activations are kept in [GELU_LO, GELU_HI] = [-4, 8], inside the
[-6, 8] on which the polynomial is within one ulp, by halving x - below -4 the polynomial's rounding differs from T(gelu64) on 5 % and more of
the grid values (tests/test_enc_ref_cpu.py lists the share per grid), which no case could meet a 1 % cap with; the device's polynomial may differ from T(gelu64) by one bf16 ulp on at most 1 % of a case's elements (GELU_ULP, GELU_SHARE); the additive
half of GELU_POS is checked bit for bit on the device's own GELU output: T(g + P) is one float32 addition and one rounding.

LayerNorm tiers.
  constant rows: x = c (two significant bits): every partial sum k c is exact, mean = c, x - mean = 0, y = T(b) - whatever rstd is.
  balanced rows: d / 2 elements +a, d / 2 elements -a, a in {1, 1.25, 1.5} 2^j: every partial sum is an integer multiple of a (of a^2 in
    the second pass), so mean = 0 and var = a^2 exactly; rstd = 1 / sqrt(a^2 + eps) is two correctly rounded float32 operations behind one
    addition; with w = +-2^i and b = 0 the expression t rstd w + b is ONE rounding (t rstd) whether or not the multiply-add is fused.
  Gaussian rows, to first order in u = 2^-24, with A = mean |x|, sigma = sqrt(var + eps), n_i = |(x_i - mean) rstd w_i|:
    the mean: a float32 sum of d terms in any order and one division,            |dmean| <= (d + 1) u A
    t_i = x_i - mean:                                                             |dt_i| <= |dmean| + u |t_i|
    the variance: squares (2 u + 2 |dmean| |t_i| each), their sum (d u), the division and the addition of eps (2 u):
                                                                                  relative (d + 4) u + 2 |dmean| / sigma  (mean |t| <= sigma)
    rstd: half of that, plus the square root and the division (2 u)
    y: two products and one addition, fused or not                               (3 u) n_i + u |y_i|
    |y - ref| <= ulp_bf16(ref) / 2 + SAFETY u [ (d + 1) A rstd |w_i| + ((d + 4) / 2 + (d + 1) A / sigma + 6) n_i + |ref_i| ]
    SAFETY = 2 (attn_ref's stated factor for what a first-order derivation leaves out); not tuned on the device.

Attention tiers (attn_ref's, for one wave per query row walking the key tiles in order):
  locator: one key per query row scores 2 * 4096 / sqrt(D), every other at most half of that: in float32 p = 1 for the target (hi = 1,
    lo = 0) and exactly 0 elsewhere, earlier tiles are erased by alpha = exp(-362 or less) = 0: out == V[target] bit for bit.
  uniform: q = 0, every p = 1 = (1, 0), V integers in [-8, 8]: out == bf16(float32(sum) / float32(T)); keys T .. tile end hold stale +-1e4
    with zero values, so a leaking mask changes the denominator.
  gaussian: attn_ref's bound with F = key tiles + 1 exp factors, kv_len = T, no eight-way combine:
    E = 2 gamma_D max a_j + u max |s_j| + 2.45 X u + 2 F u + 2^-17 + 2 gamma_(T + F) + gamma_T + 4 u,
    |out - ref| <= ulp_bf16(ref) / 2 + 2 SAFETY E sum_j p_j |v_jd|.
  Cache contract of launch_attn_prefill: keys T .. tile end of the last tile are ZERO (as k_scatter_kv leaves them) - the kernels multiply
  p = 0 by what is there; tiles behind the last one are never read (the cases put NaN there)."""
import ctypes as C
import math
import os

import numpy as np
import torch

import attn_ref as ar
import gemm_ref as gr

OK, GENERATION_FAILED, INVALID_INPUT = 0, 2, 3
BG_NONE, BG_GELU, BG_RESID, BG_GELU_POS = range(4)
K_BIG, K_BIG2, K_BIG3 = range(3)
SAFETY, U, T = ar.SAFETY, ar.U, gr.T
GELU_ULP, GELU_SHARE = 1, 0.01
GELU_LO, GELU_HI = -4.0, 8.0
NAN16 = 0x7FC0
EPS = 1e-5


def b16(v):
    """float32 -> nearest bf16 value"""
    return gr.bf16_value(gr.bf16_bits(np.asarray(v, np.float32)))


def gelu64(v):
    t = torch.as_tensor(np.asarray(v, np.float64))
    return (0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752))).numpy()


# ------------------------------------------------------------------------------------------------ GEMM: the launcher's rule, inputs, cases
def gemm_expected(M, N, K, ldx, epi, mode=1):
    """launch_gemm_big restated: ("err", status) or (kernel, epilogue, WM, WN); mode = MIS_GEMM_BIG3 (unset: 1)"""
    if K % 32 or ldx % 8 or N % 4:
        return ("err", INVALID_INPUT)
    two = K % 64 == 0 and K >= 128
    blocks3 = -(-N // 256) * -(-M // 256)
    if mode != 0 and two and (mode == 2 or blocks3 >= 200):
        return (K_BIG3, epi, 2, 4) if (N >= 4096 or K >= 4096) else (K_BIG3, epi, 4, 2)
    return (K_BIG2 if two else K_BIG, epi, 2, 2)


GEMM_INSTANTIATIONS = ({(K_BIG, e, 2, 2) for e in range(4)} | {(K_BIG2, e, 2, 2) for e in range(4)} | {(K_BIG3, e, 4, 2) for e in range(4)} |
                       {(K_BIG3, e, 2, 4) for e in range(4)})
TILE_CHECK_MAX = 5e7      # M N K above which the every-k-tile-counts check of the inputs is skipped (it costs M N K operations)


def _ldx_of(K, kind):
    """0: dense, 1: K + 8, 2 (K >= 64): rows that overlap by half, a multiple of 8 - Moonshine's conv2 / conv3"""
    return K if kind == 0 or (kind == 2 and K < 64) else K + 8 if kind == 1 else (K // 2 + 7) // 8 * 8


def gemm_cases():
    """the case table: every (K, M, N) of a kernel's edge lists, the epilogue, bias and row stride cycling through them with coprime periods"""
    cases = []

    def sweep(kernel, mode, Ks, Ms, Ns):
        i = 0
        for K in Ks:
            for M in Ms:
                for N in Ns:
                    epi, kind = i % 4, (i // 4 + i) % 3
                    cases.append(dict(kernel=kernel, mode=mode, M=M, N=N, K=K, ldx=_ldx_of(K, kind), epi=epi, bias=(i // 2 + i // 7) % 2 == 0,
                                      pos_rows=77 if M > 77 else M, seed=7000 + len(cases)))
                    i += 1

    sweep(K_BIG, 1, [32, 64, 96, 160, 288], [1, 127, 128, 129, 200], [4, 124, 128, 132, 260])
    sweep(K_BIG2, 0, [128, 192, 320], [1, 127, 128, 129, 200], [4, 124, 128, 132, 260])
    sweep(K_BIG3, 2, [128, 192], [1, 255, 256, 257, 300], [4, 252, 256, 260, 516])
    for epi in range(4):                                   # k_gemm_big3<.., 2, 4>: deep K, wide N
        cases.append(dict(kernel=K_BIG3, mode=2, M=257, N=260, K=4096, ldx=4096, epi=epi, bias=epi % 2 == 0, pos_rows=77, seed=7900 + epi))
        cases.append(dict(kernel=K_BIG3, mode=2, M=40, N=4096, K=128, ldx=136, epi=epi, bias=epi % 2 == 1, pos_rows=7, seed=7910 + epi))
    for c in cases:
        c["expect"] = gemm_expected(c["M"], c["N"], c["K"], c["ldx"], c["epi"], c["mode"])
    return cases


DEFAULT_RULE_CASES = [dict(kernel=K_BIG3, mode=None, M=200 * 256, N=4, K=128, ldx=128, epi=BG_RESID, bias=True, pos_rows=0, seed=7950),
                      dict(kernel=K_BIG2, mode=None, M=199 * 256, N=4, K=128, ldx=128, epi=BG_RESID, bias=True, pos_rows=0, seed=7951)]


def gemm_inputs(c):
    """a case's operands in float64, all exact in bf16: dict(img [(M - 1) ldx + K], x [M][K] (the rows the kernels address), w [N][K], bias [N] or
    None, R [M][N] / [pos_rows][N] or None, pre = x w^T + bias (exact)).  GELU cases: x is halved until every pre-activation lies in [GELU_LO, GELU_HI]."""
    M, N, K, ldx, epi = c["M"], c["N"], c["K"], c["ldx"], c["epi"]
    rng = np.random.default_rng(c["seed"])
    gelu = epi in (BG_GELU, BG_GELU_POS)
    e = gr.x_log2_for_std(K, gr.DENSE_W_RMS) if gelu else -5
    idx = np.arange(M)[:, None] * ldx + np.arange(K)[None, :]
    for _ in range(16):
        img = rng.integers(-1, 2, (M - 1) * ldx + K).astype(np.float64)
        w = rng.integers(-4, 5, (N, K)).astype(np.float64)
        if M * N * K > TILE_CHECK_MAX or gr._tiles_all_count(img[idx], w):
            break
    else:
        raise AssertionError("no input without an inert k-tile found")
    bias = rng.integers(0 if gelu else -3, 4, N).astype(np.float64) if c["bias"] else None
    R = None
    if epi == BG_RESID:
        R = rng.integers(-64, 65, (M, N)).astype(np.float64) * 2.0 ** -5
    elif epi == BG_GELU_POS:
        R = rng.integers(-64, 65, (c["pos_rows"], N)).astype(np.float64) * 2.0 ** -5
    acc = img[idx] @ w.T                                   # integers: exact
    b0 = 0.0 if bias is None else bias[None, :]
    if gelu:
        while (acc * 2.0 ** e + b0).min() < GELU_LO or (acc * 2.0 ** e + b0).max() > GELU_HI:
            e -= 1
    return dict(img=img * 2.0 ** e, x=img[idx] * 2.0 ** e, w=w, bias=bias, R=R, pre=acc * 2.0 ** e + b0, e=e)


def gemm_reference(c, d):
    """(the rounding-point reference [M][N] in float64, g = T(gelu(v)) or None)"""
    v = T(d["pre"])
    if c["epi"] == BG_NONE:
        return v, None
    if c["epi"] == BG_RESID:
        return T(v + d["R"]), None
    g = T(gelu64(v))
    if c["epi"] == BG_GELU:
        return g, g
    return T(g + d["R"][np.arange(c["M"]) % c["pos_rows"]]), g


def add_pos_f32(g, c, d):
    """the additive half of GELU_POS on a given bf16 g: one float32 addition, one rounding"""
    P = d["R"][np.arange(c["M"]) % c["pos_rows"]]
    return b16(np.asarray(g, np.float32) + P.astype(np.float32)).astype(np.float64)


def gemm_f32(d, c, order=None, gelu=None):
    """the specification realised in float32 with the k-tiles of 32 summed in the given order (CPU proofs)"""
    f = np.float32
    x, w = d["x"].astype(f), d["w"].astype(f)
    K = x.shape[1]
    acc = np.zeros((x.shape[0], w.shape[0]), f)
    for t in (range(K // 32) if order is None else order):
        acc = (acc + x[:, 32 * t:32 * t + 32] @ w[:, 32 * t:32 * t + 32].T).astype(f)
    if d["bias"] is not None:
        acc = (acc + d["bias"].astype(f)[None]).astype(f)
    v = b16(acc)
    if c["epi"] in (BG_GELU, BG_GELU_POS):
        v = b16(gelu(v))
    if c["epi"] == BG_RESID:
        v = b16(v + d["R"].astype(f))
    if c["epi"] == BG_GELU_POS:
        v = b16(v + d["R"][np.arange(c["M"]) % c["pos_rows"]].astype(f))
    return v.astype(np.float64)


def gelu_condition(got, want):
    """(worst bf16 ulp distance, share of elements that differ)"""
    dd = gr.bf16_ulp_distance(got, want)
    return int(dd.max()), float(np.mean(dd != 0))


# ------------------------------------------------------------------------------------------------ LayerNorm
LN8_D, LN_D, LN_ROWS = [8, 64, 1280, 2040, 2048], [4, 100, 2056, 2304], [1, 3]


def ln_expected(d):
    return 1 if d % 8 == 0 and d <= 2048 else 0            # (the entry point's buffers are 16-byte aligned)


def ln_gauss_wb(d, seed):
    rng = np.random.default_rng(seed)
    return T(1.0 + 0.5 * rng.standard_normal(d)), T(0.5 * rng.standard_normal(d) + 0.01)


def ln_constant(rows, d, seed):
    """x [rows][d] constant per row, Gaussian w, non-zero b: y == b"""
    rng = np.random.default_rng(seed)
    c = rng.choice([0.25, -0.75, 1.5, -3.0, 6.0], rows)
    w, b = ln_gauss_wb(d, seed + 1)
    b = np.where(b == 0, 0.5, b)
    return np.repeat(c[:, None], d, 1), w, b


def ln_balanced(rows, d, seed):
    """x [rows][d] = +-a_r in a random balanced arrangement, w = +-2^i, b = 0"""
    rng = np.random.default_rng(seed)
    a = rng.choice([1.0, 1.25, 1.5], rows) * 2.0 ** rng.integers(-3, 4, rows)
    sign = np.stack([rng.permutation(np.repeat([1.0, -1.0], d // 2)) for _ in range(rows)])
    w = 2.0 ** rng.integers(-2, 3, d) * rng.choice([-1.0, 1.0], d)
    return sign * a[:, None], w, np.zeros(d), a


def ln_balanced_expected(x, w, a, eps=EPS):
    """the balanced tier's y in float32 numpy: mean 0, var a^2, rstd = 1 / sqrt(a^2 + eps), y = T((x rstd) w)"""
    f = np.float32
    a = np.asarray(a, f)
    rstd = (f(1.0) / np.sqrt((a * a + f(eps)).astype(f))).astype(f)
    return b16(((x.astype(f) * rstd[:, None]).astype(f) * w.astype(f)[None]).astype(f)).astype(np.float64)


def ln_gauss(rows, d, seed):
    rng = np.random.default_rng(seed)
    w, b = ln_gauss_wb(d, seed + 1)
    return T(rng.standard_normal((rows, d)) * 2.0 ** rng.integers(-2, 3, (rows, 1)) + rng.standard_normal((rows, 1))), w, b


def ln_reference(x, w, b, eps=EPS):
    """(y before the final rounding, the per-element bound of the module docstring) in float64"""
    d = x.shape[-1]
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    sigma = np.sqrt(var + eps)
    rstd = 1.0 / sigma
    y = (x - mean) * rstd * w + b
    A = np.abs(x).mean(-1, keepdims=True)
    n = np.abs((x - mean) * rstd * w)
    pre = SAFETY * U * ((d + 1) * A * rstd * np.abs(w) + ((d + 4) / 2.0 + (d + 1) * A / sigma + 6.0) * n + np.abs(y))
    return y, pre + ar.ulp_bf16(np.abs(y) + pre) / 2


def ln_f32(x, w, b, eps=EPS, fused=False, divisor=None):
    """the kernels' arithmetic in float32 numpy (numpy's pairwise sum stands for the block reduction): y as bf16 values"""
    f = np.float32
    x, w, b = x.astype(f), w.astype(f), b.astype(f)
    dd = f(divisor or x.shape[-1])
    mean = (x.sum(-1, dtype=f, keepdims=True) / dd).astype(f)
    t = (x - mean).astype(f)
    var = ((t * t).astype(f).sum(-1, dtype=f, keepdims=True) / dd).astype(f)
    rstd = (f(1.0) / np.sqrt((var + f(eps)).astype(f))).astype(f)
    r = (t * rstd).astype(f)
    if fused:
        return b16((r.astype(np.float64) * w + b).astype(f)).astype(np.float64)     # r w is exact in float64: one rounding, as an fma
    return b16(((r * w).astype(f) + b).astype(f)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ im2col
def im2col_reference(x, Tout, stride):
    """x [B][Tin][C] float64 -> [B Tout][3 C], T() applied, zero outside"""
    B, Tin, Cc = x.shape
    out = np.zeros((B, Tout, 3, Cc))
    for k in range(3):
        ti = np.arange(Tout) * stride + k - 1
        ok = (ti >= 0) & (ti < Tin)
        out[:, ok, k, :] = x[:, ti[ok], :]
    return T(out.reshape(B * Tout, 3 * Cc))


def im2col_f32_values(shape, seed):
    """float32 values that round up, round down and tie in bf16 (payload + 0x8000: a tie, to even both ways), B rows of distinct content"""
    rng = np.random.default_rng(seed)
    hi = rng.integers(0x3C00, 0x4200, shape).astype(np.uint32) | (rng.integers(0, 2, shape).astype(np.uint32) << 15)
    lo = rng.choice(np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x4000, 0xC000], np.uint32), shape)
    return ((hi << 16) | lo).view(np.float32)


# ------------------------------------------------------------------------------------------------ scatter + attention
def scatter_reference(src, ld, kcol0, vcol0, B, Tn, H, D, Spad):
    """src payloads [B Tn][ld] -> the K and V images [B][H][Spad D] (uint16): keys Tn .. tile end zero, tiles behind 0xFFFF"""
    Tt = 32 * -(-Tn // 32)
    K = np.zeros((B, H, Tt, D), np.uint16)
    V = np.zeros((B, H, Tt, D), np.uint16)
    rows = src.reshape(B, Tn, ld)
    K[:, :, :Tn] = rows[:, :, kcol0:kcol0 + H * D].reshape(B, Tn, H, D).transpose(0, 2, 1, 3)
    V[:, :, :Tn] = rows[:, :, vcol0:vcol0 + H * D].reshape(B, Tn, H, D).transpose(0, 2, 1, 3)
    kimg = np.full((B, H, Spad * D), 0xFFFF, np.uint16)
    vimg = np.full((B, H, Spad * D), 0xFFFF, np.uint16)
    kimg[:, :, :Tt * D] = ar.k_to_image(K)
    vimg[:, :, :Tt * D] = ar.v_to_image(V)
    return kimg, vimg


def attn_expected(D, v1):
    """launch_attn_prefill restated (16-byte aligned caches): ("err", status) or (kernel, D)"""
    if D == 64 and not v1:
        return (1, 64)
    return (0, D) if D in (64, 128) else ("err", INVALID_INPUT)


ATTN_T = [1, 31, 32, 33, 64, 255, 256, 257, 300]
ATTN_INSTANTIATIONS = {(1, 64), (0, 64), (0, 128)}


def attn_case(tier, D, Tn, seed, B=2, H=2, ldo_pad=0):
    """one launch: q [B Tn][H D], logical K / V [B][H][Spad][D] float64 (NaN behind the last tile), their images, Spad = tiles + 64"""
    rng = np.random.default_rng(seed)
    Tt = 32 * -(-Tn // 32)
    Spad = Tt + 64
    KV = (B, H, Spad, D)
    j = np.arange(Spad)[None, None, :, None]
    K, V = np.zeros(KV), np.zeros(KV)
    tg = None
    if tier == "locator":
        K[:] = ar.locator_key(np.arange(Spad), D)[None, None]
        b_, h_, j_, d_ = np.meshgrid(np.arange(B), np.arange(H), np.arange(Spad), np.arange(D), indexing="ij")
        V[:] = ar.locator_v(b_, h_, j_, d_)
        tg = (rng.integers(0, 1 << 30, (B, H, 1)) + 13 * np.arange(Tn)[None, None, :]) % Tn
        tg[:, :, 0], tg[:, :, -1] = Tn - 1, 0
        q = ar.locator_key(tg, D)                                                   # [B][H][Tn][D]
    elif tier == "uniform":
        K[:] = rng.integers(-4, 5, KV)
        V[:] = rng.integers(-8, 9, KV)
        q = np.zeros((B, H, Tn, D))
    else:
        K[:] = ar.grid_bf16(0.5 * rng.standard_normal(KV))
        V[:] = ar.grid_bf16(rng.standard_normal(KV))
        q = ar.grid_bf16(rng.standard_normal((B, H, Tn, D)))
    pad = (j >= Tn) & (j < Tt)
    K = np.where(pad, ar.stale(rng, KV) if tier == "uniform" else 0.0, K)           # the cache contract: zero keys (uniform: stale keys) ...
    V = np.where(pad, 0.0, V)                                                       # ... and zero values between T and the tile end
    behind = np.broadcast_to(j >= Tt, KV)
    kb, vb = ar.bits_of(np.where(behind, 0.0, K)), ar.bits_of(np.where(behind, 0.0, V))
    kb[behind], vb[behind] = NAN16, NAN16
    K, V = np.where(behind, np.nan, K), np.where(behind, np.nan, V)
    return dict(tier=tier, D=D, T=Tn, B=B, H=H, Spad=Spad, ldq=3 * H * D, ldo=H * D + ldo_pad, q=q.transpose(0, 2, 1, 3).reshape(B * Tn, H * D),
                K=K, V=V, kimg=ar.k_to_image(kb), vimg=ar.v_to_image(vb), targets=tg)


def attn_reference(c, extra_keys=0, scale=None):
    """float64: (out [B T][H D] before the final rounding, the Gaussian tier's bound); extra_keys / scale: mutations for the CPU sensitivity checks"""
    B, H, D, Tn = c["B"], c["H"], c["D"], c["T"]
    n = Tn + extra_keys
    q = c["q"].reshape(B, Tn, H, D).transpose(0, 2, 1, 3)
    Kb, Vb = c["K"][:, :, :n], c["V"][:, :, :n]
    sc = (1.0 / math.sqrt(D)) if scale is None else scale
    s = sc * np.einsum("bhtd,bhjd->bhtj", q, Kb)
    Mx = s.max(-1, keepdims=True)
    p = np.exp(s - Mx)
    p /= p.sum(-1, keepdims=True)
    o = p @ Vb
    mag = p @ np.abs(Vb)
    a = sc * np.einsum("bhtd,bhjd->bhtj", np.abs(q), np.abs(Kb))
    X = np.abs(s - Mx).max(-1)
    gam = lambda k: k * U / (1.0 - k * U)
    F = -(-Tn // 32) + 1
    E = (2 * gam(D) * a.max(-1) + U * np.abs(s).max(-1) + 2.45 * X * U + 2 * F * U + 2.0 ** -17 + 2 * gam(n + F) + gam(n) + 4 * U)[..., None]
    pre = 2 * SAFETY * E * mag
    flat = lambda v: v.transpose(0, 2, 1, 3).reshape(B * Tn, H * D)
    return flat(o), flat(pre + ar.ulp_bf16(np.abs(o) + pre) / 2)


def attn_exact_expected(c):
    """the locator and the uniform tier's stated outputs [B T][H D]"""
    B, H, D, Tn = c["B"], c["H"], c["D"], c["T"]
    if c["tier"] == "locator":
        o = np.take_along_axis(c["V"], c["targets"][..., None], 2)                  # [B][H][Tn][D]
    else:
        sv = c["V"][:, :, :Tn].sum(2)
        o = np.repeat(b16(sv.astype(np.float32) / np.float32(Tn)).astype(np.float64)[:, :, None, :], Tn, 2)
    return o.transpose(0, 2, 1, 3).reshape(B * Tn, H * D)


def attn_f32(c, mask_leak=0):
    """the prefill kernels' arithmetic in float32 numpy: one wave per query row, 32-key tiles in order, the mask, the online softmax, P = hi + lo,
    np.exp for __expf.  Reads the ZERO / stale keys between T and the tile end as the kernels do.  mask_leak: keys past T let through."""
    f = np.float32
    B, H, D, Tn = c["B"], c["H"], c["D"], c["T"]
    q = c["q"].reshape(B, Tn, H, D).transpose(0, 2, 1, 3).astype(f)
    K, V = c["K"].astype(f), c["V"].astype(f)
    sc = f(1.0 / np.sqrt(f(D)))
    m, l, O = np.full((B, H, Tn), -np.inf, f), np.zeros((B, H, Tn), f), np.zeros((B, H, Tn, D), f)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(-(-Tn // 32)):
            Kt, Vt = K[:, :, 32 * t:32 * t + 32], V[:, :, 32 * t:32 * t + 32]
            s = (np.einsum("bhtd,bhjd->bhtj", q, Kt).astype(f) * sc).astype(f)
            s = np.where(np.arange(32 * t, 32 * t + 32) < Tn + mask_leak, s, f(-np.inf)).astype(f)
            mn = np.maximum(m, s.max(-1))
            alpha = np.exp(m - mn).astype(f)
            pe = np.exp(s - mn[..., None]).astype(f)
            hi = b16(pe)
            lo = b16(pe - hi)
            l = (l * alpha + pe.sum(-1, dtype=f)).astype(f)
            O = ((O * alpha[..., None]).astype(f) + hi @ Vt + lo @ Vt).astype(f)
            m = mn
        o = b16(O / l[..., None]).astype(np.float64)
    return o.transpose(0, 2, 1, 3).reshape(B * Tn, H * D)


# ------------------------------------------------------------------------------------------------ decoder step helpers
def embed_ln_reference(E, P, ids, active, pos_next, lw, lb, max_pos, Mpad):
    """(h [Mpad][d] exact, x before rounding, its bound, pos_cur, pos_next after)"""
    vocab, batch = E.shape[0], len(ids)
    idm = np.zeros(Mpad, np.int64)
    idm[:batch] = np.where((ids < 0) | (ids >= vocab), 0, ids)
    p = np.zeros(Mpad, np.int64)
    p[:batch] = pos_next
    h = T(E[idm] + P[np.minimum(p, max_pos - 1)])
    x, bound = ln_reference(h, lw, lb)
    return h, x, bound, np.asarray(pos_next).copy(), np.asarray(pos_next) + (np.asarray(active) != 0)


def unpack_x(img, Mpad, d):
    m, k = np.meshgrid(np.arange(Mpad), np.arange(d), indexing="ij")
    return img[ar.xpk_index(m, k, Mpad // 16)]


def suppress_reference(l, vocab, sup, bsup, n_gen, active):
    """l [batch][Vpad] float64 (bf16 values) -> after the launch"""
    out = l.copy()
    for b in range(l.shape[0]):
        if active is not None and not active[b]:
            continue
        ids = {int(i) for i in sup} | ({int(i) for i in bsup} if n_gen[b] == 0 else set())
        for i in ids:
            if 0 <= i < vocab:
                out[b, i] = b16(np.float32(l[b, i]) + np.float32(-1e9)).reshape(-1)[0]
    return out


# ------------------------------------------------------------------------------------------------ the entry points
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _L():
    from mlx_audio_swift_amd import _lib as L
    return L.lib()


def _bits(a):
    return None if a is None else np.ascontiguousarray(gr.exact_bits(a))


class env:
    """MIS_GEMM_BIG3 / MIS_ATTN_PREFILL_V1 are read per launch"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = str(self.value)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def run_gemm(c, d, epi=None):
    """mis_debug_gemm_big -> (status, C payloads [M][N] uint16, report)"""
    epi = c["epi"] if epi is None else epi
    out = np.zeros((c["M"], c["N"]), np.uint16)
    rep = np.full(4, -7, np.int32)
    img, w, bias, R = _bits(d["img"]), _bits(d["w"]), _bits(d["bias"]), _bits(d["R"])
    with env("MIS_GEMM_BIG3", c["mode"]):
        st = _L().mis_debug_gemm_big(0, epi, _ptr(img), _ptr(w), _ptr(bias), _ptr(R), c["M"], c["N"], c["K"], c["ldx"], c["pos_rows"], _ptr(out), _ptr(rep))
    return st, out, tuple(int(v) for v in rep)


def run_layernorm(x, w, b, eps=EPS):
    out = np.zeros(x.shape, np.uint16)
    rep = np.full(1, -7, np.int32)
    bx, bw, bb = _bits(x), _bits(w), _bits(b)
    st = _L().mis_debug_enc_layernorm(0, _ptr(bx), _ptr(bw), _ptr(bb), x.shape[0], x.shape[1], eps, _ptr(out), _ptr(rep))
    return st, out, int(rep[0])


def run_im2col(x, is_f32, Tout, stride):
    """x [B][Tin][C]: float32 array (is_f32) or bf16 payloads"""
    B, Tin, Cc = x.shape
    x = np.ascontiguousarray(x)
    out = np.zeros((B * Tout, 3 * Cc), np.uint16)
    st = _L().mis_debug_enc_im2col3(0, _ptr(x), int(is_f32), B, Tin, Cc, Tout, stride, _ptr(out))
    return st, out


def run_scatter(src, ld, kcol0, vcol0, B, Tn, H, D, Spad):
    src = np.ascontiguousarray(src, np.uint16)
    kc, vc = np.zeros((B, H, Spad * D), np.uint16), np.zeros((B, H, Spad * D), np.uint16)
    st = _L().mis_debug_enc_scatter_kv(0, _ptr(src), ld, kcol0, vcol0, B, Tn, H, D, Spad, _ptr(kc), _ptr(vc))
    return st, kc, vc


def run_attn(c, v1=False, kimg=None, vimg=None):
    out = np.zeros((c["B"] * c["T"], c["H"] * c["D"]), np.uint16)
    rep = np.full(2, -7, np.int32)
    q = _bits(c["q"])
    ki = np.ascontiguousarray(c["kimg"] if kimg is None else kimg, np.uint16)
    vi = np.ascontiguousarray(c["vimg"] if vimg is None else vimg, np.uint16)
    with env("MIS_ATTN_PREFILL_V1", 1 if v1 else None):
        st = _L().mis_debug_enc_attn_prefill(0, _ptr(q), c["ldq"], _ptr(ki), _ptr(vi), c["B"], c["T"], c["H"], c["D"], c["Spad"], c["ldo"], _ptr(out), _ptr(rep))
    return st, out, tuple(int(v) for v in rep)


def run_embed_ln(E, P, ids, active, pos_cur, pos_next, lw, lb, max_pos, Mpad):
    vocab, d = E.shape
    batch = len(ids)
    ids, active = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(active, np.uint8)
    pc, pn = np.ascontiguousarray(pos_cur, np.int32).copy(), np.ascontiguousarray(pos_next, np.int32).copy()
    h, x = np.zeros((Mpad, d), np.uint16), np.zeros(Mpad * d, np.uint16)
    be, bp, bw, bb = _bits(E), _bits(P), _bits(lw), _bits(lb)
    st = _L().mis_debug_whisper_embed_ln(0, _ptr(be), _ptr(bp), _ptr(ids), _ptr(active), _ptr(pc), _ptr(pn), _ptr(bw), _ptr(bb), d, vocab, max_pos, batch,
                                         Mpad, _ptr(h), _ptr(x))
    return st, h, x, pc, pn


def run_suppress(l, vocab, sup, bsup, n_gen, active):
    img = _bits(l).copy()
    sup, bsup = np.ascontiguousarray(sup, np.int32), np.ascontiguousarray(bsup, np.int32)
    n_gen = np.ascontiguousarray(n_gen, np.int32)
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    st = _L().mis_debug_whisper_suppress(0, _ptr(img), l.shape[1], vocab, _ptr(sup) if len(sup) else None, len(sup), _ptr(bsup) if len(bsup) else None,
                                         len(bsup), _ptr(n_gen), _ptr(act), l.shape[0])
    return st, img
