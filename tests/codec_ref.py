"""Operator-level reference for the codec kernels behind csrc/codec_kernels.h: launch_gemm (k_snac_gemm, k_conv_taps, k_pw_fused and the
split-bf16 path of csrc/codec_bf3.hip), launch_codec_final / _hist / _embed, launch_dw7 and launch_vq_nearest - written in float64 numpy
from the specification in codec_kernels.h and the kernel headers, not from the tile code - together with the inputs on which the
comparison is exact, the derived bounds where it cannot be, and the callers of the mis_debug_codec_* entry points.

Three input families (proven in tests/test_codec_ref_cpu.py, used by tests/test_gpu_codec_ops.py):
  grid      A^T small integers, X in {-1, 0, 1} 2^-5, bias / R / scale / noise on power-of-two grids: every value is exact in bf16 (the low
            halves of the split are zero) and every partial sum, in any order, is an integer multiple of one power of two below 2^24
            units - so every summation order gives the same float32 bits, on the exact-f32 kernels and on the split-bf16 kernels alike.
  two-limb  v = hi + lo, hi = +-(1 + h / 4), lo = l 2^-12 (|l| <= 7): bf16(v) == hi and bf16(v - hi) == lo exactly.  The split-bf16 kernels
            must return the three-term sum xh wh + xh wl + xl wh (exact in float32: multiples of 2^-14 below 2^10) - not the full product.
  gaussian  what cannot be exact (Snake with alpha != 0, GELU, the noise generator, accumulation in float32): a per-element bound derived
            from documented errors, see bound_gemm.
"""
import contextlib
import ctypes as C
import math
import os

import numpy as np

PLAIN, RESID, NOISE, CONVT, GELU, TAPS = range(6)                    # the GEMM_* modes of codec_kernels.h
K_SNAC, K_TAPS, K_FUSED, K_BF3 = range(4)                            # report[0] of mis_debug_codec_gemm
OK, GENERATION_FAILED, INVALID_INPUT = 0, 2, 3
U = 2.0 ** -24                                                       # float32 unit roundoff
SIN_SQ_ERR = 3.5e-7                                                  # mis_sin_sq, absolute (tests/test_codec_math_cpu.py)
ONE_BY_ONE = (PLAIN, RESID, NOISE, GELU)
LOW = dict(MIS_BF3_MIN_K1="32", MIS_BF3_MIN_MK_CONVT="0")            # thresholds that let small shapes reach the split-bf16 kernels

_erf = np.vectorize(math.erf, otypes=[np.float64])


# ------------------------------------------------------------------------------------------------ cases
def case(mode, M, N, K=None, batch=1, **kw):
    """a launch_gemm call: the fields of GemmParams with the defaults of a dense call (Tin = Tout = N, strides dense)"""
    c = dict(mode=mode, snake=0, batch=batch, use_pack=0, M=M, K=K, N=N, Tin=N, Tout=N, s=0, pad=0, Cin=0, ldx=0, ldy=0, x_lo=0, dup_bias_n0=0,
             split_k_ok=0, taps=0, dil=0, bias=1, resid=int(mode == RESID), scale=0, seed=1)
    c.update(kw)
    if mode == TAPS:
        c["K"] = c["taps"] * c["Cin"]
    if mode == CONVT:
        c["K"] = c["ntaps"] * c["Cin"]
        c["snake"] = 1
        c["Tin"] = c.get("Tin_", N)
    assert c["K"]
    return c


def kx_of(c):
    return c["K"] if c["mode"] in ONE_BY_ONE else c["Cin"]


def hist_of(c):
    return max(-c["x_lo"], 0)


# ------------------------------------------------------------------------------------------------ inputs
def _chunks_all_count(at, x, Cin):
    """every 16-wide channel chunk of every tap contributes something non-zero to y, and no two (tap, chunk) pairs contribute the same:
    dropping, doubling or swapping a chunk or a tap changes the result (the idea of gemm_ref._tiles_all_count).  at [J][Cin][M], x [Cin][W]"""
    J = at.shape[0]
    seen = set()
    for j in range(J):
        for c0 in range(0, Cin, 16):
            part = at[j, c0:c0 + 16].T @ x[c0:c0 + 16]
            if not part.any():
                return False
            seen.add(part.tobytes())
    return len(seen) == J * ((Cin + 15) // 16)


def _taps_of(c):
    if c["mode"] == TAPS:
        return c["taps"]
    if c["mode"] == CONVT:
        return c["ntaps"] * c["s"]
    return 1


def grid_inputs(c):
    """the grid family for a case: dict of float64 arrays (None where the case has no such operand)"""
    rng = np.random.default_rng(c["seed"])
    M, B, N, Kx, J = c["M"], c["batch"], c["N"], kx_of(c), _taps_of(c)
    W = hist_of(c) + c["Tin"]
    ck = np.arange((Kx + 15) // 16)
    row = np.minimum(ck * 16 + (5 * ck + 3) % 16, Kx - 1)                     # one forced channel per chunk
    for _ in range(32):
        at = rng.integers(-4, 5, (J, Kx, M)).astype(np.float64)
        x = rng.integers(-1, 2, (B, Kx, W)).astype(np.float64)
        for j in range(J):
            at[j, row] = (1.0 + (np.arange(M)[None, :] + ck[:, None] + 2 * j) % 4) * np.where((ck[:, None] + j) % 2 == 0, 1.0, -1.0)
        x[:, row] = np.where((np.arange(W)[None, :] + ck[:, None]) % 2 == 0, 1.0, -1.0)
        if _chunks_all_count(at, x[0], Kx):
            break
    else:                                                                      # a handful of outputs cannot tell dozens of chunks apart
        assert M * W < 64, "no grid input without an inert chunk found"
    inp = dict(AT=at.reshape(-1, M), X=x * 2.0 ** -5, bias=None, R=None, scale=None, noise=None, alpha=None, ralpha=None)
    if c["bias"]:
        inp["bias"] = rng.integers(-8, 9, M) * 2.0 ** -5
    if c["resid"]:
        inp["R"] = rng.integers(-64, 65, (B, M, c["Tout"])) * 2.0 ** -5
    if c["scale"]:
        inp["scale"] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], M)
    if c["mode"] == NOISE:
        inp["noise"] = rng.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], (B, N))
    if c["snake"]:                                                             # plumbing only: alpha = 0 is the identity, bit for bit
        inp["alpha"] = np.zeros(Kx)
        inp["ralpha"] = rng.integers(1, 5, Kx).astype(np.float64)
    return inp


def with_dead_channel_snake(c, inp):
    """second Snake plumbing case: a non-zero alpha for channels whose inputs are ALL zero (snake(0) = 0 whatever alpha is)"""
    inp = dict(inp, X=inp["X"].copy(), alpha=inp["alpha"].copy())
    dead = np.arange(1, kx_of(c), 3)
    inp["X"][:, dead] = 0.0
    inp["alpha"][dead] = 1.7
    return inp


def _two_limb(rng, shape):
    hi = (1.0 + rng.integers(0, 4, shape) / 4.0) * rng.choice([-1.0, 1.0], shape)
    lo = rng.integers(-7, 8, shape) * 2.0 ** -12
    return hi, lo


def two_limb_inputs(c):
    """split-bf16 path only.  Returns the inputs (X and A^T as hi + lo) and the limbs; asserts the distinctness the comparison leans on"""
    rng = np.random.default_rng(1000 + c["seed"])
    M, B, N, Kx, J = c["M"], c["batch"], c["N"], kx_of(c), _taps_of(c)
    W = hist_of(c) + c["Tin"]
    ah, al = _two_limb(rng, (J * Kx, M))
    xh, xl = _two_limb(rng, (B, Kx, W))
    inp = dict(AT=ah + al, X=xh + xl, bias=None, R=None, scale=None, noise=None, alpha=None, ralpha=None)
    if c["bias"]:
        inp["bias"] = rng.integers(-8, 9, M) * 2.0 ** -5
    if c["resid"]:
        inp["R"] = rng.integers(-64, 65, (B, M, c["Tout"])) * 2.0 ** -5
    if c["scale"]:
        inp["scale"] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], M)
    if c["mode"] == NOISE:
        inp["noise"] = rng.choice([-1.0, -0.5, 0.5, 1.0], (B, N))
    if c["snake"]:
        inp["alpha"] = np.zeros(Kx)
        inp["ralpha"] = np.ones(Kx)
    limbs = dict(ah=ah, al=al, xh=xh, xl=xl)
    # exactness: every partial sum of the three term sums is a multiple of 2^-14 and, bounded by the sum of magnitudes, below 2^10
    assert c["K"] * (1.75 + 7 * 2.0 ** -12) ** 2 < 2.0 ** 10, "two-limb case too long for exact float32 sums"
    t = [contract(c, dict(inp, AT=a, X=x), raw=True) for a, x in ((ah, xh), (al, xh), (ah, xl), (al, xl))]
    ok = np.isfinite(t[0]) & (contract(c, inp, raw=True, mag=True) > 0)         # outputs that some input column reaches
    distinct = ok.copy()
    for i in range(4):
        distinct &= t[i] != 0
        for k in range(i):
            distinct &= t[i] != t[k]
    assert distinct[ok].mean() > 0.9, "two-limb inputs: the term sums do not tell the cross terms apart"
    return inp, limbs


def gaussian_inputs(c, alpha=True):
    rng = np.random.default_rng(2000 + c["seed"])
    M, B, N, Kx, J = c["M"], c["batch"], c["N"], kx_of(c), _taps_of(c)
    W = hist_of(c) + c["Tin"]
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    inp = dict(AT=f(rng.standard_normal((J * Kx, M)) / math.sqrt(c["K"])), X=f(rng.standard_normal((B, Kx, W))), bias=None, R=None, scale=None,
               noise=None, alpha=None, ralpha=None)
    if c["bias"]:
        inp["bias"] = f(rng.standard_normal(M) * 0.1)
    if c["resid"]:
        inp["R"] = f(rng.standard_normal((B, M, c["Tout"])))
    if c["scale"]:
        inp["scale"] = f(rng.standard_normal(M))
    if c["mode"] == NOISE:
        inp["noise"] = f(rng.standard_normal((B, N)))
    if c["snake"]:
        a = f(np.exp(rng.standard_normal(Kx) * 0.5)) if alpha else np.zeros(Kx)
        inp["alpha"] = a
        inp["ralpha"] = f(1.0 / (a + 1e-9)) if alpha else np.ones(Kx)
    return inp


# ------------------------------------------------------------------------------------------------ reference
def snake(x, alpha, ralpha):
    """x + ra sin^2(a x) per channel; x [B][C][W]"""
    if alpha is None:
        return x
    return x + ralpha[None, :, None] * np.sin(alpha[None, :, None] * x) ** 2


def _columns(xa, hist, Tin, n):
    """columns n (any integers) of x [B][C][hist + Tin]: zero outside [-hist, Tin)"""
    n = np.asarray(n)
    ok = (n >= -hist) & (n < Tin)
    out = np.zeros(xa.shape[:2] + (n.size,))
    out[..., ok] = xa[..., n[ok] + hist]
    return out


def contract(c, inp, raw=False, mag=False, ein=np.einsum):
    """acc [B][M][Tout] of the mode (float64; CONVT: NaN where no phase writes), before bias and epilogue.  mag: sum |a| |act(x)| instead.
    raw: no Snake.  ein: the einsum that contracts one tap (emulate_f32 passes a float32 one)"""
    mode, M, N, B, Cin = c["mode"], c["M"], c["N"], c["batch"], kx_of(c)
    at = np.asarray(inp["AT"], np.float64).reshape(-1, Cin, M)
    xa = np.asarray(inp["X"], np.float64)
    if c["snake"] and not raw:
        xa = snake(xa, inp["alpha"], inp["ralpha"])
    if mag:
        at, xa = np.abs(at), np.abs(xa)
    hist, Tin = hist_of(c), c["Tin"]
    n = np.arange(N)
    out = np.full((B, M, c["Tout"]), np.nan)
    if mode == TAPS:
        acc = sum(ein("km,bkn->bmn", at[j], _columns(xa, hist, Tin, n - c["pad"] + j * c["dil"])) for j in range(c["taps"]))
        out[:, :, :N] = acc
    elif mode == CONVT:
        s, J = c["s"], c["ntaps"]
        for phase in range(s):
            q = (phase + c["pad"]) // s
            acc = sum(ein("km,bkn->bmn", at[phase * J + j], _columns(xa, hist, Tin, n + q - j)) for j in range(J))
            o = s * n + phase
            out[:, :, o[o < c["Tout"]]] = acc[:, :, o < c["Tout"]]
    else:
        out[:, :, :N] = ein("km,bkn->bmn", at[0], _columns(xa, hist, Tin, n))
    return out


def gelu(v):
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))


def epilogue(c, inp, acc, noise=None):
    """acc [B][M][Tout] -> Y, the epilogue of the mode"""
    mode, N = c["mode"], c["N"]
    v = acc.copy()
    if inp["bias"] is not None:
        v += inp["bias"][None, :, None]
        if mode == CONVT and c["dup_bias_n0"]:
            v[:, :, :c["s"]] += inp["bias"][None, :, None]                   # output frame n = 0: o = phase < s
    if mode == GELU:
        return gelu(v)
    if mode == RESID or (mode == TAPS and inp["R"] is not None):
        if inp["scale"] is not None:
            v = v * inp["scale"][None, :, None]
        return inp["R"] + v
    if mode == NOISE:
        nz = inp["noise"] if noise is None else noise
        return inp["X"][:, :c["M"], hist_of(c):hist_of(c) + N] + nz[:, None, :] * v[:, :, :N]
    return v


def ref_gemm(c, inp):
    return epilogue(c, inp, contract(c, inp))


def ref_three_term(c, inp, limbs):
    """what the split-bf16 kernels compute on two-limb inputs: xh wh + xh wl + xl wh"""
    terms = [(limbs["ah"], limbs["xh"]), (limbs["al"], limbs["xh"]), (limbs["ah"], limbs["xl"])]
    acc = sum(contract(c, dict(inp, AT=a, X=x), raw=True) for a, x in terms)
    return epilogue(c, inp, acc)


def bound_gemm(c, inp, split):
    """per-element bound of |device - ref_gemm| on Gaussian data, derived from what the sources document (factor 2 on the accumulation for
    the undocumented internal order of the MFMA):
      accumulation   2 (K + 2) u sum |a| |act(x)|              float32 sum of K products, bias and epilogue adds
      Snake          sum |a| (|ra| (3.5e-7 + u |a_c x|) + u |act(x)|): mis_sin_sq absolute error, the rounding of its argument (|d sin^2| <= 1) and of the fma
      split          (2 2^-18 + 2^-16) sum |a| |act(x)|        pair error per operand and the dropped lo.lo term (csrc/codec_bf3.hip)
      epilogue       RESID: |scale| on all of it + u |Y|; GELU: |g'| <= 1.13 on it + |v| 2^-22 (erff within 4 ulp of a value <= 1, the
                     rounding of its argument) + 2 u |Y|; NOISE: |noise| on it + u |Y|"""
    mag = contract(c, inp, mag=True)
    b = 2.0 * (c["K"] + 2) * U * mag
    if c["snake"] and inp["alpha"] is not None and np.any(inp["alpha"]):
        xa = np.abs(np.asarray(inp["X"], np.float64))
        a, ra = np.abs(inp["alpha"])[None, :, None], np.abs(inp["ralpha"])[None, :, None]
        dx = ra * (SIN_SQ_ERR + U * a * xa) + U * np.abs(snake(inp["X"], inp["alpha"], inp["ralpha"]))
        b = b + contract(c, dict(inp, X=dx, AT=np.abs(inp["AT"])), raw=True)
    if split:
        b = b + (2 * 2.0 ** -18 + 2.0 ** -16) * mag
    y = np.abs(ref_gemm(c, inp))
    v = np.abs(epilogue(dict(c, mode=PLAIN), inp, contract(c, inp)))
    mode = c["mode"]
    if mode == GELU:
        return 1.13 * b + v * 2.0 ** -22 + 2 * U * y
    if mode == RESID or (mode == TAPS and inp["R"] is not None):
        if inp["scale"] is not None:
            b = b * np.abs(inp["scale"])[None, :, None] + U * np.abs(v * inp["scale"][None, :, None])
        return b + U * y
    if mode == NOISE:
        return b * np.abs(inp["noise"])[:, None, :] + 2 * U * (y + np.abs(inp["X"][:, :c["M"], :c["N"]]))
    return b + U * y


# ---- the internal noise generator of the NOISE mode (k_snac_gemm header: Box-Muller on mis-synth-v1 uniforms keyed by (key, GLOBAL row, n))
def rng_noise(key, rows, N):
    """float64 value of the generator on its float32 uniforms, and the bound of the float32 evaluation.
    nz = sqrtf(-2 logf(u1)) cosf(2 pi u2): logf 1 ulp, sqrtf 1 ulp, cosf 2 ulp (HIP math library, documented maxima); the float32 argument
    2 pi u2 is off by at most |arg| (u + 2^-25) (product rounding, the rounded constant), |d cos| <= |d arg|"""
    M64, F = (1 << 64) - 1, np.float32
    out = np.zeros((len(rows), N))
    bnd = np.zeros((len(rows), N))

    def splitmix(z):
        z = (z + 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    for i, row in enumerate(rows):
        for n in range(N):
            u = splitmix(((key ^ ((row * 0xD1B54A32D192ED03) & M64)) + n) & M64)
            u1 = float((F(u >> 40) + F(0.5)) * F(2.0 ** -24))                 # mis-synth-v1 uniforms are DEFINED in float32 (oracle/synth.py):
            u2 = float((F((u >> 16) & 0xFFFFFF) + F(0.5)) * F(2.0 ** -24))    # 24 bits + 0.5 rounds to even from 2^23 on
            r, arg = math.sqrt(-2.0 * math.log(u1)), 2.0 * math.pi * u2
            out[i, n] = r * math.cos(arg)
            d_r = r * (0.5 * 2 * U + 2 * U)                                   # logf 1 ulp (halved by the root), sqrtf 1 ulp
            d_c = arg * (U + 2.0 ** -25) + 4 * U                              # argument, cosf 2 ulp of a value <= 1
            bnd[i, n] = d_r * abs(math.cos(arg)) + r * d_c + U * abs(out[i, n])
    return out, bnd


# ------------------------------------------------------------------------------------------------ float32 emulation (CPU proof of the bounds)
def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).view(np.float32)


def emulate_f32(c, inp, split, sin_sq_f32):
    """the kernels' arithmetic in numpy float32: Snake through the restated mis_sin_sq, float32 contraction (split: three bf16 term sums);
    the epilogue in float64 on the float32 sums, rounded once.  Not the kernels' summation order - the bound must hold for any"""
    F = np.float32
    f = {k: (None if v is None else np.asarray(v, F)) for k, v in inp.items()}
    x = f["X"]
    if c["snake"]:
        a, ra = f["alpha"][None, :, None], f["ralpha"][None, :, None]
        x = (ra.astype(np.float64) * sin_sq_f32(a * x).astype(np.float64) + x.astype(np.float64)).astype(F)                      # fmaf
    raw = dict(c, snake=0)

    def ein32(spec, a, b):
        return np.einsum(spec, a.astype(F), b.astype(F)).astype(F)

    def contract32(at, xx):
        return contract(raw, dict(AT=at, X=xx), raw=True, ein=ein32).astype(F)
    if split:
        ah, xh = bf16_round(f["AT"]), bf16_round(x)
        al, xl = bf16_round(f["AT"] - ah), bf16_round(x - xh)
        acc = sum(contract32(a_, x_) for a_, x_ in ((ah, xh), (al, xh), (ah, xl)))
    else:
        acc = contract32(f["AT"], x)
    return epilogue(c, inp, acc.astype(np.float64)).astype(F)


# ------------------------------------------------------------------------------------------------ the other launchers
def ref_final(x, w, bias, a, ra, x_lo, T):
    """x [B][C][hist + T] -> [B][T]: activation (a given: x + ra sin^2(a x), output clipped to [-1, 1]; else ELU), causal conv k (w [k][C]) + bias"""
    hist = max(-x_lo, 0)
    k = w.shape[0]
    v = snake(x, a, ra) if a is not None else np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    out = np.full((x.shape[0], T), float(bias))
    for j in range(k):
        out += np.einsum("c,bct->bt", w[j], _columns(v, hist, T, np.arange(T) - (k - 1) + j))
    return np.clip(out, -1.0, 1.0) if a is not None else out


def bound_final(x, w, bias, a, ra, x_lo, T):
    """float32 accumulation of k C products (the kernel's own order, no MFMA: no factor 2) plus the activation's error through |w|:
    SnakeBeta as in bound_gemm; ELU: expf within 1 ulp and the subtraction, 3 u"""
    hist, k = max(-x_lo, 0), w.shape[0]
    xa = np.abs(x)
    if a is not None:
        v = snake(x, a, ra)
        dv = np.abs(ra)[None, :, None] * (SIN_SQ_ERR + U * np.abs(a)[None, :, None] * xa) + U * np.abs(v)
    else:
        v = np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
        dv = np.where(x > 0, 0.0, 3 * U)
    n = np.arange(T)
    mag = sum(np.einsum("c,bct->bt", np.abs(w[j]), _columns(np.abs(v), hist, T, n - (k - 1) + j)) for j in range(k))
    err = sum(np.einsum("c,bct->bt", np.abs(w[j]), _columns(dv, hist, T, n - (k - 1) + j)) for j in range(k))
    return (k * w.shape[1] + 1) * U * (mag + abs(bias)) + err


def ref_hist(st, img, H, Tn):
    """st [B][C][H], image [B][C][ld] (H head-room columns, Tn new, padding) -> (st', image'): pure data movement"""
    img2, cat = img.copy(), np.concatenate([st, img[:, :, H:H + Tn]], axis=2)
    img2[:, :, :H] = st
    return cat[:, :, cat.shape[2] - H:], img2


def ref_embed_f32(codes_bqt, tables):
    """float32 sum over q ascending of tables[q][clamp(code)] -> [B][C][T], in the kernel's order"""
    B, nq, T = codes_bqt.shape
    bins = tables.shape[1]
    acc = np.zeros((B, T, tables.shape[2]), np.float32)
    for q in range(nq):
        acc = acc + tables[q][np.clip(codes_bqt[:, q], 0, bins - 1)].astype(np.float32)
    return acc.transpose(0, 2, 1)


def ref_dw7(x, w7, bias, dil):
    T = x.shape[2]
    return bias[None, :, None] + sum(w7[None, :, j, None] * _columns(x, 0, T, np.arange(T) + (j - 3) * dil) for j in range(7))


# ------------------------------------------------------------------------------------------------ entry points
def _lib():
    from mlx_audio_swift_amd import _lib as L
    return L


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@contextlib.contextmanager
def env(**kv):
    """the launchers read MIS_BF3_* / MIS_CODEC_* with getenv on every launch"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_gemm(c, inp, noise_rng=0, noise_key=0, row_ids=None, row_offset=0):
    """mis_debug_codec_gemm -> (status, Y float32 [B][M][Tout] or None, report)"""
    L = _lib()
    a = L.CodecGemmDebugArgsC()
    for k in ("mode", "snake", "batch", "use_pack", "M", "K", "N", "Tin", "Tout", "s", "pad", "Cin", "ldx", "ldy", "x_lo", "dup_bias_n0", "split_k_ok",
              "taps", "dil"):
        setattr(a, k, int(c[k]))
    a.noise_rng, a.noise_key, a.row_offset = noise_rng, noise_key, row_offset
    keep = {k: _f32(inp[k]) for k in ("AT", "bias", "X", "R", "scale", "noise", "alpha", "ralpha")}
    keep["row_ids"] = None if row_ids is None else np.ascontiguousarray(row_ids, np.int32)
    for k, v in keep.items():
        setattr(a, k, _ptr(v))
    y = np.zeros((c["batch"], c["M"], c["Tout"]), np.float32)
    rep = np.zeros(6, np.int32)
    a.Y, a.report = _ptr(y), _ptr(rep)
    st = L.lib().mis_debug_codec_gemm(0, C.byref(a))
    return st, (y if st == 0 else None), tuple(int(v) for v in rep)


def run_final(x, w, bias, a, ra, x_lo, T, ld, out_stride):
    B, Cc = x.shape[:2]
    x, w, a, ra = _f32(x), _f32(w), _f32(a), _f32(ra)
    out = np.zeros((B, T), np.float32)
    st = _lib().lib().mis_debug_codec_final(0, _ptr(x), _ptr(w), float(bias), _ptr(a), _ptr(ra), Cc, T, ld, x_lo, w.shape[0], B, out_stride, _ptr(out))
    return st, out


def run_hist(st_, img, H, Tn):
    B, Cc, ld = img.shape
    st_, img = _f32(st_), _f32(img)
    so, xo = np.zeros_like(st_), np.zeros_like(img)
    st = _lib().lib().mis_debug_codec_hist(0, _ptr(st_), _ptr(img), Cc, ld, H, Tn, B, _ptr(so), _ptr(xo))
    return st, so, xo


def run_embed(codes, cs_b, cs_q, cs_t, tables, ld, T, batch):
    codes, tables = np.ascontiguousarray(codes, np.int32), _f32(tables)
    nq, bins, Cc = tables.shape
    h = np.zeros((batch, Cc, T), np.float32)
    st = _lib().lib().mis_debug_codec_embed(0, _ptr(codes), codes.size, cs_b, cs_q, cs_t, _ptr(tables), nq, bins, Cc, ld, T, batch, _ptr(h))
    return st, h


def run_dw7(x, w7, bias, dil):
    B, Cc, T = x.shape
    x, w7, bias = _f32(x), _f32(w7), _f32(bias)
    y = np.zeros_like(x)
    st = _lib().lib().mis_debug_codec_dw7(0, _ptr(x), _ptr(w7), _ptr(bias), B, Cc, T, dil, _ptr(y))
    return st, y


def run_vq(ze, cn, cn2):
    B, CD, Tm = ze.shape
    ze, cn, cn2 = _f32(ze), _f32(cn), _f32(cn2)
    codes = np.zeros((B, Tm), np.int32)
    st = _lib().lib().mis_debug_codec_vq_nearest(0, _ptr(ze), _ptr(cn), _ptr(cn2), B, CD, cn.shape[0], Tm, _ptr(codes))
    return st, codes


# ------------------------------------------------------------------------------------------------ case lists
def _pick(rng, *axes):
    """one value per axis, drawn independently: no axis runs in step with the loops around it (crossings asserted in test_codec_ref_cpu.py)"""
    return tuple(a[int(rng.integers(len(a)))] for a in axes)


def snac_gemm_cases():
    """k_snac_gemm (tiles 64 x 128, k-chunk 16): M & 3 != 0 (scalar A path), one and two row blocks; K below, at and above a chunk; N = 1,
    around a tile; ldx a multiple of 4 and not, Tin < ldx (the float4 edge n + 3 < Tin lies inside a poisoned row); ldy > Tout; batch 2.
    GELU runs on the grid too: its contraction is exact there and the epilogue is held to the bound"""
    out, seed = [], 0
    modes = [(PLAIN, {}), (RESID, {}), (RESID, dict(scale=1)), (RESID, dict(snake=1)), (NOISE, {}), (GELU, {})]
    rng = np.random.default_rng(11)
    for M in (3, 64, 68):
        for K in (5, 16, 40):
            for N in (1, 127, 128, 131):
                for pad_x in (4 - N % 4 if N % 4 else 4, 3 if (N + 3) % 4 else 5):          # ldx % 4 == 0 and != 0, both > Tin
                    (mode, kw), = _pick(rng, modes)
                    seed += 1
                    out.append(case(mode, M, N, M if mode == NOISE else K, batch=2, ldx=N + pad_x, ldy=N + 3, seed=seed, **kw))   # noise: M == K
    for i, (mode, kw) in enumerate(modes):                                                  # every mode at every M, three chunks, the tail tile
        for M in (3, 64, 68):
            out.append(case(mode, M, 131, M if mode == NOISE else 40, batch=2, ldx=136, ldy=133, seed=500 + 3 * i + M, **kw))
            out.append(case(mode, M, 127, M if mode == NOISE else 40, batch=2, ldx=130, ldy=129, seed=530 + 3 * i + M, **kw))
    return out


def convt_cases(use_pack=0):
    """(s, pad) x kernel 2 s and kernel = s x Cin; Tout not a multiple of s; history column; dup_bias_n0 with and without a bias"""
    out, seed = [], 0
    rng = np.random.default_rng(12 + use_pack)
    for (s, pad) in ((2, 1), (4, 2), (8, 4), (3, 1)):
        for ntaps in (2, 1):
            for Cin in ((5, 16) if not use_pack else (32, 40)):
                for (x_lo, dup, bias) in ((0, 0, 1), (-1, 1, 1), (-1, 1, 0)):
                    seed += 1
                    N, M = _pick(rng, (1, 37, 129), (3, 64, 68) if not use_pack else (32, 40, 160))
                    out.append(case(CONVT, M, N, Cin=Cin, ntaps=ntaps, s=s, pad=pad, Tout=s * N - 1 - (s > 2),
                                    x_lo=x_lo, ldx=N + 6, ldy=s * N + 2, dup_bias_n0=dup, bias=bias, batch=2, seed=600 + seed, use_pack=use_pack))
    return out


def taps_cases():
    """k_conv_taps: taps x dil, causal and "same" pad, history, Cin below and above a 16-chunk, N = 1 / tile / tail, R with and without scale, Snake"""
    out, seed = [], 0
    rng = np.random.default_rng(13)
    for taps in (1, 3, 7):
        for dil in (1, 3, 9):
            for causal in (1, 0):
                span = (taps - 1) * dil
                pad = span if causal else span // 2
                for x_lo in ((0, -span) if span else (0,)):
                    for rep in range(2):
                        seed += 1
                        Cin, N, M, (resid, scale), sn, ld4 = _pick(rng, (5, 24), (1, 128, 131), (3, 64, 68), ((0, 0), (1, 0), (1, 1)), (0, 1), (0, 1))
                        w = N - x_lo
                        out.append(case(TAPS, M, N, Cin=Cin, taps=taps, dil=dil, pad=pad, x_lo=x_lo, ldx=w + (4 - w % 4) % 4 + (4 if ld4 else 1),
                                        ldy=N + 2, resid=resid, scale=scale, snake=sn, batch=2, seed=700 + seed))
    return out


def fused_cases():
    out = []
    for i, C_ in enumerate((64, 96, 128, 192)):
        for j, N in enumerate((1, 127, 128, 129)):
            out.append(case(RESID, C_, N, C_, snake=1, batch=2, ldx=N + 5, ldy=N + 2, seed=800 + 4 * i + j))
    return out


BF3_M, BF3_N = (32, 40, 128, 160), (1, 128, 129, 200)


def bf3_cases():
    """the split-bf16 kernels under lowered thresholds: Cin 32 / 40 (pads to Cp = 64) / 96; every (M, N) of M below / at / above the 128-row
    tile x N = 1, tile, tail, two tiles (cycled, so that each pair runs); 1x1 in every mode, 7 taps at dil 1 (NQ 9) and 3 / 9 (NQ 12), two
    taps of a dense conv (dil <= 16), the transposed conv through convt_cases(1).  Entries (case, ntaps, NQ)"""
    out, seed = [], 0
    rng = np.random.default_rng(14)
    pairs = [(M, N) for M in BF3_M for N in BF3_N]

    def next_pair():
        return pairs[(5 * seed) % 16]                                           # 5 is co-prime to 16: all sixteen pairs, none in step with a loop
    for Cin in (32, 40, 96):
        for mode, kw in ((PLAIN, {}), (GELU, {}), (RESID, {}), (RESID, dict(scale=1, snake=1)), (NOISE, {})):
            for rep in range(2):
                seed += 1
                M, N = next_pair()
                batch, ld4 = _pick(rng, (1, 3), (0, 1))
                out.append((case(mode, Cin if mode == NOISE else M, N, Cin, batch=batch, ldx=N + (4 - N % 4) % 4 + (4 if ld4 else 1), ldy=N + 1, use_pack=1,
                                 seed=900 + seed, **kw), 1, 9))
        for dil in (1, 3, 9):
            for causal in (1, 0):
                seed += 1
                span = 6 * dil
                M, N = next_pair()
                x_lo, batch, (resid, scale), sn = _pick(rng, (0, -span), (1, 3), ((0, 0), (1, 0), (1, 1)), (0, 1))
                out.append((case(TAPS, M, N, Cin=Cin, taps=7, dil=dil, pad=span if causal else span // 2, x_lo=x_lo, ldx=N - x_lo + 3, ldy=N + 1,
                                 resid=resid, scale=scale, snake=sn, batch=batch, use_pack=1, seed=900 + seed), 7, 9 if dil == 1 else 12))
        for dil in (1, 16):
            seed += 1
            M, N = next_pair()
            x_lo, batch = _pick(rng, (0, -dil), (1, 3))
            out.append((case(TAPS, M, N, Cin=Cin, taps=2, dil=dil, pad=dil, x_lo=x_lo, ldx=N - x_lo + 3, ldy=N + 1, batch=batch, use_pack=1, seed=900 + seed), 2, 9))
    for c in convt_cases(1):
        out.append((c, c["ntaps"], 9))
    return out
