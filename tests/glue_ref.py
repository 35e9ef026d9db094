"""Operator-level reference of the LM glue: k_embed_rmsnorm, k_reduce_residual_rmsnorm / k_glue4 / k_glue_cpt, k_gemm_skinny_norm
(csrc/lm_kernels.hip), the prefill row kernels and k_pf_add_resid / k_pf_pack_rows (csrc/lm_prefill.hip), k_prefill_feed, k_convert_to_bf16
and k_dequant_affine; inputs whose result is known exactly, the launchers' dispatch restated, and thin wrappers of the mis_debug_* entry
points of csrc/glue_debug.hip (include/mi_speech_debug.h).  Pure numpy, written from the rounding points stated in the kernels' comments;
nothing here calls a kernel to build its data.  tests/test_glue_ref_cpu.py proves every claim below that the GPU test leans on.

Specification, T() = round to bf16, u = 2^-24:
  o  = T(sum_s slab_s)          float32, slab order 0, 1, 2, ...
  h' = T(h + o)                 (the prefill residual: h = T(h + T(part)))
  RMSNorm    x = T(w T(h' inv)),  inv = 1 / sqrt(mean(h'^2) + eps)
  LayerNorm  x = T((h' - mean) rstd w + b), float32 statistics (two passes), one rounding
  x is written in the xpk layout (attn_ref.xpk_index); columns N .. of the last k-tile of 32 are never written.

h' IS BIT-EXACT ON EVERY INPUT.  A float32 sum in a FIXED order and two roundings have one result; numpy float32 reproduces it (hprime).
No other order is accepted - on Gaussian slabs the reverse order gives other bits (proven in the CPU test).

x, three tiers.
  zero / constant rows.  h + o cancels to 0 (or to a constant c, LayerNorm): RMSNorm of a zero row is 0 for any finite inv, i.e. for
    eps > 0 (without eps: 0 * inf = NaN); LayerNorm of a constant row: every partial sum k c is exact, mean = c, h' - mean = 0, x = T(b).
  balanced exact rows.  h' = +-a, a in {1, 1.25, 1.5} 2^j (LayerNorm: N / 2 of each sign): every partial sum of h'^2 (of h') is an integer
    multiple of a^2 (of a) below 2^24 such units, so mean(h'^2) = a^2 and mean = 0 in ANY order; inv = rstd = 1 / sqrt(a^2 + eps) is two
    correctly rounded operations behind one addition.  With w = +-2^i the product by w is exact, so x = T(fl(h' inv) w) (RMSNorm; the
    outer T() does nothing) and x = T(fl(fl(h' rstd) w + b)) (LayerNorm: one float32 rounding whether or not the multiply-add is fused).
    The rows are built THROUGH the sum: slab_s = k_s a / 4 (integers |k_s| <= 64, a tiny a 2^-12 on slab 0 so that T(sum) really rounds),
    h = h' - o, all exact.  LayerNorm, row 2: h' = 199 or 200 (slabs in units of 1): mean 199.5 and variance 1 / 4 exactly in two passes, while
    E[x^2] - mean^2 rounds the sum of the squares 39601 and 40000 (an odd difference) once it passes 2^24.
  Gaussian rows (scale and offset per row, the last four columns eight times larger; LayerNorm: rows 1 .. 3 are 256 everywhere but 1, 5 or 7
    columns at 255 - held to the same bound, which a two-pass variance meets in every order and E[x^2] - mean^2 does not).
    LayerNorm is ONE rounding: enc_ref.ln_reference's bound (derived there for any summation order, fused or not) is used as it stands.
    RMSNorm is TWO roundings with an exact product between them (w and the inner value have 8 significant bits each: 16 < 24), so the
    only freedom of a correct kernel is on which side of a bf16 rounding boundary p = h' inv falls:
      squares of bf16 values are exact in float32; their sum of N non-negative terms in any order, fused or not:   relative (N - 1) u
      the division by N and the addition of eps:                                                                  2 u
      inv = 1 / sqrt(.): half of the above, plus a square root and a division within one ulp each:               (N + 1) / 2 u + 4 u
      p = h' inv:                                                                                                 u
      => |p_dev - p| <= E = SAFETY ((N + 1) / 2 + 5) u |p|,  SAFETY = 2 (attn_ref's factor for what first order leaves out).
    E is far below a quarter of a bf16 ulp for every N <= 12288, so the inner rounding can move by at most ONE bf16 step, and only where p
    lies within E of a boundary.  The check (rms_check): x_dev must equal T(w T(p)) or, where the boundary is that close, T(w T'(p)) with
    T' the other neighbour - scaled by |w|, as the outer product is exact.  The recorded fraction of the bound is, over the elements that
    took the other neighbour, the distance of p to the boundary over E (0 when none did); an element that matches neither is infinite.

Dequantisation: each element is T(fl(fl(sc q) + bi)) (unfused) or T(fl(sc q + bi)) (fused); the test records where the two differ and which
the device gave, and requires one choice throughout.

k_gemm_skinny_norm: out = T(gelu(T(LN(h') W^T + bias))), h_out = h'.  Exact tier: the balanced LayerNorm rows with w = +-2^i, b = 0 give x in
{+-v} for ONE v per row; W holds integers in [-4, 4], so x W^T = v * integer in any order; the bias is an integer multiple of 1/4.  v is
scaled (through w) so that the pre-activations stay inside enc_ref's [GELU_LO, GELU_HI], where the device's GELU polynomial is within
GELU_ULP on at most GELU_SHARE of the elements (enc_ref.gelu_condition, tests/test_gelu_poly_cpu.py).  Gaussian tier: the float64 reference
with |dx_k| (the LayerNorm bound) propagated through sum_k |dx_k| |W_nk| plus gemm_ref's summation bound 2 gamma_K sum_k |x_k| |W_nk|."""
import ctypes as C

import numpy as np

import attn_ref as ar
import enc_ref as er
import gemm_ref as gr

OK, GENERATION_FAILED, INVALID_INPUT = 0, 2, 3
SAFETY, U, T = ar.SAFETY, ar.U, gr.T
MIS_F32, MIS_F16, MIS_BF16 = 0, 1, 2
K_GENERAL, K_GLUE4, K_CPT, K_NORM_GEMM = 0, 1, 2, 3
EPS_RMS, EPS_LN = 1e-6, 1e-5
f32 = np.float32


def b16(v):
    return er.b16(v)


def bits(v32):
    """float32 array -> bf16 payloads (round to nearest even)"""
    return gr.bf16_bits(np.asarray(v32, f32))


def val(payload):
    return gr.bf16_value(payload).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the dispatch, restated from the launcher's comment
def glue_expected(S, N, ln):
    """(kernel, SG, CPT, threads per block)"""
    sg = 2 if S <= 2 else 4 if S <= 4 else 8
    if not ln and N == 3072 and S <= 8:
        return (K_CPT, sg, 3, 256)
    if N % 4 == 0 and N // 4 <= 1024 and S <= 8:
        return (K_GLUE4, sg, 1, -(-(N // 4) // 64) * 64)
    return (K_GENERAL, sg, 0, 1024)


# the instantiations the launcher can reach: k_reduce_residual_rmsnorm<SG>, k_glue4<SG, LN>, k_glue_cpt<SG, 3, false> (LayerNorm at 3072 runs
# k_glue4, so k_glue_cpt<., 3, true> is built by no dispatch) - twelve kernels - and the general kernel's multi-pass path (N > 3072: keep[] /
# wv[] are not valid, h is read again) per SG, which the sweep must reach as well: fifteen entries.
GLUE_INSTANTIATIONS = ({(K_GENERAL, sg) for sg in (2, 4, 8)} | {(K_GENERAL, sg, "multipass") for sg in (2, 4, 8)} |
                       {(K_GLUE4, sg, ln) for sg in (2, 4, 8) for ln in (0, 1)} | {(K_CPT, sg, 3) for sg in (2, 4, 8)})
GLUE_N = [4, 100, 252, 256, 1280, 3072, 3076, 4096, 4100, 6, 3074, 6148]
GLUE_S = [1, 2, 3, 4, 5, 8]
GLUE_S_GENERAL = [9, 16]


def instantiation_key(rep, N, ln):
    k = rep[0]
    if k == K_GENERAL:
        return (k, rep[1], "multipass") if N > 3072 else (k, rep[1])
    return (k, rep[1], int(ln)) if k == K_GLUE4 else (k, rep[1], rep[2])


# ------------------------------------------------------------------------------------------------ float32 pieces
def fsum(v, order):
    """float32 sum over the last axis: 'seq' left to right; 'pair' recursive halves; 'lanes': 256 threads take columns t, t + 256, ... in turn,
    a butterfly over each 64 lanes, then the waves left to right (the shape of the kernels' block reductions)"""
    v = np.asarray(v, f32)
    if order == "seq":
        return np.cumsum(v, axis=-1, dtype=f32)[..., -1]
    if order == "pair":
        n = 1 << max(0, (v.shape[-1] - 1).bit_length())
        p = np.zeros(v.shape[:-1] + (n,), f32)
        p[..., :v.shape[-1]] = v
        while p.shape[-1] > 1:
            p = (p[..., 0::2] + p[..., 1::2]).astype(f32)
        return p[..., 0]
    n = -(-v.shape[-1] // 256) * 256
    p = np.zeros(v.shape[:-1] + (n,), f32)
    p[..., :v.shape[-1]] = v
    t = np.cumsum(p.reshape(v.shape[:-1] + (n // 256, 256)), axis=-2, dtype=f32)[..., -1, :]          # per thread
    t = t.reshape(v.shape[:-1] + (4, 64))
    while t.shape[-1] > 1:
        h = t.shape[-1] // 2
        t = (t[..., :h] + t[..., h:]).astype(f32)
    return np.cumsum(t[..., 0], axis=-1, dtype=f32)[..., -1]


ORDERS = ("seq", "pair", "lanes")


def hprime(slabs, h, reverse=False, drop_last=False, round_o=True):
    """h' as float32 values: the fixed-order float32 sum, T(), the add, T().  The keywords are the CPU test's mutations."""
    sl = np.asarray(slabs, f32)
    if drop_last:
        sl = sl[:-1]
    acc = np.zeros(sl.shape[1:], f32)
    for s in (range(len(sl) - 1, -1, -1) if reverse else range(len(sl))):
        acc = (acc + sl[s]).astype(f32)
    o = b16(acc) if round_o else acc
    return b16((np.asarray(h, f32) + o).astype(f32))


def add_resid(h, part):
    return b16((np.asarray(h, f32) + b16(np.asarray(part, f32))).astype(f32))


def rms_f32(hp, w, eps, order="pair", divisor=None, no_eps=False, w_first=False, twice=None):
    """the RMSNorm half in float32 numpy -> x as float32 (bf16 values).  divisor / no_eps / w_first / twice (a column counted twice in the
    statistics): the CPU test's mutations.  There is no fused variant: the squares and w T(p) are exact, every other step is one operation."""
    hp, w = np.asarray(hp, f32), np.asarray(w, f32)
    N = hp.shape[-1]
    sq = (hp * hp).astype(f32)                                   # exact
    ss = fsum(sq, order)
    if twice is not None:
        ss = (ss + sq[..., twice]).astype(f32)
    ms = (ss / f32(divisor or N)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (f32(1.0) / np.sqrt(ms if no_eps else (ms + f32(eps)).astype(f32))).astype(f32)
        p = (hp * inv[..., None]).astype(f32)
        if w_first:
            return b16((w * p).astype(f32))
        return b16((w * b16(p)).astype(f32))


def ln_f32(hp, w, b, eps, order="pair", fused=False, divisor=None, no_eps=False, one_pass=False, twice=None):
    """the LayerNorm half in float32 numpy.  one_pass: the variance as E[x^2] - mean^2 (a mutation)"""
    hp, w, b = np.asarray(hp, f32), np.asarray(w, f32), np.asarray(b, f32)
    dd = f32(divisor or hp.shape[-1])
    s1 = fsum(hp, order)
    if twice is not None:
        s1 = (s1 + hp[..., twice]).astype(f32)
    mean = (s1 / dd).astype(f32)
    t = (hp - mean[..., None]).astype(f32)
    if one_pass:
        var = ((fsum((hp * hp).astype(f32), order) / dd).astype(f32) - (mean * mean).astype(f32)).astype(f32)
    else:
        tt = t.astype(np.float64) ** 2 if fused else (t * t).astype(f32)         # (a fused square-accumulate rounds once: close enough to float64 squares)
        s2 = fsum(tt.astype(f32), order)
        if twice is not None:
            s2 = (s2 + (t[..., twice] * t[..., twice]).astype(f32)).astype(f32)
        var = (s2 / dd).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = (f32(1.0) / np.sqrt(var if no_eps else (var + f32(eps)).astype(f32))).astype(f32)
        r = (t * rstd[..., None]).astype(f32)
        if fused:
            return b16((r.astype(np.float64) * w + b).astype(f32))
        return b16(((r * w).astype(f32) + b).astype(f32))


# ------------------------------------------------------------------------------------------------ references and checks
def rms_reference(hp, w, eps):
    """float64: (p = h' inv, E the bound on p of the module docstring)"""
    hp = np.asarray(hp, np.float64)
    N = hp.shape[-1]
    inv = 1.0 / np.sqrt((hp ** 2).mean(-1, keepdims=True) + eps)
    p = hp * inv
    return p, SAFETY * ((N + 1) / 2.0 + 5.0) * U * np.abs(p)


def rms_check(x_dev, hp, w, eps):
    """x_dev: bf16 values [rows][N].  Returns (fraction of the bound, number of elements outside): see the module docstring."""
    p, E = rms_reference(hp, w, eps)
    w = np.asarray(w, np.float64)
    inner = T(p)
    assert np.all(E <= ar.ulp_bf16(np.abs(p)) / 4 + 1e-300)
    side = np.where(p >= inner, 1, -1)                           # the other neighbour: the next bf16 value from `inner` on p's side (taken from
    pay = bits(inner.astype(f32)).astype(np.int64)               # inner's own payload, so a p that rounds up to a power of two is handled too)
    order = np.where(pay & 0x8000, -(pay & 0x7FFF), pay & 0x7FFF) + side
    other = val(np.where(order < 0, 0x8000 | -order, order).astype(np.uint16))
    dist = np.abs((inner + other) / 2 - p)                       # the rounding boundary between the two
    ref, alt = T(w * inner), T(w * other)
    x_dev = np.asarray(x_dev, np.float64)
    same = x_dev == ref
    took = ~same & (x_dev == alt) & (dist <= E)
    bad = ~same & ~took
    frac = float((dist[took] / E[took]).max()) if took.any() else 0.0
    return (float("inf") if bad.any() else frac), int(bad.sum())


def ln_check(x_dev, hp, w, b, eps):
    """(worst fraction of enc_ref.ln_reference's bound, elements outside)"""
    y, bound = er.ln_reference(np.asarray(hp, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64), eps)
    with np.errstate(invalid="ignore"):
        r = np.abs(np.asarray(x_dev, np.float64) - y) / bound
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()), int((r > 1.0).sum())


# ------------------------------------------------------------------------------------------------ inputs
def _split(rng, total, S):
    """integers k_s, |k_s| <= 64, summing to `total` (|total| <= 16) along a new leading axis"""
    k = rng.integers(-12, 13, (S,) + total.shape)
    k[-1] = total - k[:-1].sum(0)
    return k


def exact_case(S, Mpad, N, ln, seed):
    """rows built through the sum: row 0 cancels to zero, row 1 (LayerNorm) to a constant, the others to +-a_r.  Returns dict(slabs f32, h, w, b
    (None: RMSNorm), hp the target h', a [Mpad], expect [Mpad][N] the x of the module docstring in float64)"""
    rng = np.random.default_rng(seed)
    a = rng.choice([1.0, 1.25, 1.5], Mpad) * 2.0 ** rng.integers(-3, 4, Mpad)
    if ln:
        assert N % 2 == 0
        sign = np.stack([rng.permutation(np.repeat([1.0, -1.0], N // 2)) for _ in range(Mpad)])
        sign[1] = 1.0
    else:
        sign = rng.choice([-1.0, 1.0], (Mpad, N))
    sign[0] = 0.0
    unit, off = a / 4.0, np.zeros(Mpad)
    if ln and Mpad > 2:                                          # row 2: 199 or 200 - the same exact statistics (mean 199.5, variance 1 / 4) behind a large
        a[2], unit[2], off[2] = 0.5, 1.0, 199.5                  # offset, where a variance taken as E[x^2] - mean^2 loses its low bits
    hp = sign * a[:, None] + off[:, None]
    ko = rng.integers(-8, 9, (Mpad, N))
    ko[0] = np.where(ko[0] == 0, 3, ko[0])                       # (a zero o on the zero row would leave the tiny term standing)
    slabs = _split(rng, ko, S) * unit[None, :, None]
    slabs[0] += unit[:, None] * 2.0 ** -10 * rng.choice([-1.0, 1.0], (Mpad, N))
    h = hp - ko * unit[:, None]
    w = 2.0 ** rng.integers(-2, 3, N) * rng.choice([-1.0, 1.0], N)
    eps = EPS_LN if ln else EPS_RMS
    af = a.astype(f32)
    scale = (f32(1.0) / np.sqrt((af * af + f32(eps)).astype(f32))).astype(f32)
    r = ((sign * a[:, None]).astype(f32) * scale[:, None]).astype(f32)
    if ln:
        b = T(0.5 * rng.standard_normal(N) + 0.01)
        b = np.where(b == 0, 0.5, b)
        expect = b16(((r * w.astype(f32)).astype(f32) + b.astype(f32)).astype(f32)).astype(np.float64)
        expect[:2] = b
    else:
        b = None
        expect = b16((w.astype(f32) * b16(r)).astype(f32)).astype(np.float64)
    return dict(S=S, Mpad=Mpad, N=N, ln=ln, eps=eps, slabs=slabs.astype(f32), h=h, w=w, b=b, hp=hp, a=a, sign=sign, expect=expect)


def offset_row_columns(N):
    """the columns at 255 of the three offset rows of gauss_case (LayerNorm): mean^2 / variance is about 65536 N / k, so E[x^2] - mean^2 is left
    with rounding noise wherever the float32 sums of the squares 65536 and 65025 round at all; which widths that is depends on k and on
    the order, hence three rows (tests/test_glue_ref_cpu.py lists what each catches)"""
    sets = ([N // 3], [1, N // 5, N // 3, N // 2 + 1, N - 2], [1, N // 7, N // 5, N // 3, N // 2 + 1, (3 * N) // 4, N - 2])
    return [np.array(sorted({c for c in cs if 0 <= c < N})) for cs in sets]


def gauss_case(S, Mpad, N, ln, seed):
    """Gaussian slabs (full float32 precision) and h, scale and offset per row, the last four columns eight times larger (a clamped column counted
    twice shows at every width), with three slabs or more two columns where only the order 0, 1, 2, ... keeps the small slabs"""
    rng = np.random.default_rng(seed)
    sc = 2.0 ** rng.integers(-2, 3, (Mpad, 1))
    big = np.where(np.arange(N) >= N - 4, 8.0, 1.0)[None, :]
    h = T((rng.standard_normal((Mpad, N)) * sc + rng.standard_normal((Mpad, 1))) * big)
    slabs = (rng.standard_normal((S, Mpad, N)) * (0.5 * sc * big)[None]).astype(f32)
    if S >= 3:                                                   # columns 0, 1: slab 0 and slab 1 cancel at 2^18 - in the order 0, 1, 2, ... the rest is
        slabs[0, :, :2] = (2.0 ** 18 * sc).astype(f32)           # summed at full precision, in any other order it is rounded to 2^-5 first: other bf16 bits
        slabs[1, :, :2] = -slabs[0, :, :2]
    if ln and Mpad > 3:                                          # rows 1 .. 3: h' = 256 everywhere but 1, 5 or 7 columns at 255, built through the
        for r, cols in enumerate(offset_row_columns(N), 1):      # sum in steps of 2 (o >= 0 at the odd columns: h = 255 - o stays below 256, representable)
            ko = rng.integers(-8, 9, N)
            ko[cols] = np.abs(ko[cols])
            slabs[:, r] = (2.0 * _split(rng, ko, S)).astype(f32)
            h[r] = 256.0 - 2.0 * ko
            h[r, cols] -= 1.0
    w = T(1.0 + 0.5 * rng.standard_normal(N))
    b = T(0.5 * rng.standard_normal(N) + 0.01) if ln else None
    return dict(S=S, Mpad=Mpad, N=N, ln=ln, eps=EPS_LN if ln else EPS_RMS, slabs=slabs, h=h, w=w, b=b)


def check_x(c, x_dev, hp):
    """a case's x (bf16 values, [rows][N]) against its reference on the given h': (fraction of the bound, elements outside)"""
    return ln_check(x_dev, hp, c["w"], c["b"], c["eps"]) if c["ln"] else rms_check(x_dev, hp, c["w"], c["eps"])


# ------------------------------------------------------------------------------------------------ layouts
def unpack_x(img, Mpad, N):
    """the packed image [Mpad round_up(N, 32)] -> ([Mpad][N] payloads, the payloads of the columns N .. of the last k-tile)"""
    Np = -(-N // 32) * 32
    m, k = np.meshgrid(np.arange(Mpad), np.arange(Np), indexing="ij")
    full = np.asarray(img)[ar.xpk_index(m, k, Mpad // 16)]
    return full[:, :N], full[:, N:]


def pack_x(rows):
    """[Mpad][N] payloads -> the packed image, 0xFFFF where nothing belongs"""
    Mpad, N = rows.shape
    img = np.full(Mpad * (-(-N // 32) * 32), 0xFFFF, np.uint16)
    m, k = np.meshgrid(np.arange(Mpad), np.arange(N), indexing="ij")
    img[ar.xpk_index(m, k, Mpad // 16)] = rows
    return img


def xpk_swapped(m, k, MT):
    """the CPU test's placement mutation: the row inside the tile and the 8-column group change places"""
    return ((((k >> 5) * MT + (m >> 4)) * 64) + ((m & 15) << 2) + ((k & 31) >> 3)) * 8 + (k & 7)


# ------------------------------------------------------------------------------------------------ embed, prefill rows, feed
def embed_reference(E, ids, active, pos_next, Mpad, invalid="row0"):
    """(h [Mpad][d] float64, pos_cur, pos_next after).  invalid ids: 'row0' (k_embed_rmsnorm) - rows batch .. Mpad - 1 read row 0 as well"""
    vocab, batch = E.shape[0], len(ids)
    idm = np.zeros(Mpad, np.int64)
    idm[:batch] = np.where((np.asarray(ids) < 0) | (np.asarray(ids) >= vocab), 0, ids)
    return E[idm], np.asarray(pos_next).copy(), np.asarray(pos_next) + (np.asarray(active) != 0)


def pf_tables(lens, Lmax, t0, Tc, batch, Mpad):
    """(on [Tc][Mpad] bool, pos [Tc][Mpad]) of a left-padded prompt: row b starts at Lmax - len[b]"""
    t = (t0 + np.arange(Tc))[:, None]
    ln_ = np.zeros(Mpad, np.int64)
    ln_[:batch] = lens
    on = (np.arange(Mpad)[None, :] < batch) & (t >= Lmax - ln_[None, :])
    return on, np.where(on, t - (Lmax - ln_[None, :]), 0)


def pf_embed_reference(E, prompt, lens, Lmax, t0, Tc, batch, Mpad):
    """h [Tc Mpad][d]: the embedding row of an active position, a ZERO row elsewhere and for an id outside the vocabulary (k_pf_embed_rmsnorm)"""
    on, pos = pf_tables(lens, Lmax, t0, Tc, batch, Mpad)
    h = np.zeros((Tc, Mpad, E.shape[1]))
    for tl in range(Tc):
        for b in range(batch):
            i = prompt[b, t0 + tl]
            if on[tl, b] and 0 <= i < E.shape[0]:
                h[tl, b] = E[i]
    return h.reshape(Tc * Mpad, -1), on.reshape(-1), pos.reshape(-1)


def feed_reference(prompt, lens, Lmax, j):
    on = (j >= Lmax - np.asarray(lens)) & (j < Lmax)
    ids = np.where(on, prompt[:, min(max(j, 0), Lmax - 1)], 0)
    return ids.astype(np.int32), on.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ load-time kernels
def convert_values(n, dtype, seed):
    """n source elements of `dtype`: ties both ways, the largest finite value (float32: rounds to infinity), +-0, subnormals, infinities, NaN,
    then random payloads whose low halves sit on and around the tie"""
    rng = np.random.default_rng(seed)
    if dtype == MIS_F32:
        fixed = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x00000000, 0x80000000, 0x00000001,
                          0x807FFFFF, 0x00008000, 0x00018000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF], np.uint32)
        r = (rng.integers(0, 1 << 16, n).astype(np.uint32) << 16) | rng.choice(np.array([0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF], np.uint32), n)
        return np.ascontiguousarray(np.concatenate([fixed, r])[:n]).view(np.float32)
    if dtype == MIS_F16:
        fixed = np.array([0x3C01, 0x0000, 0x8000, 0x0001, 0x83FF, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x3C00, 0x3555], np.uint16)
    else:
        fixed = np.array([0x3F81, 0x0000, 0x8000, 0x0001, 0x807F, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0x3F80, 0xFFFF], np.uint16)
    return np.ascontiguousarray(np.concatenate([fixed, rng.integers(0, 1 << 16, n).astype(np.uint16)])[:n])


def convert_reference(src, dtype):
    """(payloads, is-NaN mask): float32 -> bf16 to nearest even; f16 widens exactly first; bf16 is copied"""
    if dtype == MIS_BF16:
        return np.asarray(src, np.uint16).copy(), np.zeros(len(src), bool)
    v = np.asarray(src).view(np.float32 if dtype == MIS_F32 else np.float16).astype(np.float32)
    nan = np.isnan(v)
    with np.errstate(over="ignore"):
        return bits(np.where(nan, f32(0), v)), nan


def dequant_inputs(N, K, nbits, sb_dtype, seed):
    """codes covering 0 and the maximum in every group, Gaussian scales / biases representable in sb_dtype (float32: full precision)"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 2 ** nbits, (N, K))
    q[:, 0::64], q[:, 1::64] = 0, 2 ** nbits - 1
    sc, bi = 0.02 * (1 + rng.random((N, K // 64))), 0.3 * rng.standard_normal((N, K // 64))
    if sb_dtype == MIS_F32:
        sc, bi = sc.astype(f32), bi.astype(f32)
        # 16-bit scales times a code are exact in float32, so only here can a fused multiply-add show: plant pairs (searched, not measured) whose
        # fused and unfused results round to different bf16 values at some code, that code at column 2 of the group
        cs, cb = (0.02 * (1 + rng.random(1 << 16))).astype(f32), (0.3 * rng.standard_normal(1 << 16)).astype(f32)
        qq = np.arange(2 ** nbits, dtype=f32)[None, :]
        dif = bits(((cs[:, None] * qq).astype(f32) + cb[:, None]).astype(f32)) != bits((cs[:, None].astype(np.float64) * qq + cb[:, None]).astype(f32))
        idx = np.flatnonzero(dif.any(1))[:sc.size]
        for j, i in enumerate(idx):
            o, gi = divmod(j, sc.shape[1])
            sc[o, gi], bi[o, gi], q[o, 64 * gi + 2] = cs[i], cb[i], int(np.argmax(dif[i]))
    elif sb_dtype == MIS_F16:
        sc, bi = sc.astype(np.float16), bi.astype(np.float16)
    else:
        sc, bi = b16(sc.astype(f32)), b16(bi.astype(f32))
    return q, sc, bi


def dequant_reference(q, sc, bi):
    """(unfused, fused) payloads"""
    s, b_ = np.repeat(sc.astype(f32), 64, 1), np.repeat(bi.astype(f32), 64, 1)
    qf = q.astype(f32)
    unf = bits(((s * qf).astype(f32) + b_).astype(f32))
    fus = bits((s.astype(np.float64) * qf + b_).astype(f32))             # the product is exact in float64: one rounding, as an fma
    return unf, fus


# ------------------------------------------------------------------------------------------------ the norm-prologue GEMM
def norm_gemm_exact_case(K, N_out, nrows, S_in, seed):
    """balanced LayerNorm rows (b = 0, w = +-2^i with i chosen per case so that the pre-activations stay inside enc_ref's GELU range), integer W,
    bias in multiples of 1/4 from [0, 3]"""
    c = exact_case(S_in, 16, K, True, seed)
    rng = np.random.default_rng(seed + 1)
    # rows 0 / 1 of exact_case are the zero and the constant row: with b = 0 their x is 0 - kept, they exercise GELU(bias)
    sgn = np.sign(c["w"])
    W = rng.integers(-4, 5, (N_out, K)).astype(np.float64)
    bias = rng.integers(0, 13, N_out) / 4.0
    af = c["a"].astype(f32)
    v = np.abs(b16((af * (f32(1.0) / np.sqrt((af * af + f32(EPS_LN)).astype(f32))).astype(f32)).astype(f32)).astype(np.float64))     # |x| per row before w
    v[:2] = 0.0
    xs = c["sign"] * sgn[None, :] * v[:, None]
    xs[:2] = 0.0
    acc = xs @ W.T
    j = 0
    while (acc[:nrows] * 2.0 ** j + bias).min() < er.GELU_LO or (acc[:nrows] * 2.0 ** j + bias).max() > er.GELU_HI:
        j -= 1
    c.update(w=sgn * 2.0 ** j, b=np.zeros(K), W=W, bias=bias, x=xs * 2.0 ** j, pre=acc * 2.0 ** j + bias, nrows=nrows, N_out=N_out)
    return c


# ------------------------------------------------------------------------------------------------ the entry points
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _L():
    from mlx_audio_swift_amd import _lib as L
    return L.lib()


def _b(a):
    return None if a is None else np.ascontiguousarray(gr.exact_bits(a))


def run_glue(c, h=None, slabs=None):
    """mis_debug_lm_glue -> (status, h' payloads [Mpad][N], x payloads [Mpad][N], the untouched tail, report)"""
    S, Mpad, N = c["S"], c["Mpad"], c["N"]
    sl = np.ascontiguousarray(c["slabs"] if slabs is None else slabs, f32)
    hb = _b(c["h"] if h is None else h).copy()
    ximg = np.zeros(Mpad * (-(-N // 32) * 32), np.uint16)
    rep = np.full(4, -7, np.int32)
    w, b = _b(c["w"]), _b(c["b"])
    st = _L().mis_debug_lm_glue(0, _ptr(sl), sl.shape[0], Mpad, N, _ptr(hb), _ptr(w), _ptr(b), c["eps"], _ptr(ximg), _ptr(rep))
    x, tail = unpack_x(ximg, Mpad, N)
    return st, hb, x, tail, tuple(int(v) for v in rep)


def run_embed(E, ids, active, pos_cur, pos_next, w, eps, Mpad):
    vocab, d = E.shape
    ids, active = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(active, np.uint8)
    pc, pn = np.ascontiguousarray(pos_cur, np.int32).copy(), np.ascontiguousarray(pos_next, np.int32).copy()
    h, ximg = np.zeros((Mpad, d), np.uint16), np.zeros(Mpad * (-(-d // 32) * 32), np.uint16)
    be, bw = _b(E), _b(w)
    st = _L().mis_debug_lm_embed_rmsnorm(0, _ptr(be), _ptr(ids), _ptr(active), _ptr(pc), _ptr(pn), _ptr(bw), d, vocab, eps, len(ids), Mpad, _ptr(h), _ptr(ximg))
    return st, h, ximg, pc, pn


def run_pf(mode, *, table=None, prompt=None, lens=None, Lmax=0, t0=0, Tc=1, batch=0, Mpad=16, vocab=0, src_rows=0, w=None, part=None, n=0, d=0, eps=EPS_RMS,
           h=None, xsize=0):
    """mis_debug_pf_rows -> (status, h payloads, x payloads, pos_tab, act_tab)"""
    rows = Tc * Mpad
    hb = np.ascontiguousarray(h, np.uint16).copy() if h is not None else np.zeros((rows, d), np.uint16)
    x = np.zeros(xsize or rows * max(d, 1), np.uint16)
    pos, act = np.full(rows, -7, np.int32), np.full(rows, 7, np.uint8)
    tb, bw = _b(table), _b(w)
    pr = None if prompt is None else np.ascontiguousarray(prompt, np.int32)
    ln_ = None if lens is None else np.ascontiguousarray(lens, np.int32)
    pt = None if part is None else np.ascontiguousarray(part, f32)
    st = _L().mis_debug_pf_rows(0, mode, _ptr(tb), _ptr(pr), _ptr(ln_), Lmax, t0, Tc, batch, Mpad, vocab, src_rows, _ptr(bw), _ptr(pt), n, d, eps, _ptr(hb), _ptr(x),
                                _ptr(pos), _ptr(act))
    return st, hb, x, pos, act


def run_feed(prompt, lens, Lmax, counter):
    batch = len(lens)
    pr, ln_ = np.ascontiguousarray(prompt, np.int32), np.ascontiguousarray(lens, np.int32)
    sc = np.array([counter], np.int32)
    ids, act = np.full(batch, -7, np.int32), np.full(batch, 7, np.uint8)
    st = _L().mis_debug_prefill_feed(0, _ptr(pr), _ptr(ln_), Lmax, _ptr(sc), batch, _ptr(ids), _ptr(act))
    return st, int(sc[0]), ids, act


def run_convert(src, dtype):
    src = np.ascontiguousarray(src)
    out = np.zeros(len(src), np.uint16)
    st = _L().mis_debug_convert_to_bf16(0, _ptr(src), dtype, len(src), _ptr(out))
    return st, out


def run_dequant(q, sc, bi, nbits, sb_dtype):
    N, K = q.shape
    wq = np.ascontiguousarray(gr.pack_codes(q, nbits))
    s, b_ = np.ascontiguousarray(sc), np.ascontiguousarray(bi)
    if sb_dtype == MIS_BF16:
        s, b_ = bits(s), bits(b_)
    out = np.zeros((N, K), np.uint16)
    st = _L().mis_debug_dequant_affine(0, _ptr(wq), _ptr(s), _ptr(b_), sb_dtype, N, K, 64, nbits, _ptr(out))
    return st, out


def norm_gemm_ok(epi, R, KT, S, S_in, Mpad, nrows, ln):
    return bool(_L().mis_debug_gemm_skinny_norm_ok(epi, R, KT, S, S_in, Mpad, nrows, int(ln)))


def run_norm_gemm(c, epi=gr.EPI_GELU_PACKED, R=2, S=1, ln=True):
    """mis_debug_gemm_skinny_norm -> (status, out f32 [16][N_out], h_out payloads [16][K], h_in after, report)"""
    K, N_out = c["N"], c["N_out"]
    sl = np.ascontiguousarray(c["slabs"], f32)
    W, hb, w, b, bias = _b(c["W"]), _b(c["h"]), _b(c["w"]), _b(c["b"]) if ln else None, _b(c["bias"])
    out = np.full((max(S, 1) * 16, N_out), np.nan, f32)
    h_out, h_after = np.zeros((16, K), np.uint16), np.zeros((16, K), np.uint16)
    rep = np.full(5, -7, np.int32)
    st = _L().mis_debug_gemm_skinny_norm(0, _ptr(W), _ptr(sl), sl.shape[0], _ptr(hb), _ptr(w), _ptr(b), c["eps"], c["nrows"], epi, R, S, _ptr(bias), N_out, K,
                                         _ptr(out), out.size, _ptr(h_out), _ptr(h_after), _ptr(rep))
    return st, out, h_out, h_after, tuple(int(v) for v in rep)
