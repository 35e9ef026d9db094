"""Operator-level reference of the private kernels of csrc/lasr.hip (k_lasr_gemm<EPI, TI>, k_lasr_ln, k_lasr_rope, k_lasr_attn,
k_lasr_glu_dwconv<ACT>, k_lasr_im2col, k_lasr_pack, k_lasr_argmax, k_lasr_collapse), inputs whose result is known exactly, the case tables
of tests/test_gpu_lasr_ops.py, the launchers' rules restated, and thin wrappers of the mis_debug_lasr_* entry points
(include/mi_speech_debug.h).  Pure numpy, float64, written from the kernel header comments; nothing here calls a kernel to build its
data.  tests/test_lasr_ops_ref_cpu.py proves every claim below that the GPU test leans on.

Specification, T() = round to bf16, live(m) = cnt is None or m % Tp < cnt[m // Tp]; a row that is not live is written as ZERO whatever
the inputs hold there (the cases put NaN there):
  GEMM       v = T(sum_k x[m][k] w[n][k] + b[n]), x[m][k] = X[m ldx + k];  LG_BIAS v;  LG_RELU max(v, 0);  LG_SILU T(v sigmoid(v));
             LG_AXPBY T(a R[m][n] + b v), R may be the output buffer;  LG_F32 the sum + b[n] unrounded, float32, any N.
             Tile rule of ls_gemm_epi: TI = 4 iff ceil(N / 128) ceil(M / 128) >= 256, else 2; ls_gemm refuses K % 32, ldx % 8, and N % 4 for a
             bf16 epilogue (MIS_ERR_GENERATION_FAILED).  Both tiles do one MFMA per 32 k in ascending order: the same bits.
  LayerNorm  y = T((x - mean) rstd w + b), mean and variance two-pass in float32, rstd = 1 / sqrt(var + eps)
  RoPE       heads 0 .. nheads - 1 of 64 columns from column 0, position m % Tp, i < 32: y[i] = T(x[i] c[i] - x[i + 32] s[i]),
             y[i + 32] = T(x[i + 32] c[i] + x[i] s[i]); every other column untouched
  attention  rows [B Tp][ld] = q heads | k heads | v heads; out[b, t, h] = T(sum_j p_j v_j), p = softmax over j < n = min(cnt[b], Tp) of
             scale q . k_j with the kv head h // (H / Hkv); queries t >= n: zero
  GLU + dw   g[t] = T(a[t] sigmoid(gate[t])) for 0 <= t < n (a the first C columns of pw, gate the last), zero outside;
             y[t] = act(shift + sum_kk taps[kk] g[t - (k - 1) // 2 + kk]), act 0 SiLU / 1 ReLU, out = T(y), frames t >= n: zero
  im2col     out[b Tout + t][kk C + c] = in[b][t st + kk][c] for t < cnt[b], zero behind;  pack  out[b Fp + t][j] = T(feats[b][t][j]) for
             j < mels and t < F[b], zero elsewhere
  arg-max    the lowest index of the row's maximum, NaN never compares: a row without a comparable value gives 0
  collapse   greedy CTC (lasr_ref.greedy_ctc) of frames t < min(cnt[b], Tp), compacted; slots behind ntok[b] are never written

GEMM inputs are enc_ref's exact grid: x in {-1, 0, 1} 2^e, w integers in [-4, 4], integer bias: every partial sum is an integer multiple of
2^e below 2^24 units, exact in float32 in any order.  Residuals are multiples of 2^-5 up to 2, a in {1, 0.5, 0.75}, b in {1, 0.5, 2}: a R is
a multiple of 2^-7, b v a bf16 value of at most 8 bits above 2^-6, so a R + b v is exact in float32 (fused or not) and T() is ONE rounding.

SiLU rule (LG_SILU, and act 0 of the conv kernel).  The reference is T(silu64(v)) on the exactly known pre-activation v, |v| <= SILU_VMAX = 8.
The device evaluates v / (1 + __expf(-v)) in float32, u = 2^-24:
    __expf(x) = exp2(x log2 e): the rounded product and the rounded constant, relative 1.45 |x| u in the result (attn_ref), and the
        hardware exp2, one ulp = 2 u                                                      E = exp(-v):  (1.45 |v| + 2) u
    D = 1 + E: E / D <= 1 of that, and the addition's rounding                            (1.45 |v| + 3) u
    v / D: a division of at most 2.5 ulp                                                   5 u
    relative error of the float32 result <= (1.45 |v| + 8) u,   margin(v) = SAFETY (1.45 |v| + 8) u   (<= 39.2 u = 2.34e-6 at |v| = 8)
An element is EXEMPT when silu64(v) lies within margin(v) |silu64(v)| of a bf16 rounding boundary (the midpoint of two neighbouring bf16
values); there the device may give either neighbour (one bf16 ulp), everywhere else the bits must match.  At most SILU_SHARE = 1 % of a
case's LIVE elements (rows behind a row count are zeros by construction) may be exempt - tests/test_lasr_ops_ref_cpu.py proves that for every case, and that float32 realisations of the
expression leave T(silu64) on exempt elements only.  The same rule holds g = T(a sigmoid(gate)), |gate| <= 8, in the conv kernel's
Gaussian case (the error terms are those of v / D with a in the numerator).

GLU + depthwise exact tier: gates +32 and -128 make the float32 sigmoid exactly 1 (exp(-32) < 2^-24) and 0 (__expf(128) = inf), a small
integers (times a power of two for act 0, so that |y| <= 8), taps integers in [-2, 2], shift multiples of 2^-4: y is exact in any order.
Impulse tier: one live frame in every k carries a != 0 and tap kk weighs 2^(kk - 40): an output sees one tap, and a shifted or mirrored
tap changes it.  Gaussian tier: y is a float32 fma chain of k terms on g, |y - y64| <= SAFETY gamma_k (|shift| + sum |taps g|), plus
|taps| ulp_bf16(g) for every exempt g in the window; the output is held to delta (1 + 2^-8) + 2^-8 |ref| as the Gaussian GEMM is.

LayerNorm: enc_ref's constant, balanced and Gaussian tiers and its bound (one wave per row is one more summation order).
RoPE: dyadic tables (attn_ref) on the 2^-8 grid make x c +- partner s exact: bit for bit.  Gaussian tables (gauss_tables): the float32 result is one rounded
product and one rounded fma or two products and an addition, |r32 - r64| <= u (|x c| + |partner s| + |r|); bound = SAFETY that + half a bf16 ulp.
Attention: enc_ref's locator / uniform / gaussian tiers.  k_lasr_attn gives a wave 16 queries and walks the 32-key tiles in order: one
exp factor per tile and the final one, F = ceil(n / 32) + 1, P = hi + lo in bf16 (2^-17), no combine across waves:
    E = 2 gamma_64 max a_j + u max |s_j| + 2.45 X u + 2 F u + 2^-17 + 2 gamma_(n + F) + gamma_n + 4 u,  |out - ref| <= ulp / 2 + 2 SAFETY E sum p |v|."""
import ctypes as C
import math

import numpy as np

import attn_ref as ar
import enc_ref as er
import gemm_ref as gr
import lasr_ref as lr

OK, GENERATION_FAILED, INVALID_INPUT = 0, 2, 3
LG_BIAS, LG_RELU, LG_SILU, LG_AXPBY, LG_F32 = range(5)
SAFETY, U, T, ulp_bf16 = ar.SAFETY, ar.U, gr.T, ar.ulp_bf16
SILU_VMAX, SILU_SHARE, SILU_ULP = 8.0, er.GELU_SHARE, 1
NAN16, HD, DW_MAXK, EPS = 0x7FC0, 64, 64, 1e-5
b16 = er.b16


def bits_nan(values, dead):
    """bf16 payloads of exactly representable values, NaN where `dead`"""
    out = gr.exact_bits(np.where(dead, 0.0, values)).copy()
    out[np.broadcast_to(dead, out.shape)] = NAN16
    return out


def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def silu64(v):
    return np.asarray(v, np.float64) * sigmoid64(v)


def margin(v):
    return SAFETY * (1.45 * np.abs(v) + 8.0) * U


def _neighbours(r):
    """the bf16 values next to the bf16 values r on both sides"""
    bits = gr.bf16_bits(np.asarray(r, np.float32)).astype(np.int64)
    o = np.where(bits & 0x8000, -(bits & 0x7FFF), bits & 0x7FFF)
    back = lambda k: gr.bf16_value(np.where(k < 0, 0x8000 | -k, k).astype(np.uint16)).astype(np.float64)
    return back(o - 1), back(o + 1)


def near_boundary(s, m):
    """s float64, m the relative margin: (T(s), True where s lies within m |s| of a bf16 rounding boundary)"""
    s = np.asarray(s, np.float64)
    r = T(s)
    dn, up = _neighbours(r)
    dist = np.minimum(np.abs(s - (r + dn) / 2), np.abs(s - (r + up) / 2))
    return r, dist <= m * np.abs(s)


def silu_reference(v):
    """(T(silu64(v)), exempt) of exactly known pre-activations"""
    return near_boundary(silu64(v), margin(v))


def rule_holds(got, want, exempt, live=None):
    """the SiLU rule on bf16 values: (ok over every element, observed share of differing elements among the LIVE ones - rows behind a row
    count are zeros by construction and would dilute it -, worst ulp distance, live elements)"""
    d = gr.bf16_ulp_distance(got, want)
    n = d.size if live is None else int(np.broadcast_to(live, d.shape).sum())
    return bool(np.all(d[~exempt] == 0) and d.max(initial=0) <= SILU_ULP), float(np.sum(d != 0)) / max(n, 1), int(d.max(initial=0)), n


def exempt_share(exempt, live=None):
    """exempt elements over the case's LIVE elements (exempt is false on the others)"""
    n = exempt.size if live is None else int(np.broadcast_to(live, exempt.shape).sum())
    return float(exempt.sum()) / max(n, 1)


def silu_f32(v, variant=0):
    """float32 realisations of v / (1 + exp(-v)): 0 numpy's exp, 1 exp2(x log2 e) as __expf does, 2 v sigmoid(v) with a reciprocal"""
    f = np.float32
    v = np.asarray(v, f)
    with np.errstate(over="ignore"):
        e = np.exp(-v).astype(f) if variant != 1 else np.exp2((-v * f(1.4426950408889634)).astype(f)).astype(f)
        if variant == 2:
            return b16((v * (f(1.0) / (f(1.0) + e)).astype(f)).astype(f)).astype(np.float64)
        return b16((v / (f(1.0) + e)).astype(f)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ row counts
def live_rows(M, cnt, Tp):
    m = np.arange(M)
    return np.ones(M, bool) if cnt is None else (m % Tp) < np.asarray(cnt)[m // Tp]


def mask_of(M, mode, seed):
    """(cnt or None, Tp): 0 no counts; 1 Tp = 7 with random counts (masked rows inside a tile); 2 Tp = 64, counts 3, 0, 1 (the 64-tile of rows
    64 .. 127 wholly masked); 3 Tp = 128, counts 0, 1 (the first 128-tile wholly masked)"""
    if mode == 0:
        return None, 1
    Tp = (7, 64, 128)[mode - 1]
    n = -(-M // Tp)
    if mode == 1:
        cnt = np.random.default_rng(seed).integers(0, 8, n)
        cnt[0] = 3
    else:
        cnt = np.resize([3, 0, 1] if mode == 2 else [0, 1], n)
    return cnt.astype(np.int32), Tp


# ------------------------------------------------------------------------------------------------ GEMM
def gemm_tile_rule(M, N):
    return 4 if -(-N // 128) * -(-M // 128) >= 256 else 2


def gemm_expected(epi, M, N, K, ldx, tile=0):
    """ls_gemm restated: ("err", status) or (epilogue, TI)"""
    if K % 32 or ldx % 8 or (epi != LG_F32 and N % 4) or M < 1:
        return ("err", GENERATION_FAILED)
    return (epi, tile or gemm_tile_rule(M, N))


GEMM_INSTANTIATIONS = {(e, t) for e in range(5) for t in (2, 4)}
GEMM_M = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129]
GEMM_N16 = [4, 8, 12, 16, 20, 60, 64, 68, 72, 124, 128, 132]        # N % 16 in {0, 4, 8, 12} around both tile sizes
GEMM_NF32 = [1, 3, 15, 17, 63, 65, 127, 129, 257]
GEMM_K = [32, 64, 96, 288]
AXPBY_A, AXPBY_B = [1.0, 0.5, 0.75], [1.0, 0.5, 2.0]


def gemm_cases(epi):
    """every (M, N) = (GEMM_M[i], Ns[j]) with (i + j) % 3 == 0: an N meets the M with i = r, r + 3, r + 6 (, r + 9), an M the N with j = r',
    r' + 3, ...  The other attributes are functions of (i, j, epi) chosen so that they vary ALONG those two progressions:
      K        index (i // 3 + j + epi) % 4: three or four different K per N, and per M
      bias     absent where (i // 3 + j) % 3 == 0: every N with and without a bias
      ldx      K + 8 where (i + j // 3) % 2
      counts   only the modes that leave a live row AND mask what they are for at this M (mask_of): 0, 1 always, 2 from M = 65, 3 at
               M = 129; index (j // 3 + i + epi) over the allowed ones - every case has live rows, M = 129 meets every mode in a bf16 epilogue
      AXPBY    in place where (i + j) // 3 is even; a index (i + j) // 3 % 3, b index i % 3: all nine (a, b)
    Every case runs on BOTH forced tiles.  tests/test_lasr_ops_ref_cpu.py asserts the coverage over the live rows."""
    cases = []
    Ns = GEMM_NF32 if epi == LG_F32 else GEMM_N16
    for i, M in enumerate(GEMM_M):
        allowed = [0, 1] + ([2] if M > 64 else []) + ([3] if M > 128 else [])
        for j, N in enumerate(Ns):
            if (i + j) % 3:
                continue
            s = (i + j) // 3
            K = GEMM_K[(i // 3 + j + epi) % 4]
            cases.append(dict(epi=epi, M=M, N=N, K=K, ldx=K + 8 * ((i + j // 3) % 2), bias=(i // 3 + j) % 3 != 0, mask=allowed[(j // 3 + i + epi) % len(allowed)],
                              in_place=s % 2 == 0, a=AXPBY_A[s % 3], b=AXPBY_B[i % 3], seed=31000 + 1000 * epi + 20 * i + j))
    return cases


THRESHOLD_CASES = [dict(epi=LG_BIAS, M=1925, N=1924, K=32, ldx=32, bias=True, mask=0, in_place=False, a=0.0, b=0.0, seed=31900),
                   dict(epi=LG_BIAS, M=1925, N=1920, K=32, ldx=32, bias=True, mask=0, in_place=False, a=0.0, b=0.0, seed=31901)]


def gemm_inputs(c):
    """a case's operands: x [M][K], w, bias, R in float64 (exact in bf16), pre = x w^T + bias (exact), live [M], and the payloads the entry point
    takes: img [(M - 1) ldx + K] and Rb [M][N] with NaN in the rows that are not live"""
    M, N, K, ldx, epi = c["M"], c["N"], c["K"], c["ldx"], c["epi"]
    rng = np.random.default_rng(c["seed"])
    cnt, Tp = mask_of(M, c["mask"], c["seed"])
    live = live_rows(M, cnt, Tp)
    for _ in range(64):
        e = gr.x_log2_for_std(K, gr.DENSE_W_RMS) if epi == LG_SILU else -5
        x = rng.integers(-1, 2, (M, K)).astype(np.float64)
        w = rng.integers(-4, 5, (N, K)).astype(np.float64)
        bias = rng.integers(-3, 4, N).astype(np.float64) if c["bias"] else None
        if not (M * N * K > er.TILE_CHECK_MAX or gr._tiles_all_count(x[live], w)):   # every k-slab counts on the LIVE rows
            continue
        acc, b0 = x @ w.T, 0.0 if bias is None else bias[None, :]
        if epi != LG_SILU:
            break
        while np.abs(acc * 2.0 ** e + b0).max() > SILU_VMAX:
            e -= 1
        # SiLU: a draw whose exempt share of the LIVE elements passes the cap is drawn again (a property of the inputs alone - the float64
        # values' distance to a bf16 boundary; a case of few live elements keeps no exempt element at all)
        if exempt_share(silu_reference(T(acc * 2.0 ** e + b0))[1] & live[:, None], live[:, None]) <= SILU_SHARE:
            break
    else:
        raise AssertionError("no input without an inert k-tile (SiLU: within the exempt cap) found")
    R = rng.integers(-64, 65, (M, N)).astype(np.float64) * 2.0 ** -5 if epi == LG_AXPBY else None
    x = x * 2.0 ** e
    img = np.full((M - 1) * ldx + K, NAN16, np.uint16)
    idx = np.arange(M)[:, None] * ldx + np.arange(K)[None, :]
    img[idx] = bits_nan(x, ~live[:, None])
    return dict(x=x, w=w, bias=bias, R=R, pre=acc * 2.0 ** e + b0, live=live, cnt=cnt, Tp=Tp, img=img,
                Rb=None if R is None else bits_nan(R, ~live[:, None]))


def gemm_reference(c, d, mut=None):
    """(the output [M][N] in float64 - bf16 values, LG_F32: the exact sums -, exempt or None).  mut: a wrong kernel for the CPU sensitivity checks"""
    pre, epi = d["pre"], c["epi"]
    if mut == "bias_shift" and d["bias"] is not None:
        pre = pre - d["bias"][None] + np.roll(d["bias"], 1)[None]
    ex = None
    if epi == LG_F32:
        out = pre.copy()
    else:
        v = T(pre)
        if epi == LG_RELU:
            v = np.maximum(v, 0.0)
        elif epi == LG_SILU:
            v, ex = silu_reference(v)
        elif epi == LG_AXPBY:
            R = d["R"] if mut != "r_from_c" else np.zeros_like(d["R"])
            v = T(c["a"] * R + c["b"] * v)
        out = v
    out = np.where(d["live"][:, None], out, 0.0)
    return out, (None if ex is None else ex & d["live"][:, None])


def gemm_f32(c, d, order=None):
    """the specification in float32 with the k-slabs of 32 summed in the given order (CPU proofs; SiLU via silu_f32)"""
    f = np.float32
    x, w = d["x"].astype(f), d["w"].astype(f)
    acc = np.zeros((c["M"], c["N"]), f)
    for t in (range(c["K"] // 32) if order is None else order):
        acc = (acc + x[:, 32 * t:32 * t + 32] @ w[:, 32 * t:32 * t + 32].T).astype(f)
    if d["bias"] is not None:
        acc = (acc + d["bias"].astype(f)[None]).astype(f)
    if c["epi"] == LG_F32:
        return np.where(d["live"][:, None], acc.astype(np.float64), 0.0)
    v = b16(acc)
    if c["epi"] == LG_RELU:
        v = np.maximum(v, f(0))
    if c["epi"] == LG_SILU:
        v = silu_f32(v).astype(f)
    if c["epi"] == LG_AXPBY:
        v = b16((f(c["a"]) * d["R"].astype(f)).astype(f) + (f(c["b"]) * v).astype(f))
    return np.where(d["live"][:, None], v.astype(np.float64), 0.0)


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_D, LN_M = [64, 128, 192, 130, 2], [1, 3, 4, 5]


def ln_counts(M, seed):
    """Tp = 2, counts in 0 .. 2 with a masked and a live row where M allows"""
    cnt = np.random.default_rng(seed).integers(0, 3, -(-M // 2)).astype(np.int32)
    cnt[0] = 1 if M > 1 else 0
    return cnt, 2


# ------------------------------------------------------------------------------------------------ RoPE
def rope_reference(rows, nheads, Tp, cs, sn, mut=None):
    """rows [M][ld] float64 -> (y before the rounding [M][nheads 64], bound)"""
    M = rows.shape[0]
    x = rows[:, :nheads * HD].reshape(M, nheads, HD)
    pos = (np.arange(M) + (1 if mut == "pos" else 0)) % Tp
    c, s = cs[pos][:, None, :], sn[pos][:, None, :]
    x1, x2 = x[..., :32], x[..., 32:]
    y = np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    mag = np.concatenate([np.abs(x1 * c) + np.abs(x2 * s), np.abs(x2 * c) + np.abs(x1 * s)], -1)
    pre = SAFETY * U * (mag + np.abs(y))
    return y.reshape(M, nheads * HD), (pre + ulp_bf16(np.abs(y) + pre) / 2).reshape(M, nheads * HD)


def gauss_tables(rng, Tp):
    """Gaussian cos / sin [Tp][32], exact in float32 (not a rotation - the kernel only multiplies by the table): every element exercises the
    bound, where a real table is (1, ~0) at position 0 and in the high dimensions"""
    f = lambda: rng.standard_normal((Tp, 32)).astype(np.float32).astype(np.float64)
    return f(), f()


def rope_f32_rows(rows, nheads, Tp, cs, sn, fused):
    M = rows.shape[0]
    x = rows[:, :nheads * HD].reshape(M, nheads, HD)
    pos = np.arange(M) % Tp
    return b16(ar.rope_f32(x, cs[pos][:, None, :], sn[pos][:, None, :], fused)).astype(np.float64).reshape(M, nheads * HD)


# ------------------------------------------------------------------------------------------------ attention
ATTN_CNT = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97]
ATTN_HEADS = [(1, 1), (2, 1), (4, 2)]
ATTN_TIERS = ["locator", "uniform", "gaussian"]
ATTN_PAD = 8


def attn_launches():
    """every cnt at Tp = cnt, cnt + 1 and 130; three rows a launch: the count, another of the list (clipped to Tp) and cnt = Tp; the tier and
    the head arrangement cycle so that every count meets every tier and every arrangement every tier"""
    out = []
    for ic, n in enumerate(ATTN_CNT):
        for it, Tp in enumerate((n, n + 1, 130)):
            cnt = [n, min(ATTN_CNT[(ic + 3 + it) % len(ATTN_CNT)], Tp), Tp]
            out.append(dict(tier=ATTN_TIERS[(ic + it) % 3], heads=ATTN_HEADS[ic % 3], cnt=cnt, Tp=Tp, seed=33000 + 10 * ic + it))
    return out


def attn_case(c):
    """one launch: logical q [B][H][Tp][64], K, V [B][Hkv][Tp][64] in float64 (rows >= cnt: NaN; uniform tier: stale keys, zero values), the
    payload rows [B Tp][ld] (padding columns NaN), locator targets"""
    (H, Hkv), cnt, Tp = c["heads"], np.asarray(c["cnt"]), c["Tp"]
    B, tier = len(cnt), c["tier"]
    rng = np.random.default_rng(c["seed"])
    QS, KS = (B, H, Tp, HD), (B, Hkv, Tp, HD)
    tg = None
    if tier == "locator":
        K = np.broadcast_to(ar.locator_key(np.arange(Tp), HD)[None, None], KS).copy()
        b_, h_, j_, d_ = np.meshgrid(np.arange(B), np.arange(Hkv), np.arange(Tp), np.arange(HD), indexing="ij")
        V = ar.locator_v(b_, h_, j_, d_)
        tg = (rng.integers(0, 1 << 30, (B, H, 1)) + 13 * np.arange(Tp)[None, None, :]) % cnt[:, None, None]
        tg[:, :, 0] = cnt[:, None] - 1
        for b in range(B):
            tg[b, :, cnt[b] - 1] = 0
        q = ar.locator_key(tg, HD)
    elif tier == "uniform":
        K = rng.integers(-4, 5, KS).astype(np.float64)
        V = rng.integers(-8, 9, KS).astype(np.float64)
        q = np.zeros(QS)
    else:
        K = ar.grid_bf16(0.5 * rng.standard_normal(KS))
        V = ar.grid_bf16(rng.standard_normal(KS))
        q = ar.grid_bf16(rng.standard_normal(QS))
    dead = (np.arange(Tp)[None, :] >= cnt[:, None])[:, None, :, None]          # [B][1][Tp][1]
    qd, kd = np.broadcast_to(dead, QS), np.broadcast_to(dead, KS)
    if tier == "uniform":
        K, V, kd = np.where(kd, ar.stale(rng, KS), K), np.where(kd, 0.0, V), np.zeros(KS, bool)
    ld, ldo = (H + 2 * Hkv) * HD + ATTN_PAD, H * HD + ATTN_PAD
    rows = np.full((B, Tp, ld), NAN16, np.uint16)
    flat = lambda a, n: a.transpose(0, 2, 1, 3).reshape(B, Tp, n * HD)
    rows[:, :, :H * HD] = flat(bits_nan(q, qd), H)
    rows[:, :, H * HD:(H + Hkv) * HD] = flat(bits_nan(K, kd), Hkv)
    rows[:, :, (H + Hkv) * HD:(H + 2 * Hkv) * HD] = flat(bits_nan(V, kd), Hkv)
    return dict(c, H=H, Hkv=Hkv, B=B, cnt=cnt, ld=ld, ldo=ldo, scale=0.125, q=q, K=K, V=V, rows=rows.reshape(B * Tp, ld), targets=tg)


def attn_reference(c, extra_keys=0):
    """float64: (out [B Tp][H 64] before the final rounding, zero rows behind cnt; the Gaussian tier's bound).  extra_keys: a mask that lets
    that many keys too many through (CPU sensitivity checks)"""
    B, H, Hkv, Tp = c["B"], c["H"], c["Hkv"], c["Tp"]
    out, bound = np.zeros((B, Tp, H, HD)), np.zeros((B, Tp, H, HD))
    gam = lambda k: k * U / (1.0 - k * U)
    for b in range(B):
        n = int(min(c["cnt"][b], Tp))
        nk = min(n + extra_keys, Tp)
        for h in range(H):
            hk = h // (H // Hkv)
            q, Kb, Vb = c["q"][b, h, :n], c["K"][b, hk, :nk], c["V"][b, hk, :nk]
            s = c["scale"] * (q @ Kb.T)
            Mx = s.max(-1, keepdims=True)
            p = np.exp(s - Mx)
            p /= p.sum(-1, keepdims=True)
            o, mag = p @ Vb, p @ np.abs(Vb)
            a = c["scale"] * (np.abs(q) @ np.abs(Kb).T)
            X = np.abs(s - Mx).max(-1)
            F = -(-n // 32) + 1
            E = (2 * gam(HD) * a.max(-1) + U * np.abs(s).max(-1) + 2.45 * X * U + 2 * F * U + 2.0 ** -17 + 2 * gam(n + F) + gam(n) + 4 * U)[:, None]
            pre = 2 * SAFETY * E * mag
            out[b, :n, h], bound[b, :n, h] = o, pre + ulp_bf16(np.abs(o) + pre) / 2
    return out.reshape(B * Tp, H * HD), bound.reshape(B * Tp, H * HD)


def attn_exact_expected(c):
    """the locator and the uniform tier's stated outputs [B Tp][H 64], zero rows behind cnt"""
    B, H, Hkv, Tp = c["B"], c["H"], c["Hkv"], c["Tp"]
    out = np.zeros((B, Tp, H, HD))
    for b in range(B):
        n = int(c["cnt"][b])
        for h in range(H):
            hk = h // (H // Hkv)
            if c["tier"] == "locator":
                out[b, :n, h] = c["V"][b, hk][c["targets"][b, h, :n]]
            else:
                out[b, :n, h] = b16(c["V"][b, hk, :n].sum(0).astype(np.float32) / np.float32(n)).astype(np.float64)[None]
    return out.reshape(B * Tp, H * HD)


def attn_f32(c, mask_leak=0):
    """k_lasr_attn's arithmetic in float32 numpy: keys >= n staged as zero, 32-key tiles in order, the mask, the online softmax, P = hi + lo"""
    f = np.float32
    B, H, Hkv, Tp = c["B"], c["H"], c["Hkv"], c["Tp"]
    out = np.zeros((B, Tp, H, HD))
    sc = f(c["scale"])
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            n = int(c["cnt"][b])
            nt = -(-n // 32)
            for h in range(H):
                hk = h // (H // Hkv)
                q = c["q"][b, h, :n].astype(f)
                K, V = np.zeros((32 * nt, HD), f), np.zeros((32 * nt, HD), f)
                stage = min(n + mask_leak, Tp, 32 * nt)
                K[:stage], V[:stage] = c["K"][b, hk, :stage], c["V"][b, hk, :stage]
                m, l, O = np.full(n, -np.inf, f), np.zeros(n, f), np.zeros((n, HD), f)
                for t in range(nt):
                    Kt, Vt = K[32 * t:32 * t + 32], V[32 * t:32 * t + 32]
                    s = ((q @ Kt.T).astype(f) * sc).astype(f)
                    s = np.where(np.arange(32 * t, 32 * t + 32)[None] < n + mask_leak, s, f(-np.inf)).astype(f)
                    mn = np.maximum(m, s.max(-1))
                    alpha = np.exp(m - mn).astype(f)
                    pe = np.exp(s - mn[:, None]).astype(f)
                    hi = b16(pe)
                    lo = b16(pe - hi)
                    l = (l * alpha + pe.sum(-1, dtype=f)).astype(f)
                    O = ((O * alpha[:, None]).astype(f) + hi @ Vt + lo @ Vt).astype(f)
                    m = mn
                out[b, :n, h] = b16(O / l[:, None]).astype(np.float64)
    return out.reshape(B * Tp, H * HD)


# ------------------------------------------------------------------------------------------------ GLU + depthwise conv
DW_K, DW_C, DW_CNT = [1, 2, 3, 8, 9, 63, 64], [64, 72, 136], [1, 2, 63, 64, 65, 129]
GATE_ONE, GATE_ZERO = 32.0, -128.0


def dw_launches():
    """every k with every tier and both activations; C, the counts (three rows a launch) and Tp in {largest count, 130} cycle"""
    out, n = [], 0
    for ik, k in enumerate(DW_K):
        for tier in ("dense", "impulse"):
            for act in (1, 0):
                cnt = [DW_CNT[(n + j) % 6] for j in range(3)]
                out.append(dict(tier=tier, act=act, k=k, C=DW_C[n % 3], cnt=cnt, Tp=max(cnt) if n // 2 % 2 else 130, seed=34000 + n))
                n += 1
    return out


DW_GAUSS = [dict(tier="gauss", act=1, k=9, C=72, cnt=[65, 129, 2], Tp=130, seed=34900),
            dict(tier="gauss", act=1, k=64, C=64, cnt=[129, 64, 63], Tp=129, seed=34901)]
DW_GATE_PROBE = dict(tier="gauss", act=1, k=1, C=136, cnt=[129, 65, 1], Tp=130, seed=34902, probe=True)      # taps +1 / -1, shift 0: the launch returns max(+-g, 0)


def dw_case(c):
    """a [B][Tp][C], gate, taps [k][C], shift [C] in float64 and the payload rows pw [B Tp][2 C] (frames >= cnt: NaN)"""
    k, Cc, Tp, cnt = c["k"], c["C"], c["Tp"], np.asarray(c["cnt"])
    B = len(cnt)
    rng = np.random.default_rng(c["seed"])
    live = np.arange(Tp)[None, :] < cnt[:, None]
    S = (B, Tp, Cc)
    if c["tier"] == "gauss":
        a, gate = ar.grid_bf16(rng.standard_normal(S)), np.clip(ar.grid_bf16(2.0 * rng.standard_normal(S)), -8.0, 8.0)
        taps = (rng.standard_normal((k, Cc)) / math.sqrt(k)).astype(np.float32).astype(np.float64)
        shift = (0.1 * rng.standard_normal(Cc)).astype(np.float32).astype(np.float64) * (0.0 if c.get("probe") else 1.0)
    elif c["tier"] == "dense":
        a = rng.integers(-4, 5, S).astype(np.float64)
        gate = np.where(rng.integers(0, 4, S) > 0, GATE_ONE, GATE_ZERO)
        taps = rng.integers(-2, 3, (k, Cc)).astype(np.float64)
        taps[np.arange(k), (7 * np.arange(k)) % Cc] = 1.0 + np.arange(k) % 2                # no tap is zero everywhere
        shift = rng.integers(-16, 17, Cc).astype(np.float64) * 2.0 ** -4
    else:
        a, gate = np.zeros(S), np.full(S, GATE_ZERO)
        for b in range(B):                                    # impulses at the row's first and last frame and every k + 3 between, never two in a window
            n = int(cnt[b])
            for t in [0] + list(range(k, n - k, k + 3)) + [n - 1]:
                ch = slice(None) if n - 1 >= k or n == 1 else slice(0, None, 2) if t == 0 else slice(1, None, 2)
                a[b, t, ch] = (rng.integers(1, 4, Cc) * rng.choice([-1.0, 1.0], Cc))[ch]
                gate[b, t, ch] = GATE_ONE
        taps = np.repeat((2.0 ** (np.arange(k) - 40.0))[:, None], Cc, 1) * rng.choice([-1.0, 1.0], (1, Cc))
        shift = np.zeros(Cc)
    d = dict(c, B=B, cnt=cnt, live=live, a=a, gate=gate, taps=taps, shift=shift)
    if c["act"] == 0 and c["tier"] != "gauss":                # keep the SiLU pre-activations inside +-SILU_VMAX: halve a
        if c["tier"] == "dense":
            d["shift"] = shift = shift / 2.0
        while np.abs(dw_pre(d)[0]).max() > SILU_VMAX:
            d["a"] = d["a"] / 2.0
        # as gemm_inputs: a draw whose exempt share of the live elements passes the cap is drawn again (a property of the inputs alone)
        if exempt_share(dw_reference(d)[1], live.reshape(-1, 1)) > SILU_SHARE:
            assert c.get("redraw", 0) < 16, "no input within the exempt cap found"
            return dw_case(dict(c, seed=c["seed"] + 1000, redraw=c.get("redraw", 0) + 1))
    dead = np.broadcast_to(~live[:, :, None], S)
    d["pw"] = np.concatenate([bits_nan(d["a"], dead), bits_nan(d["gate"], dead)], -1).reshape(B * Tp, 2 * Cc)
    return d


def dw_pre(d, mut=None):
    """(y = shift + sum taps g before the activation [B][Tp][C], sum |taps g| + |shift|, g, exempt g) in float64; frames >= cnt of g are zero"""
    k, Tp = d["k"], d["Tp"]
    if d["tier"] == "gauss":
        g, ex = near_boundary(d["a"] * sigmoid64(d["gate"]), margin(d["gate"]))
    else:
        g, ex = np.where(d["gate"] == GATE_ONE, d["a"], 0.0), np.zeros(d["a"].shape, bool)
    g = np.where(d["live"][:, :, None], g, 0.0)
    ex = ex & d["live"][:, :, None]
    padl = (k - 1) // 2 if mut != "pad_side" else k - 1 - (k - 1) // 2
    gp = np.pad(g, ((0, 0), (padl, k - 1 - padl), (0, 0)))
    exu = np.pad(np.where(ex, ulp_bf16(g), 0.0), ((0, 0), (padl, k - 1 - padl), (0, 0)))
    y, mag, slack = np.zeros(g.shape) + d["shift"], np.zeros(g.shape) + np.abs(d["shift"]), np.zeros(g.shape)
    for kk in range(k):
        if mut == ("drop_tap", kk):
            continue
        w = d["taps"][kk if mut != "mirror" else k - 1 - kk][None, None, :]
        y = y + w * gp[:, kk:kk + Tp]
        mag = mag + np.abs(w * gp[:, kk:kk + Tp])
        slack = slack + np.abs(w) * exu[:, kk:kk + Tp]
    return y, mag, g, slack


def dw_reference(d, mut=None):
    """(out [B Tp][C] in float64: bf16 values for the exact tiers, the unrounded y for the Gaussian tier; exempt (act 0) or None; the Gaussian
    tier's delta)"""
    y, mag, g, slack = dw_pre(d, mut)
    k, live = d["k"], d["live"][:, :, None]
    ex = delta = None
    if d["tier"] == "gauss":
        out = np.maximum(y, 0.0)
        delta = SAFETY * (k * U / (1.0 - k * U)) * mag + slack
    elif d["act"] == 1:
        out = T(np.maximum(y, 0.0))
    else:
        out, ex = silu_reference(y)
        ex = (ex & live).reshape(-1, d["C"])
    flat = lambda v: None if v is None else np.where(live, v, 0.0).reshape(-1, d["C"])
    return flat(out), ex, flat(delta)


# ------------------------------------------------------------------------------------------------ im2col, pack
IM2COL_KS_ST, IM2COL_C = [(3, 2), (5, 2), (2, 1)], [8, 72]
NAN_PAYLOADS = np.array([0x7FC1, 0xFFC2, 0x7F81, 0xFFFF], np.uint16)


def im2col_case(ks, st, Cc, seed):
    """payloads in [B][Tin][C] with NaN payloads among the live frames; Tin = (Tout - 1) st + ks: the last live frame of the row with cnt = Tout
    reads exactly to the end of the input"""
    rng = np.random.default_rng(seed)
    Tout = 6
    Tin = (Tout - 1) * st + ks
    cnt = np.array([3, 0, Tout], np.int32)
    x = rng.integers(0x3C00, 0x4200, (3, Tin, Cc)).astype(np.uint16) | (rng.integers(0, 2, (3, Tin, Cc)).astype(np.uint16) << 15)
    x[:, ::3, 1::5] = NAN_PAYLOADS[rng.integers(0, 4, x[:, ::3, 1::5].shape)]
    return dict(x=x, cnt=cnt, Tin=Tin, Tout=Tout, ks=ks, st=st, C=Cc)


def im2col_reference(c):
    B, Tout, ks, st, Cc = 3, c["Tout"], c["ks"], c["st"], c["C"]
    out = np.zeros((B, Tout, ks, Cc), np.uint16)
    for b in range(B):
        for t in range(int(c["cnt"][b])):
            out[b, t] = c["x"][b, t * st:t * st + ks]
    return out.reshape(B * Tout, ks * Cc)


def pack_reference(feats, F, Kp):
    B, Fp, mels = feats.shape
    out = np.zeros((B, Fp, Kp), np.uint16)
    out[:, :, :mels] = gr.bf16_bits(feats)
    out[np.arange(Fp)[None, :] >= np.asarray(F)[:, None]] = 0
    return out.reshape(B * Fp, Kp)


# ------------------------------------------------------------------------------------------------ arg-max, collapse
ARGMAX_V = [1, 63, 64, 65, 257, 1000]


def argmax_rows(V, seed):
    """seven rows (M % 4 != 0): Gaussian; a tie inside a lane's stride (i, i + 64) and across lanes (i, i + 1); +inf ties; all -inf; all NaN;
    NaN in front of the maximum; the maximum in the last column"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((7, V)).astype(np.float32)
    i = V // 3
    x[1, [i, min(i + 64, V - 1), min(i + 1, V - 1)]] = 9.0
    x[2, [V - 1, V // 2]] = np.inf
    x[3], x[4] = -np.inf, np.nan
    x[5, :V // 2] = np.nan
    x[6, V - 1] = 9.0
    return x


def argmax_reference(x, highest=False):
    y = np.where(np.isnan(x), -np.inf, x)
    if highest:
        return (x.shape[1] - 1 - np.argmax(y[:, ::-1], axis=1)).astype(np.int32)
    return np.argmax(y, axis=1).astype(np.int32)


COLLAPSE_CNT = [0, 1, 255, 256, 257, 513]
COLLAPSE_TP, BLANK, NTOKEN = 520, 2, 5


def collapse_launches():
    """two launches of three rows: cnt (0, 255, 513) and (1, 256, 257).  Row patterns: 0 every frame kept (alternating tokens), 1 random with
    repeats and blanks, a repeat astride frames 255 | 256 and `a blank a` at 253 .. 255, 2 blanks only.  Frames behind cnt hold tokens."""
    out = []
    for li, (cnt, pats) in enumerate((([0, 255, 513], [0, 2, 1]), ([1, 256, 257], [1, 1, 0]))):
        rng = np.random.default_rng(35000 + li)
        pred = rng.integers(0, NTOKEN, (3, COLLAPSE_TP)).astype(np.int32)
        for b in range(3):
            pat = pats[b]
            if pat == 0:
                pred[b] = np.where(np.arange(COLLAPSE_TP) % 2 == 0, 3, 4)
            elif pat == 1:
                pred[b, 250:253] = BLANK
                pred[b, 253:258] = [1, BLANK, 1, 1, 0]
            else:
                pred[b, :cnt[b]] = BLANK
                pred[b, cnt[b]:] = 3
        out.append(dict(pred=pred, cnt=np.asarray(cnt, np.int32)))
    return out


def collapse_reference(pred, cnt, blank=BLANK, drop_at=None):
    """(tokens [B][Tp] with -1 behind ntok, ntok) through lasr_ref.greedy_ctc on one-hot logits; drop_at: a kernel that loses a kept token at that frame"""
    B, Tp = pred.shape
    tokens, ntok = np.full((B, Tp), -1, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        n = int(min(cnt[b], Tp))
        onehot = np.eye(max(int(pred.max()) + 1, blank + 1))[pred[b, :n]]
        toks = lr.greedy_ctc(onehot, blank) if n else []
        if drop_at is not None and n > drop_at and pred[b, drop_at] != blank and pred[b, drop_at] != pred[b, drop_at - 1]:
            kept = [t for t in range(n) if pred[b, t] != blank and (t == 0 or pred[b, t] != pred[b, t - 1])]
            toks = [int(pred[b, t]) for t in kept if t != drop_at]
        tokens[b, :len(toks)], ntok[b] = toks, len(toks)
    return tokens, ntok


# ------------------------------------------------------------------------------------------------ the operators on values (the block chain)
def op_gemm(x, w, bias, epi, R=None, a=0.0, b=0.0):
    v = T(x @ w.T + (0.0 if bias is None else bias))
    if epi == LG_RELU:
        v = np.maximum(v, 0.0)
    elif epi == LG_SILU:
        v = T(silu64(v))
    elif epi == LG_AXPBY:
        v = T(a * R + b * v)
    return v


def op_ln(x, w, b, eps):
    return T(er.ln_reference(x, w, b, eps)[0])


def op_rope(rows, nheads, Tp, cs, sn):
    out = rows.copy()
    out[:, :nheads * HD] = T(rope_reference(rows, nheads, Tp, cs, sn)[0])
    return out


def op_attn(qkv, H, Hkv, n, scale):
    """one row of the batch: qkv [n][(H + 2 Hkv) 64] -> [n][H 64]"""
    split = lambda a, nh: a.reshape(n, nh, HD).transpose(1, 0, 2)[None]
    c = dict(B=1, H=H, Hkv=Hkv, Tp=n, cnt=np.array([n]), scale=scale, q=split(qkv[:, :H * HD], H), K=split(qkv[:, H * HD:(H + Hkv) * HD], Hkv),
             V=split(qkv[:, (H + Hkv) * HD:], Hkv))
    return T(attn_reference(c)[0])


def op_glu_dwconv(pw, taps, shift, k, act):
    """one row of the batch: pw [n][2 C] -> [n][C]"""
    n, C2 = pw.shape
    g = T(pw[None, :, :C2 // 2] * sigmoid64(pw[None, :, C2 // 2:]))
    padl = (k - 1) // 2
    gp = np.pad(g, ((0, 0), (padl, k - 1 - padl), (0, 0)))
    y = sum(taps[kk][None, None] * gp[:, kk:kk + n] for kk in range(k)) + shift
    return T(np.maximum(y, 0.0) if act == 1 else silu64(y))[0]


# ------------------------------------------------------------------------------------------------ the entry points
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _L():
    from mlx_audio_swift_amd import _lib as L
    return L.lib()


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def run_gemm(c, d, tile, epi=None):
    """mis_debug_lasr_gemm -> (status, C payloads [M][N] (LG_F32: float32), R as the launch left it or None, report)"""
    epi = c["epi"] if epi is None else epi
    M, N = c["M"], c["N"]
    out = np.zeros((M, N), np.float32 if epi == LG_F32 else np.uint16)
    rep = np.full(2, -7, np.int32)
    sep = d.get("Rb") is not None and not c["in_place"]
    Ra = np.zeros((M, N), np.uint16) if sep else None
    w, bias, cnt = gr.exact_bits(d["w"]), None if d["bias"] is None else gr.exact_bits(d["bias"]), _i32(d["cnt"])
    img, Rb = np.ascontiguousarray(d["img"]), None if d.get("Rb") is None else np.ascontiguousarray(d["Rb"])
    st = _L().mis_debug_lasr_gemm(0, epi, _ptr(img), _ptr(w), _ptr(bias), _ptr(Rb), c["a"], c["b"], _ptr(cnt), d["Tp"], int(c["in_place"] and Rb is not None), tile,
                                  M, N, c["K"], c["ldx"], _ptr(out), _ptr(Ra), _ptr(rep))
    return st, out, Ra, tuple(int(v) for v in rep)


def run_ln(xb, w, b, eps=EPS, cnt=None, Tp=1):
    """xb: payloads [M][d]"""
    xb = np.ascontiguousarray(xb, np.uint16)
    out = np.zeros(xb.shape, np.uint16)
    bw, bb, cnt = gr.exact_bits(w), gr.exact_bits(b), _i32(cnt)
    st = _L().mis_debug_lasr_ln(0, _ptr(xb), _ptr(bw), _ptr(bb), xb.shape[0], xb.shape[1], eps, _ptr(cnt), Tp, _ptr(out))
    return st, out


def run_rope(rows, nheads, Tp, cs, sn):
    """rows: payloads [M][ld] -> (status, the rows after the launch)"""
    img = np.ascontiguousarray(rows, np.uint16).copy()
    c32, s32 = np.ascontiguousarray(cs, np.float32), np.ascontiguousarray(sn, np.float32)
    st = _L().mis_debug_lasr_rope(0, _ptr(img), img.shape[0], img.shape[1], nheads, Tp, _ptr(c32), _ptr(s32))
    return st, img


def run_attn(c):
    out = np.zeros((c["B"] * c["Tp"], c["H"] * HD), np.uint16)
    rows, cnt = np.ascontiguousarray(c["rows"]), _i32(c["cnt"])
    st = _L().mis_debug_lasr_attn(0, _ptr(rows), c["ld"], c["H"], c["Hkv"], _ptr(cnt), c["B"], c["Tp"], c["scale"], c["ldo"], _ptr(out))
    return st, out


def run_glu_dwconv(d, taps=None, act=None):
    out = np.zeros((d["B"] * d["Tp"], d["C"]), np.uint16)
    rep = np.full(1, -7, np.int32)
    pw, cnt = np.ascontiguousarray(d["pw"]), _i32(d["cnt"])
    tp, sh = np.ascontiguousarray(d["taps"] if taps is None else taps, np.float32), np.ascontiguousarray(d["shift"], np.float32)
    st = _L().mis_debug_lasr_glu_dwconv(0, d["act"] if act is None else act, _ptr(pw), _ptr(tp), _ptr(sh), _ptr(cnt), d["B"], d["Tp"], d["C"], tp.shape[0],
                                        _ptr(out), _ptr(rep))
    return st, out, int(rep[0])


def run_im2col(c):
    out = np.zeros((3 * c["Tout"], c["ks"] * c["C"]), np.uint16)
    x, cnt = np.ascontiguousarray(c["x"]), _i32(c["cnt"])
    st = _L().mis_debug_lasr_im2col(0, _ptr(x), _ptr(cnt), 3, c["Tin"], c["Tout"], c["C"], c["ks"], c["st"], _ptr(out))
    return st, out


def run_pack(feats, F, Kp):
    B, Fp, mels = feats.shape
    out = np.zeros((B * Fp, Kp), np.uint16)
    feats, F = np.ascontiguousarray(feats, np.float32), _i32(F)
    st = _L().mis_debug_lasr_pack(0, _ptr(feats), _ptr(F), B, Fp, mels, Kp, _ptr(out))
    return st, out


def run_argmax(x):
    x = np.ascontiguousarray(x, np.float32)
    pred = np.full(x.shape[0], -7, np.int32)
    st = _L().mis_debug_lasr_argmax(0, _ptr(x), x.shape[0], x.shape[1], _ptr(pred))
    return st, pred


def run_collapse(pred, cnt, blank=BLANK):
    pred, cnt = _i32(pred), _i32(cnt)
    tokens, ntok = np.full(pred.shape, -7, np.int32), np.full(pred.shape[0], -7, np.int32)
    st = _L().mis_debug_lasr_collapse(0, _ptr(pred), _ptr(cnt), pred.shape[0], pred.shape[1], blank, _ptr(tokens), _ptr(ntok))
    return st, tokens, ntok
