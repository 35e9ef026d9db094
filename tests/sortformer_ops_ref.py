"""Operator-level reference of the private kernels of csrc/sortformer.hip (k_sf_gemm<LOAD>, k_sf_attn<ND, REL>, k_sf_glu_dwconv, k_sf_conv0,
k_sf_stats, k_sf_ln, k_sf_intake, k_sf_peak), inputs whose result is known exactly, the case tables of tests/test_gpu_sortformer_ops.py, the
launchers' rules restated, and thin wrappers of the mis_debug_sortformer_* entry points (include/mi_speech_debug.h).  Pure numpy, float64,
written from the kernel header comments; nothing here calls a kernel to build its data.  tests/test_sortformer_ops_ref_cpu.py proves every
claim below that the GPU test leans on.  Every tensor is float32 on the device: the exact tiers compare float32 BIT PATTERNS with the
float64 result rounded once (it is representable, so the rounding is the identity).

Specification.  live(b, t) = t < min(cnt[b], Tp) (cnt None: every row); a row that is not live is written as ZERO whatever the inputs hold
there (the cases put NaN there):
  GEMM       rows [B][Tp rowmul][.], row r of a batch entry is live iff r < min(cnt[b], Tp) rowmul.  v = sum_k load(X)[r][k] W[n][k] + bias[n];
             act: none, SiLU v / (1 + exp(-v)), ReLU, sigmoid 1 / (1 + exp(-v));  R given: v = R[r][n] + ra v (R may BE the output buffer);
             pos given: v += pos[r // rowmul][n].  Loads (sf_gemm dispatches on p.load, anything else is the plain load):
               0 plain X[r ldx + k];  1 LayerNorm (X - stats[r][0]) stats[r][1] lnw[k] + lnb[k];  2 max(X, 0);
               3 depthwise: X [B][Tin][Fin][K] channels last, r = t Fout + f, value = dwb[k] + sum_{i, j < 3} dww[3 i + j][k] X[2 t + i - 1][2 f + j - 1][k],
                 X zero outside 0 <= frame < min(cnt_in[b], Tin) and 0 <= bin < Fin.
  attention  qkv [B Tp][ld]: q of head h at column h hd, k at koff + h hd, v at voff + h hd.  n = min(cnt[b], Tp).
             score[i][j] = ((q_i qscale + u_h) . k_j + (q_i qscale + v_h) . P[i - j + Tcap - 1][h]) / sdk  (REL; table rows outside
             0 .. 2 Tcap - 2 read as zero), (q_i qscale) . k_j / sdk without REL;  out_i = sum_{j < n} softmax_j(score) v_j;  queries >= n: zero.
             sf_attn: ND = 1 iff hd <= 32 (the head is zero-padded to 32 ND columns).  Call sites: Conformer qscale 1, sdk sqrt(hd), REL;
             BART qscale hd^-1/2, sdk 1.
  GLU + dw   g[t] = a[t] sigmoid(gate[t]) for 0 <= t < n (a the first C columns of pw, gate the last), zero outside;
             y[t] = shift + sum_kk taps[kk] g[t - (k - 1) // 2 + kk];  out = y / (1 + exp(-y)), frames >= n: zero
  conv0      out[b][t][f][c] = max(bias[c] + sum_{i, j < 3} w[3 i + j][c] feats[b][2 t + i - 1][2 f + j - 1], 0) for t < T1[b], zero behind; feats
             zero outside 0 <= frame < min(F[b], Fp), 0 <= bin < mels
  stats      mean and 1 / sqrt(var + eps), two-pass in float32;  ln  y = (x - mean) rstd w + b, rows t >= cnt: zero;  intake  y = x g
  peak       scale[b] = 1 / (max_{i < N[b]} |x_i| + 1e-3) if on else 1

Exact GEMM tier (enc_ref's grid): x in {-1, 0, 1} 2^-5, w integers in [-4, 4], integer bias, R and pos multiples of 2^-5 up to 2, ra in
{1, 0.5}: every partial sum is an integer multiple of 2^-7 below 2^24 units, exact in float32 in any order, fused or not.  LayerNorm load:
mean a multiple of 2^-3 up to 4, rstd in {0.5, 1, 2, 4}, lnw in +-{0.5, 1, 2}, lnb a multiple of 2^-5 up to 2, X = mean + s 2^-5, |s| <= 2:
the loaded value is a multiple of 2^-7 below 1.  Depthwise load: x in {-1, 0, 1} 2^-5, integer taps in [-2, 2], dwb multiples of 2^-5:
a multiple of 2^-5 of at most 19 + 2 units.  Activations of this tier: none and ReLU.

SiLU / sigmoid rule.  On the exactly known pre-activation v the device evaluates v / (1 + expf(-v)) in float32, u = 2^-24: expf is ROCm's
precise routine (1 ulp = 2 u relative), D = 1 + E one rounding on top of E / D <= 1 of that (3 u), the division is correctly rounded
(the Makefile compiles with -O3 and neither -ffast-math nor a relaxed-division flag, so hipcc keeps IEEE float32 division and sqrt) (u):
relative error <= 4 u, margin = SAFETY 4 u = 8 u.  The cases keep |v| <= ACT_VMAX = 64 (expf(88.8) overflows: below -88 the
expression returns -0 where v sigmoid(v) is still a normal number).  The output is float32: no rounding-boundary exemption.

Gaussian GEMM tier: |out - ref| <= SAFETY (gamma_K sum |x w| + sum dload |w| + u (|v| + |out| [R] + |out| [pos])), gamma_K = K u / (1 - K u)
(gemm_ref's float32 summation bound), dload = 3 u (|t rstd lnw| + |lnb|) for the LayerNorm load (two products and an fma) and
gamma_10 (|dwb| + sum |dww x|) for the depthwise load (a chain of nine fma).

Attention tiers.
  content locator (attn_ref's): key j = locator_key(j), q_i qscale + u = locator_key(target_i): the target scores 2 * 4096, every other key
    at most 4096; the band term is bounded by sum |q + v| max |P| <= 600 (P in {-1, 0, 1}, v small integers), so the target leads by more
    than 3400 / sdk >= 425 and every other exp is exactly 0 in float32: out == V[target] bit for bit.  u = -locator_key(s_h) for a fixed key
    s_h per head and q = (locator_key(target) - u) / qscale: a kernel that drops u scores key s_h as high as
    the target and leaves V[target]; one that scales u by qscale (the cases include qscale 0.5) is caught by the Gaussian tier.  Two keys j, j' of locator_key
    coincide only if j // hd + j' // hd + 2 is a multiple of hd: the tier runs where 2 ((n - 1) // hd) + 2 < hd (hd 8: up to 24 frames; the
    distance locator takes its place above).
  uniform: q = u = v = 0, every score 0, V integers in [-8, 8]: out == float32(sum) / float32(n), one correctly rounded division; K holds
    stale +-1e4 and V zeros behind n, so an admitted key changes the denominator.
  distance locator (REL): k = 0 (the content term vanishes), q = 0, v_h = the unit vector of column c_h, P[d][h hd + c_h] = -1024 |d - delta_h|:
    score[i][j] = -1024 |i - j - delta_h| / sdk.  Query i returns V[j*], j* = clip(i - delta_h, 0, n - 1), the one live key nearest distance
    delta_h (unique: the distances of j < n to i - delta_h are distinct integers on one side when clipped); the runner-up trails by
    1024 / sdk >= 128, its exp is exactly 0.  u_h = the unit vector of column c_h + 1, whose P column locates distance -delta_h - 1: a kernel
    that exchanges u and v lands there.  Every other P column holds small integers (they meet q + v = 0 there).
  tight table: the distance locator at Tcap == max cnt with delta = +-(n - 1) among the heads reads table rows 0 and 2 Tcap - 2 into a live
    output; at Tcap > max cnt every table row of a distance no live pair of the launch has (|d| >= max cnt) holds NaN.  Why NaN there cannot
    reach a live output: the band product G[r][i] = sum_c Pb[r][c] (q_i + v)[c] is a matrix product, element (r, i) reads band row r and
    query i only (the 32 x 32 MFMA computes D[r][i] = sum_k A[r][k] B[k][i] + C[r][i]: no term mixes rows of A or columns of B).  The entry
    added to score (i, j) is band row i - j + 31 of the tile, table row i - j + Tcap - 1: for a live query and a live key that distance IS a
    live pair's.  A key j >= n is replaced by -inf through a select after the addition; a query i >= n owns column i of S and of O = V^T P^T
    (again one column of B per output column), its running maximum and sum are per query, and its row is written as zero.
  gaussian: |out - ref| <= u |ref| + 2 SAFETY E sum_j p_j |v_j|,
    E = 2 gamma_hd max (a_c + a_b) + 3 u max |s| + 2 X u + 2 F u + 3 gamma_(n + F) + 4 u:  the content and the band product, each hd products
    on the MFMA (a_c = sum |(q + u) k| / sdk, a_b = sum |(q + v) P| / sdk: the band term's second 2 gamma); the rounding of q qscale, of the
    addition and of the division by sdk (3 u |s|);  float32 P, so no 2^-17;  expf(x) of a rounded x = s - m, X = max |s - M|, one factor per
    32-key tile and the final one, F = ceil(n / 32) + 1, precise expf 2 u each;  the accumulation of P V over n keys with F rescales (2 gamma)
    and the denominator, two half-lanes per query combined at the end (gamma);  the division and the store (4 u).  A 64-query block
    changes no term: every query's chain is its own.

GLU + depthwise tiers.  exact: gates +32 / -128 make the float32 sigmoid exactly 1 (expf(-32) < 2^-24) and 0 (expf(128) = inf, 1 / inf = 0),
a integers in [-4, 4], taps integers in [-2, 2], shift 1024 + an integer in [-16, 16]: y is an integer in [512, 1536], exact in any order,
and 1 + expf(-y) == 1, so the SiLU returns y.  impulse: isolated frames carry a != 0, tap kk weighs 2^(kk - 40), shift 0: an output sees
one tap (a mirrored or shifted tap changes it by a factor of 2 or more); y is exact and the output is held to the SiLU margin.  gaussian:
dg = 5 u |g| (the sigmoid and one product), dy = gamma_(k + 1) (|shift| + sum |taps g|) + sum |taps| dg, |out - ref| <= SAFETY (1.1 dy + 4 u |ref|)
(|silu'| <= 1.1).

LayerNorm / stats: enc_ref's constant, balanced and Gaussian tiers and its derivation with the final float32 rounding in place of the bf16
one: |y - ref| <= SAFETY u [(d + 1) A rstd |w| + ((d + 4) / 2 + (d + 1) A / sigma + 6) n_i + |ref|]; mean within SAFETY (d + 1) u A, rstd within
SAFETY ((d + 4) / 2 + (d + 1) A / sigma + 2) u relative.  intake: one float32 product, bit for bit.  peak: one addition and one correctly
rounded division (the Makefile note above), bit for bit."""
import ctypes as C
import math

import numpy as np

import attn_ref as ar
import enc_ref as er
import gemm_ref as gr

OK, GENERATION_FAILED, INVALID_INPUT = 0, 2, 3
LOAD_ACT, LOAD_LN, LOAD_RELU, LOAD_DW = range(4)
ACT_NONE, ACT_SILU, ACT_RELU, ACT_SIGMOID = range(4)
SAFETY, U = ar.SAFETY, ar.U
POISON, EPS, DW_MAXK = 0xFFFFFFFF, 1e-5, 31
ACT_MARGIN, ACT_VMAX = SAFETY * 4.0 * U, 64.0
f32 = np.float32


def gam(k):
    return k * U / (1.0 - k * U)


def r32(v):
    """float64 -> the nearest float32, kept in float64"""
    return np.asarray(v, np.float64).astype(f32).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, want64):
    """got float32 (device), want float64 values that are float32-representable (+0 and -0 are told apart: the kernels write +0)"""
    return np.array_equal(bits(got), bits(np.asarray(want64, np.float64).astype(f32)))


def nan_where(v, dead):
    out = np.array(v, np.float64, copy=True)
    out[np.broadcast_to(dead, out.shape)] = np.nan
    return out


def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def silu64(v):
    return np.asarray(v, np.float64) * sigmoid64(v)


def half(t):
    return (t - 1) // 2 + 1 if t >= 1 else 0


# ------------------------------------------------------------------------------------------------ launchers restated
def gemm_load_rule(load):
    """sf_gemm: the LayerNorm, ReLU and depthwise loads by name, everything else the plain load"""
    return load if load in (LOAD_LN, LOAD_RELU, LOAD_DW) else LOAD_ACT


def attn_rule(hd, rel):
    """sf_attn: (ND, REL)"""
    return (1 if hd <= 32 else 2, 1 if rel else 0)


GEMM_INSTANTIATIONS = {0, 1, 2, 3}
ATTN_INSTANTIATIONS = {(1, 0), (1, 1), (2, 0), (2, 1)}

# ------------------------------------------------------------------------------------------------ GEMM
GEMM_ROWS = {1: [(1, 1)], 63: [(63, 1), (21, 3), (9, 7)], 64: [(64, 1), (32, 2)], 65: [(65, 1), (13, 5)], 129: [(129, 1), (43, 3)]}
GEMM_N = [1, 4, 63, 64, 65, 130]
GEMM_K = [8, 31, 32, 33, 72, 96, 288]
# depthwise load: rows = Tout Fout, Fout = half(Fin): (Fin, Tout) for the row counts above (Fin 1 gives the single row)
DW_ROWS = {1: (1, 1), 63: (5, 21), 64: (3, 32), 65: (10, 13), 129: (5, 43)}


def _counts(Tp, rowmul, mode, k):
    """mode 0: None at batch 1 (the finalize-time table GEMM).  mode 1: three rows - a count inside a tile, cnt > Tp (the min clamp), and a
    short row whose later 64-row tiles are wholly dead (0 or 1 frames)"""
    if mode == 0:
        return None
    return [max(1, (Tp * 5) // 8), Tp + 3, k % 2]


def gemm_cases(tier):
    """tier exact: every load x every rows x every N (120 launches), K, bias, the residual, pos, padding, the counts and the activation
    cycling along both progressions; tier gauss / act: every third of them.  Padded layouts (NaN between the rows of X and R, poison between those of Y) where (i + j + load) % 6 == 0: every load, in every tier."""
    out = []
    for load in range(4):
        n = 0
        for i, rows in enumerate(GEMM_ROWS):
            for j, N in enumerate(GEMM_N):
                n += 1
                if tier != "exact" and (i + j + load) % 3:
                    continue
                Tp, rowmul = GEMM_ROWS[rows][(j + load) % len(GEMM_ROWS[rows])]
                c = dict(tier=tier, load=load, N=N, K=GEMM_K[(i + 2 * j + load) % 7], bias=(i + j) % 3 != 0, pad=(i + j + load) % 6 == 0,
                         seed=36000 + 1000 * load + 10 * n + dict(exact=0, gauss=1, act=2)[tier])
                if load == LOAD_DW:
                    Fin, Tout = DW_ROWS[rows]
                    Tp, rowmul = Tout, half(Fin)
                    c.update(Fin=Fin, Tin=2 * Tout - (i + j) % 2)                 # Tin odd and even: half(Tin) == Tout both ways
                c.update(Tp=Tp, rowmul=rowmul, cnt=_counts(Tp, rowmul, (i + j) % 3 != 1, i + j))
                if tier == "act":
                    c.update(act=(ACT_SILU, ACT_SIGMOID)[(i + j) % 2], R=None, ra=1.0, pos=False)
                else:
                    c.update(act=(ACT_NONE, ACT_RELU)[(i + j // 2) % 2], R=(None, "in", "sep")[(i + 2 * j + load) % 3], ra=(1.0, 0.5)[(i + j) % 2],
                             pos=(i + j + load) % 2 == 0)
                out.append(c)
    return out


def gemm_case(c):
    """a case's operands in float64 (all float32-representable) and the payloads (NaN behind the counts and in the padding)"""
    rng = np.random.default_rng(c["seed"])
    load, K, N, Tp, rm = c["load"], c["K"], c["N"], c["Tp"], c["rowmul"]
    cnt = None if c["cnt"] is None else np.asarray(c["cnt"], np.int32)
    B = 1 if cnt is None else len(cnt)
    nr = Tp * rm
    rows = B * nr
    T = np.full(B, Tp) if cnt is None else np.minimum(cnt, Tp)
    live = (np.arange(nr)[None, :] < (T * rm)[:, None]).reshape(rows)
    exact = c["tier"] != "gauss"
    d = dict(c, B=B, rows=rows, live=live, cntv=cnt)
    gi = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)
    gs = lambda shape, s=1.0: r32(s * rng.standard_normal(shape))
    d["w"] = gi(-4, 4, (N, K)) if exact else gs((N, K), 1.0 / math.sqrt(K))
    d["bias"] = None if not c["bias"] else gi(-3, 3, N) if exact else gs(N, 0.5)
    d["Rv"] = None if c["R"] is None else gi(-64, 64, (rows, N)) * 2.0 ** -5 if exact else gs((rows, N))
    d["posv"] = None if not c["pos"] else gi(-64, 64, (Tp, N)) * 2.0 ** -5 if exact else gs((Tp, N))
    if load == LOAD_DW:
        Fin, Tin, Fout = c["Fin"], c["Tin"], rm
        # cnt_in: the row's own input frames.  Row 0 of a ragged launch gets the count that CUTS OFF the last frame its final output frame reads
        cin = np.full(B, Tin, np.int32)
        for b in range(B):
            t = int(T[b])
            cin[b] = max(1, min(Tin, 2 * t - 1 if b == 0 else 2 * t))            # frame t - 1 reads 2 t - 3 .. 2 t - 1
        x = gi(-1, 1, (B, Tin, Fin, K)) * 2.0 ** -5 if exact else gs((B, Tin, Fin, K))
        d["dww"] = gi(-2, 2, (9, K)) if exact else gs((9, K), 1.0 / 3.0)
        d["dwb"] = gi(-2, 2, K) * 2.0 ** -5 if exact else gs(K, 0.1)
        dead_in = np.arange(Tin)[None, :] >= cin[:, None]
        d.update(x=np.where(dead_in[:, :, None, None], 0.0, x), xfull=x, cin=cin, img=nan_where(x, dead_in[:, :, None, None]).reshape(-1), ldx=K)
    else:
        if load == LOAD_LN:
            if exact:
                mean, rstd = gi(-32, 32, (rows, 1)) * 2.0 ** -3, rng.choice([0.5, 1.0, 2.0, 4.0], (rows, 1))
                d["lnw"] = rng.choice([0.5, 1.0, 2.0], K) * rng.choice([-1.0, 1.0], K)
                d["lnb"] = gi(-64, 64, K) * 2.0 ** -5
                x = mean + gi(-2, 2, (rows, K)) * 2.0 ** -5
            else:
                x = gs((rows, K)) * 2.0 + gs((rows, 1))
                mean = r32(x.mean(-1, keepdims=True))
                rstd = r32(1.0 / np.sqrt(x.var(-1, keepdims=True) + EPS))
                d["lnw"], d["lnb"] = gs(K, 0.3) + 1.0, gs(K, 0.3)
                d["lnw"] = r32(d["lnw"])
            d["stats"] = np.concatenate([mean, rstd], -1)
        else:
            x = gi(-1, 1, (rows, K)) * 2.0 ** -5 if exact else gs((rows, K))
        ldx = K + (5 if c["pad"] else 0)
        img = np.full((rows - 1) * ldx + K, np.nan)
        img[np.arange(rows)[:, None] * ldx + np.arange(K)[None, :]] = nan_where(x, ~live[:, None])
        d.update(x=x, img=img, ldx=ldx)
    if c["tier"] == "act":                                      # keep |pre-activation| <= ACT_VMAX: w times a power of two (still exact)
        d.update(ldy=N, ldr=N)
        while np.abs(gemm_reference(d)[2]).max() > ACT_VMAX:
            d["w"] = d["w"] / 2.0
    d["ldy"] = N + (3 if c["pad"] else 0)
    d["ldr"] = N + (2 if c["pad"] else 0)
    return d


def gemm_loaded(d, mut=None):
    """(load(X) [rows][K] in float64, its float32 error bound dload)"""
    load, x = d["load"], d["x"]
    if load == LOAD_LN:
        t = (x - d["stats"][:, :1]) * d["stats"][:, 1:] * d["lnw"][None]
        return t + d["lnb"][None], 3 * U * (np.abs(t) + np.abs(d["lnb"][None]))
    if load == LOAD_RELU:
        return np.maximum(x, 0.0), np.zeros(x.shape)
    if load == LOAD_DW:
        B, Tin, Fin, K = x.shape
        Tout, Fout = d["Tp"], d["rowmul"]
        xin = x if mut != "cnt_in" else d["xfull"]
        xp = np.pad(xin, ((0, 0), (1, 2), (1, 2), (0, 0)))
        val, mag = np.zeros((B, Tout, Fout, K)) + d["dwb"], np.zeros((B, Tout, Fout, K)) + np.abs(d["dwb"])
        for i in range(3):
            for j in range(3):
                tap = d["dww"][3 * i + j] if mut not in ("dw_transpose", "dw_mirror") else d["dww"][3 * j + i] if mut == "dw_transpose" else d["dww"][8 - 3 * i - j]
                term = tap[None, None, None] * xp[:, i:i + 2 * Tout:2, j:j + 2 * Fout:2]
                val, mag = val + term, mag + np.abs(term)
        return val.reshape(-1, K), (gam(10) * mag).reshape(-1, K)
    return x, np.zeros(x.shape)


def gemm_reference(d, mut=None):
    """(out [rows][N] float64, zero rows behind the counts; the Gaussian tier's bound; the pre-activation)"""
    xl, dl = gemm_loaded(d, mut)
    xl, dl = np.where(d["live"][:, None], xl, 0.0), np.where(d["live"][:, None], dl, 0.0)
    w, N, Tp, rm = d["w"], d["N"], d["Tp"], d["rowmul"]
    acc = xl @ w.T
    e = gam(d["K"]) * (np.abs(xl) @ np.abs(w).T) + dl @ np.abs(w).T
    bias = d["bias"]
    if bias is not None:
        acc = acc + (np.roll(bias, 1) if mut == "bias_shift" else bias)[None]
        e = e + U * np.abs(acc)
    pre = acc
    act = d["act"] if mut != "act_swap" else {ACT_SILU: ACT_SIGMOID, ACT_SIGMOID: ACT_SILU}.get(d["act"], d["act"])
    v = silu64(acc) if act == ACT_SILU else np.maximum(acc, 0.0) if act == ACT_RELU else sigmoid64(acc) if act == ACT_SIGMOID else acc
    if d["Rv"] is not None:
        ra = d["ra"] if mut != "ra" else 1.0 if d["ra"] != 1.0 else 0.5
        v = np.where(d["live"][:, None], d["Rv"], 0.0) + ra * v
        e = abs(ra) * e + U * np.abs(v)
    if d["posv"] is not None:
        r = np.arange(d["rows"]) % (Tp * rm)
        v = v + d["posv"][(r // rm) if mut != "pos_row" else np.minimum(r, Tp - 1)]
        e = e + U * np.abs(v)
    live = d["live"][:, None]
    return np.where(live, v, 0.0), np.where(live, SAFETY * e, 0.0), np.where(live, pre, 0.0)


def gemm_f32(d, order=None, fused=True):
    """k_sf_gemm's arithmetic in float32 numpy: the load, K slabs of 32 in the given order, bias, activation, R + ra v, pos"""
    load, x = d["load"], d["x"].astype(f32)
    if load == LOAD_LN:
        st = d["stats"].astype(f32)
        t = ((x - st[:, :1]).astype(f32) * st[:, 1:]).astype(f32)
        xl = (t.astype(np.float64) * d["lnw"][None] + d["lnb"][None]).astype(f32) if fused else ((t * d["lnw"].astype(f32)[None]).astype(f32) + d["lnb"].astype(f32)[None]).astype(f32)
    elif load == LOAD_RELU:
        xl = np.maximum(x, f32(0))
    elif load == LOAD_DW:
        B, Tin, Fin, K = x.shape
        Tout, Fout = d["Tp"], d["rowmul"]
        xp = np.pad(x, ((0, 0), (1, 2), (1, 2), (0, 0)))
        val = np.zeros((B, Tout, Fout, K), f32) + d["dwb"].astype(f32)
        for i in range(3):
            for j in range(3):
                term = d["dww"][3 * i + j][None, None, None] * xp[:, i:i + 2 * Tout:2, j:j + 2 * Fout:2].astype(np.float64)
                val = (val.astype(np.float64) + term).astype(f32) if fused else (val + term.astype(f32)).astype(f32)
        xl = val.reshape(-1, K)
    else:
        xl = x
    xl = np.where(d["live"][:, None], xl, f32(0)).astype(f32)
    w, K = d["w"].astype(f32), d["K"]
    acc = np.zeros((d["rows"], d["N"]), f32)
    slabs = range(-(-K // 32))
    for s in (slabs if order is None else order):
        acc = (acc + xl[:, 32 * s:32 * s + 32] @ w[:, 32 * s:32 * s + 32].T).astype(f32)
    if d["bias"] is not None:
        acc = (acc + d["bias"].astype(f32)[None]).astype(f32)
    with np.errstate(over="ignore"):
        if d["act"] == ACT_SILU:
            acc = (acc / (f32(1) + np.exp(-acc).astype(f32)).astype(f32)).astype(f32)
        elif d["act"] == ACT_RELU:
            acc = np.maximum(acc, f32(0))
        elif d["act"] == ACT_SIGMOID:
            acc = (f32(1) / (f32(1) + np.exp(-acc).astype(f32)).astype(f32)).astype(f32)
    if d["Rv"] is not None:
        R = np.where(d["live"][:, None], d["Rv"], 0.0)
        acc = (d["ra"] * acc.astype(np.float64) + R).astype(f32) if fused else ((f32(d["ra"]) * acc).astype(f32) + R.astype(f32)).astype(f32)
    if d["posv"] is not None:
        r = np.arange(d["rows"]) % (d["Tp"] * d["rowmul"])
        acc = (acc + d["posv"][r // d["rowmul"]].astype(f32)).astype(f32)
    return np.where(d["live"][:, None], acc, f32(0)).astype(f32)


# ------------------------------------------------------------------------------------------------ attention
ATTN_CNT = [1, 31, 32, 33, 63, 64, 65, 97]
ATTN_HD_REL, ATTN_HD_PLAIN = [8, 24, 32, 48, 64], [24, 32, 64]
ATTN_TIERS_REL, ATTN_TIERS_PLAIN = ["locator", "distance", "uniform", "gaussian", "tight", "tight_nan"], ["locator", "uniform", "gaussian"]
ATTN_DELTAS = [(3, -5), (-33, 40), (0, -64), (70, -1), (-31, 32), (1, -32)]
ATTN_PAD = 3


def attn_launches():
    """every cnt at Tp = cnt, cnt + 1 and 130; three rows a launch: the count, another of the list (clipped to Tp) and cnt = Tp.  REL and
    plain alternate; the tier, the head size, the number of heads and (REL) qscale in {1, 0.5} cycle so that every head size meets every
    tier (tests/test_sortformer_ops_ref_cpu.py asserts the coverage)."""
    out, n = [], 0
    for rep in range(2):
        for ic, cn in enumerate(ATTN_CNT):
            for it, Tp in enumerate((cn, cn + 1, 130)):
                for rel in (1, 0):
                    tiers, hds = (ATTN_TIERS_REL, ATTN_HD_REL) if rel else (ATTN_TIERS_PLAIN, ATTN_HD_PLAIN)
                    k = 3 * ic + it + 5 * rep
                    tier, hd = tiers[k % len(tiers)], hds[(k // len(tiers) + ic + rep) % len(hds)]
                    cnt = [cn, min(ATTN_CNT[(ic + 3 + it) % len(ATTN_CNT)], Tp), Tp]
                    if tier == "locator" and 2 * ((max(cnt) - 1) // hd) + 2 >= hd:
                        tier = "distance" if rel else "uniform"
                    heads = 1 + (k + rep) % 2
                    qscale, sdk = (0.5 if (k // 6 + k) % 2 == 0 else 1.0, math.sqrt(hd)) if rel else (float(f32(hd) ** f32(-0.5)), 1.0)
                    out.append(dict(tier=tier, rel=rel, hd=hd, heads=heads, cnt=cnt, Tp=Tp, qscale=qscale, sdk=float(f32(sdk)), seed=37000 + n,
                                    deltas=ATTN_DELTAS[n % len(ATTN_DELTAS)]))
                    n += 1
    return out


def _loc_v(B, H, Tp, hd):
    b_, h_, j_, d_ = np.meshgrid(np.arange(B), np.arange(H), np.arange(Tp), np.arange(hd), indexing="ij")
    return ar.locator_v(b_, h_, j_, d_)


def attn_case(c):
    """one launch: q, K, V [B][H][Tp][hd], u, v [H][hd], P [2 Tcap - 1][H][hd] in float64 (float32-representable), the payload rows
    [B Tp][ld] = q | pad | k | v | pad (padding NaN; rows >= cnt NaN, uniform tier: stale keys, zero values), locator targets"""
    H, hd, Tp, cnt, tier, rel = c["heads"], c["hd"], c["Tp"], np.asarray(c["cnt"]), c["tier"], c["rel"]
    B, nmax = len(cnt), int(np.max(np.minimum(c["cnt"], c["Tp"])))
    rng = np.random.default_rng(c["seed"])
    S = (B, H, Tp, hd)
    gi = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)
    Tcap = nmax if tier == "tight" else nmax + 7 if tier == "tight_nan" else max(126, nmax + 3)     # 126: max_seconds 10, as every model test
    u, v, P = np.zeros((H, hd)), np.zeros((H, hd)), np.zeros((2 * Tcap - 1, H, hd))
    tg = deltas = None
    qscale = c["qscale"]
    if tier == "locator":
        K = np.broadcast_to(ar.locator_key(np.arange(Tp), hd)[None, None], S).copy()
        V = _loc_v(B, H, Tp, hd)
        tg = (rng.integers(0, 1 << 30, (B, H, 1)) + 13 * np.arange(Tp)[None, None, :]) % cnt[:, None, None]
        tg[:, :, 0] = cnt[:, None] - 1
        for b in range(B):
            tg[b, :, cnt[b] - 1] = 0
        if rel:
            u = -ar.locator_key((5 + 3 * np.arange(H)) % max(int(cnt.min()), 1), hd)
            v, P = gi(-2, 2, (H, hd)), gi(-1, 1, P.shape)
        q = (ar.locator_key(tg, hd) - u[None, :, None, :]) / (qscale if rel else 1.0)
    elif tier == "uniform":
        K, V, q = gi(-4, 4, S), gi(-8, 8, S), np.zeros(S)
        if rel:
            P = gi(-3, 3, P.shape)
    elif tier in ("distance", "tight", "tight_nan"):
        K, q, V = np.zeros(S), np.zeros(S), _loc_v(B, H, Tp, hd)
        deltas = [(nmax - 1) * (1 if h % 2 == 0 else -1) for h in range(H)] if tier == "tight" else [c["deltas"][h % 2] for h in range(H)]
        P = gi(-3, 3, P.shape)
        dist = np.arange(2 * Tcap - 1) - (Tcap - 1)
        for h in range(H):
            cv = (3 + 5 * h) % hd
            cu = (cv + 1) % hd
            v[h, cv], u[h, cu] = 1.0, 1.0
            P[:, h, cv] = -1024.0 * np.abs(dist - deltas[h])
            P[:, h, cu] = -1024.0 * np.abs(dist + deltas[h] + 1)
        if tier == "tight_nan":
            P[np.abs(dist) >= nmax] = np.nan
    else:
        K, V, q = r32(0.5 * rng.standard_normal(S)), r32(rng.standard_normal(S)), r32(rng.standard_normal(S))
        if rel:
            u, v, P = r32(0.3 * rng.standard_normal((H, hd))), r32(0.3 * rng.standard_normal((H, hd))), r32(0.5 * rng.standard_normal(P.shape))
    dead = (np.arange(Tp)[None, :] >= cnt[:, None])[:, None, :, None]
    Kp, Vp = nan_where(K, dead), nan_where(V, dead)
    if tier == "uniform":
        Kp, Vp = np.where(dead, ar.stale(rng, S), K), np.where(dead, 0.0, V)
    W = H * hd
    koff, voff = W + ATTN_PAD, 2 * W + ATTN_PAD
    ld, ldo, ldp = 3 * W + 2 * ATTN_PAD, W + ATTN_PAD, W + ATTN_PAD
    rows = np.full((B, Tp, ld), np.nan)
    flat = lambda a: a.transpose(0, 2, 1, 3).reshape(B, Tp, W)
    rows[:, :, :W], rows[:, :, koff:koff + W], rows[:, :, voff:voff + W] = flat(nan_where(q, dead)), flat(Kp), flat(Vp)
    Pimg = np.full((2 * Tcap - 1, ldp), np.nan)
    Pimg[:, :W] = P.reshape(2 * Tcap - 1, W)
    return dict(c, B=B, cnt=cnt, Tcap=Tcap, q=q, K=K, V=V, u=u, v=v, P=P, rows=rows.reshape(B * Tp, ld), Pimg=Pimg, ld=ld, ldo=ldo, ldp=ldp, koff=koff,
                voff=voff, targets=tg, dl=deltas, nmax=nmax)


def attn_scores(c, b, h, n, mut=None):
    """float64 scores [n][nk] of one (row, head) and the magnitude sums a_c + a_b [n][nk]; mut: a wrong kernel (CPU sensitivity checks)"""
    hd, Tcap, H = c["hd"], c["Tcap"], c["heads"]
    nk = n + 1 if mut == "key_n" and n < c["Tp"] else n
    qs = c["q"][b, h, :n] * c["qscale"]
    hh = (h + 1) % H if mut in ("head_u", "head_v", "head_P") else h
    u, v = c["u"][hh if mut == "head_u" else h], c["v"][hh if mut == "head_v" else h]
    if mut == "swap_uv":
        u, v = v, u
    if mut == "u_qscale":
        u = u * c["qscale"]
    if mut == "drop_u":
        u = np.zeros_like(u)
    Kb = np.nan_to_num(c["K"][b, h, :nk])
    s = (qs + u) @ Kb.T
    a = np.abs(qs + u) @ np.abs(Kb).T
    if c["rel"]:
        i, j = np.arange(n)[:, None], np.arange(nk)[None, :]
        dd = (j - i) if mut == "sign" else (i - j)
        idx = dd + (Tcap if mut == "tcap" else Tcap - 1) + (1 if mut == "band+1" else -1 if mut == "band-1" else 0)
        ok = (idx >= 0) & (idx < 2 * Tcap - 1)
        Pg = np.where(ok[:, :, None], c["P"][np.clip(idx, 0, 2 * Tcap - 2), hh if mut == "head_P" else h], 0.0)     # [n][nk][hd]
        s = s + np.einsum("ic,ijc->ij", qs + v, Pg)
        a = a + np.einsum("ic,ijc->ij", np.abs(qs + v), np.abs(Pg))
    return s / c["sdk"], a / c["sdk"], nk


def attn_reference(c, mut=None):
    """float64: (out [B Tp][H hd], zero rows behind cnt; the Gaussian tier's bound)"""
    B, H, Tp, hd = c["B"], c["heads"], c["Tp"], c["hd"]
    out, bound = np.zeros((B, Tp, H, hd)), np.zeros((B, Tp, H, hd))
    for b in range(B):
        n = int(min(c["cnt"][b], Tp))
        for h in range(H):
            s, a, nk = attn_scores(c, b, h, n, mut)
            Vb = np.nan_to_num(c["V"][b, h, :nk])
            Mx = s.max(-1, keepdims=True)
            p = np.exp(s - Mx)
            p /= p.sum(-1, keepdims=True)
            o, mag = p @ Vb, p @ np.abs(Vb)
            X, F = np.abs(s - Mx).max(-1), -(-n // 32) + 1
            E = (2 * gam(hd) * a.max(-1) + 3 * U * np.abs(s).max(-1) + 2 * X * U + 2 * F * U + 3 * gam(n + F) + 4 * U)[:, None]
            out[b, :n, h], bound[b, :n, h] = o, 2 * SAFETY * E * mag + U * np.abs(o)
    return out.reshape(B * Tp, H * hd), bound.reshape(B * Tp, H * hd)


def attn_exact_expected(c):
    """the exact tiers' stated outputs [B Tp][H hd], zero rows behind cnt"""
    B, H, Tp, hd = c["B"], c["heads"], c["Tp"], c["hd"]
    out = np.zeros((B, Tp, H, hd))
    for b in range(B):
        n = int(min(c["cnt"][b], Tp))
        for h in range(H):
            if c["tier"] == "locator":
                out[b, :n, h] = c["V"][b, h][c["targets"][b, h, :n]]
            elif c["tier"] == "uniform":
                out[b, :n, h] = (c["V"][b, h, :n].sum(0).astype(f32) / f32(n)).astype(np.float64)[None]
            else:
                out[b, :n, h] = c["V"][b, h][np.clip(np.arange(n) - c["dl"][h], 0, n - 1)]
    return out.reshape(B * Tp, H * hd)


def attn_f32(c, shuffle=None):
    """k_sf_attn's arithmetic in float32 numpy: q qscale staged, keys >= n staged as zero, 32-key tiles in order, the band read by distance
    (table rows outside 0 .. 2 Tcap - 2 zero), the select, the online softmax in float32.  shuffle: a permutation seed for the order of
    the head columns in both products (the exact tiers must not depend on it)"""
    B, H, Tp, hd, Tcap = c["B"], c["heads"], c["Tp"], c["hd"], c["Tcap"]
    out = np.zeros((B, Tp, H, hd), f32)
    qsc, sdk = f32(c["qscale"]), f32(c["sdk"])
    perm = np.arange(hd) if shuffle is None else np.random.default_rng(shuffle).permutation(hd)
    dot = lambda A, Bm: sum(((A[:, perm[g:g + 8]] @ Bm[:, perm[g:g + 8]].T).astype(f32) for g in range(0, hd, 8)), np.zeros((A.shape[0], Bm.shape[0]), f32)).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            n = int(min(c["cnt"][b], Tp))
            nt = -(-n // 32)
            for h in range(H):
                q = (c["q"][b, h, :n].astype(f32) * qsc).astype(f32)
                K, V = np.zeros((32 * nt, hd), f32), np.zeros((32 * nt, hd), f32)
                K[:n], V[:n] = c["K"][b, h, :n], c["V"][b, h, :n]
                qu, qv = (q + c["u"][h].astype(f32)).astype(f32), (q + c["v"][h].astype(f32)).astype(f32)
                m, l, O = np.full(n, -np.inf, f32), np.zeros(n, f32), np.zeros((n, hd), f32)
                for t in range(nt):
                    s = dot(qu, K[32 * t:32 * t + 32])
                    j = np.arange(32 * t, 32 * t + 32)
                    if c["rel"]:
                        idx = np.arange(n)[:, None] - j[None, :] + Tcap - 1
                        ok = (idx >= 0) & (idx < 2 * Tcap - 1)
                        Pg = np.where(ok[:, :, None], c["P"][np.clip(idx, 0, 2 * Tcap - 2), h], 0.0).astype(f32)
                        band = sum((np.einsum("ic,ijc->ij", qv[:, perm[g:g + 8]], Pg[:, :, perm[g:g + 8]]).astype(f32) for g in range(0, hd, 8)), np.zeros((n, 32), f32))
                        s = (s + np.where(j[None] < n, band.astype(f32), f32(0))).astype(f32)      # a dead key's entry is discarded by the select
                    s = np.where(j[None] < n, (s / sdk).astype(f32), f32(-np.inf)).astype(f32)
                    mn = np.maximum(m, s.max(-1))
                    alpha = np.exp(m - mn).astype(f32)
                    pe = np.exp(s - mn[:, None]).astype(f32)
                    l = (l * alpha + pe.sum(-1, dtype=f32)).astype(f32)
                    O = ((O * alpha[:, None]).astype(f32) + (pe @ V[32 * t:32 * t + 32]).astype(f32)).astype(f32)
                    m = mn
                out[b, :n, h] = (O / l[:, None]).astype(f32)
    return out.reshape(B * Tp, H * hd)


# ------------------------------------------------------------------------------------------------ GLU + depthwise conv
DW_K, DW_C, DW_CNT = [3, 5, 9, 31], [8, 64, 72, 136], [1, 2, 63, 64, 65, 129]
GATE_ONE, GATE_ZERO = 32.0, -128.0


def dw_launches():
    """every k with every C in the exact tier, every k in the impulse and the Gaussian tier; the counts (three rows a launch) and Tp in
    {largest count, 130} cycle"""
    out, n = [], 0
    for ik, k in enumerate(DW_K):
        for ic, Cc in enumerate(DW_C):
            for tier in ["exact"] + (["impulse", "gauss"] if (ik + ic) % 2 == 0 else []):
                cnt = [DW_CNT[(n + 2 * j) % 6] for j in range(3)]
                out.append(dict(tier=tier, k=k, C=Cc, cnt=cnt, Tp=max(cnt) if n % 2 else 130, seed=38000 + n))
                n += 1
    return out


def dw_case(c):
    """a, gate [B][Tp][C], taps [k][C], shift [C] in float64 and the payload rows pw [B Tp][2 C] (frames >= cnt: NaN)"""
    k, Cc, Tp, cnt = c["k"], c["C"], c["Tp"], np.asarray(c["cnt"])
    B = len(cnt)
    rng = np.random.default_rng(c["seed"])
    live = np.arange(Tp)[None, :] < cnt[:, None]
    S = (B, Tp, Cc)
    if c["tier"] == "gauss":
        a, gate = r32(rng.standard_normal(S)), r32(2.0 * rng.standard_normal(S))
        taps, shift = r32(rng.standard_normal((k, Cc)) / math.sqrt(k)), r32(0.1 * rng.standard_normal(Cc))
    elif c["tier"] == "exact":
        a = rng.integers(-4, 5, S).astype(np.float64)
        gate = np.where(rng.integers(0, 4, S) > 0, GATE_ONE, GATE_ZERO)
        taps = rng.integers(-2, 3, (k, Cc)).astype(np.float64)
        taps[np.arange(k), (7 * np.arange(k)) % Cc] = 1.0 + np.arange(k) % 2                # no tap is zero everywhere
        shift = 1024.0 + rng.integers(-16, 17, Cc).astype(np.float64)
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
    dead = np.broadcast_to(~live[:, :, None], S)
    pw = np.concatenate([nan_where(a, dead), nan_where(gate, dead)], -1).reshape(B * Tp, 2 * Cc)
    return dict(c, B=B, cnt=cnt, live=live, a=a, gate=gate, taps=taps, shift=shift, pw=pw)


def dw_reference(d, mut=None):
    """(out [B Tp][C] float64, zero rows behind cnt; bound (gauss) or the relative margin's absolute value (impulse) or None (exact))"""
    k, Tp, live = d["k"], d["Tp"], d["live"][:, :, None]
    a, gate = (d["gate"], d["a"]) if mut == "halves" else (d["a"], d["gate"])
    if d["tier"] == "gauss" or mut == "halves":
        g = a * sigmoid64(gate)
    else:
        g = np.where(gate == GATE_ONE, a, 0.0)
    g = np.where(live, g, 0.0)
    padl = (k - 1) // 2 + (1 if mut == "padl" else 0)
    gp = np.pad(g, ((0, 0), (padl, k + 1 - padl), (0, 0)))
    y, mag, dg = np.zeros(g.shape) + d["shift"], np.zeros(g.shape) + np.abs(d["shift"]), np.zeros(g.shape)
    for kk in range(k):
        w = d["taps"][kk if mut != "mirror" else k - 1 - kk][None, None, :]
        term = w * gp[:, kk:kk + Tp]
        y, mag, dg = y + term, mag + np.abs(term), dg + 5 * U * np.abs(term)
    if d["tier"] == "exact":
        out, bound = np.where((y >= 512.0) & (y <= 1536.0), y, silu64(y)), None
    else:
        out = silu64(y)
        dy = gam(k + 1) * mag + dg if d["tier"] == "gauss" else 0.0
        bound = SAFETY * (1.1 * dy + 4 * U * np.abs(out))
        bound = np.where(live, bound, 0.0).reshape(-1, d["C"])
    return np.where(live, out, 0.0).reshape(-1, d["C"]), bound


def dw_f32(d, reverse=False, fused=True):
    """k_sf_glu_dwconv's arithmetic in float32 numpy; reverse: the taps accumulated in descending order"""
    k, Tp, live = d["k"], d["Tp"], d["live"][:, :, None]
    with np.errstate(over="ignore", invalid="ignore"):
        a, gate = np.where(live, d["a"], 0.0).astype(f32), np.where(live, d["gate"], 0.0).astype(f32)
        sg = (f32(1) / (f32(1) + np.exp(-gate).astype(f32)).astype(f32)).astype(f32)
        g = np.where(live, (a * sg).astype(f32), f32(0)).astype(f32)
        padl = (k - 1) // 2
        gp = np.pad(g, ((0, 0), (padl, k - 1 - padl), (0, 0)))
        y = np.zeros(g.shape, f32) + d["shift"].astype(f32)
        for kk in (range(k - 1, -1, -1) if reverse else range(k)):
            term = d["taps"][kk][None, None, :] * gp[:, kk:kk + Tp].astype(np.float64)
            y = (y.astype(np.float64) + term).astype(f32) if fused else (y + term.astype(f32)).astype(f32)
        out = (y / (f32(1) + np.exp(-y).astype(f32)).astype(f32)).astype(f32)
    return np.where(live, out, f32(0)).reshape(-1, d["C"]).astype(f32)


# ------------------------------------------------------------------------------------------------ conv0
CONV0_CASES = [dict(mels=20, C=24, Fp=9, F=[5, 6, 9], seed=39000), dict(mels=32, C=5, Fp=12, F=[12, 1, 7], seed=39001),
               dict(mels=20, C=8, Fp=7, F=[7, 9, 2], seed=39002)]            # F 5, 7: the last output frame's last input frame is cut off; F 9 > Fp: the clamp


def conv0_case(c):
    rng = np.random.default_rng(c["seed"])
    mels, Cc, Fp, F = c["mels"], c["C"], c["Fp"], np.asarray(c["F"], np.int32)
    B, T1p, F1 = len(F), half(Fp), half(mels)
    T1 = np.array([half(min(int(f), Fp)) for f in F], np.int32)
    x = rng.integers(-2, 3, (B, Fp, mels)).astype(np.float64) * 2.0 ** -3
    dead = np.arange(Fp)[None, :] >= F[:, None]
    return dict(c, B=B, T1p=T1p, F1=F1, T1=T1, Fv=F, x=np.where(dead[:, :, None], 0.0, x), img=nan_where(x, dead[:, :, None]),
                w=rng.integers(-2, 3, (9, Cc)).astype(np.float64), bias=rng.integers(-3, 4, Cc).astype(np.float64) * 2.0 ** -2)


def conv0_reference(d, mut=None):
    B, T1p, F1, Cc = d["B"], d["T1p"], d["F1"], d["C"]
    xp = np.pad(d["x"], ((0, 0), (1, 2), (1, 2)))
    out = np.zeros((B, T1p, F1, Cc)) + d["bias"]
    for i in range(3):
        for j in range(3):
            tap = d["w"][3 * j + i] if mut == "transpose" else d["w"][3 * i + j]
            out = out + tap[None, None, None] * xp[:, i:i + 2 * T1p:2, j:j + 2 * F1:2][..., None]
    out = np.maximum(out, 0.0)
    return np.where((np.arange(T1p)[None, :] < d["T1"][:, None])[:, :, None, None], out, 0.0)


# ------------------------------------------------------------------------------------------------ stats, LayerNorm, intake, peak
LN_D, LN_M = [8, 48, 64, 65, 128], [5, 7]


def ln_counts(M, seed):
    """Tp = 3, counts in 0 .. 3 (cnt > row count never masks), a masked and a live row"""
    cnt = np.random.default_rng(seed).integers(0, 4, -(-M // 3)).astype(np.int32)
    cnt[0] = 2
    return cnt, 3


def ln_live(M, cnt, Tp):
    m = np.arange(M)
    return (m % Tp) < np.asarray(cnt)[m // Tp]


def ln_rows(tier, M, d, seed):
    """(x, w, b) of enc_ref's tiers in float64, float32-representable; balanced needs an even d (d 65: the constant and Gaussian tiers)"""
    if tier == "constant":
        return er.ln_constant(M, d, seed)
    if tier == "balanced":
        x, w, b, _ = er.ln_balanced(M, d, seed)
        return x, w, b
    x, w, b = er.ln_gauss(M, d, seed)
    return x, w, b


def stats_reference(x, eps=EPS):
    """(mean, rstd, bound of the mean, relative bound of rstd) in float64"""
    d = x.shape[-1]
    mean = x.mean(-1)
    sigma = np.sqrt(((x - mean[:, None]) ** 2).mean(-1) + eps)
    A = np.abs(x).mean(-1)
    return mean, 1.0 / sigma, SAFETY * (d + 1) * U * A, SAFETY * ((d + 4) / 2.0 + (d + 1) * A / sigma + 2.0) * U


def ln_reference(x, w, b, eps=EPS):
    """(y, bound) in float64: enc_ref.ln_reference's derivation with the float32 store (u |y|) in place of the bf16 rounding"""
    d = x.shape[-1]
    mean = x.mean(-1, keepdims=True)
    sigma = np.sqrt(((x - mean) ** 2).mean(-1, keepdims=True) + eps)
    y = (x - mean) / sigma * w + b
    A, n = np.abs(x).mean(-1, keepdims=True), np.abs((x - mean) / sigma * w)
    return y, SAFETY * U * ((d + 1) * A / sigma * np.abs(w) + ((d + 4) / 2.0 + (d + 1) * A / sigma + 6.0) * n + np.abs(y))


def stats_f32(x, eps=EPS, reverse=False):
    """wave_mean_rstd in float32 numpy: two passes; reverse: the other summation order"""
    x = x.astype(f32)[:, ::-1] if reverse else x.astype(f32)
    dd = f32(x.shape[-1])
    mean = (np.cumsum(x, -1, dtype=f32)[:, -1] / dd).astype(f32)
    t = (x - mean[:, None]).astype(f32)
    var = (np.cumsum((t * t).astype(f32), -1, dtype=f32)[:, -1] / dd).astype(f32)
    return mean, (f32(1) / np.sqrt((var + f32(eps)).astype(f32))).astype(f32)


def ln_f32(x, w, b, eps=EPS, reverse=False, fused=True):
    mean, rstd = stats_f32(x, eps, reverse)
    r = ((x.astype(f32) - mean[:, None]).astype(f32) * rstd[:, None]).astype(f32)
    if fused:
        return (r.astype(np.float64) * w + b).astype(f32)
    return ((r * w.astype(f32)).astype(f32) + b.astype(f32)).astype(f32)


def balanced_expected(x, w, eps=EPS):
    """the balanced tier in float32: mean 0, var a^2, y = (x rstd) w, one rounding (w a power of two)"""
    a = np.abs(x[:, 0]).astype(f32)
    rstd = (f32(1) / np.sqrt((a * a + f32(eps)).astype(f32))).astype(f32)
    return np.zeros(len(a), f32), rstd, ((x.astype(f32) * rstd[:, None]).astype(f32) * w.astype(f32)[None]).astype(f32)


PEAK_N = [0, 1, 255, 256, 257]


def peak_case(seed):
    """rows of PEAK_N samples at stride 300, NaN behind n; the maximum sits at the row's last sample (n >= 1) with a negative sign on odd rows"""
    rng = np.random.default_rng(seed)
    x = r32(0.3 * rng.standard_normal((len(PEAK_N), 300)))
    for b, n in enumerate(PEAK_N):
        if n:
            x[b, n - 1] = (2.5 + b) * (-1.0 if b % 2 else 1.0)
        x[b, n:] = np.nan
    return x, np.asarray(PEAK_N, np.int32)


def peak_reference(x, N, on):
    m = np.array([np.abs(x[b, :n]).max(initial=0.0) for b, n in enumerate(N)]).astype(f32)
    return (f32(1) / (m + f32(1e-3)).astype(f32)).astype(f32) if on else np.ones(len(N), f32)


# ------------------------------------------------------------------------------------------------ the operators on values (the model chain)
def op_gemm(x, w, bias=None, act=ACT_NONE, R=None, ra=1.0, pos=None):
    v = x @ w.T + (0.0 if bias is None else bias)
    v = silu64(v) if act == ACT_SILU else np.maximum(v, 0.0) if act == ACT_RELU else sigmoid64(v) if act == ACT_SIGMOID else v
    v = v if R is None else R + ra * v
    return v if pos is None else v + pos[:v.shape[0]]


def op_stats_ln(x, eps=EPS):
    mean = x.mean(-1, keepdims=True)
    return mean, 1.0 / np.sqrt(((x - mean) ** 2).mean(-1, keepdims=True) + eps)


def op_ln(x, w, b, eps=EPS):
    mean, rstd = op_stats_ln(x, eps)
    return (x - mean) * rstd * w + b


def op_conv0(x, w9, bias):
    """x [F][mels] -> [T1][F1][C]"""
    d = dict(B=1, T1p=half(x.shape[0]), F1=half(x.shape[1]), C=w9.shape[1], x=x[None], w=w9, bias=bias, T1=np.array([half(x.shape[0])]))
    return conv0_reference(d)[0]


def op_dw_load(x, dww, dwb):
    """x [Tin][Fin][C] -> rows [Tout Fout][C]"""
    Tin, Fin, K = x.shape
    d = dict(load=LOAD_DW, x=x[None], Tp=half(Tin), rowmul=half(Fin), dww=dww, dwb=dwb)
    return gemm_loaded(d)[0]


def op_attn(qkv, H, hd, qscale, sdk, u=None, v=None, P=None, Tcap=0):
    """one row of the batch: qkv [n][3 H hd] -> [n][H hd]; P [2 Tcap - 1][H hd]"""
    n = qkv.shape[0]
    sp = lambda a: a.reshape(n, H, hd).transpose(1, 0, 2)[None]
    rel = P is not None
    c = dict(B=1, heads=H, hd=hd, Tp=n, cnt=np.array([n]), qscale=qscale, sdk=sdk, rel=rel, Tcap=Tcap, q=sp(qkv[:, :H * hd]), K=sp(qkv[:, H * hd:2 * H * hd]),
             V=sp(qkv[:, 2 * H * hd:]), u=u if rel else np.zeros((H, hd)), v=v if rel else np.zeros((H, hd)), P=P.reshape(-1, H, hd) if rel else None)
    return attn_reference(c)[0]


def op_glu_dwconv(pw, taps, shift, k):
    """one row of the batch: pw [n][2 C] -> [n][C]"""
    n, C2 = pw.shape
    d = dict(tier="gauss", k=k, Tp=n, C=C2 // 2, live=np.ones((1, n), bool), a=pw[None, :, :C2 // 2], gate=pw[None, :, C2 // 2:], taps=taps, shift=shift)
    return dw_reference(d)[0]


# ------------------------------------------------------------------------------------------------ the entry points
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _L():
    from mlx_audio_swift_amd import _lib as L
    return L.lib()


def _f(a):
    return None if a is None else np.ascontiguousarray(a, f32)


def _i(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def poison(shape):
    return np.full(shape, POISON, np.uint32).view(f32)


def run_gemm(d, only=None, **over):
    """mis_debug_sortformer_gemm -> (status, Y float32 [rows][N], R as the launch left it [rows][N] or None, report).  only: that batch entry alone"""
    g = dict(d, **over)
    B, rows, N, K, nr = g["B"], g["rows"], g["N"], g["K"], g["Tp"] * g["rowmul"]
    img, cnt, cin, R, stats = g["img"], g["cntv"], g.get("cin"), g["Rv"], g.get("stats")
    if R is not None:
        R = nan_where(R, ~g["live"][:, None])
    if stats is not None:
        stats = nan_where(stats, ~g["live"][:, None])
    if only is not None:
        b = only
        sl = slice(b * nr, (b + 1) * nr)
        if g["load"] == LOAD_DW:
            per = g["Tin"] * g["Fin"] * K
            img = img[b * per:(b + 1) * per]
        else:
            img = img[b * nr * g["ldx"]:][:(nr - 1) * g["ldx"] + K]
        cnt, cin = None if cnt is None else cnt[b:b + 1], None if cin is None else cin[b:b + 1]
        R, stats = None if R is None else R[sl], None if stats is None else stats[sl]
        B, rows = 1, nr
    sep = R is not None and g["R"] == "sep"
    ldr = g["ldr"] if sep else N
    Rimg = None
    if sep:
        Rimg = np.full((rows - 1) * ldr + N, np.nan)
        Rimg[np.arange(rows)[:, None] * ldr + np.arange(N)[None, :]] = R
    Y, rep = poison((rows, N)), np.full(1, -7, np.int32)
    Ra = poison((rows - 1) * ldr + N) if sep else None
    a = [_f(img), _f(g["w"]), _f(g["bias"]), _i(cnt), _f(stats), _f(g.get("lnw")), _f(g.get("lnb")), _f(Rimg if sep else R), _f(g["posv"]), _i(cin),
         _f(g.get("dww")), _f(g.get("dwb"))]
    st = _L().mis_debug_sortformer_gemm(0, g["load"], g["act"], _ptr(a[0]), g["ldx"], _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), B, g["Tp"], g["rowmul"], K, N, g["ldy"],
                                        _ptr(a[4]), _ptr(a[5]), _ptr(a[6]), _ptr(a[7]), ldr, g["ra"], int(R is not None and not sep), _ptr(a[8]), _ptr(a[9]),
                                        g.get("Tin", 0), g.get("Fin", 0), g["rowmul"] if g["load"] == LOAD_DW else 0, _ptr(a[10]), _ptr(a[11]), _ptr(Y),
                                        _ptr(Ra), _ptr(rep))
    if sep:
        Ra = Ra[np.arange(rows)[:, None] * ldr + np.arange(N)[None, :]]
    return st, Y, Ra, int(rep[0])


def run_attn(c, only=None, **over):
    """mis_debug_sortformer_attn -> (status, out float32 [B Tp][H hd], report)"""
    g = dict(c, **over)
    B, Tp, W = g["B"], g["Tp"], g["heads"] * g["hd"]
    rows, cnt = g["rows"], _i(g["cnt"])
    if only is not None:
        rows, cnt, B = rows[only * Tp:(only + 1) * Tp], cnt[only:only + 1], 1
    out, rep = poison((B * Tp, W)), np.full(2, -7, np.int32)
    rel = g["rel"]
    a = [_f(rows), _f(g["u"]) if rel else None, _f(g["v"]) if rel else None, _f(g["Pimg"]) if rel else None]
    st = _L().mis_debug_sortformer_attn(0, rel, _ptr(a[0]), g["ld"], g["koff"], g["voff"], _ptr(cnt), B, Tp, g["heads"], g["hd"], g["qscale"], g["sdk"], _ptr(a[1]),
                                        _ptr(a[2]), _ptr(a[3]), g["ldp"], g["Tcap"], g["ldo"], _ptr(out), _ptr(rep))
    return st, out, (int(rep[0]), int(rep[1]))


def run_glu_dwconv(d, only=None, k=None):
    B, Tp, Cc = d["B"], d["Tp"], d["C"]
    pw, cnt = d["pw"], _i(d["cnt"])
    if only is not None:
        pw, cnt, B = pw[only * Tp:(only + 1) * Tp], cnt[only:only + 1], 1
    out = poison((B * Tp, Cc))
    a = [_f(pw), _f(d["taps"]), _f(d["shift"])]
    st = _L().mis_debug_sortformer_glu_dwconv(0, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(cnt), B, Tp, Cc, d["k"] if k is None else k, _ptr(out))
    return st, out


def run_conv0(d):
    out = poison((d["B"], d["T1p"], d["F1"], d["C"]))
    a = [_f(d["img"]), _i(d["Fv"]), _i(d["T1"]), _f(d["w"]), _f(d["bias"])]
    st = _L().mis_debug_sortformer_conv0(0, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), _ptr(a[4]), d["B"], d["Fp"], d["mels"], d["T1p"], d["F1"], d["C"], _ptr(out))
    return st, out


def run_stats(x, eps=EPS):
    x = _f(x)
    out = poison((x.shape[0], 2))
    st = _L().mis_debug_sortformer_stats(0, _ptr(x), x.shape[0], x.shape[1], eps, _ptr(out))
    return st, out


def run_ln(x, w, b, cnt, Tp, in_place, eps=EPS):
    x, w, b, cnt = _f(x), _f(w), _f(b), _i(cnt)
    out = poison(x.shape)
    st = _L().mis_debug_sortformer_ln(0, _ptr(x), _ptr(w), _ptr(b), x.shape[0], x.shape[1], eps, _ptr(cnt), Tp, int(in_place), _ptr(out))
    return st, out


def run_intake(x, cnt, Tp, g):
    x, cnt = _f(x), _i(cnt)
    out = poison(x.shape)
    st = _L().mis_debug_sortformer_intake(0, _ptr(x), _ptr(cnt), len(cnt), Tp, x.shape[1], g, _ptr(out))
    return st, out


def run_peak(x, N, on):
    x, N = _f(x), _i(N)
    out = poison(len(N))
    st = _L().mis_debug_sortformer_peak(0, _ptr(x), x.shape[1], _ptr(N), len(N), int(on), _ptr(out))
    return st, out
