"""Operator-level reference of the LM GEMM kernels (csrc/lm_kernels.hip k_gemm_skinny, csrc/lm_qgemm.hip k_gemm_skinny_q / _q1,
csrc/lm_prefill.hip k_gemm_pf), inputs that make the reference EXACT, the case lists of tests/test_gpu_gemm_ops.py, and thin wrappers of
the mis_debug_gemm_* entry points (include/mi_speech_debug.h).

Written from the specification in the kernel headers: y[m][n] = sum_k x[m][k] w[n][k] (quantised: w = scale * code + bias per group of
64), float32 accumulation, split-K slab s covering k-tiles [KT s / S, KT (s + 1) / S) with the output bias on slab 0, and the rounding
points T() = round-to-bf16 written in gemm_epilogue / qgemm_epilogue.  Packing is the library's business and is not mirrored here.

Why the comparison can be bit-exact: bf16 x bf16 products are exact in float32, and with the generators below every partial sum is an
integer multiple of one power of two and stays below 2^24 of those units - so every float32 summation order gives the same bits
(tests/test_gemm_ref_cpu.py proves it by permuting and regrouping k)."""
import ctypes as C
import math

import numpy as np
import torch

EPI_PARTIAL, EPI_BF16, EPI_SILU_MUL, EPI_GELU_PACKED, EPI_SILU_PACKED = range(5)
PF_F32, PF_RESID, PF_SILU = range(3)
MIS_F16, MIS_BF16 = 1, 2
K_DENSE, K_QSTREAM, K_QONESHOT, K_PF = range(4)          # report[0] of the entry points
NONLINEAR = (EPI_SILU_MUL, EPI_GELU_PACKED, EPI_SILU_PACKED)


# ------------------------------------------------------------------------------------------------ number formats
def bf16_bits(a):
    """float32 -> bf16 payload, round to nearest even"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def exact_bits(a, sb_dtype=MIS_BF16):
    """16-bit payload of values that MUST be representable (generators only produce such)"""
    a = np.asarray(a, np.float64)
    if sb_dtype == MIS_F16:
        h = a.astype(np.float16)
        assert np.array_equal(h.astype(np.float64), a), "value not exact in f16"
        return np.ascontiguousarray(h).view(np.uint16)
    b = bf16_bits(a.astype(np.float32))
    assert np.array_equal(bf16_value(b).astype(np.float64), a), "value not exact in bf16"
    return b


def _T64(v):
    """float64 -> nearest bf16 value (ONE rounding, ties to even), kept in float64"""
    _, e = torch.frexp(v)
    q = torch.ldexp(torch.ones_like(v), torch.clamp(e, min=-125) - 8)
    return torch.round(v / q) * q


def _T32(v):
    return v.to(torch.bfloat16).to(torch.float32)


def T(v):
    return _T64(torch.as_tensor(np.asarray(v, np.float64))).numpy()


def bf16_ulp_distance(a, b):
    """distance in bf16 steps between two arrays of bf16-representable values"""
    def order(v):
        bits = bf16_bits(np.asarray(v, np.float32)).astype(np.int64)
        return np.where(bits & 0x8000, -(bits & 0x7FFF), bits & 0x7FFF)
    return np.abs(order(a) - order(b))


# ------------------------------------------------------------------------------------------------ exact inputs
def _tiles_all_count(x, w):
    """every 32-wide k-tile's contribution to y is non-zero and no two tiles contribute the same: dropping, doubling or swapping one shows"""
    M, K = x.shape
    c = np.einsum("mtk,ntk->tmn", x.reshape(M, K // 32, 32), w.reshape(w.shape[0], K // 32, 32)).reshape(K // 32, -1)
    return bool(np.all(np.any(c != 0, axis=1))) and len({r.tobytes() for r in c}) == K // 32


def dense_inputs(M, N, K, seed, x_log2=-5):
    """x in {-1, 0, 1} * 2^x_log2 [M][K], w integers in [-4, 4] [N][K]; one column per k-tile is forced non-zero with a kt-dependent value"""
    rng = np.random.default_rng(seed)
    kt = np.arange(K // 32)
    col = kt * 32 + (5 * kt + 3) % 32
    for _ in range(16):
        x = rng.integers(-1, 2, (M, K)).astype(np.float64)
        w = rng.integers(-4, 5, (N, K)).astype(np.float64)
        x[:, col] = np.where((np.arange(M)[:, None] + kt[None, :]) % 2 == 0, 1.0, -1.0)
        w[:, col] = 1.0 + (np.arange(N)[:, None] + kt[None, :]) % 4
        if _tiles_all_count(x, w):
            return x * 2.0 ** x_log2, w
    raise AssertionError("no input without an inert k-tile found")


def pack_codes(q, bits):
    N, K = q.shape
    epw = 32 // bits
    sh = (np.arange(epw, dtype=np.uint64) * bits)[None, None, :]
    return (q.reshape(N, K // epw, epw).astype(np.uint64) << sh).sum(-1).astype(np.uint32)


def quant_inputs(M, N, K, bits, seed, x_log2=-5):
    """MLX layout: codes uniform in [0, 2^bits), scales in {2^-4, 2^-5} and biases = -scale * m (integer m in [0, 2^bits)) per (row, group of 64).
    Returns x [M][K], codes q [N][K], scales / biases [N][K/64] and the dequantised w = s q + b [N][K] (all float64, all exact in bf16 / f16)."""
    rng = np.random.default_rng(seed)
    G = K // 64
    for _ in range(16):
        x = rng.integers(-1, 2, (M, K)).astype(np.float64)
        q = rng.integers(0, 2 ** bits, (N, K))
        sc = 2.0 ** rng.integers(-5, -3, (N, G))
        m = rng.integers(0, 2 ** bits, (N, G)).astype(np.float64)
        bi = -sc * m
        w = np.repeat(sc, 64, axis=1) * q + np.repeat(bi, 64, axis=1)
        if _tiles_all_count(x, w):
            return x * 2.0 ** x_log2, q, sc, bi, w
    raise AssertionError("no input without an inert k-tile found")


def out_bias(ncols, seed, lo=-3):
    return np.random.default_rng(seed + 77).integers(lo, 4, ncols).astype(np.float64)


def gelu_safe_shift(x, wi):
    """GELU inputs: 0.5 h (1 + erf(h / sqrt 2)) cancels in float32 for h < -4 (1 + erf -> 1e-5: the relative error of ANY float32 evaluation
    passes a bf16 ulp there), so a comparison in ulps says nothing below that point.  Returns how many times to halve x so that every
    pre-activation is >= -4 (GELU cases also take their output bias from [0, 3])."""
    lo, j = float((x @ wi.T).min()), 0
    while lo * 2.0 ** -j < -4.0:
        j += 1
    return j


def interleave(w, w2):
    """rows of w and w2 alternating in tiles of 16: the gate / up layout (tile 2t from w, 2t + 1 from w2)"""
    N, K = w.shape
    return np.stack([w.reshape(N // 16, 16, K), w2.reshape(N // 16, 16, K)], axis=1).reshape(2 * N, K)


def x_log2_for_std(K, w_rms, target=2.0):
    """power-of-two x amplitude that puts the pre-activations' standard deviation at `target` within a factor sqrt(2) (x is non-zero 2 / 3 of the time)"""
    return int(round(math.log2(target / (math.sqrt(2.0 * K / 3.0) * w_rms))))


DENSE_W_RMS = math.sqrt(60.0 / 9.0)


def quant_w_rms(bits):
    return math.sqrt((2.0 ** -8 + 2.0 ** -10) / 2.0 * 2.0 * (4.0 ** bits - 1.0) / 12.0)


# ------------------------------------------------------------------------------------------------ reference
def k_slices(units, S):
    return [(units * s // S, units * (s + 1) // S) for s in range(S)]


def ref_slabs(x, w, S, unit, bias=None):
    """float64 [S][M][N]: slab s = x . w^T over k-units [units s / S, units (s + 1) / S) (unit = 32: k-tiles, 64: scale groups); bias on slab 0"""
    out = np.zeros((S, x.shape[0], w.shape[0]))
    for s, (a, b) in enumerate(k_slices(x.shape[1] // unit, S)):
        out[s] = x[:, a * unit:b * unit] @ w[:, a * unit:b * unit].T
    if bias is not None:
        out[0] += bias[None, :]
    return out


def apply_epilogue(epi, acc, bias=None, prec=64):
    """the rounding points of gemm_epilogue / qgemm_epilogue on exact pre-activations acc [M][cols]; prec 64: float64 between roundings (the
    reference), 32: a float32 realisation of the same specification (what tests/test_gemm_ref_cpu.py holds the inputs to)"""
    dt, Tr = (torch.float64, _T64) if prec == 64 else (torch.float32, _T32)
    a = torch.as_tensor(np.asarray(acc, np.float64)).to(dt)
    if bias is not None and epi != EPI_SILU_MUL:
        a = a + torch.as_tensor(np.asarray(bias, np.float64)).to(dt)[None, :]
    sig = lambda v: 1.0 / (1.0 + torch.exp(-v))
    if epi == EPI_BF16:
        r = Tr(a)
    elif epi == EPI_GELU_PACKED:
        h = Tr(a)
        r = Tr(0.5 * h * (1.0 + torch.erf(h * 0.70710678118654752)))
    elif epi == EPI_SILU_PACKED:
        h = Tr(a)
        r = Tr(h * Tr(sig(h)))
    elif epi == EPI_SILU_MUL:
        M, cols = a.shape
        t = a.reshape(M, cols // 32, 2, 16)
        g, u = Tr(t[:, :, 0]), Tr(t[:, :, 1])
        r = Tr(Tr(g * Tr(sig(g))) * u).reshape(M, cols // 2)
    else:
        raise ValueError(epi)
    return r.to(torch.float64).numpy()


def apply_resid(h, acc, prec=64):
    dt, Tr = (torch.float64, _T64) if prec == 64 else (torch.float32, _T32)
    return Tr(torch.as_tensor(h).to(dt) + Tr(torch.as_tensor(acc).to(dt))).to(torch.float64).numpy()


def mismatch(a, b):
    """(share of elements that differ, worst bf16 ulp distance)"""
    d = bf16_ulp_distance(a, b)
    return float(np.mean(d != 0)), int(d.max())


# ------------------------------------------------------------------------------------------------ case lists
# mirrors GEMM_CASE in launch_gemm_mt (csrc/lm_kernels.hip): (epilogue, R, KSB, U); R = 4 is built for <= 32 rows only
DENSE_TABLE = [
    (EPI_PARTIAL, 1, 1, 4), (EPI_PARTIAL, 1, 4, 4), (EPI_PARTIAL, 2, 1, 4), (EPI_PARTIAL, 2, 2, 4), (EPI_PARTIAL, 2, 4, 4),
    (EPI_BF16, 2, 1, 4), (EPI_BF16, 2, 4, 4), (EPI_SILU_MUL, 2, 1, 4), (EPI_SILU_MUL, 2, 4, 4),
    (EPI_SILU_MUL, 4, 4, 3), (EPI_PARTIAL, 4, 4, 2), (EPI_PARTIAL, 4, 4, 3), (EPI_PARTIAL, 4, 2, 2), (EPI_PARTIAL, 4, 2, 3),
    (EPI_BF16, 4, 4, 3), (EPI_BF16, 4, 4, 2), (EPI_BF16, 4, 2, 3),
    (EPI_GELU_PACKED, 2, 4, 4), (EPI_GELU_PACKED, 1, 4, 4), (EPI_BF16, 1, 4, 4), (EPI_SILU_PACKED, 2, 4, 4),
]
# mirrors QGEMM_CASE in launch_qgemm_mt (csrc/lm_qgemm.hip): (epilogue, R, KSB) -> scale formats; U follows from the launcher (R = 4: 1, else
# 2 up to 32 rows and 1 above); R = 4 and KSB = 8 are built for <= 32 rows
QSTREAM_TABLE = {
    (EPI_PARTIAL, 2, 4): (0, 1), (EPI_GELU_PACKED, 2, 4): (0, 1), (EPI_BF16, 2, 1): (0, 1),
    (EPI_PARTIAL, 1, 4): (0,), (EPI_PARTIAL, 2, 1): (0,), (EPI_BF16, 2, 4): (0,), (EPI_SILU_MUL, 2, 1): (0,), (EPI_SILU_MUL, 2, 4): (0,),
    (EPI_SILU_MUL, 4, 4): (0,), (EPI_SILU_MUL, 4, 8): (0,), (EPI_BF16, 4, 4): (0,), (EPI_BF16, 4, 8): (0,), (EPI_PARTIAL, 4, 4): (0,),
    (EPI_PARTIAL, 4, 8): (0,), (EPI_SILU_MUL, 2, 8): (0,), (EPI_BF16, 2, 8): (0,),
}
# mirrors QGEMM1_CASE in launch_qgemm1_mt: <= 32 rows, U in {2, 4, 6}
QONESHOT_TABLE = {(EPI_PARTIAL, 1, 4): (0,), (EPI_BF16, 2, 4): (0,), (EPI_SILU_MUL, 2, 4): (0,), (EPI_PARTIAL, 2, 4): (0, 1), (EPI_GELU_PACKED, 2, 4): (0, 1)}
ROWS = [1, 16, 17, 32, 33, 48, 64]


def q_expected(M, epi, R, ksb, G, S, v2=True):
    """the launcher's rule (launch_gemm_skinny_q): (kernel, U) for a launch"""
    mt = (M + 15) // 16
    if R == 4:
        return K_QSTREAM, 1
    if ksb == 8:
        return K_QSTREAM, 2
    n = -(-(-(-G // S)) // ksb)
    if v2 and mt <= 2 and ksb != 1 and n <= 6:
        return K_QONESHOT, 2 if n <= 2 else 4 if n <= 4 else 6
    return K_QSTREAM, 2 if mt <= 2 else 1


def dense_cases():
    """every GEMM_CASE: per-wave k-tile counts 0 .. 5 U + 1 with equal (KT = KSB n) and unequal (KT = KSB n + 1 .. KSB - 1) waves - KT = 9 and
    13, the Moonshine widths, are among them for every arrangement - at rows cycling through ROWS; every row count at one width; NT around
    multiples of R (the tile clamp) and NT = 1; split-K S in {1, 2, 3, KT} for the partial epilogue"""
    cases = []
    for ai, (epi, R, ksb, U) in enumerate(DENSE_TABLE):
        rows = [m for m in ROWS if R < 4 or m <= 32]
        add = lambda **kw: cases.append(dict(dict(epi=epi, R=R, ksb=ksb, U=U, NT=R, S=1, bias=len(cases) % 2 == 0, seed=1000 + len(cases)), **kw))
        i = ai
        for n in range(0, 5 * U + 2):
            for r in range(ksb):
                if ksb * n + r >= 1:
                    add(M=rows[i % len(rows)], KT=ksb * n + r)
                    i += 1
        for M in rows:
            add(M=M, KT=2 * ksb * U + ksb + 1)
        step = 2 if epi == EPI_SILU_MUL else 1
        for NT in sorted({step} | set(range(R, 2 * R + 1, step)) | set(range(2 * R, 3 * R, step))):
            if NT >= 1:
                add(M=rows[i % len(rows)], KT=ksb + 2, NT=NT)
                i += 1
        if epi == EPI_PARTIAL:
            for KT in (9, 13, 2 * ksb + 3):
                for S in (1, 2, 3, KT):
                    add(M=rows[i % len(rows)], KT=KT, S=S, NT=R + 1)
                    i += 1
    return cases


def quant_cases(v2=True):
    """every QGEMM_CASE / QGEMM1_CASE at both bit widths and scale formats.  Streaming kernel: scale groups per wave 0 .. 5 U + 1 (U = 2), equal and
    unequal waves; one-shot kernel: every share 1 .. 6 (buffers of 2, 4, 6 full and with dead groups), even and uneven splits over the four
    waves, and S == G (waves without a group).  Which kernel a case reaches is the launcher's decision (q_expected)."""
    cases = []
    for (epi, R, ksb), sbts in QSTREAM_TABLE.items():
        for sbt in sbts:
            for bits in (8, 4):
                rows = [m for m in ROWS if (R < 4 and ksb < 8) or m <= 32]
                i = len(cases)
                NT = max(R, 2 if epi == EPI_SILU_MUL else 1)
                add = lambda **kw: cases.append(dict(dict(epi=epi, R=R, ksb=ksb, bits=bits, sbt=sbt, NT=NT, S=1, bias=len(cases) % 2 == 0,
                                                          seed=5000 + len(cases)), **kw))
                for n in range(0, 12):
                    for r in sorted({0, 1, ksb - 1}):
                        if ksb * n + r >= 1:
                            add(M=rows[i % len(rows)], G=ksb * n + r)
                            i += 1
                if ksb == 4 and R <= 2:                      # the one-shot shapes: shares 1 .. 6 even / uneven at 16 and 32 rows
                    for n in range(1, 7):
                        for G in sorted({4 * n, max(4 * n - 1, 1), max(4 * n - 3, 1)}):
                            for M in (9, 32):
                                add(M=M, G=G)
                    if epi == EPI_PARTIAL:
                        for G, S in ((5, 5), (8, 8), (7, 2), (24, 2), (13, 3), (40, 3)):
                            add(M=rows[i % 4], G=G, S=S, NT=R + 1)
                            i += 1
                step = 2 if epi == EPI_SILU_MUL else 1
                for NT2 in sorted({step} | set(range(R, 2 * R, step))):
                    add(M=rows[i % len(rows)], G=ksb + 1, NT=NT2)
                    i += 1
    for c in cases:
        c["expect"] = q_expected(c["M"], c["epi"], c["R"], c["ksb"], c["G"], c["S"], v2)
    return cases


def dense_case_inputs(c):
    """(x, w_interleaved, w, w2, bias) of a dense case; non-linear epilogues get the x amplitude that keeps the pre-activations unsaturated"""
    K = 32 * c["KT"]
    e = x_log2_for_std(K, DENSE_W_RMS) if c["epi"] in NONLINEAR else -5
    two = c["epi"] == EPI_SILU_MUL or c.get("two", False)
    N = 16 * c["NT"] // (2 if two else 1)
    x, w = dense_inputs(c["M"], N, K, c["seed"], e)
    w2 = dense_inputs(c["M"], N, K, c["seed"] + 500000, e)[1] if two else None
    wi = interleave(w, w2) if two else w
    if c["epi"] == EPI_GELU_PACKED:
        x = x * 2.0 ** -gelu_safe_shift(x, wi)
    bias = out_bias(16 * c["NT"], c["seed"], 0 if c["epi"] == EPI_GELU_PACKED else -3) if c["bias"] and c["epi"] != EPI_SILU_MUL else None
    return x, wi, w, w2, bias


def quant_case_inputs(c):
    K = 64 * c["G"]
    e = x_log2_for_std(K, quant_w_rms(c["bits"]), 1.7) if c["epi"] in NONLINEAR else -5
    two = c["epi"] == EPI_SILU_MUL
    N = 16 * c["NT"] // (2 if two else 1)
    a = quant_inputs(c["M"], N, K, c["bits"], c["seed"], e)
    b = quant_inputs(c["M"], N, K, c["bits"], c["seed"] + 500000, e) if two else None
    wi = interleave(a[4], b[4]) if two else a[4]
    x = a[0]
    if c["epi"] == EPI_GELU_PACKED:
        x = x * 2.0 ** -gelu_safe_shift(x, wi)
    bias = out_bias(16 * c["NT"], c["seed"], 0 if c["epi"] == EPI_GELU_PACKED else -3) if c["bias"] and c["epi"] != EPI_SILU_MUL else None
    return x, wi, a, b, bias


# ------------------------------------------------------------------------------------------------ the entry points
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _lib():
    from mlx_audio_swift_amd import _lib as L
    return L


def run_skinny(x, w, w2, bias, epi, R, ksb, U, S):
    """mis_debug_gemm_skinny -> (status, out float32 [S][Mpad][cols] / [Mpad][features] or None, report)"""
    M, K = x.shape
    N = w.shape[0]
    cols = (2 if w2 is not None else 1) * N
    Mpad = (M + 15) // 16 * 16
    shape = (S, Mpad, cols) if epi == EPI_PARTIAL else (Mpad, cols // 2 if epi == EPI_SILU_MUL else cols)
    out = np.empty(shape, np.float32)
    rep = np.full(8, -1, np.int32)
    bw, bw2, bx = exact_bits(w), None if w2 is None else exact_bits(w2), exact_bits(x)
    bb = None if bias is None else exact_bits(bias)
    st = _lib().lib().mis_debug_gemm_skinny(0, _ptr(bw), _ptr(bw2), _ptr(bx), _ptr(bb), M, N, K, epi, R, ksb, U, S, _ptr(out), out.size, _ptr(rep))
    return st, (out if st == 0 else None), tuple(int(v) for v in rep)


def run_skinny_q(x, a, b, bias, bits, sbt, epi, R, ksb, S):
    """mis_debug_gemm_skinny_q on quant_inputs tuples a (and b, interleaved behind it) -> (status, out, report)"""
    M, K = x.shape
    N = a[1].shape[0]
    sbd = MIS_F16 if sbt else MIS_BF16
    cols = (2 if b is not None else 1) * N
    Mpad = (M + 15) // 16 * 16
    shape = (S, Mpad, cols) if epi == EPI_PARTIAL else (Mpad, cols // 2 if epi == EPI_SILU_MUL else cols)
    out = np.empty(shape, np.float32)
    rep = np.full(8, -1, np.int32)
    pk = lambda t: (None, None, None) if t is None else (pack_codes(t[1], bits), exact_bits(t[2], sbd), exact_bits(t[3], sbd))
    qa, qb = pk(a), pk(b)
    bx = exact_bits(x)
    bb = None if bias is None else exact_bits(bias)
    st = _lib().lib().mis_debug_gemm_skinny_q(0, bits, sbd, _ptr(qa[0]), _ptr(qa[1]), _ptr(qa[2]), _ptr(qb[0]), _ptr(qb[1]), _ptr(qb[2]), _ptr(bx),
                                              _ptr(bb), M, N, K, epi, R, ksb, S, _ptr(out), out.size, _ptr(rep))
    return st, (out if st == 0 else None), tuple(int(v) for v in rep)


def run_pf(x, w, w2, h, epi):
    M, K = x.shape
    N = w.shape[0]
    cols = (2 if w2 is not None else 1) * N
    out = np.empty((M, cols // 2 if epi == PF_SILU else cols), np.float32)
    rep = np.full(8, -1, np.int32)
    bw, bw2, bx = exact_bits(w), None if w2 is None else exact_bits(w2), exact_bits(x)
    bh = None if h is None else exact_bits(h)
    st = _lib().lib().mis_debug_gemm_pf(0, _ptr(bw), _ptr(bw2), _ptr(bx), _ptr(bh), M, N, K, epi, _ptr(out), out.size, _ptr(rep))
    return st, (out if st == 0 else None), tuple(int(v) for v in rep)


def quant_instantiations():
    """(expect = (kernel, U), epilogue, R, KSB, bits, scale format, MT) of every instantiation in QGEMM_CASE / QGEMM1_CASE"""
    want = set()
    for bits in (8, 4):
        for (epi, R, ksb), sbts in QSTREAM_TABLE.items():
            for sbt in sbts:
                for mt in ((1, 2) if R == 4 or ksb == 8 else (1, 2, 3, 4)):
                    want.add(((K_QSTREAM, 1 if R == 4 else 2 if (ksb == 8 or mt <= 2) else 1), epi, R, ksb, bits, sbt, mt))
        for (epi, R, ksb), sbts in QONESHOT_TABLE.items():
            for sbt in sbts:
                for mt in (1, 2):
                    for U in (2, 4, 6):
                        want.add(((K_QONESHOT, U), epi, R, ksb, bits, sbt, mt))
    return want


# prefill GEMM: M x N x K of the issue; PF_F32 takes the whole product, the two bf16 epilogues a diagonal through it
PF_M, PF_N, PF_K = [1, 63, 64, 127, 128, 129, 300], [16, 112, 128, 144, 272], [128, 192, 1024]
PF_SILU_SHAPES = [(PF_M[i % 7], PF_N[i % 5], PF_K[i % 3], 9000 + i) for i in range(35)]
PF_RESID_SHAPES = [(PF_M[i % 7], PF_N[(i + 2) % 5], PF_K[(i + 1) % 3], 9500 + i) for i in range(35)]
