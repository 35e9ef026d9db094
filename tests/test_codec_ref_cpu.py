"""CPU proof of what tests/test_gpu_codec_ops.py leans on (no GPU, no library call): the grid and two-limb references of tests/codec_ref.py
do not depend on the summation order, the two-limb inputs tell the three products of the split apart, and a float32 emulation of the
Gaussian cases stays inside the derived bounds."""
import numpy as np

import codec_ref as cr
from test_codec_math_cpu import sin_sq_f32

F = np.float32


def _cases():
    return [cr.case(cr.PLAIN, 40, 33, 96, batch=2, seed=1), cr.case(cr.RESID, 32, 17, 40, scale=1, snake=1, seed=2),
            cr.case(cr.NOISE, 40, 20, 40, seed=3), cr.case(cr.TAPS, 33, 21, Cin=40, taps=7, dil=3, pad=18, x_lo=-18, resid=1, scale=1, seed=4),
            cr.case(cr.CONVT, 32, 9, Cin=40, ntaps=2, s=4, pad=2, Tout=34, x_lo=-1, dup_bias_n0=1, seed=5),
            cr.case(cr.CONVT, 32, 9, Cin=32, ntaps=1, s=3, pad=1, Tout=25, seed=6)]


def _f32_any_order(c, at, x, rng):
    """the contraction of one batch row accumulated in float32, one product at a time, in a random order of (tap, channel)"""
    Cin, M = cr.kx_of(c), c["M"]
    at = at.reshape(-1, Cin, M)
    terms = []                                                          # per (tap, channel): its [M][Tout] contribution
    for j in range(at.shape[0]):
        for k in range(Cin):
            a1 = np.zeros_like(at)
            a1[j, k] = at[j, k]
            terms.append(cr.contract(c, dict(AT=a1.reshape(-1, M), X=x), raw=True))
    acc = np.zeros_like(terms[0], dtype=F)
    for i in rng.permutation(len(terms)):
        acc = (acc + np.nan_to_num(terms[i]).astype(F)).astype(F)       # every term is exact in float32; the running sum is rounded every step
    groups = np.array_split(rng.permutation(len(terms)), 7)             # and regrouped: seven partial sums, then their sum
    parts = [sum((np.nan_to_num(terms[i]).astype(F) for i in g), np.zeros_like(acc)) for g in groups]
    acc2 = np.zeros_like(acc)
    for p in parts:
        acc2 = (acc2 + p).astype(F)
    return acc, acc2


def test_grid_reference_is_order_independent():
    rng = np.random.default_rng(0)
    for c in _cases():
        c = dict(c, batch=1, N=min(c["N"], 9))
        c["Tin"] = c["N"]
        c["Tout"] = min(c["Tout"], c["s"] * c["N"] if c["mode"] == cr.CONVT else c["N"])
        inp = cr.grid_inputs(c)
        ref = np.nan_to_num(cr.contract(c, inp, raw=True))
        a, b = _f32_any_order(c, inp["AT"], inp["X"], rng)
        assert np.array_equal(a, ref.astype(F)) and np.array_equal(b, ref.astype(F)) and np.array_equal(ref, ref.astype(F)), c
        y = cr.ref_gemm(c, inp)
        assert np.array_equal(np.nan_to_num(y), np.nan_to_num(y).astype(F))                  # the epilogue stays exact in float32 too


def test_two_limb_split_is_exact_and_the_three_term_sum_order_independent():
    rng = np.random.default_rng(1)
    for c in _cases():
        c = dict(c, batch=1, N=min(c["N"], 9))
        c["Tin"] = c["N"]
        c["Tout"] = min(c["Tout"], c["s"] * c["N"] if c["mode"] == cr.CONVT else c["N"])
        inp, l = cr.two_limb_inputs(c)                                   # asserts the distinctness of the four term sums itself
        for v, hi, lo in ((inp["AT"], l["ah"], l["al"]), (inp["X"], l["xh"], l["xl"])):
            v32 = np.asarray(v, F)
            assert np.array_equal(v32, v) and np.array_equal(cr.bf16_round(v32), hi.astype(F)) and np.array_equal(cr.bf16_round(v32 - hi.astype(F)), lo.astype(F))
        sums = [np.nan_to_num(cr.contract(c, dict(AT=a, X=x), raw=True)) for a, x in ((l["ah"], l["xh"]), (l["al"], l["xh"]), (l["ah"], l["xl"]))]
        want = sum(sums)
        assert np.array_equal(want, want.astype(F))
        got = np.zeros_like(want, dtype=F)
        order = [(a, x) for a, x in ((l["ah"], l["xh"]), (l["al"], l["xh"]), (l["ah"], l["xl"]))]
        for i in rng.permutation(3):                                     # term by term, each term one product at a time in a random order
            t1, t2 = _f32_any_order(c, order[i][0], order[i][1], rng)
            assert np.array_equal(t1, sums[i].astype(F)) and np.array_equal(t2, sums[i].astype(F))
            got = (got + t1).astype(F)
        assert np.array_equal(got, want.astype(F))
        full = np.nan_to_num(cr.contract(c, inp, raw=True))
        assert (full != want).mean() > 0.9                               # the full product (lo.lo kept) is a different answer


def test_two_limb_generator_rejects_a_contraction_too_long_to_be_exact():
    try:
        cr.two_limb_inputs(cr.case(cr.TAPS, 32, 8, Cin=96, taps=7, dil=1, pad=6))
    except AssertionError:
        return
    raise AssertionError("K = 672 accepted")


def test_float32_emulation_of_the_gaussian_cases_stays_inside_the_bound():
    cases = [cr.case(cr.PLAIN, 40, 33, 96, batch=2, seed=1), cr.case(cr.GELU, 40, 33, 96, seed=2), cr.case(cr.RESID, 32, 17, 40, scale=1, snake=1, seed=3),
             cr.case(cr.NOISE, 40, 20, 40, seed=4), cr.case(cr.TAPS, 33, 21, Cin=40, taps=7, dil=3, pad=18, x_lo=-18, resid=1, snake=1, seed=5),
             cr.case(cr.CONVT, 32, 9, Cin=40, ntaps=2, s=4, pad=2, Tout=34, x_lo=-1, seed=6)]
    for c in cases:
        inp = cr.gaussian_inputs(c)
        ref = cr.ref_gemm(c, inp)
        for split in (False, True):
            got = cr.emulate_f32(c, inp, split, sin_sq_f32).astype(np.float64)
            ratio = np.abs(got - ref) / cr.bound_gemm(c, inp, split)
            assert np.isfinite(ratio).all() and ratio.max() <= 0.5, (c["mode"], split, ratio.max())    # 0.5: the bound carries a factor 2 for the MFMA's order


def test_noise_generator_reference_is_a_standard_normal():
    nz, bnd = cr.rng_noise(0x1234, [0, 1, 1 << 33], 4096)
    assert abs(nz.mean()) < 0.03 and abs(nz.std() - 1.0) < 0.03 and not np.array_equal(nz[0], nz[1]) and bnd.max() < 1e-5


def test_case_lists_cross_the_axes_the_kernels_treat_independently():
    """the attributes of a case are drawn independently of the loops: every pair the kernels can combine is run"""
    def cross(cs, *keys):
        return {tuple(c[k] for k in keys) for c in cs}
    t = cr.taps_cases()
    assert cross(t, "M", "N") == {(m, n) for m in (3, 64, 68) for n in (1, 128, 131)}
    for k in ("snake", "scale", "resid"):
        assert cross(t, "Cin", k) == {(c, v) for c in (5, 24) for v in (0, 1)}, k
    assert {(c["Cin"], c["x_lo"] != 0) for c in t} == {(c, h) for c in (5, 24) for h in (False, True)}
    assert cross(t, "taps", "dil", "Cin") >= {(7, d, c) for d in (1, 3, 9) for c in (5, 24)}
    for cv, Ms in ((cr.convt_cases(), (3, 64, 68)), (cr.convt_cases(1), (32, 40, 160))):
        assert cross(cv, "M", "N") == {(m, n) for m in Ms for n in (1, 37, 129)}
        assert cross(cv, "N", "x_lo", "bias") == {(n, x, b) for n in (1, 37, 129) for (x, b) in ((0, 1), (-1, 1), (-1, 0))}
    b = [c for c, _, _ in cr.bf3_cases() if c["mode"] != cr.CONVT]
    assert cross(b, "M", "N") >= {(m, n) for m in cr.BF3_M for n in cr.BF3_N}
    assert {(c["batch"], c["x_lo"] != 0, c["resid"]) for c in b} == {(p, h, r) for p in (1, 3) for h in (False, True) for r in (0, 1)}
    s = cr.snac_gemm_cases()
    assert cross(s, "mode", "M") >= {(m, M) for m in (cr.PLAIN, cr.RESID, cr.NOISE, cr.GELU) for M in (3, 64, 68)}
