"""The codec kernels as OPERATORS: every kernel family behind launch_gemm (k_snac_gemm in its five modes, k_conv_taps, k_pw_fused, and the
split-bf16 path k_bf3_pack_w / k_bf3_split / k_bf3_gemm / k_bf3_splitk_epilogue), launch_codec_final / _hist / _embed, launch_dw7 and
launch_vq_nearest, one launch at a time through mis_debug_codec_* (csrc/codec_debug.hip) against tests/codec_ref.py.

On grid inputs every kernel must equal the float64 reference BIT FOR BIT, on two-limb inputs the split-bf16 kernels must equal the three-term
sum bit for bit (both proven order-independent in tests/test_codec_ref_cpu.py): a dropped or doubled product of the split, a tap shifted by
a column, a phase written past Tout, a float4 read past Tin (the padding of every row is NaN) or a tail tile multiplied by stale LDS cannot
hide behind a tolerance.  What cannot be exact (Snake with alpha != 0, GELU, the noise generator, float32 accumulation) is held to the
per-element bounds derived in codec_ref.py; the measured worst fraction of each bound is recorded.  Every case asserts the kernel that ran."""
import functools

import numpy as np
import pytest

import codec_ref as cr
from gpu_util import record

pytestmark = pytest.mark.gpu
OK, GENERATION_FAILED, INVALID_INPUT = cr.OK, cr.GENERATION_FAILED, cr.INVALID_INPUT


def _bits_equal(got, want64):
    want = np.asarray(want64, np.float64).astype(np.float32)
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _tag(c):
    return str({k: v for k, v in c.items() if v not in (0, None)})


def _ran(st, y, rep, want, c, errors):
    """status, the kernel that ran and no poison left; False (and an error) otherwise"""
    if st != OK or rep[:len(want)] != tuple(want):
        errors.append(f"status {st}, ran {rep}, expected {tuple(want)}: {_tag(c)}")
        return False
    if np.isnan(y).any():
        errors.append(f"NaN (element never written, or an input over-read) at {int(np.isnan(y).sum())} of {y.size}: {_tag(c)}")
        return False
    return True


def _worst_ratio(err, bound):
    """max of err / bound over ALL elements; an element with a zero bound must be exact, a NaN anywhere is infinitely wrong"""
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.where(np.isnan(ratio), np.inf, ratio).max())


def _exact(c, inp, want, errors, ref=None, what="grid"):
    st, y, rep = cr.run_gemm(c, inp)
    if _ran(st, y, rep, want, c, errors) and not _bits_equal(y, cr.ref_gemm(c, inp) if ref is None else ref):
        errors.append(f"{what}: differs from the reference: {_tag(c)}")
    return y


def _within(c, inp, want, split, worst, key, errors):
    """tolerance cases: every element against its own bound, none left out"""
    st, y, rep = cr.run_gemm(c, inp)
    if not _ran(st, y, rep, want, c, errors):
        return
    worst[key] = max(worst.get(key, 0.0), _worst_ratio(np.abs(y - cr.ref_gemm(c, inp)), cr.bound_gemm(c, inp, split)))


def _grid_sweep(cases, want_of, worst=None):
    errors = []
    for c in cases:
        inp = cr.grid_inputs(c)
        if c["mode"] == cr.GELU:                                       # exact contraction, erff in the epilogue: held to the bound
            _within(c, inp, want_of(c), False, worst, "gelu_on_grid", errors)
            continue
        _exact(c, inp, want_of(c), errors)
        if c["snake"] and c["mode"] != cr.CONVT:
            _exact(c, cr.with_dead_channel_snake(c, inp), want_of(c), errors, what="Snake on all-zero channels")
    return errors


@functools.lru_cache(maxsize=None)
def _snac_sweep():
    worst = {}
    return _grid_sweep(cr.snac_gemm_cases(), lambda c: (cr.K_SNAC,), worst), worst


@functools.lru_cache(maxsize=None)
def _convt_sweep():
    errors = _grid_sweep(cr.convt_cases(), lambda c: (cr.K_SNAC,))
    for c in cr.convt_cases()[::5]:                                    # the Snake plumbing of the transposed conv (it always runs the prologue)
        inp = cr.grid_inputs(c)
        _exact(c, cr.with_dead_channel_snake(c, inp), (cr.K_SNAC,), errors, what="Snake on all-zero channels")
    return errors


@functools.lru_cache(maxsize=None)
def _taps_sweep():
    return _grid_sweep(cr.taps_cases(), lambda c: (cr.K_TAPS, c["taps"]))


@functools.lru_cache(maxsize=None)
def _bf3_sweep():
    errors, seen, worst = [], set(), {}
    with cr.env(**cr.LOW):
        for c, ntaps, nq in cr.bf3_cases():
            want = (cr.K_BF3, ntaps, nq, 1)
            inp = cr.grid_inputs(c)
            if c["mode"] == cr.GELU:                                   # exact contraction, erff in the epilogue: the bound with no accumulation error
                _within(c, inp, want, False, worst, "gelu_on_grid", errors)
            else:
                _exact(c, inp, want, errors)
                if c["snake"] and c["mode"] != cr.CONVT:
                    _exact(c, cr.with_dead_channel_snake(c, inp), want, errors, what="Snake on all-zero channels")
            seen.add((c["mode"], ntaps, nq))
            if c["mode"] != cr.GELU and c["K"] <= 320:                 # the K up to which the three-term sum is exact in float32 (two_limb_inputs)
                inp, limbs = cr.two_limb_inputs(c)
                _exact(c, inp, want, errors, ref=cr.ref_three_term(c, inp, limbs), what="two-limb")
    return errors, seen, worst


def _report(errors):
    assert not errors, f"{len(errors)} failures, first: " + "\n".join(errors[:8])


def test_snac_gemm_every_mode_every_tail():
    """k_snac_gemm: M in {3, 64, 68} x K in {5, 16, 40} x N in {1, 127, 128, 131}, ldx a multiple of 4 and not with Tin < ldx, ldy > Tout, batch 2;
    PLAIN, RESID with and without scale and Snake plumbing, NOISE with an explicit tensor, GELU (exact contraction, epilogue to the bound)"""
    errors, worst = _snac_sweep()
    _report(errors)
    record("codec_ops_snac_gelu_on_grid", fraction_of_bound=worst["gelu_on_grid"])
    assert worst["gelu_on_grid"] <= 1.0, worst


def test_transposed_conv_phases_history_and_double_bias():
    _report(_convt_sweep())


def test_conv_taps_every_tap_dilation_and_padding():
    _report(_taps_sweep())


def test_conv_taps_halo_limit_is_the_launchers_status():
    c = cr.case(cr.TAPS, 8, 16, Cin=8, taps=7, dil=16, pad=96)
    st, _, rep = cr.run_gemm(c, cr.grid_inputs(c))
    assert (st, rep[0]) == (INVALID_INPUT, -1)


def test_pw_fused_equals_reference_and_the_unfused_kernel():
    errors = []
    for c in cr.fused_cases():
        inp = cr.grid_inputs(c)
        y = _exact(c, inp, (cr.K_FUSED,), errors)
        _exact(c, cr.with_dead_channel_snake(c, inp), (cr.K_FUSED,), errors, what="Snake on all-zero channels")
        with cr.env(MIS_CODEC_FUSED_UNITS="0"):
            y0 = _exact(c, inp, (cr.K_SNAC,), errors)
        if y is not None and y0 is not None and not np.array_equal(y.view(np.uint32), y0.view(np.uint32)):
            errors.append("fused and unfused kernels differ " + _tag(c))
    _report(errors)


def test_noise_generator_rows_and_offset():
    """NOISE with noise_rng: Box-Muller on mis-synth-v1 uniforms keyed by (key, GLOBAL row, n), row = row_offset + row_ids[b].  Grid inputs:
    acc + bias is exact, so the error is the generator's (bound derived in codec_ref.rng_noise) times |acc + bias|, plus the last two roundings"""
    c = cr.case(cr.NOISE, 20, 131, 20, batch=3, ldx=135, ldy=133, seed=41)
    inp = cr.grid_inputs(c)
    v = cr.epilogue(dict(c, mode=cr.PLAIN), inp, cr.contract(c, inp))
    worst = 0.0
    for row_ids, off in ((None, 0), ([7, 2, 900000], 5), (None, 1 << 33)):
        rows = [off + (b if row_ids is None else row_ids[b]) for b in range(3)]
        nz, dnz = cr.rng_noise(0x1234ABCD5678, rows, c["N"])
        st, y, rep = cr.run_gemm(c, dict(inp, noise=None), noise_rng=1, noise_key=0x1234ABCD5678, row_ids=row_ids, row_offset=off)
        assert st == OK and rep[0] == cr.K_SNAC and not np.isnan(y).any(), (st, rep)
        ref = cr.epilogue(c, inp, cr.contract(c, inp), noise=nz)
        bound = dnz[:, None, :] * np.abs(v) + 2 * cr.U * (np.abs(ref) + np.abs(inp["X"][:, :c["M"]]))
        worst = max(worst, _worst_ratio(np.abs(y - ref), bound))
    record("codec_ops_noise_rng", fraction_of_bound=worst)
    assert worst <= 1.0, worst
    cb = cr.case(cr.NOISE, 40, 131, 40, batch=3, ldx=135, ldy=133, use_pack=1, seed=42)     # the generator is written out again in bf3_body
    inpb = cr.grid_inputs(cb)
    vb = cr.epilogue(dict(cb, mode=cr.PLAIN), inpb, cr.contract(cb, inpb))
    nz, dnz = cr.rng_noise(77, [5 + r for r in (7, 2, 900000)], cb["N"])
    with cr.env(**cr.LOW):
        st, y, rep = cr.run_gemm(cb, dict(inpb, noise=None), noise_rng=1, noise_key=77, row_ids=[7, 2, 900000], row_offset=5)
    assert st == OK and rep[0] == cr.K_BF3 and not np.isnan(y).any(), (st, rep)
    ref = cr.epilogue(cb, inpb, cr.contract(cb, inpb), noise=nz)
    worst_b = _worst_ratio(np.abs(y - ref), dnz[:, None, :] * np.abs(vb) + 2 * cr.U * (np.abs(ref) + np.abs(inpb["X"][:, :cb["M"]])))
    record("codec_ops_noise_rng_split_bf16", fraction_of_bound=worst_b)
    assert worst_b <= 1.0, worst_b
    st, y, _ = cr.run_gemm(c, dict(inp, noise=None), noise_rng=0)      # no tensor, no generator: zeros
    assert st == OK and _bits_equal(y, inp["X"][:, :c["M"]])


def test_split_bf16_grid_and_two_limb():
    """the split-bf16 kernels under lowered thresholds: all six modes, 1 / 2 / 7 taps, NQ 9 and 12, Cin padded to Cp; grid inputs bit for bit and
    two-limb inputs against the three-term sum bit for bit"""
    errors, seen, worst = _bf3_sweep()
    _report(errors)
    for mode in (cr.PLAIN, cr.GELU, cr.RESID, cr.NOISE):
        assert (mode, 1, 9) in seen
    assert {(cr.TAPS, 7, 9), (cr.TAPS, 7, 12), (cr.CONVT, 1, 9), (cr.CONVT, 2, 9)} <= seen
    record("codec_ops_bf3_gelu_on_grid", fraction_of_bound=worst["gelu_on_grid"])
    assert worst["gelu_on_grid"] <= 1.0, worst


@pytest.mark.parametrize("Cin,ksplit", [(512, 2), (1024, 4)])
def test_split_k_factor_is_the_shapes_alone(Cin, ksplit):
    errors = []
    with cr.env(**cr.LOW):
        for mode, kw in ((cr.PLAIN, {}), (cr.RESID, dict(scale=1)), (cr.GELU, {})):
            for batch in (1, 3):
                c = cr.case(mode, 32, 16, Cin, batch=batch, ldy=19, split_k_ok=1, use_pack=1, seed=Cin + batch, **kw)
                inp = cr.grid_inputs(c)
                want = (cr.K_BF3, 1, 9, ksplit)
                if mode == cr.GELU:
                    w = {}
                    _within(c, inp, want, False, w, "g", errors)
                    assert not w or w["g"] <= 1.0, w
                    continue
                y = _exact(c, inp, want, errors)
                with cr.env(MIS_BF3_NO_SPLITK="1"):
                    y1 = _exact(c, inp, (cr.K_BF3, 1, 9, 1), errors)
                if y is not None and y1 is not None and not np.array_equal(y.view(np.uint32), y1.view(np.uint32)):
                    errors.append("split-K and one-pass results differ " + _tag(c))
    _report(errors)


def test_ineligible_shapes_stay_on_the_exact_kernels():
    errors = []
    with cr.env(**cr.LOW):
        for c, want in ((cr.case(cr.PLAIN, 31, 40, 64, use_pack=1), cr.K_SNAC),                                        # M < 32
                        (cr.case(cr.TAPS, 32, 40, Cin=32, taps=7, dil=11, pad=66, use_pack=1), cr.K_TAPS),              # span 66 > 64
                        (cr.case(cr.TAPS, 32, 40, Cin=32, taps=3, dil=1, pad=2, use_pack=1), cr.K_TAPS),                # 3 taps
                        # two taps further apart than the 144-column tile of the two-tap body reaches (it was dispatched there once)
                        (cr.case(cr.TAPS, 40, 200, Cin=40, taps=2, dil=17, pad=17, x_lo=-17, ldx=220, batch=3, use_pack=1, seed=3), cr.K_TAPS),
                        (cr.case(cr.TAPS, 160, 129, Cin=32, taps=2, dil=64, pad=32, resid=1, use_pack=1, seed=4), cr.K_TAPS)):
            _exact(c, cr.grid_inputs(c), (want,), errors)
        c = cr.case(cr.PLAIN, 64, 40, 64, use_pack=1)
        _exact(c, cr.grid_inputs(c), (cr.K_BF3,), errors)
        with cr.env(MIS_CODEC_EXACT_F32="1"):
            _exact(c, cr.grid_inputs(c), (cr.K_SNAC,), errors)
    c = cr.case(cr.PLAIN, 64, 40, 64, use_pack=1)                       # the default MIS_BF3_MIN_K1 keeps a 64-channel 1x1 off the split path
    _exact(c, cr.grid_inputs(c), (cr.K_SNAC,), errors)
    _report(errors)


def test_snake_flag_is_ignored_where_the_mode_has_no_prologue():
    """PLAIN / GELU / NOISE have no Snake prologue on either path: the flag and a non-zero alpha change nothing"""
    errors = []
    for use_pack in (0, 1):
        for mode in (cr.PLAIN, cr.NOISE):
            c = cr.case(mode, 40, 129, 40, use_pack=use_pack, seed=9)
            inp = cr.grid_inputs(c)
            with cr.env(**cr.LOW):
                _exact(dict(c, snake=1), dict(inp, alpha=np.full(40, 1.7), ralpha=np.ones(40)), (cr.K_BF3 if use_pack else cr.K_SNAC,), errors,
                       ref=cr.ref_gemm(c, inp), what="Snake flag on a mode without prologue")
    _report(errors)


def test_split_bf16_row_does_not_depend_on_the_batch():
    """codec_kernels.h: "a row's result is the same whatever batch it shares" - Gaussian data, bitwise"""
    with cr.env(**cr.LOW):
        for c3 in (cr.case(cr.PLAIN, 40, 200, 96, batch=3, use_pack=1, seed=5), cr.case(cr.PLAIN, 32, 16, 512, batch=3, split_k_ok=1, use_pack=1, seed=6),
                   cr.case(cr.TAPS, 40, 129, Cin=40, taps=7, dil=3, pad=18, batch=3, use_pack=1, seed=7)):
            inp = cr.gaussian_inputs(c3)
            st3, y3, rep3 = cr.run_gemm(c3, inp)
            c1 = dict(c3, batch=1)
            st1, y1, rep1 = cr.run_gemm(c1, {k: (v[:1] if k == "X" else v) for k, v in inp.items()})
            assert st3 == OK and st1 == OK and rep3[0] == rep1[0] == cr.K_BF3 and rep3[3] == rep1[3], (rep3, rep1)
            assert np.array_equal(y3[:1].view(np.uint32), y1.view(np.uint32)), _tag(c3)


def test_gaussian_data_within_the_derived_bounds():
    """one pass per kernel family (and Snake with alpha != 0, GELU) on Gaussian data: |dev - ref64| <= codec_ref.bound_gemm, element by element"""
    errors, worst = [], {}
    exact = [("snac_plain", cr.case(cr.PLAIN, 68, 131, 40, batch=2, ldx=136, seed=1), (cr.K_SNAC,)),
             ("snac_gelu", cr.case(cr.GELU, 68, 131, 40, batch=2, seed=2), (cr.K_SNAC,)),
             ("snac_resid_snake", cr.case(cr.RESID, 68, 131, 40, batch=2, snake=1, scale=1, seed=3), (cr.K_SNAC,)),
             ("snac_noise", cr.case(cr.NOISE, 68, 131, 68, batch=2, seed=4), (cr.K_SNAC,)),
             ("snac_convt_snake", cr.case(cr.CONVT, 68, 37, Cin=16, ntaps=2, s=4, pad=2, Tout=146, x_lo=-1, ldx=40, batch=2, seed=5), (cr.K_SNAC,)),
             ("taps_snake", cr.case(cr.TAPS, 68, 131, Cin=24, taps=7, dil=3, pad=18, x_lo=-18, ldx=152, resid=1, snake=1, batch=2, seed=6), (cr.K_TAPS, 7)),
             ("fused_snake", cr.case(cr.RESID, 96, 129, 96, snake=1, batch=2, seed=7), (cr.K_FUSED,))]
    for key, c, want in exact:
        _within(c, cr.gaussian_inputs(c), want, False, worst, key, errors)
    split = [("bf3_plain", cr.case(cr.PLAIN, 40, 200, 96, batch=3, use_pack=1, seed=11), 1, 9),
             ("bf3_gelu", cr.case(cr.GELU, 160, 129, 40, use_pack=1, seed=12), 1, 9),
             ("bf3_resid_snake", cr.case(cr.RESID, 128, 129, 96, snake=1, scale=1, use_pack=1, seed=13), 1, 9),
             ("bf3_taps_snake", cr.case(cr.TAPS, 40, 200, Cin=40, taps=7, dil=9, pad=54, x_lo=-54, ldx=256, snake=1, resid=1, batch=3, use_pack=1, seed=14), 7, 12),
             ("bf3_convt_snake", cr.case(cr.CONVT, 40, 129, Cin=40, ntaps=2, s=8, pad=4, Tout=1030, x_lo=-1, ldx=132, batch=3, use_pack=1, seed=15), 2, 9)]
    with cr.env(**cr.LOW):
        for key, c, ntaps, nq in split:
            _within(c, cr.gaussian_inputs(c), (cr.K_BF3, ntaps, nq), True, worst, key, errors)
    for k, v in worst.items():
        record(f"codec_ops_gaussian_{k}", fraction_of_bound=v)
    _report(errors)
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ the stream kernels
def _final_inputs(rng, B, C_, T, k, hist, snake_act, grid):
    if grid:                                                            # ELU restricted to non-negative operands: the identity
        x = rng.integers(0 if not snake_act else -1, 2, (B, C_, hist + T)) * 2.0 ** -5
        w = rng.integers(-4, 5, (k, C_)).astype(np.float64)
        a, ra = (np.zeros(C_), np.ones(C_)) if snake_act else (None, None)
        return x, w, 0.25, a, ra
    f = lambda v: np.asarray(v, np.float32).astype(np.float64)
    a = f(np.exp(rng.standard_normal(C_) * 0.5)) if snake_act else None
    return f(rng.standard_normal((B, C_, hist + T))), f(rng.standard_normal((k, C_)) / np.sqrt(k * C_)), 0.03, a, (f(1.0 / (a + 1e-9)) if snake_act else None)


def test_codec_final_exact_clipped_and_within_bound():
    errors, worst = [], 0.0
    rng = np.random.default_rng(77)
    i = 0
    for snake_act in (1, 0):
        for k in (1, 7, 8):
            for C_ in (1, 16, 17):
                for T in (1, 256, 257):
                    i += 1
                    hist = (0, k - 1)[i % 2]
                    ld, stride = hist + T + (0, 3)[i % 2], T + (2, 0)[i % 3 == 0]
                    for grid in (1, 0):
                        x, w, bias, a, ra = _final_inputs(rng, 2, C_, T, k, hist, snake_act, grid)
                        if grid and snake_act and i % 2:
                            w = w * 8.0                                 # the clip to [-1, 1] is reached on purpose
                        st, out = cr.run_final(x, w, bias, a, ra, -hist, T, ld, stride)
                        ref = cr.ref_final(x, w, bias, a, ra, -hist, T)
                        tag = f"act {snake_act} k {k} C {C_} T {T} hist {hist} grid {grid}"
                        if st != OK or np.isnan(out).any():
                            errors.append(f"status {st} or NaN (element never written, or an input over-read): {tag}")
                        elif grid and not _bits_equal(out, ref):
                            errors.append("differs: " + tag)
                        elif grid and snake_act and i % 2 and C_ >= 16 and T >= 256 and not ((np.abs(ref) == 1.0).any() and (np.abs(ref) < 1.0).any()):
                            errors.append("the clip was not reached: " + tag)
                        elif not grid:
                            worst = max(worst, _worst_ratio(np.abs(out - ref), cr.bound_final(x, w, bias, a, ra, -hist, T)))
    x, w, bias, a, ra = _final_inputs(rng, 1, 17, 300, 7, 0, 1, 1)
    record("codec_ops_final_gaussian", fraction_of_bound=worst)
    _report(errors)
    assert worst <= 1.0, worst
    assert cr.run_final(x, np.zeros((9, 17)), 0.0, a, ra, 0, 300, 300, 300)[0] == GENERATION_FAILED          # k = 9: the launcher's status


@pytest.mark.parametrize("snake_act", [1, 0])
@pytest.mark.parametrize("chunk", [1, 3, 255])
def test_any_chunking_equals_the_whole_decode(snake_act, chunk):
    """the header's claim itself: Gaussian input fed in chunks through launch_codec_hist (H = k - 1) and launch_codec_final equals the one-shot
    output bitwise"""
    rng = np.random.default_rng(5)
    B, C_, T, k = 2, 17, 300, 7
    H = k - 1
    x, w, bias, a, ra = _final_inputs(rng, B, C_, T, k, 0, snake_act, 0)
    st, whole = cr.run_final(x, w, bias, a, ra, 0, T, T, T)
    assert st == OK
    state, parts = np.zeros((B, C_, H)), []
    for t0 in range(0, T, chunk):
        Tn = min(chunk, T - t0)
        img = np.zeros((B, C_, H + Tn + 1))
        img[:, :, H:H + Tn] = x[:, :, t0:t0 + Tn]
        st, state, img = cr.run_hist(state, img, H, Tn)
        assert st == OK
        st, out = cr.run_final(img[:, :, :H + Tn], w, bias, a, ra, -H, Tn, H + Tn + 1, Tn)
        assert st == OK
        parts.append(out)
    got = np.concatenate(parts, axis=1)
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))


def test_codec_hist_is_pure_data_movement():
    rng = np.random.default_rng(9)
    for H in (0, 1, 6, 64):
        for Tn in sorted({1, max(H - 1, 1), H or 2, H + 3}):
            st_ = rng.standard_normal((2, 5, H)).astype(np.float32)
            img = rng.standard_normal((2, 5, H + Tn + 2)).astype(np.float32)
            st, so, xo = cr.run_hist(st_, img, H, Tn)
            rs, rx = cr.ref_hist(st_, img, H, Tn)
            assert st == OK and np.array_equal(so.view(np.uint32), rs.view(np.uint32)) and np.array_equal(xo.view(np.uint32), rx.view(np.uint32)), (H, Tn)
    assert cr.run_hist(np.zeros((1, 2, 65)), np.zeros((1, 2, 70)), 65, 3)[0] == GENERATION_FAILED


def test_codec_embed_clamps_and_sums_in_q_order():
    rng = np.random.default_rng(3)
    for C_ in (1, 257):
        B, nq, T, bins = 2, 5, 9, 11
        tables = rng.standard_normal((nq, bins, C_)).astype(np.float32)
        codes = rng.integers(-3, bins + 3, (B, nq, T))                          # below 0 and at or above bins: clamped
        buf = np.full((B, T + 1, nq + 2), 12345, np.int32)                        # time-major, strided: cs_t != 1
        buf[:, :T, :nq] = codes.transpose(0, 2, 1)
        st, h = cr.run_embed(buf, (T + 1) * (nq + 2), 1, nq + 2, tables, T + 3, T, B)
        assert st == OK and not np.isnan(h).any()
        assert np.array_equal(h.view(np.uint32), np.ascontiguousarray(cr.ref_embed_f32(codes, tables)).view(np.uint32)), C_
        st, h2 = cr.run_embed(codes, nq * T, T, 1, tables, T, T, B)              # dense
        assert st == OK and np.array_equal(h2.view(np.uint32), h.view(np.uint32))


def test_dw7_exact_around_the_tile():
    rng = np.random.default_rng(4)
    for dil in (1, 3, 9):
        for T in (1, 1023, 1024, 1025):
            x = rng.integers(-1, 2, (2, 3, T)) * 2.0 ** -5
            w7, bias = rng.integers(-4, 5, (3, 7)).astype(np.float64), rng.integers(-8, 9, 3) * 2.0 ** -5
            st, y = cr.run_dw7(x, w7, bias, dil)
            assert st == OK and not np.isnan(y).any() and _bits_equal(y, cr.ref_dw7(x, w7, bias, dil)), (dil, T)


def test_vq_nearest_first_index_on_ties():
    """duplicate codebook rows across the 256-thread stride, across waves and inside a wave: the lowest index must win the shuffle reduce and
    the cross-wave step.  Exact: integer latents and codebooks, so equal rows give equal float32 distances whatever the normalisation"""
    rng = np.random.default_rng(8)
    for CD in (8, 64):
        for CB in (1, 255, 257):
            cb = rng.integers(-3, 4, (CB, CD)).astype(np.float64)
            Tm = 6
            pick = rng.integers(0, CB, (2, Tm))
            ze = cb[pick].transpose(0, 2, 1) * 2.0                                 # the latent points along a codebook row: that row (and its copies) is nearest
            dup = {}
            if CB > 1:
                for t, (lo, hi) in enumerate(((1, 70), (3, 200), (0, CB - 1), (65, 66), (130, 254), (5, 129))):
                    lo, hi = min(lo, CB - 1), min(hi, CB - 1)
                    dup[t] = (lo, hi)
            cn = (cb / np.maximum(np.linalg.norm(cb, axis=1, keepdims=True), 1e-12)).astype(np.float32)
            # duplicates: rows `hi` become copies of rows `lo`; every column t looks for row lo's direction
            for t, (lo, hi) in dup.items():
                cn[hi] = cn[lo]
                ze[:, :, t] = cb[lo][None, :] * 2.0 if cb[lo].any() else ze[:, :, t]
            cn2 = (cn.astype(np.float64) ** 2).sum(1).astype(np.float32)
            e = ze / np.maximum(np.linalg.norm(ze, axis=1, keepdims=True), 1e-12)
            dist = (e ** 2).sum(1)[:, None, :] - 2 * np.einsum("kd,bdt->bkt", cn.astype(np.float64), e) + cn2[None, :, None]
            st, codes = cr.run_vq(ze, cn, cn2)
            assert st == OK, st
            for b in range(2):
                for t in range(Tm):
                    d = dist[b, :, t]
                    near = np.flatnonzero(d <= d.min() + 1e-5)                    # float32 candidates: within rounding of the float64 minimum
                    assert codes[b, t] in near, (CD, CB, b, t, codes[b, t], near)
                    same = np.flatnonzero((cn == cn[codes[b, t]]).all(1))          # bitwise-equal rows have bitwise-equal distances
                    assert codes[b, t] == same.min(), (CD, CB, b, t, codes[b, t], same)
    assert cr.run_vq(np.zeros((1, 65, 2)), np.zeros((4, 65)), np.zeros(4))[0] == INVALID_INPUT
