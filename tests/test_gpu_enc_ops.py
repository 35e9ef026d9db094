"""The encoder kernels of csrc/whisper_kernels.hip as OPERATORS: k_gemm_big / k_gemm_big2 / k_gemm_big3 with their four epilogues, k_layernorm /
k_layernorm8, k_im2col3, k_scatter_kv, k_attn_prefill / k_attn_prefill2, k_whisper_embed_ln and k_whisper_suppress, one launch at a time through
the mis_debug_* entry points of csrc/enc_debug.hip, against the float64 specification of tests/enc_ref.py (its claims are proven in
tests/test_enc_ref_cpu.py).  Inputs whose result is exact are compared BIT FOR BIT - a residual row read from the wrong tile edge, a bias
shifted by a column, a key too many in the masked tile or a LayerNorm with the wrong divisor cannot hide behind a tolerance; Gaussian data
is held to the derived bounds.  Every launch asserts its status, the kernel the launcher's rule names, that no poison (0xFFFF) is left where
the kernel must write and that it is intact where it must not (the entry points fail on a touched guard or padding column)."""
import functools

import numpy as np
import pytest

import attn_ref as ar
import enc_ref as er
import gemm_ref as gr
from gpu_util import record

pytestmark = pytest.mark.gpu
OK, INVALID_INPUT = er.OK, er.INVALID_INPUT


def _val(bits):
    return gr.bf16_value(bits).astype(np.float64)


def _same(bits, want64):
    """payloads == the bf16 payloads of exactly representable values"""
    return np.array_equal(bits, gr.bf16_bits(np.asarray(want64, np.float64).astype(np.float32)).reshape(bits.shape))


def _poison(bits):
    return bool(np.any(bits == 0xFFFF))


def _fail(errors):
    assert not errors, f"{len(errors)} failures, first: " + "\n".join(str(e) for e in errors[:8])


# ------------------------------------------------------------------------------------------------ GEMM
def _gemm_one(c, errors, gelu_stats, seen):
    tag = str({k: v for k, v in c.items() if k not in ("seed", "expect")})
    d = er.gemm_inputs(c)
    want = er.gemm_expected(c["M"], c["N"], c["K"], c["ldx"], c["epi"], 1 if c["mode"] is None else c["mode"])
    st, out, rep = er.run_gemm(c, d)
    if st != OK or rep != want:
        errors.append(f"status {st}, ran {rep}, the launcher's rule says {want}: {tag}")
        return None
    seen.add(rep)
    if _poison(out):
        errors.append("poison left (element never written) " + tag)
        return out
    ref, g = er.gemm_reference(c, d)
    if c["epi"] in (er.BG_NONE, er.BG_RESID):
        if not _same(out, ref):
            errors.append("output differs " + tag)
        return out
    gdev = out
    if c["epi"] == er.BG_GELU_POS:                         # the GELU half from a BG_GELU launch of the same operands; the additive half bit for bit on it
        st, gdev, rep2 = er.run_gemm(c, d, epi=er.BG_GELU)
        if st != OK or rep2 != want[:1] + (er.BG_GELU,) + want[2:] or _poison(gdev):
            errors.append(f"GELU launch of a GELU_POS case: status {st}, ran {rep2}: {tag}")
            return out
        if not _same(out, er.add_pos_f32(_val(gdev), c, d)):
            errors.append("positional add differs from T(g + P[m % pos_rows]) " + tag)
    worst, share = er.gelu_condition(_val(gdev), g)
    print(f"GELU {tag}: worst {worst} ulp, share differing {share:.5f}")
    t = gelu_stats.setdefault(c["kernel"], [0, 0.0, 0, 0])
    t[0], t[1] = max(t[0], worst), max(t[1], share)
    t[2] += int(round(share * gdev.size)); t[3] += gdev.size
    if worst > er.GELU_ULP or share > er.GELU_SHARE:
        errors.append(f"GELU: {worst} bf16 ulp from the rounding-point reference, {share:.4f} of the elements differ (caps {er.GELU_ULP}, {er.GELU_SHARE}) " + tag)
    return out


@functools.lru_cache(maxsize=None)
def _gemm_sweep(kernel):
    errors, stats, seen, outs = [], {}, set(), {}
    for c in er.gemm_cases():
        if c["kernel"] == kernel:
            out = _gemm_one(c, errors, stats, seen)
            if kernel == er.K_BIG3 and out is not None and c["K"] < 4096 and c["N"] < 4096:
                c2 = dict(c, mode=0)                       # the same operands through k_gemm_big2: the same bits, GELU included
                st, out2, rep = er.run_gemm(c2, er.gemm_inputs(c))
                if st != OK or rep[0] != er.K_BIG2 or not np.array_equal(out, out2):
                    errors.append(f"k_gemm_big2 and k_gemm_big3 disagree (status {st}, ran {rep}): {c}")
                seen.add(rep)
    for k, (worst, share, bad, n) in stats.items():
        record(f"enc_ops_gemm_kernel{k}_gelu", worst_ulp=worst, worst_case_share_differing=share, share_differing=bad / n, elements=n)
    return errors, seen


@pytest.mark.parametrize("kernel", [er.K_BIG, er.K_BIG2, er.K_BIG3])
def test_gemm_every_epilogue_every_edge(kernel):
    """k_gemm_big (K in 32 .. 288), k_gemm_big2 (MIS_GEMM_BIG3=0; odd and even tile counts), k_gemm_big3<4, 2> and <2, 4> (MIS_GEMM_BIG3=2):
    rows and columns around the tile sizes, dense, padded and overlapping rows, bias and none, pos_rows wrapping inside a tile"""
    errors, _ = _gemm_sweep(kernel)
    _fail(errors)


def test_gemm_every_instantiation_ran():
    seen = set()
    for kernel in (er.K_BIG, er.K_BIG2, er.K_BIG3):
        seen |= _gemm_sweep(kernel)[1]
    assert seen == er.GEMM_INSTANTIATIONS, sorted(er.GEMM_INSTANTIATIONS - seen)


def test_gemm_default_rule_switches_at_200_blocks():
    errors, seen = [], set()
    for c in er.DEFAULT_RULE_CASES:
        _gemm_one(c, errors, {}, seen)
    _fail(errors)
    assert {r[0] for r in seen} == {er.K_BIG2, er.K_BIG3}


def test_gemm_refused_shapes_launch_nothing():
    base = dict(kernel=0, mode=None, M=8, N=8, K=128, ldx=128, epi=er.BG_NONE, bias=True, pos_rows=0, seed=1)
    d = er.gemm_inputs(dict(base, K=160, ldx=160))
    assert er.run_gemm(base, d)[0] == OK
    for kw in (dict(K=144), dict(ldx=132), dict(N=6), dict(K=48, ldx=48)):
        st, out, rep = er.run_gemm(dict(base, **kw), d)
        assert (st, rep[0]) == (INVALID_INPUT, -1), (kw, st, rep)
    st, _, rep = er.run_gemm(dict(base, epi=er.BG_RESID), d)              # an epilogue without its R: the entry point's refusal
    assert (st, rep[0]) == (INVALID_INPUT, -1)


@pytest.mark.parametrize("kernel,mode,K", [(er.K_BIG, 1, 288), (er.K_BIG2, 0, 1280), (er.K_BIG3, 2, 1280)])
def test_gemm_gaussian_within_the_float32_summation_bound(kernel, mode, K):
    """|dev - ref64| <= delta (1 + 2^-8) + 2^-8 |ref|, delta = 2 gamma_K sum_k |x_k| |w_k| (gemm_ref's float32 summation bound; the second
    term: half a bf16 ulp of the perturbed value)"""
    rng = np.random.default_rng(K + kernel)
    M, N = 257, 132
    gam = 2.0 * (K * er.U) / (1.0 - K * er.U)
    x, w = er.T(rng.standard_normal((M, K))), er.T(0.05 * rng.standard_normal((N, K)))
    c = dict(kernel=kernel, mode=mode, M=M, N=N, K=K, ldx=K, epi=er.BG_NONE, pos_rows=0)
    st, out, rep = er.run_gemm(c, dict(img=x.reshape(-1), w=w, bias=None, R=None))
    assert st == OK and rep == er.gemm_expected(M, N, K, K, er.BG_NONE, mode) and rep[0] == kernel and not _poison(out)
    ref, delta = x @ w.T, gam * (np.abs(x) @ np.abs(w).T)
    ratio = float((np.abs(_val(out) - ref) / (delta * (1 + 2.0 ** -8) + 2.0 ** -8 * np.abs(ref))).max())
    record(f"enc_ops_gemm_gaussian_kernel{kernel}_K{K}", fraction_of_bound=ratio)
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ LayerNorm
def test_layernorm_exact_tiers_and_bound():
    errors, seen, worst = [], set(), {}
    for d in er.LN8_D + er.LN_D:
        for rows in er.LN_ROWS:
            tag = f"d = {d}, rows = {rows}"
            x, w, b = er.ln_constant(rows, d, d + rows)
            st, y, rep = er.run_layernorm(x, w, b)
            if st != OK or rep != er.ln_expected(d):
                errors.append(f"status {st}, ran {rep}: {tag}")
                continue
            seen.add(rep)
            if not _same(y, np.broadcast_to(b, x.shape)):
                errors.append("constant rows: y != b " + tag)
            x, w, b, a = er.ln_balanced(rows, d, 3 * d + rows)
            st, y, rep = er.run_layernorm(x, w, b)
            if st != OK or rep != er.ln_expected(d) or not _same(y, er.ln_balanced_expected(x, w, a)):
                errors.append(f"balanced rows differ (status {st}, ran {rep}) " + tag)
            x, w, b = er.ln_gauss(rows, d, 50 + d + rows)
            st, y, rep = er.run_layernorm(x, w, b)
            ref, bound = er.ln_reference(x, w, b)
            if st != OK or rep != er.ln_expected(d) or _poison(y):
                errors.append(f"gaussian rows: status {st}, ran {rep}, or poison left " + tag)
                continue
            r = float((np.abs(_val(y) - ref) / bound).max())
            worst[rep] = max(worst.get(rep, 0.0), r)
            if r > 1.0:
                errors.append(f"gaussian rows: {r:.3f} of the bound " + tag)
    for k, v in worst.items():
        record(f"enc_ops_layernorm_kernel{k}", fraction_of_bound=v)
    _fail(errors)
    assert seen == {0, 1}


# ------------------------------------------------------------------------------------------------ im2col
def test_im2col_bit_for_bit():
    errors = []
    for i, (Cc, Tin, stride, f32) in enumerate([(Cc, Tin, s, f) for Cc in (3, 80) for Tin in (10, 11) for s in (1, 2) for f in (True, False)]):
        B, Tout = 2, (Tin + stride - 1) // stride if stride == 2 else Tin
        if f32:
            xin = er.im2col_f32_values((B, Tin, Cc), 90 + i)
            x64 = xin.astype(np.float64)
        else:
            x64 = er.T(np.random.default_rng(90 + i).standard_normal((B, Tin, Cc)))
            xin = gr.exact_bits(x64)
        st, out = er.run_im2col(xin, f32, Tout, stride)
        if st != OK or not _same(out, er.im2col_reference(x64, Tout, stride)):
            errors.append(f"status {st} or output differs: C {Cc}, Tin {Tin}, stride {stride}, f32 {f32}")
    _fail(errors)


# ------------------------------------------------------------------------------------------------ scatter_kv, attn_prefill
SCATTER_T = [1, 31, 32, 33, 70]


def test_scatter_kv_whole_images():
    errors = []
    B, H = 2, 2
    for D in (64, 128):
        for i, Tn in enumerate(SCATTER_T):
            for extra in (0, 64):
                Spad = 32 * -(-Tn // 32) + extra
                ld, k0, v0 = 3 * H * D + 16, H * D + 8, 2 * H * D + 16
                src = np.random.default_rng(D + Tn + extra).integers(1, 0x7F00, (B * Tn, ld)).astype(np.uint16)
                st, kc, vc = er.run_scatter(src, ld, k0, v0, B, Tn, H, D, Spad)
                kw, vw = er.scatter_reference(src, ld, k0, v0, B, Tn, H, D, Spad)
                if st != OK or not np.array_equal(kc, kw) or not np.array_equal(vc, vw):
                    errors.append(f"status {st} or image differs: D {D}, T {Tn}, Spad {Spad}")
    _fail(errors)
    src = np.ones((2 * 5, 128), np.uint16)
    assert er.run_scatter(src, 128, 32, 64, 2, 5, 1, 32, 32)[0] == INVALID_INPUT
    assert er.run_scatter(src, 128, 0, 64, 2, 5, 1, 64, 0)[0] == INVALID_INPUT         # no room for the tile: the entry point's refusal


ATTN_KERNELS = [("prefill2_d64", 64, False), ("prefill_d64", 64, True), ("prefill_d128", 128, False)]


@functools.lru_cache(maxsize=None)
def _attn_sweep():
    errors, seen, worst = [], set(), {}
    for ti, Tn in enumerate(er.ATTN_T):
        for tier in ("locator", "uniform", "gauss"):
            outs = {}
            for ki, (name, D, v1) in enumerate(ATTN_KERNELS):
                c = _attn_case(tier, D, Tn, 8 * ((ti + ki) % 2))
                tag = f"{name} {tier} T = {Tn} ldo = {c['ldo']}"
                st, out, rep = er.run_attn(c, v1)
                if st != OK or rep != er.attn_expected(D, v1):
                    errors.append(f"status {st}, ran {rep}: {tag}")
                    continue
                seen.add(rep)
                outs[name] = out
                if _poison(out):
                    errors.append("poison left " + tag)
                elif tier == "gauss":
                    ref, bound = er.attn_reference(c)
                    r = float((np.abs(_val(out) - ref) / bound).max())
                    worst[name] = max(worst.get(name, 0.0), r)
                    if r > 1.0:
                        errors.append(f"{r:.3f} of the bound " + tag)
                elif not _same(out, er.attn_exact_expected(c)):
                    errors.append("exact tier differs " + tag)
            if "prefill2_d64" in outs and "prefill_d64" in outs and not np.array_equal(outs["prefill2_d64"], outs["prefill_d64"]):
                errors.append(f"k_attn_prefill2<64> and k_attn_prefill<64> disagree: {tier} T = {Tn}")
    for k, v in worst.items():
        record(f"enc_ops_attn_{k}", fraction_of_bound=v)
    return errors, seen


@functools.lru_cache(maxsize=None)
def _attn_case(tier, D, Tn, ldo_pad):
    return er.attn_case(tier, D, Tn, 1000 + 7 * Tn + D + len(tier), ldo_pad=ldo_pad)


def test_attn_prefill_every_kernel_every_length():
    """T in 1 .. 300 (one key, one ragged tile, whole tiles, one ragged 256-row block): locator and uniform tiers bit for bit, the Gaussian tier
    under the bound, the two D = 64 kernels bit-identical, padding columns of ldo = H D + 8 and the NaN tiles behind Spad untouched / unread"""
    errors, seen = _attn_sweep()
    _fail(errors)
    assert seen == er.ATTN_INSTANTIATIONS


def test_attn_prefill_refuses_other_head_dims():
    c = dict(er.attn_case("uniform", 64, 5, 1), D=96)
    c["q"], c["ldq"], c["ldo"] = np.zeros((2 * 5, 2 * 96)), 3 * 2 * 96, 2 * 96
    c["kimg"], c["vimg"] = np.zeros((2, 2, c["Spad"] * 96), np.uint16), np.zeros((2, 2, c["Spad"] * 96), np.uint16)
    st, _, rep = er.run_attn(c)
    assert (st, rep[0]) == (INVALID_INPUT, -1)


def test_scatter_then_attention_as_the_encoder_chains_them():
    """qkv rows [B T][3 H D] -> k_scatter_kv -> k_attn_prefill2 on the scatter's own images (0xFFFF behind the last tile)"""
    B, H, D, Tn = 2, 2, 64, 70
    c = er.attn_case("gauss", D, Tn, 77)
    Spad, HD = c["Spad"], H * D
    src = np.zeros((B * Tn, 3 * HD), np.uint16)
    src[:, :HD] = gr.exact_bits(c["q"])
    src[:, HD:2 * HD] = gr.exact_bits(c["K"][:, :, :Tn].transpose(0, 2, 1, 3).reshape(B * Tn, HD))
    src[:, 2 * HD:] = gr.exact_bits(c["V"][:, :, :Tn].transpose(0, 2, 1, 3).reshape(B * Tn, HD))
    st, kc, vc = er.run_scatter(src, 3 * HD, HD, 2 * HD, B, Tn, H, D, Spad)
    assert st == OK
    Tt = 32 * -(-Tn // 32)
    assert np.array_equal(kc[:, :, :Tt * D], c["kimg"][:, :, :Tt * D]) and np.array_equal(vc[:, :, :Tt * D], c["vimg"][:, :, :Tt * D])
    assert np.all(kc[:, :, Tt * D:] == 0xFFFF) and np.all(vc[:, :, Tt * D:] == 0xFFFF)
    ref, bound = er.attn_reference(c)
    for v1 in (False, True):
        st, out, rep = er.run_attn(c, v1, kimg=kc, vimg=vc)
        assert st == OK and rep == er.attn_expected(D, v1) and not _poison(out)
        assert (np.abs(_val(out) - ref) / bound).max() <= 1.0
        st, out2, _ = er.run_attn(c, v1)
        assert st == OK and np.array_equal(out, out2)


# ------------------------------------------------------------------------------------------------ decoder step helpers
def test_whisper_embed_ln():
    rng = np.random.default_rng(11)
    errors = []
    for d, Mpad in ((64, 16), (384, 32)):
        vocab, max_pos, batch = 50, 12, 7
        E, P = er.T(rng.standard_normal((vocab, d))), er.T(0.5 * rng.standard_normal((max_pos, d)))
        lw, lb = er.ln_gauss_wb(d, d)
        ids = np.array([3, -1, vocab, 49, 0, 2 ** 30, 17])
        act = np.array([1, 0, 1, 1, 0, 1, 1])
        pn = np.array([0, 5, max_pos - 1, max_pos, max_pos + 7, 3, 11])
        pc = np.full(batch, -5)
        h_ref, x_ref, bound, pc_ref, pn_ref = er.embed_ln_reference(E, P, ids, act, pn, lw, lb, max_pos, Mpad)
        st, h, x, pc2, pn2 = er.run_embed_ln(E, P, ids, act, pc, pn, lw, lb, max_pos, Mpad)
        if st != OK:
            errors.append(f"status {st}, d = {d}")
            continue
        if not _same(h, h_ref):
            errors.append(f"h differs, d = {d}")
        if list(pc2) != list(pc_ref) or list(pn2) != list(pn_ref):
            errors.append(f"positions {list(pc2)} {list(pn2)}, expected {list(pc_ref)} {list(pn_ref)}")
        xu = er.unpack_x(x, Mpad, d)
        r = float((np.abs(_val(xu) - x_ref) / bound).max()) if not _poison(xu) else np.inf
        record(f"enc_ops_embed_ln_d{d}", fraction_of_bound=r)
        if not r <= 1.0:
            errors.append(f"x: {r} of the LayerNorm bound (inf: poison left), d = {d}")
    _fail(errors)


def test_whisper_suppress():
    rng = np.random.default_rng(12)
    batch, vocab, Vpad = 4, 70, 96
    l = er.T(4.0 * rng.standard_normal((batch, Vpad)))
    sup, bsup = [1, 5, 69, 70, 95, -3, 33], [5, 7, 69, 200, 0]
    n_gen, act = [0, 2, 0, 0], [1, 1, 0, 1]
    for active in (act, None):
        st, img = er.run_suppress(l, vocab, sup, bsup, n_gen, active)
        assert st == OK and _same(img, er.suppress_reference(l, vocab, sup, bsup, n_gen, active))
    st, img = er.run_suppress(l, vocab, [], bsup, n_gen, act)
    assert st == OK and _same(img, er.suppress_reference(l, vocab, [], bsup, n_gen, act))
    st, img = er.run_suppress(l, vocab, sup, [], n_gen, act)
    assert st == OK and _same(img, er.suppress_reference(l, vocab, sup, [], n_gen, act))
