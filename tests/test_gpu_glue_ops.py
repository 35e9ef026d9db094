"""The LM glue as OPERATORS: k_embed_rmsnorm, k_reduce_residual_rmsnorm / k_glue4 / k_glue_cpt, k_gemm_skinny_norm, the prefill row kernels,
k_prefill_feed, k_convert_to_bf16 and k_dequant_affine, one launch at a time through the mis_debug_* entry points of csrc/glue_debug.hip,
against tests/glue_ref.py (its claims are proven in tests/test_glue_ref_cpu.py).  h' = T(h + T(sum of the slabs)) is compared BIT FOR BIT on
every input; x bit for bit on the zero, constant and balanced rows and against the derived bounds on Gaussian rows.  Every launch asserts its
status, the instantiation the dispatch comment names, that no poison (0xFFFF) is left where the kernel must write and that it is intact where
it must not (the entry points fail on a touched guard)."""
import functools

import numpy as np
import pytest

import enc_ref as er
import gemm_ref as gr
import glue_ref as g
from gpu_util import record

pytestmark = pytest.mark.gpu
OK, INVALID_INPUT, GENERATION_FAILED = g.OK, g.INVALID_INPUT, g.GENERATION_FAILED
KNAME = {g.K_GENERAL: "k_reduce_residual_rmsnorm", g.K_GLUE4: "k_glue4", g.K_CPT: "k_glue_cpt"}


def _fail(errors):
    assert not errors, f"{len(errors)} failures, first: " + "\n".join(str(e) for e in errors[:8])


def _same(payload, want64):
    """payloads == those of exactly representable values; zeros of either sign are one value"""
    want = gr.bf16_bits(np.asarray(want64, np.float64).astype(np.float32)).reshape(payload.shape)
    return bool(np.all((payload == want) | (((payload | want) & 0x7FFF) == 0)))


# ------------------------------------------------------------------------------------------------ the glue sweep
def _glue_one(c, exact, errors, seen, worst):
    tag = f"{'exact' if exact else 'gaussian'} S {c['S']} Mpad {c['Mpad']} N {c['N']} {'LayerNorm' if c['ln'] else 'RMSNorm'}"
    want = g.glue_expected(c["S"], c["N"], c["ln"])
    st, hb, x, tail, rep = g.run_glue(c)
    if st != OK or rep != want:
        errors.append(f"status {st}, ran {rep}, the dispatch comment says {want}: {tag}")
        return None
    seen.add(g.instantiation_key(rep, c["N"], c["ln"]))
    hp = g.hprime(c["slabs"], c["h"])
    if not np.array_equal(hb, g.bits(hp)):
        errors.append(f"h' differs on {int((hb != g.bits(hp)).sum())} elements: {tag}")
        return None
    if np.any(x == 0xFFFF) or not np.all(tail == 0xFFFF):
        errors.append("x: poison left, or the columns behind N of the last k-tile were written: " + tag)
        return None
    if exact:
        if not _same(x, c["expect"]):
            errors.append(f"x differs from the exact tier on {int((g.val(x) != c['expect']).sum())} elements: {tag}")
    else:
        frac, bad = g.check_x(c, g.val(x), hp)
        key = (rep[0], c["ln"])
        worst[key] = max(worst.get(key, 0.0), frac)
        if bad or frac > 1.0:
            errors.append(f"x: {bad} elements outside, {frac:.3f} of the bound: {tag}")
    return hb, x


@functools.lru_cache(maxsize=None)
def _glue_sweep(N):
    errors, seen, worst = [], set(), {}
    S_list = g.GLUE_S + (g.GLUE_S_GENERAL if N in (4, 100, 256, 3072) else [])
    for S in S_list:
        for Mpad in (16, 48):
            for ln in (False, True):
                seed = 1000 * N + 10 * S + Mpad
                _glue_one(g.exact_case(S, Mpad, N, ln, seed), True, errors, seen, worst)
                _glue_one(g.gauss_case(S, Mpad, N, ln, seed + 1), False, errors, seen, worst)
    for (k, ln), v in worst.items():
        record(f"glue_ops_{KNAME[k]}_{'layernorm' if ln else 'rmsnorm'}_N{N}", fraction_of_bound=v)
    return errors, seen


@pytest.mark.parametrize("N", g.GLUE_N)
def test_glue_every_width_every_slab_count(N):
    """one live thread (4), N % 32 != 0 (100), a ragged last wave (252), k_glue_cpt only at 3072 and k_glue4 there with LayerNorm, 1024 threads
    (4096), the general kernel at N / 4 > 1024 (4100), at N % 4 != 0 (6, 3074) and in two and three passes of its c0 loop (3076 .. 6148)"""
    errors, _ = _glue_sweep(N)
    _fail(errors)


def test_glue_every_instantiation_ran():
    seen = set()
    for N in g.GLUE_N:
        seen |= _glue_sweep(N)[1]
    assert seen == g.GLUE_INSTANTIATIONS, sorted(map(str, g.GLUE_INSTANTIATIONS - seen))


def test_glue_kernels_agree_on_the_same_rows():
    """N = 3072: k_glue_cpt (RMSNorm, S = 8), k_glue4 (the same rows as LayerNorm input give the same h'), the general kernel (S = 9, a zero
    ninth slab): h' identical bits on Gaussian rows; x identical on the exact tier between the two RMSNorm kernels"""
    for exact in (False, True):
        c = (g.exact_case if exact else g.gauss_case)(8, 16, 3072, False, 4242)
        st, h_cpt, x_cpt, _, rep = g.run_glue(c)
        assert st == OK and rep[0] == g.K_CPT
        c9 = dict(c, S=9, slabs=np.concatenate([c["slabs"], np.zeros((1,) + c["slabs"].shape[1:], np.float32)]))
        st, h_gen, x_gen, _, rep = g.run_glue(c9)
        assert st == OK and rep[0] == g.K_GENERAL
        cl = dict(c, ln=True, b=np.zeros(3072), eps=g.EPS_LN)
        st, h_g4, _, _, rep = g.run_glue(cl)
        assert st == OK and rep[0] == g.K_GLUE4
        assert np.array_equal(h_cpt, h_gen) and np.array_equal(h_cpt, h_g4)
        if exact:
            assert np.array_equal(x_cpt, x_gen)
        else:                                                   # each inside the bound of the same reference
            hp = g.hprime(c["slabs"], c["h"])
            for x in (x_cpt, x_gen):
                frac, bad = g.check_x(c, g.val(x), hp)
                assert bad == 0 and frac <= 1.0


# ------------------------------------------------------------------------------------------------ embed + RMSNorm
@pytest.mark.parametrize("d", [8, 2048, 2056, 12288])
def test_embed_rmsnorm(d):
    """one chunk, a full slot, a ragged slot, the limit.  ids in range, -1 and vocab (pinned: embedding row 0 - the hosts reject such ids before a
    launch, see include/mi_speech_debug.h), the last row of the table with the NaN guard behind it; rows >= batch are written from row 0"""
    rng = np.random.default_rng(d)
    vocab, errors, worst = 6, [], 0.0
    a = 1.25 * 2.0 ** -2
    E = g.T(rng.standard_normal((vocab, d)) * np.array([1, 0, 0, 4, 0.25, 2])[:, None])
    E[2] = a * rng.choice([-1.0, 1.0], d)                                   # row 1 zero, row 2 balanced
    w_g, w_p = g.T(1.0 + 0.5 * rng.standard_normal(d)), 2.0 ** rng.integers(-2, 3, d) * rng.choice([-1.0, 1.0], d)
    for Mpad, ids, active in ((16, [3, -1, vocab, vocab - 1, 1, 2, 0], [1, 0, 1, 1, 1, 0, 1]), (32, [vocab - 1, 2, 1] + [4] * 14, [1] * 17)):
        batch = len(ids)
        pos_next = rng.integers(0, 100, batch)
        for w, exact in ((w_g, False), (w_p, True)):
            st, h, ximg, pc, pn = g.run_embed(E, ids, active, np.full(batch, -5), pos_next, w, g.EPS_RMS, Mpad)
            href, pc_w, pn_w = g.embed_reference(E, np.asarray(ids), active, pos_next, Mpad)
            tag = f"d {d} Mpad {Mpad} exact {exact}"
            if st != OK or not _same(h, href) or not np.array_equal(pc, pc_w) or not np.array_equal(pn, pn_w):
                errors.append(f"status {st}, or h / positions differ: {tag}")
                continue
            x, tail = g.unpack_x(ximg, Mpad, d)
            if np.any(x == 0xFFFF) or not np.all(tail == 0xFFFF):
                errors.append("x: poison left or the tail written: " + tag)
                continue
            c = dict(ln=False, w=w, b=None, eps=g.EPS_RMS)
            frac, bad = g.check_x(c, g.val(x), href)
            worst = max(worst, frac)
            if bad or frac > 1.0:
                errors.append(f"x: {bad} outside, {frac:.3f} of the bound: {tag}")
            if exact:                                           # the zero row and the balanced row, bit for bit
                f = np.float32
                inv = f(1.0) / np.sqrt(f(f(a) * f(a) + f(g.EPS_RMS)))
                want = g.b16((w.astype(f) * g.b16((E[2].astype(f) * inv).astype(f))).astype(f)).astype(np.float64)
                for m, i in enumerate(ids):
                    if i == 1 and not np.all((x[m] & 0x7FFF) == 0):
                        errors.append("zero row: x != 0 " + tag)
                    if i == 2 and not _same(x[m], want):
                        errors.append("balanced row differs " + tag)
    record(f"glue_ops_k_embed_rmsnorm_d{d}", fraction_of_bound=worst)
    _fail(errors)


def test_embed_rmsnorm_refuses_unsupported_widths():
    E, w = np.zeros((2, 12296)), np.ones(12296)
    for d in (12296, 12):
        st = g.run_embed(E[:, :d], [0], [1], [0], [0], w[:d], g.EPS_RMS, 16)[0]
        assert st == INVALID_INPUT, d


def test_hosts_reject_ids_outside_the_vocabulary_before_a_launch():
    """decode (mis_lm_forward, active rows) and prefill (mis_lm_prefill) alike: MIS_ERR_INVALID_INPUT, and the positions have not advanced"""
    import mlx_audio_swift_amd as mas
    from gpu_util import lm_pair
    from oracle import llama as ollama
    cfg = ollama.TINY
    _, _, dev = lm_pair(cfg)
    dev.lm_reset(2, 64)
    good = dev.lm_forward(np.asarray([5, 6], np.int32))
    for bad in (-1, cfg.vocab_size):
        with pytest.raises(mas.AudioGenerationError):
            dev.lm_forward(np.asarray([5, bad], np.int32))
        with pytest.raises(mas.AudioGenerationError):
            dev.lm_prefill([np.asarray([1, bad, 2], np.int32)])
    dev.lm_reset(2, 64)
    again = dev.lm_forward(np.asarray([5, cfg.vocab_size], np.int32), np.asarray([1, 0], np.uint8))      # an inactive row's id is not consumed
    assert np.array_equal(again[0], good[0])


# ------------------------------------------------------------------------------------------------ prefill rows
@pytest.mark.parametrize("d", [8, 264, 1024])
def test_prefill_rows(d):
    rng = np.random.default_rng(d)
    errors, worst, vocab = [], 0.0, 7
    E = g.T(rng.standard_normal((vocab, d)) * 2.0 ** rng.integers(-2, 3, (vocab, 1)))
    w = g.T(1.0 + 0.5 * rng.standard_normal(d))
    c = dict(ln=False, w=w, b=None, eps=g.EPS_RMS)
    for Lmax, lens, t0, Tc, Mpad in ((1, [1, 0, 1], 0, 1, 16), (5, [5, 0, 3, 1, 2], 0, 5, 16), (5, [5, 0, 3, 1, 2], 2, 3, 5), (5, [4, 5], 3, 2, 16)):
        batch = len(lens)
        prompt = rng.integers(0, vocab, (batch, Lmax))
        prompt[0, Lmax - 1] = vocab                             # an id outside the vocabulary: pinned as a ZERO row (the hosts reject it before a launch)
        if batch > 2 and lens[2] > 0:
            prompt[2, Lmax - 1] = -1
        src_rows = batch + 3
        rows = g.T(rng.standard_normal((Lmax, src_rows, d)))
        for mode in (0, 1):
            tag = f"mode {mode} d {d} Lmax {Lmax} t0 {t0} Tc {Tc} Mpad {Mpad}"
            st, h, x, pos, act = g.run_pf(mode, table=E if mode == 0 else rows, prompt=prompt, lens=lens, Lmax=Lmax, t0=t0, Tc=Tc, batch=batch, Mpad=Mpad,
                                          vocab=vocab, src_rows=src_rows, w=w, d=d)
            href, on, pw = g.pf_embed_reference(E, prompt, lens, Lmax, t0, Tc, batch, Mpad)
            if mode == 1:                                       # the caller's matrix keeps its own rows per position
                href = np.zeros((Tc, Mpad, d))
                href[:, :batch] = rows[t0:t0 + Tc, :batch]
                href = np.where(on.reshape(Tc, Mpad, 1), href, 0.0).reshape(Tc * Mpad, d)
            if st != OK or not np.array_equal(pos, pw) or not np.array_equal(act, on.astype(np.uint8)) or not _same(h, href):
                errors.append(f"status {st}, or h / tables differ: {tag}")
                continue
            x = x.reshape(Tc * Mpad, d)
            frac, bad = g.check_x(c, g.val(x), href)
            worst = max(worst, frac)
            if bad or frac > 1.0 or np.any(x == 0xFFFF):
                errors.append(f"x: {bad} outside, {frac:.3f} of the bound: {tag}")
    record(f"glue_ops_k_pf_rows_rmsnorm_d{d}", fraction_of_bound=worst)
    # pf_rmsnorm against the decode glue on the same h': bit for bit on the exact tier, both inside the bound on Gaussian rows
    if d % 4 == 0:
        for exact in (True, False):
            cg = (g.exact_case if exact else g.gauss_case)(3, 16, d, False, 77 + d)
            st, hb, xg, _, _ = g.run_glue(cg)
            st2, h2, xp, _, _ = g.run_pf(2, w=cg["w"], d=d, Tc=1, Mpad=16, h=hb)
            assert st == OK and st2 == OK and np.array_equal(h2, hb)
            xp = xp.reshape(16, d)
            if exact:
                assert np.array_equal(xp, xg) and _same(xp, cg["expect"])
            else:
                hp = g.val(hb)
                for x in (xp, xg):
                    frac, bad = g.check_x(cg, g.val(x), hp)
                    assert bad == 0 and frac <= 1.0
    _fail(errors)


def test_prefill_add_resid_and_pack_rows():
    rng = np.random.default_rng(5)
    for n in (1, 1000, 1025):
        h, part = g.T(rng.standard_normal(n) * 4), (rng.standard_normal(n) * 4).astype(np.float32)
        st, hb, _, _, _ = g.run_pf(3, part=part, n=n, h=gr.exact_bits(h))
        assert st == OK and np.array_equal(hb.reshape(-1), g.bits(g.add_resid(h, part))), n
    for Mpad, d in ((16, 8), (48, 264), (16, 1024)):
        rows = rng.integers(0, 0x7F00, (Mpad, d)).astype(np.uint16)
        st, hb, x, _, _ = g.run_pf(4, Mpad=Mpad, d=d, h=rows, xsize=Mpad * (-(-d // 32) * 32))
        back, tail = g.unpack_x(x, Mpad, d)
        assert st == OK and np.array_equal(back, rows) and np.all(tail == 0xFFFF) and np.array_equal(hb, rows), (Mpad, d)
        assert np.array_equal(x, g.pack_x(rows))


@pytest.mark.parametrize("batch", [1, 64, 65])
def test_prefill_feed(batch):
    rng = np.random.default_rng(batch)
    Lmax = 5
    lens = rng.integers(0, Lmax + 1, batch)
    lens[0] = 3
    prompt = rng.integers(1, 1000, (batch, Lmax))
    for j in (0, 1, 2, 4, 5, 9):                                # before row 0's prompt, inside it, past the end
        st, after, ids, act = g.run_feed(prompt, lens, Lmax, j)
        wi, wa = g.feed_reference(prompt, lens, Lmax, j)
        assert st == OK and after == j + 1 and np.array_equal(ids, wi) and np.array_equal(act, wa), (batch, j)


# ------------------------------------------------------------------------------------------------ the norm-prologue GEMM
def _gelu_ref(pre):
    return g.T(er.gelu64(g.T(pre)))


def test_norm_gemm_exact_tier():
    errors, worst, share_max, seen = [], 0, 0.0, set()
    i = 0
    for K in (32, 384, 1280):
        for N_out in (32, 48):
            for nrows in (1, 8, 9, 16):
                S_in = (1, 4, 5, 8)[i % 4]
                i += 1
                c = g.norm_gemm_exact_case(K, N_out, nrows, S_in, 9000 + i)
                tag = f"K {K} N_out {N_out} nrows {nrows} S_in {S_in}"
                st, out, h_out, h_after, rep = g.run_norm_gemm(c)
                if st != OK or rep != (g.K_NORM_GEMM, gr.EPI_GELU_PACKED, 1, 4 if S_in <= 4 else 8, 5):
                    errors.append(f"status {st}, ran {rep}: {tag}")
                    continue
                seen.add(rep[3])
                hp = g.bits(g.hprime(c["slabs"], c["h"]))
                if not np.array_equal(h_out[:nrows], hp[:nrows]) or not np.all(h_out[nrows:] == 0xFFFF) or not np.array_equal(h_after, gr.exact_bits(c["h"])):
                    errors.append("h_out rows < nrows != h', rows >= nrows touched, or h_in changed: " + tag)
                want = _gelu_ref(np.where(np.arange(16)[:, None] < nrows, c["pre"], c["bias"][None, :]))      # rows >= nrows: zero fragments, GELU(bias)
                if np.any(np.isnan(out)):
                    errors.append("output: poison left " + tag)
                    continue
                ulp, share = er.gelu_condition(out.astype(np.float64), want)
                worst, share_max = max(worst, ulp), max(share_max, share)
                if ulp > er.GELU_ULP or share > er.GELU_SHARE:
                    errors.append(f"output: {ulp} bf16 ulp, {share:.4f} of the elements differ (caps {er.GELU_ULP}, {er.GELU_SHARE}) " + tag)
    record("glue_ops_k_gemm_skinny_norm_exact", worst_ulp=worst, worst_case_share_differing=share_max)
    _fail(errors)
    assert seen == {4, 8}


def test_norm_gemm_gaussian_within_the_propagated_bound():
    K, N_out, nrows, S_in = 1280, 48, 9, 5
    rng = np.random.default_rng(31)
    c = g.gauss_case(S_in, 16, K, True, 31)
    W = g.T(rng.standard_normal((N_out, K)) * 1.2 / np.sqrt(K))
    bias = g.T(0.25 * rng.standard_normal(N_out))
    c.update(W=W, bias=bias, nrows=nrows, N_out=N_out)
    st, out, h_out, h_after, rep = g.run_norm_gemm(c)
    hp = g.hprime(c["slabs"], c["h"])
    assert st == OK and rep[0] == g.K_NORM_GEMM and np.array_equal(h_out[:nrows], g.bits(hp)[:nrows]) and np.all(h_out[nrows:] == 0xFFFF)
    y, bx = er.ln_reference(hp.astype(np.float64)[:nrows], c["w"], c["b"], c["eps"])
    gam = 2.0 * (K * g.U) / (1.0 - K * g.U)
    pre = y @ W.T + bias
    D = bx @ np.abs(W).T + gam * ((np.abs(y) + bx) @ np.abs(W).T + np.abs(bias))
    ref = er.gelu64(pre)
    # |gelu'| <= 1.13; the inner T() adds half a bf16 ulp of the pre-activation; the device polynomial and the outer T(): 1.5 ulp of the result
    e1 = 1.13 * (D + g.ar.ulp_bf16(np.abs(pre) + D) / 2)
    bound = e1 + 1.5 * g.ar.ulp_bf16(np.abs(ref) + e1)
    ratio = float((np.abs(out[:nrows].astype(np.float64) - ref) / bound).max())
    record("glue_ops_k_gemm_skinny_norm_gaussian", fraction_of_bound=ratio)
    assert ratio <= 1.0
    want_pad = _gelu_ref(np.tile(bias, (16 - nrows, 1)))
    assert er.gelu_condition(out[nrows:].astype(np.float64), want_pad)[0] <= er.GELU_ULP


def test_norm_gemm_capability_check_equals_the_launcher():
    """gemm_skinny_norm_ok answers true exactly for what launch_gemm_skinny_norm builds; everything else returns the launcher's status and
    launches nothing"""
    c = g.norm_gemm_exact_case(384, 32, 8, 4, 1)
    assert g.norm_gemm_ok(gr.EPI_GELU_PACKED, 2, 12, 1, 4, 16, 8, True) and g.run_norm_gemm(c)[0] == OK
    refused = [dict(epi=gr.EPI_PARTIAL), dict(epi=gr.EPI_PARTIAL, S=2), dict(S=2), dict(ln=False), dict(R=1), dict(R=4), dict(epi=gr.EPI_BF16), dict(epi=gr.EPI_SILU_PACKED)]
    for kw in refused:
        a = dict(epi=gr.EPI_GELU_PACKED, R=2, S=1, ln=True)
        a.update(kw)
        assert not g.norm_gemm_ok(a["epi"], a["R"], 12, a["S"], 4, 16, 8, a["ln"]), kw
        st, _, h_out, _, rep = g.run_norm_gemm(c, **a)
        assert (st, rep[0]) == (GENERATION_FAILED, -1) and np.all(h_out == 0), kw           # (h_out is not even copied back)
    for nrows, S_in, K in ((0, 4, 384), (17, 4, 384), (8, 9, 384), (8, 4, 1312)):
        assert not g.norm_gemm_ok(gr.EPI_GELU_PACKED, 2, K // 32, 1, S_in, 16, nrows, True)
        c2 = g.norm_gemm_exact_case(K, 32, 8, S_in, 2)
        c2["nrows"] = nrows
        st, _, _, _, rep = g.run_norm_gemm(c2)
        assert (st, rep[0]) == (GENERATION_FAILED, -1), (nrows, S_in, K)
    assert not g.norm_gemm_ok(gr.EPI_GELU_PACKED, 2, 12, 1, 4, 32, 8, True)


# ------------------------------------------------------------------------------------------------ load-time kernels
@pytest.mark.parametrize("dtype", [g.MIS_F32, g.MIS_F16, g.MIS_BF16])
def test_convert_to_bf16(dtype):
    for n in (1, 255, 257):
        src = g.convert_values(n, dtype, 10 * n + dtype)
        st, out = g.run_convert(src, dtype)
        want, nan = g.convert_reference(src, dtype)
        assert st == OK
        assert np.array_equal(out[~nan], want[~nan]), (dtype, n)
        assert np.all((out[nan] & 0x7FC0) == 0x7FC0), "a NaN must come back as a quiet NaN"


def test_dequant_affine_fused_or_unfused_throughout():
    votes = {"fused": 0, "unfused": 0}
    differ = total = 0
    for nbits in (4, 8):
        for sbt in (g.MIS_F32, g.MIS_F16, g.MIS_BF16):
            for K in (64, 192):
                q, sc, bi = g.dequant_inputs(16, K, nbits, sbt, 100 * nbits + 10 * sbt + K)
                st, out = g.run_dequant(q, sc, bi, nbits, sbt)
                unf, fus = g.dequant_reference(q, sc, bi)
                assert st == OK and np.all((out == unf) | (out == fus)), (nbits, sbt, K)
                d = unf != fus
                differ += int(d.sum()); total += d.size
                votes["fused"] += int((out[d] == fus[d]).sum()); votes["unfused"] += int((out[d] == unf[d]).sum())
    record("glue_ops_k_dequant_affine", share_fused_differs_from_unfused=differ / total, elements_that_differ=differ, device_gave_fused=votes["fused"],
           device_gave_unfused=votes["unfused"])
    assert differ > 0 and (votes["fused"] == 0 or votes["unfused"] == 0), votes
