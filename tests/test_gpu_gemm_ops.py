"""The LM GEMM kernels as OPERATORS: k_gemm_skinny (csrc/lm_kernels.hip), k_gemm_skinny_q / k_gemm_skinny_q1 (csrc/lm_qgemm.hip), k_gemm_pf
(csrc/lm_prefill.hip) and the load-time pack kernels, one launch at a time through mis_debug_gemm_* on inputs whose result is exact in
float32 whatever the summation order (tests/gemm_ref.py, proven in tests/test_gemm_ref_cpu.py) - so the linear epilogues are compared BIT
FOR BIT: a dropped, doubled or misplaced k-tile, a dead scale group that is not dropped, a bias on the wrong slab or a tile written where
none belongs cannot hide behind a tolerance.  The non-linear epilogues are held to the rounding-point reference within 2 bf16 ulp, at most
1 % of the elements differing at all; one pass per family on Gaussian data is held to the derived float32 summation bound."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gemm_ref as gr
from gpu_util import record
from oracle import mlxquant as mq

pytestmark = pytest.mark.gpu
V2 = os.environ.get("MIS_QGEMM_V2", "1") != "0"            # the library reads the switch once per process
OK, GENERATION_FAILED, INVALID_INPUT = 0, 2, 3


def _bits_equal(got, want64):
    want = np.asarray(want64, np.float64).astype(np.float32)
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def _check(c, out, x, wi, bias, unit, errors, nl):
    """the asserts shared by the dense and the quantised sweep"""
    M, epi, S = c["M"], c["epi"], c["S"]
    tag = str({k: v for k, v in c.items() if k != "seed"})
    if np.isnan(out).any():
        errors.append("NaN (element never written, or an input over-read) " + tag)
        return
    if epi == gr.EPI_PARTIAL:
        ref = gr.ref_slabs(x, wi, S, unit, bias)
        for s in range(S):                                   # slab s alone = the reference restricted to its K range; the bias on slab 0 only
            if not _bits_equal(out[s, :M], ref[s]):
                errors.append(f"slab {s} differs " + tag)
        if not _bits_equal(out[:, :M].astype(np.float64).sum(0).astype(np.float32), ref.sum(0)):
            errors.append("slab sum differs " + tag)
        pad = np.zeros((S,) + out.shape[1:]) if bias is None else np.concatenate([np.broadcast_to(bias, out.shape[1:])[None], np.zeros((S - 1,) + out.shape[1:])])
        if not _bits_equal(out[:, M:], pad[:, M:]):
            errors.append("rows >= M are not the bias / zero " + tag)
        return
    acc = gr.ref_slabs(x, wi, 1, unit)[0]
    accp = np.concatenate([acc, np.zeros((out.shape[0] - M, acc.shape[1]))])          # rows >= M: x = 0
    ref = gr.apply_epilogue(epi, accp, bias)
    if epi == gr.EPI_BF16:
        if not _bits_equal(out, ref):
            errors.append("bf16 output differs " + tag)
        return
    d = gr.bf16_ulp_distance(out, ref)
    if d.max() > 2:
        errors.append(f"non-linear epilogue {epi}: {int(d.max())} bf16 ulp from the rounding-point reference " + tag)
    t = nl.setdefault(epi, [0, 0, 0])
    t[0] += int((d != 0).sum()); t[1] += d.size; t[2] = max(t[2], int(d.max()))


def _nonlinear_gate(nl, family, errors):
    for epi, (bad, n, worst) in sorted(nl.items()):
        record(f"gemm_ops_{family}_epilogue_{epi}", share_differing=bad / n, worst_ulp=worst, elements=n)
        if bad / n > 0.01:
            errors.append(f"{family} epilogue {epi}: {bad} of {n} elements differ from the rounding-point reference (cap 1 %)")


@functools.lru_cache(maxsize=None)
def _dense_sweep():
    errors, nl, seen = [], {}, set()
    for c in gr.dense_cases():
        x, wi, w, w2, bias = gr.dense_case_inputs(c)
        st, out, rep = gr.run_skinny(x, w, w2, bias, c["epi"], c["R"], c["ksb"], c["U"], c["S"])
        want = (gr.K_DENSE, (c["M"] + 15) // 16, c["R"], c["epi"], c["ksb"], c["U"], 16, 0)
        if st != OK or rep != want:
            errors.append(f"status {st}, ran {rep}, expected {want}: {c}")
            continue
        seen.add(rep)
        _check(c, out, x, wi, bias, 32, errors, nl)
    _nonlinear_gate(nl, "dense", errors)
    return errors, seen


@functools.lru_cache(maxsize=None)
def _quant_sweep():
    errors, nl, seen = [], {}, set()
    for c in gr.quant_cases(V2):
        if not V2 and gr.q_expected(c["M"], c["epi"], c["R"], c["ksb"], c["G"], c["S"], True)[0] == gr.K_QSTREAM:
            continue                                         # the child process repeats only what the one-shot kernel took in the parent
        x, wi, a, b, bias = gr.quant_case_inputs(c)
        st, out, rep = gr.run_skinny_q(x, a, b, bias, c["bits"], c["sbt"], c["epi"], c["R"], c["ksb"], c["S"])
        kernel, U = c["expect"]
        want = (kernel, (c["M"] + 15) // 16, c["R"], c["epi"], c["ksb"], U, c["bits"], c["sbt"])
        if st != OK or rep != want:
            errors.append(f"status {st}, ran {rep}, the launcher's rule says {want}: {c}")
            continue
        seen.add(rep)
        _check(c, out, x, wi, bias, 64, errors, nl)
    _nonlinear_gate(nl, "quant" if V2 else "quant_streaming_only", errors)
    return errors, seen


def test_dense_every_arrangement_every_tail():
    """every GEMM_CASE x rows 1 .. 64, per-wave k-tile counts 0 .. 5 U + 1 (equal and unequal waves; KT = 9 and 13 among them), NT around
    multiples of R (tile clamp) and NT = 1, S in {1, 2, 3, KT}: partial slabs and bf16 outputs bit for bit, rows >= M exactly the bias or 0,
    no poison left, guards intact (the entry point fails otherwise)"""
    errors, _ = _dense_sweep()
    assert not errors, f"{len(errors)} failures, first: " + "\n".join(errors[:8])


def test_quantised_every_arrangement_every_share():
    """every QGEMM_CASE / QGEMM1_CASE, 8 and 4 bit, bf16 and f16 scales: streaming shares 0 .. 11 groups per wave, one-shot shares 1 .. 6 in buffers
    of 2, 4 and 6 (full and with dead groups), even and uneven splits, S == G; the entry point's report must name the kernel and buffer depth
    the launcher's rule gives.  With MIS_QGEMM_V2=0 (child process) the cases the one-shot kernel took run on the streaming kernel."""
    errors, seen = _quant_sweep()
    assert not errors, f"{len(errors)} failures, first: " + "\n".join(errors[:8])
    assert {r[0] for r in seen} == ({gr.K_QSTREAM, gr.K_QONESHOT} if V2 else {gr.K_QSTREAM})


def test_quantised_streaming_kernel_at_one_shot_shares():
    if not V2:
        return                                               # this IS the child process (which selects the sweep alone anyway)
    env = dict(os.environ, MIS_QGEMM_V2="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu", "-k",
                        "test_quantised_every_arrangement_every_share"], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_every_instantiation_of_the_launcher_tables_ran():
    _, dense = _dense_sweep()
    for (epi, R, ksb, U) in gr.DENSE_TABLE:
        for mt in ((1, 2) if R == 4 else (1, 2, 3, 4)):
            assert (gr.K_DENSE, mt, R, epi, ksb, U, 16, 0) in dense
    _, quant = _quant_sweep()
    for ((kernel, U), epi, R, ksb, bits, sbt, mt) in gr.quant_instantiations():
        if V2 or kernel == gr.K_QSTREAM:
            assert (kernel, mt, R, epi, ksb, U, bits, sbt) in quant, (kernel, mt, R, epi, ksb, U, bits, sbt)


def test_error_statuses_launch_nothing():
    x, w = gr.dense_inputs(4, 32, 128, 1)
    run = lambda M=4, **kw: gr.run_skinny(x[:1].repeat(M, 0), w, None, None, **dict(dict(epi=gr.EPI_PARTIAL, R=2, ksb=4, U=4, S=1), **kw))
    assert run()[0] == OK
    for want, kw in ((GENERATION_FAILED, dict(R=3)), (INVALID_INPUT, dict(S=5)), (GENERATION_FAILED, dict(epi=gr.EPI_BF16, S=2)),
                     (GENERATION_FAILED, dict(R=4, U=3, M=33)), (GENERATION_FAILED, dict(U=5))):
        st, _, rep = run(**kw)
        assert (st, rep[0]) == (want, -1), (kw, st, rep)
    a = gr.quant_inputs(4, 32, 128, 4, 2)
    runq = lambda M=4, sbt=0, **kw: gr.run_skinny_q(a[0][:1].repeat(M, 0), a, None, None, 4, sbt, **dict(dict(epi=gr.EPI_PARTIAL, R=2, ksb=4, S=1), **kw))
    assert runq()[0] == OK and runq(sbt=1)[0] == OK
    for kw in (dict(S=3), dict(R=4, M=33), dict(ksb=8, epi=gr.EPI_BF16, M=33), dict(sbt=1, R=1), dict(epi=gr.EPI_BF16, S=2), dict(R=3)):
        st, _, rep = runq(**kw)
        assert (st, rep[0]) == (GENERATION_FAILED, -1), (kw, st, rep)


def test_dequantise_then_dense_gives_the_same_bits():
    """s q + b is exact in bf16 for the generator's inputs (|q - m| <= 255 needs 8 significant bits), so the dense kernel on the dequantised
    matrix and the code-streaming kernels must agree bit for bit"""
    for i, (bits, G, M, S) in enumerate([(4, 1, 3, 1), (4, 13, 17, 1), (8, 6, 16, 2), (8, 43, 32, 1), (4, 64, 5, 3), (8, 64, 33, 1)]):
        a = gr.quant_inputs(M, 48, 64 * G, bits, 300 + i)
        st, q, _ = gr.run_skinny_q(a[0], a, None, None, bits, 0, gr.EPI_PARTIAL, 2, 4, S)
        st2, d, _ = gr.run_skinny(a[0], a[4], None, None, gr.EPI_PARTIAL, 2, 4, 4, S)
        assert st == OK and st2 == OK
        assert np.array_equal(q.sum(0).view(np.uint32), d.sum(0).view(np.uint32)) and _bits_equal(q.sum(0)[:M], a[0] @ a[4].T)


@pytest.mark.parametrize("N", [16, 48, 80])
def test_interleaved_packing_alternates_the_two_matrices(N):
    """k_pack_weight / k_pack_qweight with tile stride 2, offsets 0 and 1: n-tile 2 t of the result is tile t of the first matrix, 2 t + 1 of the second"""
    M, K = 5, 192
    x, w = gr.dense_inputs(M, N, K, 40 + N)
    w2 = gr.dense_inputs(M, N, K, 41 + N)[1]
    st, out, _ = gr.run_skinny(x, w, w2, None, gr.EPI_PARTIAL, 2, 4, 4, 1)
    assert st == OK
    t = out[0, :M].reshape(M, N // 16, 2, 16)
    assert _bits_equal(t[:, :, 0].reshape(M, N), x @ w.T) and _bits_equal(t[:, :, 1].reshape(M, N), x @ w2.T)
    for bits in (8, 4):
        a, b = gr.quant_inputs(M, N, K, bits, 50 + N), gr.quant_inputs(M, N, K, bits, 51 + N)
        st, out, _ = gr.run_skinny_q(a[0], a, b, None, bits, 0, gr.EPI_PARTIAL, 2, 4, 1)
        assert st == OK
        t = out[0, :M].reshape(M, N // 16, 2, 16)
        assert _bits_equal(t[:, :, 0].reshape(M, N), a[0] @ a[4].T) and _bits_equal(t[:, :, 1].reshape(M, N), a[0] @ b[4].T)


def test_prefill_gemm_exact():
    """k_gemm_pf: M x N x K of partial row blocks, partial and clamped n-tiles, 2 .. 16 k-steps.  PF_F32 bit for bit; PF_RESID against T(h + T(acc))
    (acc, and h + T(acc), are exact in float32, so the roundings are deterministic); rows >= M and columns >= N never written (guards)"""
    errors = []
    for M in gr.PF_M:
        for N in gr.PF_N:
            for K in gr.PF_K:
                x, w = gr.dense_inputs(M, N, K, M * 7 + N + K)
                st, out, rep = gr.run_pf(x, w, None, None, gr.PF_F32)
                if st != OK or rep[0] != gr.K_PF or not _bits_equal(out, x @ w.T):
                    errors.append(("f32", M, N, K, st))
    for (M, N, K, seed) in gr.PF_RESID_SHAPES:
        x, w = gr.dense_inputs(M, N, K, seed)
        h = np.random.default_rng(seed).integers(-64, 65, (M, N)).astype(np.float64) * 2.0 ** -5
        st, out, _ = gr.run_pf(x, w, None, h, gr.PF_RESID)
        if st != OK or not _bits_equal(out, gr.apply_resid(h, x @ w.T)):
            errors.append(("resid", M, N, K, st))
    nl = [0, 0, 0]
    for (M, N, K, seed) in gr.PF_SILU_SHAPES:
        e = gr.x_log2_for_std(K, gr.DENSE_W_RMS)
        x, w = gr.dense_inputs(M, N, K, seed, e)
        w2 = gr.dense_inputs(M, N, K, seed + 500000, e)[1]
        st, out, _ = gr.run_pf(x, w, w2, None, gr.PF_SILU)
        if st != OK or np.isnan(out).any():
            errors.append(("silu", M, N, K, st))
            continue
        d = gr.bf16_ulp_distance(out, gr.apply_epilogue(gr.EPI_SILU_MUL, x @ gr.interleave(w, w2).T))
        nl[0] += int((d != 0).sum()); nl[1] += d.size; nl[2] = max(nl[2], int(d.max()))
    record("gemm_ops_prefill_silu", share_differing=nl[0] / nl[1], worst_ulp=nl[2], elements=nl[1])
    assert not errors, errors[:10]
    assert nl[2] <= 2 and nl[0] / nl[1] <= 0.01, nl


def _gauss_bf16(rng, shape, amp=1.0):
    return gr.bf16_value(gr.bf16_bits((rng.standard_normal(shape) * amp).astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize("K", [1024, 2752])
def test_gaussian_data_within_the_float32_summation_bound(K):
    """what integer data cannot catch - accumulation in less than float32.  |dev - ref64| <= 2 gamma_K sum_k |x_k| |w_k|, gamma_K = K u / (1 - K u),
    u = 2^-24 (derived: the standard bound of a float32 sum of K exact products in any order; the factor 2 because the MFMA's internal
    addition order and rounding are not documented as IEEE per add), plus half a bf16 ulp of the reference (2^-8 |ref|) for bf16 outputs"""
    rng = np.random.default_rng(K)
    M, N = 33, 96
    gam = 2.0 * (K * 2.0 ** -24) / (1.0 - K * 2.0 ** -24)
    x, w = _gauss_bf16(rng, (M, K)), _gauss_bf16(rng, (N, K), 0.05)
    ref, mag = x @ w.T, np.abs(x) @ np.abs(w).T
    worst = {}
    st, out, _ = gr.run_skinny(x, w, None, None, gr.EPI_PARTIAL, 2, 4, 4, 1)
    assert st == OK
    worst["dense_f32"] = float((np.abs(out[0, :M] - ref) / (gam * mag)).max())
    st, out, _ = gr.run_skinny(x, w, None, None, gr.EPI_BF16, 2, 4, 4, 1)
    assert st == OK
    worst["dense_bf16"] = float((np.abs(out[:M] - ref) / (gam * mag + 2.0 ** -8 * np.abs(ref))).max())
    st, out, _ = gr.run_pf(x, w, None, None, gr.PF_F32)
    assert st == OK
    worst["prefill_f32"] = float((np.abs(out - ref) / (gam * mag)).max())
    for bits in (8, 4):
        words, sc, bi = mq.quantize(w.astype(np.float32), 64, bits)
        sc, bi = gr.bf16_value(gr.bf16_bits(sc)).astype(np.float64), gr.bf16_value(gr.bf16_bits(bi)).astype(np.float64)
        q = np.stack([(words >> np.uint32(bits * j)) & np.uint32(2 ** bits - 1) for j in range(32 // bits)], -1).reshape(N, K).astype(np.float64)
        sq, bb = np.repeat(sc, 64, 1) * q, np.repeat(bi, 64, 1)
        refq, magq = x @ (sq + bb).T, np.abs(x) @ (np.abs(sq) + np.abs(bb)).T
        for M2 in (16, M):                                   # 16 rows: the one-shot kernel at K = 1024 (4 groups per wave), else the streaming one
            a = (x[:M2], q.astype(np.int64), sc, bi, sq + bb)
            st, out, rep = gr.run_skinny_q(a[0], a, None, None, bits, 0, gr.EPI_PARTIAL, 2, 4, 1)
            assert st == OK
            worst[f"quant{bits}_kernel{rep[0]}_mt{rep[1]}"] = float((np.abs(out[0, :M2] - refq[:M2]) / (gam * magq[:M2])).max())
    for k, v in worst.items():
        record(f"gemm_ops_gaussian_K{K}_{k}", fraction_of_bound=v)
    assert max(worst.values()) <= 1.0, worst
