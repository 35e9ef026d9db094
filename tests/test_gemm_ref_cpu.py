"""tests/gemm_ref.py is what tests/test_gpu_gemm_ops.py holds the GEMM kernels to, bit for bit - so its own claims are proven here, on the CPU:
the exact-input generators give sums that do not depend on the float32 summation order, and on the inputs of the non-linear-epilogue
cases a float32 realisation of the rounding-point specification differs from the float64 reference on fewer than 0.1 % of the elements
(which is what entitles the GPU test to cap the device's share at 1 %)."""
import numpy as np
import pytest

import gemm_ref as gr


def _orders_f32(terms, rng, n_orders=4):
    """sums of float32 terms [..., k] along k in several orders: sequential, numpy's pairwise, and random permutations cut into random chunks
    (chunk sums pairwise, chunk totals sequential) - the shapes a split over waves, slabs and MFMA blocks can take"""
    terms = np.ascontiguousarray(terms, np.float32)
    K = terms.shape[-1]
    yield np.cumsum(terms, axis=-1, dtype=np.float32)[..., -1]
    yield np.add.reduce(terms, axis=-1, dtype=np.float32)
    for _ in range(n_orders):
        p = terms[..., rng.permutation(K)]
        cuts = np.sort(rng.choice(np.arange(1, K), size=min(K - 1, int(rng.integers(1, 9))), replace=False)) if K > 1 else np.array([], int)
        parts = [np.add.reduce(c, axis=-1, dtype=np.float32) for c in np.split(p, cuts, axis=-1)]
        yield np.cumsum(np.stack(parts, -1), axis=-1, dtype=np.float32)[..., -1]


@pytest.mark.parametrize("K,x_log2", [(32, -5), (416, -5), (4096, -5), (4096, -8), (32, -2), (2784, -6)])
def test_dense_generator_sums_are_order_independent(K, x_log2):
    """K up to 4096 and every x amplitude the cases use (x_log2_for_std gives -2 .. -8 between K = 32 and K = 4096)"""
    rng = np.random.default_rng(K)
    x, w = gr.dense_inputs(3, 16, K, seed=K + x_log2, x_log2=x_log2)
    gr.exact_bits(x), gr.exact_bits(w)                                   # representable in bf16
    bias = gr.out_bias(16, K)
    y64 = x @ w.T + bias[None, :]
    assert np.array_equal(y64.astype(np.float32).astype(np.float64), y64)
    terms = np.concatenate([(x[:, None, :] * w[None, :, :]), np.broadcast_to(bias[None, :, None], (3, 16, 1))], axis=-1)
    assert np.array_equal(terms.astype(np.float32).astype(np.float64), terms)      # bf16 x bf16 products are exact
    for y32 in _orders_f32(terms, rng):
        assert np.array_equal(y32.view(np.uint32), y64.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("bits,sbd", [(8, gr.MIS_BF16), (4, gr.MIS_BF16), (8, gr.MIS_F16), (4, gr.MIS_F16)])
@pytest.mark.parametrize("K,x_log2", [(64, -5), (4096, -5), (6080, -5), (4096, -1), (64, 3)])
def test_quant_generator_sums_are_order_independent(bits, sbd, K, x_log2):
    """the kernel's arithmetic - per group sc * sum(x q) + bi * sum(x), groups added in any order - and the dequantised form sum x (s q + b)
    both equal the float64 value in every order; scales, biases and s q + b are exact in bf16 and f16"""
    rng = np.random.default_rng(K + bits)
    x, q, sc, bi, w = gr.quant_inputs(2, 16, K, bits, seed=K + bits, x_log2=x_log2)
    gr.exact_bits(sc, sbd), gr.exact_bits(bi, sbd), gr.exact_bits(w), gr.exact_bits(x)
    G = K // 64
    y64 = x @ w.T
    want = y64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), y64)
    xq = (x[:, None, :] * q[None, :, :]).reshape(2, 16, G, 64)
    xs = np.broadcast_to(x[:, None, :], (2, 16, K)).reshape(2, 16, G, 64)
    for ag, sx in zip(_orders_f32(xq, rng), _orders_f32(xs, np.random.default_rng(1))):
        per_group = sc.astype(np.float32)[None] * ag + bi.astype(np.float32)[None] * sx         # float32 arithmetic throughout
        assert per_group.dtype == np.float32
        for y32 in _orders_f32(per_group, rng, 2):
            assert np.array_equal(y32.view(np.uint32), want.view(np.uint32))
    for y32 in _orders_f32(x[:, None, :] * w[None, :, :], rng, 2):
        assert np.array_equal(y32.view(np.uint32), want.view(np.uint32))


def test_bf16_rounding_of_the_reference_is_round_to_nearest_even():
    v = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.140625, 1e-40, 0.0, 255.5, 256.5 * 2.0 ** -9])
    got = gr.T(v)
    want = gr.bf16_value(gr.bf16_bits(v.astype(np.float32))).astype(np.float64)            # these are exact in float32: one rounding either way
    assert np.array_equal(got, want)
    assert gr.T(np.array([1.0 + 2.0 ** -8 + 2.0 ** -40]))[0] == 1.0 + 2.0 ** -7            # above the tie: up (a float32 detour would round to even)
    assert list(gr.bf16_ulp_distance(np.array([1.0, -0.0]), np.array([1.0078125, 0.0]))) == [1, 0]


def _nonlinear_share(cases, inputs, unit):
    tot = {e: [0, 0] for e in gr.NONLINEAR}
    stds = []
    for c in cases:
        if c["epi"] not in gr.NONLINEAR:
            continue
        x, wi, _, _, bias = inputs(c)
        acc = gr.ref_slabs(x, wi, 1, unit)[0]
        stds.append((float(acc.std()), c["epi"], float(acc.min()), acc.size))
        r64, r32 = gr.apply_epilogue(c["epi"], acc, bias, 64), gr.apply_epilogue(c["epi"], acc, bias, 32)
        d = gr.bf16_ulp_distance(r64, r32)
        assert d.max() <= 1
        tot[c["epi"]][0] += int((d != 0).sum())
        tot[c["epi"]][1] += d.size
    return tot, stds


@pytest.mark.parametrize("family", ["dense", "quant"])
def test_nonlinear_epilogue_inputs_keep_float32_and_float64_references_together(family):
    cases, inputs, unit = (gr.dense_cases(), gr.dense_case_inputs, 32) if family == "dense" else (gr.quant_cases(), gr.quant_case_inputs, 64)
    tot, stds = _nonlinear_share(cases, inputs, unit)
    for epi, (bad, n) in tot.items():
        if family == "quant" and epi == gr.EPI_SILU_PACKED:
            assert n == 0                                      # the code-streaming kernels have no such epilogue
            continue
        assert n > 20000, (epi, n)
        print(family, "epilogue", epi, "float32 vs float64 reference: share", bad / n, "of", n)
        assert bad / n < 1e-3, (epi, bad, n)
    # not saturated, not vanishing: standard deviation of the pre-activations between 1 and 3.  GELU inputs are also kept above -4 (see
    # gemm_ref.gelu_safe_shift) by halving x no more often than that takes: where it was halved the smallest pre-activation lies in [-4, -2)
    # (the smallest cases have 16 or 32 outputs of one or two scale groups, whose sample deviation scatters: they are held to 0.7 .. 4)
    for s, epi, lo, n in stds:
        assert s <= (3.0 if n >= 512 else 4.0) and (s >= (1.0 if n >= 512 else 0.7) or (epi == gr.EPI_GELU_PACKED and -4.0 <= lo < -2.0)), (s, epi, lo, n)


def test_prefill_nonlinear_inputs():
    tot = [0, 0]
    for (M, N, K, seed) in gr.PF_SILU_SHAPES:
        e = gr.x_log2_for_std(K, gr.DENSE_W_RMS)
        x, w = gr.dense_inputs(M, N, K, seed, e)
        w2 = gr.dense_inputs(M, N, K, seed + 500000, e)[1]
        acc = x @ gr.interleave(w, w2).T
        assert 1.0 <= acc.std() <= 3.0
        d = gr.bf16_ulp_distance(gr.apply_epilogue(gr.EPI_SILU_MUL, acc, None, 64), gr.apply_epilogue(gr.EPI_SILU_MUL, acc, None, 32))
        tot[0] += int((d != 0).sum()); tot[1] += d.size
    assert tot[0] / tot[1] < 1e-3, tot


def test_case_tables_cover_every_row_tile_count_of_every_arrangement():
    """the case lists reach (arrangement, MT) for every instantiation the launcher tables name"""
    d = {(c["epi"], c["R"], c["ksb"], c["U"], (c["M"] + 15) // 16) for c in gr.dense_cases()}
    for (epi, R, ksb, U) in gr.DENSE_TABLE:
        for mt in ((1, 2) if R == 4 else (1, 2, 3, 4)):
            assert (epi, R, ksb, U, mt) in d
    q = {(c["expect"], c["epi"], c["R"], c["ksb"], c["bits"], c["sbt"], (c["M"] + 15) // 16) for c in gr.quant_cases()}
    for want in gr.quant_instantiations():
        assert want in q, want
