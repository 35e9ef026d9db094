"""-m gpu: the bf16 big GEMMs on Gaussian-like operands, bit for bit against tests/golden/bf16_gemm_bits.json.

k_gemm_big (csrc/whisper_kernels.hip) and k_lasr_gemm (csrc/lasr.hip) share the register-staged main loop of csrc/bf16_tile.h;
k_gemm_big / k_gemm_big2 / k_gemm_big3 share one epilogue, and all four the bf16 quad pack.  The operator tests compare bit for bit
only on operands whose sums are exact in any order; here the sums round, so a change to the k order, to a rounding point or to the
staging of an edge tile moves a hash.  The hashes were recorded from the kernels before they shared anything, each with its own copy
of the loop and the epilogue.  tools/record_bf16_gemm_bits.py holds the cases (and says which path each shape reaches) and
regenerates the file when numerics change on purpose."""
import importlib.util
import json
import os

import pytest

import enc_ref as er
import lasr_ops_ref as lo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_bf16_gemm_bits", os.path.join(ROOT, "tools", "record_bf16_gemm_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "bf16_gemm_bits.json")) as f:
        return json.load(f)


def test_the_golden_file_names_every_case_and_every_instantiation():
    golden, tool = _golden(), _tool()
    assert sorted(golden) == sorted(tool.cases())
    ran = {tuple(v["ran"]) for v in golden.values()}
    assert {r for r in ran if len(r) == 4} == er.GEMM_INSTANTIATIONS
    assert {r for r in ran if len(r) == 2} == lo.GEMM_INSTANTIATIONS and len(lo.GEMM_INSTANTIATIONS) == 10


def test_outputs_match_the_recorded_bits():
    golden, errors = _golden(), []
    for name, fn in sorted(_tool().cases().items()):
        got = fn()
        if got != golden[name]:
            errors.append(f"{name}: {got} != recorded {golden[name]}")
    assert not errors, "\n".join(errors)
