"""-m gpu: what tiny models compute after every way of loading LM and MLX-quantised tensors, bit for bit against
tests/golden/lm_load_bits.json.

Which checkpoint key lands where (csrc/lm_tensor_roles.h) and how a quantised tensor is checked, staged and dequantised
(csrc/quant_intake.h) is host code shared by the LM handle, Whisper, Qwen3-TTS, Marvis and Soprano.  The golden file was recorded from
the engines as they were before the two headers existed, so a change to either, or to one engine's use of it, that moves a bit of any
model's output fails here.  tools/record_lm_load_bits.py holds the cases (and says which path each one reaches) and regenerates the file
when numerics change on purpose."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_lm_load_bits", os.path.join(ROOT, "tools", "record_lm_load_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "lm_load_bits.json")) as f:
        return json.load(f)


CASES = sorted(_tool().CASES)


def test_the_golden_file_covers_every_case():
    assert sorted(_golden()) == CASES


@pytest.mark.parametrize("case", CASES)
def test_outputs_match_the_recorded_bits(case):
    want, got = _golden()[case], _tool().CASES[case]()
    assert got == want, f"{case}: {got} != recorded {want}"
