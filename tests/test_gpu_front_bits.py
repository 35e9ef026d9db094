"""-m gpu: the outputs of the small audio engines on synthetic models, bit for bit against tests/golden/front_bits.json.

The FFT twiddles, the filter bin ranges and the block reductions are shared between engines (csrc/audio_front.h, csrc/common.h), and the
FFT and exact-f32 MFMA loops exist once per engine, word for word; the file was recorded before anything was shared, so a change to a
shared piece, or to one copy, that moves a bit of any engine fails here.
tools/record_front_bits.py holds the cases (and says which path each shape reaches) and regenerates the file when numerics change on
purpose."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_front_bits", os.path.join(ROOT, "tools", "record_front_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "front_bits.json")) as f:
        return json.load(f)


def test_the_golden_file_covers_every_engine():
    assert sorted(_golden()) == sorted(_tool().ENGINES)


@pytest.mark.parametrize("engine", ["lasr", "fsmn_vad", "ecapa_lid", "moonshine"])
def test_outputs_match_the_recorded_bits(engine):
    want, got = _golden()[engine], _tool().ENGINES[engine]()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], f"{engine}.{name}: {got[name]} != recorded {want[name]}"
