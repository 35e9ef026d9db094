"""-m gpu: the outputs of the small audio engines on synthetic models, bit for bit against tests/golden/front_bits.json.

The FFT twiddles, the filter bin ranges and the block reductions are shared between engines (csrc/audio_front.h, csrc/common.h), and so
are pieces of the exact-f32 MFMA contraction of the four f32 engines (csrc/f32_tile.h: the 16-step MFMA loop, the zero-tile exit, the
C/D row map) with the per-frame mean / rstd of common.h; the staging loops of the contractions and the FFT butterfly loops exist once
per engine.  What these engines promise is a row's bits in any batch, and the time: after a change to a shared piece, or to one copy,
no output may move.  Every entry was recorded from kernels that shared none of this (mossformer2 and sortformer from each file's own
copy of the contraction, before f32_tile.h), so a change to a shared piece, or to one kernel, that moves a bit of any engine fails here.
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


@pytest.mark.parametrize("engine", ["lasr", "fsmn_vad", "ecapa_lid", "moonshine", "mossformer2", "sortformer"])
def test_outputs_match_the_recorded_bits(engine):
    want, got = _golden()[engine], _tool().ENGINES[engine]()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], f"{engine}.{name}: {got[name]} != recorded {want[name]}"
