"""csrc/host_weights.h - the host weight stash every codec / STT / VAD engine stages its checkpoint in, the host arena builder and the
synthetic-tensor helper - checked by a stand-alone program (tests/host_weights_main.cpp) built with the address and undefined-behaviour
sanitizers: dtype widening against constants, need()'s statuses and messages, shape rejection, replacement, arena offsets / zero fill /
round-to-nearest-even, the arena's bindings (resolve() against fake bases: base + offset for every bound pointer, nullptr for an
unbound one, one offset bound twice, the two arenas independently), fold_bn_dwconv with and without a conv bias, the NeMo front end's
host tables of csrc/audio_front.h (hann_padded, slaney_filterbank at 80 and 128 mels against the formulas in double, the ranges against
filter_bin_ranges), the synthetic key sequence; the codec engines' F32Arena (offsets, zero padding, lin / conv and their messages) and
the weight re-layouts and quantiser-table fold, each against its index formula written out.  Host code only; no device is opened."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_host_weights_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_weights_check")
    build = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                            "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "host_weights_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "host_weights ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
