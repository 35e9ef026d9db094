"""csrc/lm_tensor_roles.h - what a checkpoint key of a Llama-shaped LM is, and which keys a configuration requires - checked by a
stand-alone program (tests/lm_tensor_roles_main.cpp) built with the address and undefined-behaviour sanitizers.  For two sets of
dimensions (untied; tied with qk_norm, head_dim 64, vocabulary 100) every required name is held to the kind, layer, shape, packed role,
role rows, tile stride and tile offset the LM engine places it with, the enumeration to the list, keys and amplitudes of the synthetic
initialisers, and malformed names to the three ways of being unknown (unexpected tensor, bad tensor name, layer index out of range).
Host code only; no device is opened."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_lm_tensor_roles_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lm_tensor_roles_check")
    build = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                            "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "lm_tensor_roles_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "lm_tensor_roles ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
