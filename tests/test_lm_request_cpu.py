"""csrc/lm_request.h - the two pure pieces of the Orpheus / VyvoTTS / Soprano generate call - checked by a stand-alone program
(tests/lm_request_main.cpp) built with the address and undefined-behaviour sanitizers: build_lm_request (left-padded prompt matrix,
all_ids, repetition windows of a ragged batch, both argument errors) and snac_decode_plan (order and grouping of the codec sub-batches:
fast path, rows grouped by code count, chunked rows) are compared with arrays and plans written out as constants.  Host code only; no
device is opened."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_lm_request_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lm_request_check")
    build = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                            "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "lm_request_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "lm_request ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
