"""csrc/step_loop.h - run_frame_loop, the frame loop that Marvis and Qwen3-TTS share - checked by a stand-alone program
(tests/step_loop_main.cpp) built with the address and undefined-behaviour sanitizers: the loop is driven by recording fakes and its full
call trace (launch groups, chunk boundaries, done copy / pre_sync / synchronise / poll, done before cancel, loop_done and the tail boundary,
a throwing frame body) is compared with traces written out as constants.  Host code only; no device is opened."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_step_loop_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "step_loop_check")
    build = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function",
                            "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "step_loop_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "step_loop ok" in run.stdout, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
