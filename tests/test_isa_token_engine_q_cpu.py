"""CPU tier: the compiled code-streaming token engine (csrc/token_engine_q.hip, k_token_engine_q<xcds, bits, head_q>) keeps the dense
kernel's register bounds (tests/test_isa_cpu.py::test_token_engine_keeps_its_tile_buffers_in_registers): at most 256 VGPRs, no scratch
on 2 / 4 / 8 XCDs, on 1 XCD no more scratch than the dense kernel's bound, and the barrier the two programs meet at waits for LDS traffic
only.  All sixteen instantiations must exist (1 / 2 / 4 / 8 XCDs x 8 / 4 bit x head as codes / dense)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlx-audio-swift_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def compiled():
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "k.s")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                            os.path.join(CSRC, "token_engine_q.hip"), "-o", asm, "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(asm).read()
    use, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = use.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        m = re.search(r"remark:\s+VGPRs: (\d+)", line)
        if m:
            cur["vgprs"] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            cur["scratch"] = int(m.group(1))
    return text, {k: v for k, v in use.items() if "k_token_engine_q" in k}


def test_every_instantiation_is_built(compiled):
    _, eng = compiled
    want = {f"ILi{x}ELi{b}ELb{h}E" for x in (1, 2, 4, 8) for b in (8, 4) for h in (0, 1)}
    got = {re.search(r"ILi\d+ELi\d+ELb\dE", k).group(0) for k in eng}
    assert got == want, sorted(got)


def test_register_and_scratch_bounds(compiled):
    _, eng = compiled
    for k, v in eng.items():
        one = "ILi1E" in k
        assert v["vgprs"] <= 256, (k, v)
        assert v["scratch"] <= (256 if one else 0), (k, v)


def test_barriers_wait_for_lds_only(compiled):
    text, eng = compiled
    for name in [k for k in eng if k.startswith("_ZN12_GLOBAL__N_116k_token_engine_qILi4E")]:
        i = text.index("\n" + name + ":")
        body = [l.strip() for l in text[i: text.index(".Lfunc_end", i)].split("\n")]
        waits = [body[j - 1] for j, l in enumerate(body) if l.startswith("s_barrier") and j > 0]
        assert len(waits) >= 40, name
        assert sum(1 for w in waits if w.startswith("s_waitcnt") and "vmcnt" not in w) >= 0.9 * len(waits), (name, waits[:8])
