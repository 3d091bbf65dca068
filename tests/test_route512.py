"""route512 (mel_spec_amd/csrc/fused512_route.hpp), the one function the fused 512-point family -- the Kaldi fbank object, the NeMo
frontend, Whisper at n_fft = 512 -- takes a batch's kernel, waves, LDS size and grid rule from: tests/cpp/route512_host.cpp on the host --
the objects the GPU suite builds against a literal table, the invariants of the decision over every combination of its inputs, and the
clip kernel's eligibility rules.  Built plain and with -fsanitize=address,undefined; a stand-alone program, no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_route512_host(tmp_path, sanitize):
    exe = tmp_path / "route512_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "route512_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("route512_host: ok"), p.stdout + p.stderr
