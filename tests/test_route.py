"""route400 (mel_spec_amd/csrc/ctx_route.hpp), the one function the n_fft = 400 contexts take a batch's unit size, its launches and
the reported kernel name from: tests/cpp/route_host.cpp on the host -- the seven context shapes of the whole-batch matrix against a
literal table, and the invariants of the decision over every combination of its inputs.  Built plain and with
-fsanitize=address,undefined; a stand-alone program, no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_route_host(tmp_path, sanitize):
    exe = tmp_path / "route_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "route_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("route_host: ok"), p.stdout + p.stderr
