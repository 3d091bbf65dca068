"""The side of the resampler that is arithmetic only (mel_spec_amd/csrc/resample_plan.hpp): tests/cpp/resample_plan_host.cpp checks the
geometry and the per-phase inside ranges against brute force for nine rate pairs, the kernel's tap windows against the dense table, and
the tiles (every output covered once, every span holding its outputs' windows, no read outside the clip), also with offsets and lengths
near 2^40.  Built plain and with -fsanitize=address,undefined; a stand-alone program, no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_resample_plan_host(tmp_path, sanitize):
    exe = tmp_path / "resample_plan_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "resample_plan_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("resample_plan_host: ok"), p.stdout + p.stderr
