"""The host side of the centred Whisper features that is arithmetic only (mel_spec_amd/csrc/whisper_centered_plan.hpp):
tests/cpp/whisper_centered_host.cpp checks, against literal tables and against the definition sample by sample, the frame count, the class
of every frame, the gather rule, the interior table, the edge list and the order of the argument verdicts.  Built plain and with
-fsanitize=address,undefined; a stand-alone program, no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_whisper_centered_host(tmp_path, sanitize):
    exe = tmp_path / "whisper_centered_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "whisper_centered_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("whisper_centered_host: ok"), p.stdout + p.stderr
