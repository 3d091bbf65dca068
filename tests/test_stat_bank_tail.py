"""The table behind a push's entries of the Kaldi and the NeMo / Parakeet stream bank (mel_spec_amd/csrc/stat_bank_tail.hpp): the bank's
own table (continues u32[n]; len u64[n] then org0 i32[n]) and TypedTail, which for a push with 16-bit rows appends the plan's packed
offsets at the own size rounded up to 8 -- n in {1, 2, 3, 5, 8}, both banks: tests/cpp/stat_bank_tail_host.cpp.  Built plain and with
-fsanitize=address,undefined; a stand-alone program, no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stat_bank_tail_host(tmp_path, sanitize):
    exe = tmp_path / "stat_bank_tail_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "stat_bank_tail_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("stat_bank_tail_host: ok"), p.stdout + p.stderr
