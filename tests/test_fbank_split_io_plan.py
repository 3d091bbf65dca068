"""The host side of the Kaldi fbank's split output for ragged batches and with 16-bit ends that is arithmetic only
(mel_spec_amd/csrc/fbank_split_io_plan.hpp): tests/cpp/fbank_split_io_host.cpp checks, against literal tables, the io codes, the order of
the argument verdicts and the side table's slots -- exactly ten kernels, every slot once, no new K512.  Built plain and with
-fsanitize=address,undefined; a stand-alone program, no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_fbank_split_io_host(tmp_path, sanitize):
    exe = tmp_path / "fbank_split_io_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fbank_split_io_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("fbank_split_io_host: ok"), p.stdout + p.stderr
