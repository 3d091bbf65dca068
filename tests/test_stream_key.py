"""What the stream banks' planners share (mel_spec_amd/csrc/stream_plan.hpp): the admission of a push's entries -- id range, once per
push, max_chunk, through the Whisper and the Kaldi planner -- and the key under which the Whisper bank keeps its last plan for the
pushes that repeat it, against a hit / miss pattern written out by hand: tests/cpp/stream_key_host.cpp.  Built plain and with
-fsanitize=address,undefined; a stand-alone program, no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stream_key_host(tmp_path, sanitize):
    exe = tmp_path / "stream_key_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "stream_key_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("stream_key_host: ok"), p.stdout + p.stderr
