"""From a config to the kernel it runs: tests/cpp/reach512_host.cpp builds the tables of the create calls (fbank_tables.hpp), takes the
shape of the object with the library's own rule (reach512 / shape512, mel_spec_amd/csrc/fused512_route.hpp) and prints route512's kernel
per kind of batch.  The configs and the expected K512 names are the list the GPU tests of the four-wave kernels declare
(tests/test_four_wave.REACH): one list.  Built plain and with -fsanitize=address,undefined; a stand-alone program, no GPU."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_four_wave import KALDI_BINS, NEMO_HOLES, NEMO_MELS, REACH, W512

LDS_LIMIT = 160 * 1024
SLICE = 17408


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def reach(request, tmp_path_factory):
    sanitize = request.param
    exe = tmp_path_factory.mktemp("reach512") / "reach512_host"
    flags = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "reach512_host.cpp"), "-o", str(exe)])

    def run(*args):
        p = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.rstrip().endswith("reach512_host: ok"), p.stdout + p.stderr
        return p.stdout.splitlines()[:-1]
    run.sanitize = sanitize
    return run


def _fields(line):
    key, *rest = line.split()
    return key, {k: (int(v) if v.isdigit() else v) for k, v in (f.split("=") for f in rest if "=" in f)}


def test_configs_of_the_gpu_tests_reach_their_kernels(reach):
    """every config of test_four_wave.REACH: blob bytes, waves, fused, the LDS of the launch and the kernel per kind of batch"""
    got = dict(_fields(line) for line in reach(*REACH))
    assert set(got) == set(REACH)
    for key, want in REACH.items():
        g = got[key]
        flavor = key.split(":")[0]
        assert g["tables"] == 1 and g["fused"] == 1, (key, g)
        assert (g["blob"], g["waves"], g["plain"], g["layout"], g["stream"]) == (want["blob"], want["waves"], want["plain"], want["layout"], want["stream"]), (key, g)
        per_wave, tail = SLICE + (512 if flavor == "whisper" else 0), 64 if flavor == "nemo" else 0
        lds = g["blob"] + g["waves"] * per_wave + tail
        assert g["lds"] == lds <= LDS_LIMIT and g["lds"] == want.get("lds", lds), (key, g)
        # four waves exactly when eight do not fit; then no workgroup-per-clip kernel, no 16-bit kernel, no split output
        assert (g["blob"] + 8 * per_wave + tail > LDS_LIMIT) == (g["waves"] == 4), (key, g)
        if g["waves"] == 4:
            assert (g["clip"], g["clip_ragged"], g["io"], g["stats"], g["clip_shape_ok"]) == ("kNone", "kNone", "kNone", "kNone", 0), (key, g)
    # the GPU tests' parameters are on the kernels they are there for
    for b in KALDI_BINS:
        assert (REACH[f"kaldi:16000:{b}"]["plain"], REACH[f"kaldi:16000:{b}"]["stream"]) == (("kKaldiRt4", "kStreamRt4") if b < 5 else ("kKaldiRtRuns", "kStreamRt"))
    for m in NEMO_MELS:
        assert REACH[f"nemo:16000:{m}"]["layout"] == ("kNemoRt6x4" if m < 5 else "kNemoRt6")
    for sr, m in NEMO_HOLES:
        assert REACH[f"nemo:{sr}:{m}"]["layout"] == "kNemoRt6x4" and REACH[f"nemo:{sr}:{m}"]["blob"] == 24576
    for hop, m, sr in W512:
        assert REACH[f"whisper:{int(sr)}:{m}"]["plain"] == ("kWRt6Runs" if m == 9 else "kWRt6x4")


def test_which_bin_counts_take_four_waves(reach):
    """the rows of the table: at 16 kHz Kaldi and NeMo banks of 1 .. 4 bins and Whisper banks of 1 .. 8, 15 and 16 mels are on four waves,
    their neighbours on eight; at 8 kHz the Whisper flavour is on four waves up to 6 mels"""
    def waves(flavor, sr, counts):
        return {n: _fields(line)[1]["waves"] for n, line in zip(counts, reach(*[f"{flavor}:{sr}:{n}" for n in counts]))}
    assert waves("kaldi", 16000, range(1, 9)) == {n: (4 if n <= 4 else 8) for n in range(1, 9)}
    assert waves("nemo", 16000, range(1, 9)) == {n: (4 if n <= 4 else 8) for n in range(1, 9)}
    assert waves("whisper", 16000, range(1, 25)) == {n: (4 if n <= 8 or n in (15, 16) else 8) for n in range(1, 25)}
    assert waves("whisper", 8000, range(1, 13)) == {n: (4 if n <= 6 else 8) for n in range(1, 13)}
    assert waves("whisper", 16000, [40, 64, 80, 128, 140]) == {n: 8 for n in (40, 64, 80, 128, 140)}


def test_sweeps(reach):
    """(a) NeMo banks of 1 .. 16 mels at 4 .. 48 kHz, Slaney and HTK: every fused object's launch fits 160 KiB (the program checks each), and
    the banks whose blob is exactly 24 576 bytes -- 165 of them -- run fused on four waves; (b) 90 .. 149 mels at 4 .. 96 kHz, Slaney and HTK,
    two f_min values, NeMo and Whisper: none is on four waves, so kNemoRt10x4 and kWRt10x4 are not reachable.  The sanitized build walks
    every eighth rate."""
    few, many = (_fields(line)[1] for line in reach("--sweep-coarse" if reach.sanitize else "--sweep"))
    assert few["four_wave"] > 0 and few["holes"] == (17 if reach.sanitize else 165), few
    assert many["configs"] == (5760 if reach.sanitize else 44640) and many["four_wave"] == 0 and many["ten_slot_four_wave"] == 0 and many["largest_blob"] == 16384, many
