"""The decoder core of k_inflate_bgzf (2fast2q_amd/csrc/f2q_inflate_kernels.h), compiled for the host with the
wave-parallel steps as lane loops, against zlib under ASan + UBSan.  Host only; the checker is
tests/emu/inflate_dev_fuzz.cpp."""
import os
import struct
import subprocess

import pytest

import inflate_cases as IC
from conftest import sprinkle_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "inflate_dev_fuzz.cpp")
BIN = os.path.join(HERE, "emu", "inflate_dev_fuzz.bin")
HDR = os.path.join(os.path.dirname(HERE), "2fast2q_amd", "csrc", "f2q_inflate_kernels.h")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


@pytest.fixture(scope="module")
def fuzz_bin():
    if not os.path.exists(BIN) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(BIN):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", BIN, SRC, "-lz"])
    return BIN


def test_core_equals_zlib_on_the_corpus(fuzz_bin):
    """synthetic FASTQ, random bytes, distance-1 runs, periodic text; levels 0 1 6 9; default, fixed, Huffman-only, RLE
    and filtered strategies; empty members and members of exactly 65536 bytes"""
    res = subprocess.run([fuzz_bin, "corpus"], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:]
    assert res.stdout.startswith("ok "), res.stdout


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_core_rejects_what_zlib_rejects(fuzz_bin, seed):
    """bit flips, cut-off payloads, overwritten bytes, a byte before the trailer: accept / reject as zlib does, the same
    bytes when both accept, no sanitizer finding, no hang"""
    res = subprocess.run([fuzz_bin, "fuzz", "1500", str(seed)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:]
    assert res.stdout.startswith("ok 1500 "), res.stdout


def test_core_names_each_kind_of_damage(fuzz_bin, tmp_path):
    import synth
    text = sprinkle_symbols(synth.make_fastq(synth.Spec(seed=3, n_reads=200, read_len=100), synth.make_library(20, 20, 1)), 1)[:60000]
    cases = IC.damaged(text)
    good = [IC.member(text, lv) for lv in (0, 1, 6, 9)] + [IC.member(b""), IC.member(b"A" * 65536, 9)]
    path = tmp_path / "members.bin"
    path.write_bytes(b"".join(struct.pack("<I", len(m)) + m for m in good + [m for m, _ in cases.values()]))
    res = subprocess.run([fuzz_bin, "file", str(path)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:]
    got = [int(x) for x in res.stdout.split()]
    assert got[:len(good)] == [IC.OK] * len(good)
    for (name, (_, want)), st in zip(cases.items(), got[len(good):]):
        assert st != IC.OK and (want is None or st == want), (name, st, want)
