"""Extract+Count keys one base apart collapsed, without a GPU: the per-lane functions of f2q_ec_collapse (ec64_find,
ecc_probe, ecc_parent_lane, ecc_root_lane of f2q_device.h) compiled for the host by tests/emu/f2q_ec_collapse_emu.cpp, in
the lane-per-slot form and in the wave-cooperative round of k_ec_parent, against the plain-Python rule of
tests/ec_collapse_cases.py; the shapes of the GPU list checked for what they hold; the command line's flags and refusals;
the header against the binding's export list."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import ec_collapse_cases as EC
import emu_helper
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_ec_collapse_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_ec_collapse_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
_L = None


def _lib():
    global _L
    if _L is None:
        deps = [SRC, os.path.join(TESTS, "emu", "f2q_emu.cpp")] + [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h", "f2q_synth.h", "f2q_reader.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                                   "-o", LIB, SRC, "-lz", "-lpthread"])
        _L = C.CDLL(LIB)
        _L.ecemu_collapse.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    return _L


def emu_collapse(table, ratio, dist=1, wave=0, bits=None):
    """({key: (centroid, cluster_reads)}, extra) from the lane logic over a single-word table of 1 << bits slots"""
    keys = list(table)
    enc = [k.encode() for k in keys]
    offs = np.zeros(len(enc) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(b) for b in enc])
    reads = np.array([table[k] for k in keys], dtype=np.int64)
    if bits is None:
        bits = max(7, (2 * len(keys)).bit_length())
    cent = np.zeros(max(len(keys), 1), dtype=np.uint64)
    cluster = np.zeros(max(len(keys), 1), dtype=np.int64)
    extra = np.zeros(4, dtype=np.int64)
    rc = _lib().ecemu_collapse(b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), reads.ctypes.data_as(C.POINTER(C.c_int64)), len(keys), bits,
                               dist, ratio, wave, cent.ctypes.data_as(C.POINTER(C.c_uint64)), cluster.ctypes.data_as(C.POINTER(C.c_int64)),
                               extra.ctypes.data_as(C.POINTER(C.c_int64)))
    assert rc == 0
    return ({k: (keys[int(cent[i])], int(cluster[i])) for i, k in enumerate(keys)},
            dict(zip(binding.Counter.ECC_EXTRA, (int(x) for x in extra))))


@pytest.mark.parametrize("wave", [0, 1], ids=["lane", "wave"])
@pytest.mark.parametrize("name", sorted(EC.shapes()))
def test_lane_logic_vs_rule_on_the_gpu_shapes(name, wave):
    _run, table, ratio, _fq = EC.shapes()[name]
    assert emu_collapse(table, ratio, wave=wave) == EC.ec_collapse(table, ratio)


@pytest.mark.parametrize("name", sorted(EC.shapes()))
def test_shapes_hold_the_tables_they_claim(name):
    run, table, _ratio, fq = EC.shapes()[name]
    e = emu_helper.Emu(mode="EC", **run)
    assert e.count_block(fq) == len(fq)
    assert {k: n for k, n, _first in e.ec_rows()} == table
    e.close()


def test_shapes_reach_what_they_are_meant_to():
    S = EC.shapes()
    want = {n: EC.ec_collapse(S[n][1], S[n][2]) for n in S}
    assert want["len1"][0] == {"A": ("A", 66), "C": ("A", 0), "G": ("A", 0), "T": ("A", 0)}
    for n in ("len21", "len22", "len29", "len21_r2", "len22_r2", "len29_r2", "roads"):
        assert want[n][1]["absorbed_keys"] >= 20 and want[n][1]["longest_chain"] >= (2 if n.endswith("_r2") else 1), n
    cent = {k: v[0] for k, v in want["lengths_share_codes"][0].items()}
    assert cent == {"ACG": "ACG", "ACGA": "ACGC", "ACT": "ACG", "ACGC": "ACGC", "ACGT": "ACGC", "AAG": "AAG", "AAGA": "AAGA"}
    for r in (2, 255):
        assert want["boundary_r%d" % r][1]["absorbed_keys"] == 1 and want["boundary_r%d" % r][1]["absorbed_reads"] == 3
    cent = {k: v[0] for k, v in want["ties"][0].items()}
    assert cent["AAAAAAAA"] == "CAAAAAAA" and cent["GGGGGGGG"] == "GGGCGGGG" and want["ties"][1]["absorbed_keys"] == 2
    assert want["chains"][1] == dict(eligible_keys=12, absorbed_keys=9, absorbed_reads=1 + 3 + 63, longest_chain=6)
    assert sorted(v[1] for v in want["chains"][0].values() if v[1]) == [3, 7, 127]
    cent = {k: v for k, v in want["n_keys"][0].items()}
    assert cent["ACGTNCGT"] == ("ACGTNCGT", 50) and cent["ACGTACGT"] == ("ACGTACGT", 3) and cent["NTGTACGA"] == ("NTGTACGA", 1)
    assert cent["TTGTACGC"] == ("TTGTACGA", 0) and want["n_keys"][1]["eligible_keys"] == 4
    assert want["len30"][1] == dict(eligible_keys=0, absorbed_keys=0, absorbed_reads=0, longest_chain=0)


@pytest.mark.parametrize("block", range(10))
def test_invariants_on_random_tables(block):
    for seed in range(20 * block, 20 * block + 20):
        table = EC.random_table(seed)
        assert 100 <= len(table) <= 900
        total = sum(table.values())
        absorbed_at = {}
        for ratio in (2, 3, 5, 6, 255):
            want = EC.ec_collapse(table, ratio)
            for wave in (0, 1):
                got, extra = emu_collapse(table, ratio, wave=wave)
                assert (got, extra) == want, (seed, ratio, wave)
            assert sum(v[1] for v in got.values()) == total
            for k, (cent, cluster) in got.items():
                assert got[cent][0] == cent and (cluster == 0) == (cent != k)
                assert EC.eligible(k) or cent == k
            absorbed_at[ratio] = {k for k, v in got.items() if v[0] != k}
            assert extra["absorbed_keys"] == len(absorbed_at[ratio])
        assert absorbed_at[3] <= absorbed_at[2] and absorbed_at[6] <= absorbed_at[5] and absorbed_at[255] <= absorbed_at[6]
        assert absorbed_at[2]
        got, extra = emu_collapse(table, 5, dist=0)
        assert got == {k: (k, n) for k, n in table.items()} and not any(extra.values())
        assert (got, extra) == EC.ec_collapse(table, 5, dist=0)


def test_the_result_does_not_depend_on_the_table_size():
    table = EC.random_table(4242)
    want = EC.ec_collapse(table, 5)
    for bits in (11, 12, 16):
        for wave in (0, 1):
            assert emu_collapse(table, 5, wave=wave, bits=bits) == want


BASE = ["-c", "--mo", "EC"]


@pytest.mark.parametrize("argv,words", [
    (["--ecm", "2"], ["--ecm", "0 or 1"]),
    (["--ecm", "one"], ["--ecm", "0 or 1"]),
    (["--ecm", "1", "--ecr", "1"], ["--ecr", "2 to 255"]),
    (["--ecm", "1", "--ecr", "256"], ["--ecr", "2 to 255"]),
    (["--ecm", "1", "--ecr", "5.5"], ["--ecr", "2 to 255"]),
    (["--ecr", "5"], ["--ecr", "--ecm 1"]),
    (["--ecm", "0", "--ecr", "5"], ["--ecr", "--ecm 1"]),
    (["--mo", "C", "--ecm", "1"], ["--ecm 1", "--mo EC"]),
    (["--ecm", "1", "--pe", "--st2", "0"], ["--ecm 1", "--pe"]),
    (["--ecm", "1", "--st", "0,30"], ["--ecm 1", "--st 0,30"]),
    (["--ecm", "1", "--us", "ACGTAC,GGTTCA", "--ds", "TTGACA,CATGCA"], ["--ecm 1", "--us/--ds"]),
    (["--ecm", "1", "--l", "30"], ["--ecm 1", "--l 30", "29"]),
])
def test_command_line_refusals(argv, words, tmp_path, capsys):
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "a.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    with pytest.raises(SystemExit):
        fast2q.main(BASE + ["--s", str(tmp_path / "in"), "--o", str(tmp_path / "out")] + argv)
    said = capsys.readouterr().out
    assert "FATAL" in said
    for w in words:
        assert w in said, (w, said)
    assert not (tmp_path / "out").exists() and [p.name for p in tmp_path.iterdir()] == ["in"]


def test_several_ranks_are_refused_before_any_output(tmp_path, capsys, monkeypatch):
    (tmp_path / "a.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    p = fast2q.input_parser(BASE + ["--s", str(tmp_path), "--o", str(tmp_path / "out"), "--ecm", "1"])
    assert p["ec_collapse"] == (1, 5)
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(dict(p))
    said = capsys.readouterr().out
    assert "--ecm 1" in said and "several ranks" in said and not (tmp_path / "out").exists()
    p["Progress bar"] = False
    with pytest.raises(RuntimeError, match="--ecm 1.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a.fastq"), {}, p, {})


def test_the_flags_are_taken_and_ecm_0_is_a_run_without_the_flag(tmp_path):
    argv = BASE + ["--s", str(tmp_path), "--o", str(tmp_path), "--l", "29"]
    plain = fast2q.input_parser(argv)
    assert "ec_collapse" not in plain
    assert fast2q.input_parser(argv + ["--ecm", "0"]) == plain                       # the parameters, the recorded command line too
    p = fast2q.input_parser(argv + ["--ecm", "1", "--ecr", "255"])
    assert p["ec_collapse"] == (1, 255) and p["used_cmd"].endswith("--ecm 1 --ecr 255")
    assert {k: v for k, v in p.items() if k not in ("ec_collapse", "used_cmd")} == {k: v for k, v in plain.items() if k != "used_cmd"}
    both = fast2q.input_parser(argv + ["--ecm", "1", "--as", "--g", str(tmp_path / "lib.csv")])
    assert both["ec_collapse"] == (1, 5) and both["assign"] is True
    anchored = fast2q.input_parser(BASE + ["--s", str(tmp_path), "--o", str(tmp_path), "--us", "ACGTAC", "--ds", "TTGACA", "--l", "40", "--ecm", "1"])
    assert anchored["ec_collapse"] == (1, 5)                                           # --l does not bound an anchored key
    assert fast2q.ec_collapse_header(p) == "#Extracted sequences collapsed, mismatches, ratio: 1,255"
    assert fast2q.ec_collapse_header(p) in fast2q.run_headers(dict(p, version="x"))


def test_header_declares_the_collapse_calls_and_the_binding_exports_them():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    for name in ("f2q_ec_collapse", "f2q_ec_fetch_collapsed"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in binding.EXPORTS
    assert "def ec_collapse(table, ratio):" in text
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(f2q_[a-z_0-9]+)\s*\(", bare))) == sorted(binding.EXPORTS)
    if os.path.exists(binding.LIB_PATH):
        L = binding.load()
        assert all(hasattr(L, s) for s in binding.EXPORTS)
