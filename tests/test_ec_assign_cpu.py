"""Extract+Count with a library, without a GPU: the per-key functions of f2q_ec_assign (assign_entry_lane /
assign_slot_lane, f2q_device.h) compiled for the host by tests/emu/f2q_assign_emu.cpp and run over the Extract+Count tables
of the existing emulation, against the oracle in Counter mode (tests/assign_cases.py) -- the inputs of the GPU list in
tests/test_ec_assign_gpu.py; the command line's refusals; the header against the binding's export list."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import assign_cases as AC
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_assign_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_assign_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")


def _lib():
    deps = [SRC, os.path.join(TESTS, "emu", "f2q_emu.cpp")] + [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h", "f2q_synth.h", "f2q_reader.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-o", LIB, SRC, "-lz", "-lpthread"])
    L = C.CDLL(LIB)
    vp = C.c_void_p
    L.emu_create.restype = vp
    L.emu_create.argtypes = [C.POINTER(binding.Params)]
    L.emu_destroy.argtypes = [vp]
    L.emu_count_block.restype = C.c_size_t
    L.emu_count_block.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.emu_ec_n.restype = C.c_uint64
    L.emu_ec_n.argtypes = [vp]
    L.emu_ec_overflow.restype = C.c_uint64
    L.emu_ec_overflow.argtypes = [vp]
    L.emu_ec_get.argtypes = [vp, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
    L.aemu_assign.restype = C.c_longlong
    L.aemu_assign.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                              C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    return L


def emu_assign(lib, fq, miss, **run):
    """(counts, stats, rows) of an Extract+Count emulation of fq whose keys are then assigned to lib"""
    L = _lib()
    p, keep = binding.make_params(mode="EC", miss=miss, **run)
    h = C.c_void_p(L.emu_create(C.byref(p)))
    assert h
    assert L.emu_count_block(h, fq, len(fq)) == len(fq)
    assert L.emu_ec_overflow(h) == 0
    n = L.emu_ec_n(h)
    enc = [s.encode() for s in lib]
    offs = np.zeros(len(enc) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(b) for b in enc])
    counts, stats = (C.c_int64 * len(lib))(), (C.c_int64 * 5)()
    feat, dist = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    assert L.aemu_assign(h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc), counts, stats, feat, dist) == n
    rows = []
    for e in range(n):
        key, ln, cnt, first = C.create_string_buffer(4096), C.c_uint32(), C.c_int64(), C.c_uint64()
        L.emu_ec_get(h, e, key, C.byref(ln), C.byref(cnt), C.byref(first))
        rows.append((key.raw[:ln.value].decode("latin-1"), cnt.value, first.value, feat[e], dist[e]))
    L.emu_destroy(h)
    return list(counts), list(stats), rows


CASES = {"fixed": AC.fixed_window, "ties": AC.ties, "irregular": AC.irregular, "two_windows": AC.two_windows,
         "anchored": lambda: AC.anchored(3000)}


MISSES = {"fixed": (0, 1, 2, 3), "ties": (1, 2, 3), "irregular": (0, 1, 2), "two_windows": (0, 1, 2), "anchored": (0, 1, 2)}


@pytest.mark.parametrize("name,miss", [(n, m) for n in CASES for m in MISSES[n]])
def test_per_key_functions_vs_oracle(name, miss):
    lib, fq, run, misses = CASES[name]()[:4]
    assert misses == MISSES[name]
    want = AC.aggregate(lib, fq, miss, **run)
    counts, stats, rows = emu_assign(lib, fq, miss, **run)
    assert (counts, stats) == want
    AC.check_rows(lib, rows, counts, stats, miss)
    assert stats[1] > 0 and stats[3] > 0 and (miss == 0 or stats[2] > 0)


def test_the_fixed_window_case_reaches_both_tables_and_every_key_form():
    lib, fq, run, _ = AC.fixed_window()
    _, _, rows = emu_assign(lib, fq, 2, **run)
    keys = [r[0] for r in rows]
    plain = [k for k in keys if set(k) <= set("ACGT")]
    assert "" in keys and any(len(k) == 18 for k in plain) and any(len(k) == 20 for k in plain)
    assert any(1 <= k.count("N") <= 3 and set(k) <= set("ACGTN") for k in keys)          # single-word form with 'N's
    assert any(k.count("N") >= 4 for k in keys) and any(set(k) & set("RY.") for k in keys)   # byte-string table


def test_ties_are_unassigned_and_the_nearer_feature_wins():
    lib, fq, run, _, mids, near = AC.ties()
    for miss in (1, 2, 3):
        _, _, rows = emu_assign(lib, fq, miss, **run)
        got = {r[0]: (r[3], r[4]) for r in rows}
        for m in mids:
            assert got[m.decode()] == (-1, -1)
        for key, f in near:
            assert got[key.decode()] == (f, 1)


@pytest.mark.parametrize("argv,word", [(["--mo", "EC", "--as"], "--as"), (["--as", "--g", "y"], "--as"),
                                       (["-t", "--mo", "EC", "--as", "--g", "y"], "--as")])
def test_command_line_refusals(argv, word, capsys):
    with pytest.raises(SystemExit):
        fast2q.input_parser(["-c", "--s", "x", "--o", "z"] + argv)
    said = capsys.readouterr().out
    assert word in said and "FATAL" in said


def test_command_line_takes_the_flag_and_refuses_several_ranks(tmp_path, capsys, monkeypatch):
    (tmp_path / "a.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path), "--mo", "EC"]
    p = fast2q.input_parser(argv + ["--as"])
    assert p["assign"] is True and p["used_cmd"].endswith("--as")
    plain = fast2q.input_parser(argv)
    assert "assign" not in plain and {k: v for k, v in p.items() if k not in ("assign", "used_cmd")} == {k: v for k, v in plain.items() if k != "used_cmd"}
    p["test_mode"] = False
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(dict(p))
    said = capsys.readouterr().out
    assert "--as" in said and "several ranks" in said
    p["Progress bar"], p["assign_features"] = False, {"ACGT": fast2q.Features("g", 0)}
    with pytest.raises(RuntimeError, match="--as.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a.fastq"), {}, p, {})


def test_header_declares_the_assign_calls_and_the_binding_exports_them():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    for name in ("f2q_set_assign_library", "f2q_ec_assign", "f2q_ec_fetch_assigned"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in binding.EXPORTS
    assert "fast2q.py:362-380" in text and ":692-750" in text
    assert re.search(r"#define\s+F2Q_ABI_VERSION\s+1\b", text)
    if os.path.exists(binding.LIB_PATH):
        L = binding.load()
        assert all(hasattr(L, s) for s in binding.EXPORTS)
