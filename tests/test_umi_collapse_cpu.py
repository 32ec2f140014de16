"""--mu 1 without a GPU: the lane logic of f2q_umi_collapse (umi_find, uf_find / uf_union, umi_link_one, umi_root_one of
f2q_device.h) compiled for the host by tests/emu/f2q_umi_collapse_emu.cpp and run over the emulated (feature, UMI) set,
against the plain-Python expectation of tests/umi_collapse_cases.py -- the shapes of tests/test_umi_collapse_gpu.py; the
command line's flag and refusals; the header against the binding's export list."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import umi_collapse_cases as CC
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
SRC = os.path.join(TESTS, "emu", "f2q_umi_collapse_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_umi_collapse_emu.so")
_L = []


def _lib():
    if _L:
        return _L[0]
    deps = [SRC] + [os.path.join(TESTS, "emu", f) for f in ("f2q_umi_emu.cpp", "f2q_emu.cpp")] + [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h", "f2q_synth.h", "f2q_reader.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-o", LIB, SRC, "-lz", "-lpthread"])
    L = C.CDLL(LIB)
    vp, i64p = C.c_void_p, C.POINTER(C.c_int64)
    L.uemu_create.restype = vp
    L.uemu_create.argtypes = [C.POINTER(binding.Params), C.c_int32, C.c_int32, C.c_uint64]
    L.uemu_destroy.argtypes = [vp]
    L.uemu_set_features.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32]
    L.uemu_count_block.restype = C.c_size_t
    L.uemu_count_block.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.uemu_read.restype = C.c_longlong
    L.uemu_read.argtypes = [vp, i64p, i64p, i64p, i64p]
    L.uemu_set_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.uemu_reset.argtypes = [vp]
    L.uemu_collapse.argtypes = [vp, C.c_int32, C.c_int32, i64p, i64p]
    _L.append(L)
    return L


class CEmu:
    """an emulated UMI context (as tests/test_umi_cpu.py's) that can also collapse its set"""

    def __init__(self, lib, umi, slots=0, **run):
        self.L, self.n = _lib(), len(lib)
        p, self._keep = binding.make_params(mode="C", **run)
        self.h = C.c_void_p(self.L.uemu_create(C.byref(p), umi[0], umi[1], slots))
        assert self.h
        enc = [s.encode() for s in lib]
        offs = np.zeros(len(enc) + 1, dtype=np.uint32)
        offs[1:] = np.cumsum([len(b) for b in enc])
        self.L.uemu_set_features(self.h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc))

    def count(self, fq):
        assert self.L.uemu_count_block(self.h, fq, len(fq)) == len(fq)

    def umis(self):
        """umis per feature, rehashes"""
        counts, umis = (C.c_int64 * self.n)(), (C.c_int64 * self.n)()
        stats, extra = (C.c_int64 * 5)(), (C.c_int64 * 2)()
        rehashes = self.L.uemu_read(self.h, counts, stats, umis, extra)
        assert rehashes >= 0                                         # (-1: the overflow flag)
        return list(umis), rehashes

    def collapse(self, dist=1, order=0):
        molecules, extra = (C.c_int64 * self.n)(), (C.c_int64 * 2)()
        rc = self.L.uemu_collapse(self.h, dist, order, molecules, extra)
        assert rc in (0, -1), rc                                     # (-2: parent[x] > x)
        return (list(molecules), extra[0], extra[1]) if rc == 0 else None

    def reset(self):
        self.L.uemu_reset(self.h)

    def close(self):
        self.L.uemu_destroy(self.h)


def collapsed(name, slots=0, per=0):
    lib, fq, run, umi = CC.shape(name)
    e = CEmu(lib, umi, slots, **run)
    for piece in (CC.pieces(fq, per) if per else [fq]):
        e.count(piece)
    umis, rehashes = e.umis()
    got = [e.collapse(1, order) for order in (0, 1)]
    assert e.collapse(0) == (umis, sum(umis), 0) and e.collapse(2) is None
    assert e.umis()[0] == umis                                       # the set is as it was
    e.close()
    assert got[0] == got[1]
    return got[0], umis, rehashes


def test_known_answers():
    got, umis, _ = collapsed("known")
    want = CC.known()[4]
    assert got == want == CC.expected("known")
    assert want[1:] == (262, 1538) and umis[:4] == [256, 3, 2, 1]


@pytest.mark.parametrize("length", [1, 2])
def test_one_and_two_base_umis(length):
    got, umis, _ = collapsed("short%d" % length)
    assert got == CC.expected("short%d" % length)
    assert sum(1 for n in umis if n > 1) > 10
    if length == 1:
        assert got[0] == [min(n, 1) for n in umis]                   # every two one-base UMIs are neighbours
    else:
        assert any(m < n for m, n in zip(got[0], umis)) and any(m == n > 1 for m, n in zip(got[0], umis))


def test_sixteen_base_umis_next_to_wide_feature_indices():
    got, umis, _ = collapsed("wide")
    assert got == CC.expected("wide")
    assert sum(got[0][:512]) == 0 and got[2] > 0 and any(m < n for m, n in zip(got[0], umis))


def test_the_contention_input_is_what_it_says():
    codes = CC.contention()[4]
    assert len(set(codes)) == CC.GRAY_N
    for a, b in zip(codes, codes[1:]):
        x = a ^ b
        assert x and x >> (((x & -x).bit_length() - 1) & ~1) < 4      # one 2-bit field differs
    assert CC.components({CC.text_of(c, 8) for c in codes}) == CC.CONTENTION_WANT[::2]
    mol, pairs, edges = CC.expected("contention")
    lib, fq, run, umi = CC.shape("contention")
    umis = [len(s) for s in CC.umi_sets(lib, fq, umi, **run)]
    assert (mol[CC.GRAY_FEATURE], umis[CC.GRAY_FEATURE]) == CC.CONTENTION_WANT[:2] and pairs == sum(umis)
    rest = edges - CC.CONTENTION_WANT[2]
    assert rest > 0 and any(m < n for m, n in zip(mol, umis)) and any(m == n > 1 for m, n in zip(mol, umis))
    assert sum(n > 0 for n in umis) == len(lib)


@pytest.mark.parametrize("slots,per", [(0, 0), (64, 30)])
def test_contention_from_the_first_set_and_from_a_rehashed_one(slots, per):
    got, umis, rehashes = collapsed("contention", slots, per)
    assert got == CC.expected("contention")
    assert (rehashes >= 5) == bool(slots)


def test_nothing_counted_and_reset_give_zeros():
    lib, fq, run, umi = CC.shape("known")
    e = CEmu(lib, umi, **run)
    zeros = ([0] * len(lib), 0, 0)
    assert e.collapse(1) == zeros and e.collapse(0) == zeros
    e.count(fq)
    assert e.collapse(1) == CC.known()[4]
    e.reset()
    assert e.collapse(1) == zeros
    e.close()


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE_ARGV = ["-c", "--s", "x", "--g", "y", "--o", "z"]


@pytest.mark.parametrize("argv", [["--mu", "1"], ["--umi", "20,8", "--mu", "2"], ["--umi", "20,8", "--mu=-1"], ["--mu", "0"]])
def test_command_line_refusals(argv, capsys):
    with pytest.raises(SystemExit):
        fast2q.input_parser(BASE_ARGV + argv)
    said = capsys.readouterr().out
    assert "--mu" in said and "FATAL" in said


def test_command_line_takes_the_flag(tmp_path, capsys):
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path), "--umi", "20,8"]
    plain = fast2q.input_parser(argv)
    zero = fast2q.input_parser(argv + ["--mu", "0"])
    one = fast2q.input_parser(argv + ["--mu", "1"])
    assert "umi_mismatch" not in plain and one["umi_mismatch"] == 1 and one["used_cmd"].endswith("--umi 20,8 --mu 1")
    strip = lambda p: {k: v for k, v in p.items() if k not in ("umi_mismatch", "used_cmd")}
    assert strip(zero) == strip(plain) == strip(one) and not zero.get("umi_mismatch")
    # --mu changes no context: the context cache key is the one of --umi alone
    assert fast2q._counter_kwargs(one) == fast2q._counter_kwargs(plain)
    headers = lambda p: [h for h in fast2q.run_headers(fast2q.initializer(dict(p))) if not h.startswith("#cmd used")]
    assert headers(plain) == headers(zero)
    capsys.readouterr()
    p = fast2q.initializer(one)
    assert "UMIs of one feature that differ in one base are collapsed (--mu 1)" in capsys.readouterr().out
    assert "#UMI mismatches collapsed: 1" in fast2q.run_headers(p)
    assert "#UMI mismatches collapsed" not in "".join(headers(plain))
    assert fast2q.UMI_COLLAPSE_STATS_HEAD[0].startswith("#") and fast2q.UMI_COLLAPSE_STATS_HEAD != fast2q.UMI_STATS_HEAD


def test_header_declares_the_call_and_the_binding_exports_it():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    assert re.search(r"\bint\s+f2q_umi_collapse\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int32_t\s+dist\s*,\s*int64_t\s*\*\s*molecules\s*,\s*int64_t\s+extra\[2\]\s*\)", text)
    assert "f2q_umi_collapse" in binding.EXPORTS and hasattr(binding.Counter, "collapse_umis")
    assert re.search(r"#define\s+F2Q_ABI_VERSION\s+1\b", text)
    if os.path.exists(binding.LIB_PATH):
        assert hasattr(binding.load(), "f2q_umi_collapse")
