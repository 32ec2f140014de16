"""--mur directional without a GPU: the lane logic of reads per (feature, UMI) pair and of f2q_umi_collapse_directional
(umi_claim_at / umi_insert<true> / UmiHook<P, true>, umi_rehash_one<true>, umi_link_dir_one, umi_dir_spread_one,
umi_dir_root_one of f2q_device.h) compiled for the host by tests/emu/f2q_umi_dir_emu.cpp and run over the emulated set,
against the literal restatement of UMI-tools in tests/umi_dir_cases.py under three tie orders -- the shapes of
tests/test_umi_dir_gpu.py; the command line's flag and refusals; the header against the binding's export list."""
import collections
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import umi_cases as UC
import umi_collapse_cases as CC
import umi_dir_cases as DC
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
SRC = os.path.join(TESTS, "emu", "f2q_umi_dir_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_umi_dir_emu.so")
_L = []


def _lib():
    if _L:
        return _L[0]
    deps = [SRC] + [os.path.join(TESTS, "emu", f) for f in ("f2q_umi_collapse_emu.cpp", "f2q_umi_emu.cpp", "f2q_emu.cpp")]
    deps += [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h", "f2q_synth.h", "f2q_reader.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-o", LIB, SRC, "-lz", "-lpthread"])
    L = C.CDLL(LIB)
    vp, i64p, u32p = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    L.demu_create.restype = vp
    L.demu_create.argtypes = [C.POINTER(binding.Params), C.c_int32, C.c_int32, C.c_uint64]
    L.uemu_destroy.argtypes = [vp]
    L.uemu_set_features.argtypes = [vp, C.c_char_p, u32p, C.c_uint32]
    L.uemu_count_block.restype = C.c_size_t
    L.uemu_count_block.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.uemu_reset.argtypes = [vp]
    L.demu_directional.argtypes = [vp, C.c_int32, i64p, i64p]
    L.demu_pairs.restype = C.c_uint64
    L.demu_pairs.argtypes = [vp, C.c_uint64, u32p, u32p, u32p, u32p]
    L.uemu_read.restype = C.c_longlong
    L.uemu_read.argtypes = [vp, i64p, i64p, i64p, i64p]
    L.uemu_collapse.argtypes = [vp, C.c_int32, C.c_int32, i64p, i64p]
    L.uemu_set_info.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 3
    _L.append(L)
    return L


ORDERS = (0, 1, 2, 3)                                                # slots front to back, back to front, two shuffles


class DEmu:
    """an emulated UMI context that keeps reads per pair"""

    def __init__(self, lib, umi, slots=0, **run):
        self.L, self.n = _lib(), len(lib)
        p, self._keep = binding.make_params(mode="C", **run)
        self.h = C.c_void_p(self.L.demu_create(C.byref(p), umi[0], umi[1], slots))
        assert self.h
        self.set = self.h                                            # one handle: the set with its reads
        enc = [s.encode() for s in lib]
        offs = np.zeros(len(enc) + 1, dtype=np.uint32)
        offs[1:] = np.cumsum([len(b) for b in enc])
        self.L.uemu_set_features(self.h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc))

    def count(self, fq):
        assert self.L.uemu_count_block(self.h, fq, len(fq)) == len(fq)

    def state(self):
        """counts, stats, umis, valid, invalid, rehashes"""
        counts, umis = (C.c_int64 * self.n)(), (C.c_int64 * self.n)()
        stats, extra = (C.c_int64 * 5)(), (C.c_int64 * 2)()
        rehashes = self.L.uemu_read(self.set, counts, stats, umis, extra)
        assert rehashes >= 0                                         # (-1: the overflow flag)
        return list(counts), list(stats), list(umis), extra[0], extra[1], rehashes

    def cluster(self):
        molecules, extra = (C.c_int64 * self.n)(), (C.c_int64 * 2)()
        assert self.L.uemu_collapse(self.set, 1, 0, molecules, extra) == 0
        return list(molecules), extra[0], extra[1]

    def directional(self, order=0):
        molecules, extra = (C.c_int64 * self.n)(), (C.c_int64 * 4)()
        assert self.L.demu_directional(self.h, order, molecules, extra) == 0          # (-2: parent[x] > x)
        return (list(molecules),) + tuple(extra)

    def pairs(self):
        """[(feature, codes, reads)] sorted, and the slot of each"""
        n = self.L.demu_pairs(self.h, 0, None, None, None, None)
        arrs = [(C.c_uint32 * max(n, 1))() for _ in range(4)]
        assert self.L.demu_pairs(self.h, n, *arrs) == n
        f, c, r, s = (list(a)[:n] for a in arrs)
        return list(zip(f, c, r)), s

    def set_info(self):
        """pairs held (the counter), occupied slots, slots"""
        held, occupied, slots = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.L.uemu_set_info(self.h, C.byref(held), C.byref(occupied), C.byref(slots))
        return held.value, occupied.value, slots.value

    def reset(self):
        self.L.uemu_reset(self.h)

    def close(self):
        self.L.uemu_destroy(self.h)


def counted(name, slots=0, per=0):
    lib, fq, run, umi = DC.shape(name)
    e = DEmu(lib, umi, slots, **run)
    for piece in (CC.pieces(fq, per) if per else [fq]):
        e.count(piece)
    return e


def checked(name, slots=0, per=0):
    """the shape counted and collapsed under every visiting order, with the invariants every shape must keep"""
    e = counted(name, slots, per)
    before = e.state()
    got = [e.directional(order) for order in ORDERS]
    assert all(g == got[0] for g in got)
    assert e.state() == before
    want = DC.expected(name)
    assert DC.separates(name)                                        # the expectation itself tells the rules apart
    assert got[0] == want
    cl = e.cluster()
    (wcl, wpairs, wedges), wumis = DC.expected_cluster(name)
    assert cl == (wcl, wpairs, wedges) and before[2] == wumis
    assert all(a <= b <= c for a, b, c in zip(cl[0], got[0][0], before[2]))
    assert got[0][2] == cl[2] and got[0][1] == cl[1] and got[0][4] == before[3]
    table, slots_of = e.pairs()
    assert table == DC.expected_pairs(name)
    return e, got[0], before, (table, slots_of)


def test_known_answers():
    e, got, before, (table, slot) = checked("known")
    dirw, clw, umiw = DC.known()[4]
    assert got[0] == dirw and e.cluster()[0] == clw and before[2] == umiw
    # features 6 .. 21: the dominated single read Y is the root of its two-slot tree in some (the lower slot), below it in
    # others (the spread launch has work to do there)
    at = {(f, c): s for (f, c, _), s in zip(table, slot)}
    code = lambda u: sum(b"ACGT".index(ch) << (2 * j) for j, ch in enumerate(u))
    sides = {at[(f, code(y))] < at[(f, code(x))] for f, (x, y, z) in enumerate(DC.known()[5], 6)}
    assert sides == {True, False}
    e.close()


def test_one_base_umis():
    e, got, before, _ = checked("known1")
    assert got[0][:2] == [1, 4] == DC.known1()[4][0][:2] and e.cluster()[0][:2] == [1, 1] and before[2][:2] == [4, 4]
    e.close()


def test_sixteen_base_umis_next_to_wide_feature_indices():
    e, got, _, _ = checked("wide")
    assert sum(got[0][:512]) == 0 and got[2] > 0
    e.close()


def test_a_set_smaller_than_one_wave():
    """a dozen records from a first set of 2 slots: the answers by hand, and the 32 slots the sizing rule gives"""
    e, got, before, (table, _) = checked("tiny", slots=2)
    assert got == DC.TINY_WANT and e.cluster() == CC.TINY_WANT and before[2] == DC.TINY_UMIS
    assert len(UC.records(DC.shape("tiny")[1])) == CC.TINY_RECORDS <= 12
    assert e.set_info() == (5, 5, 32) and before[5] == 0              # the smallest power of two >= 2 x 11; one block: no rehash
    assert table == [(0, 0, 5), (0, 1 << 6, 1), (0, 1 << 4 | 1 << 6, 1), (1, 0, 2), (1, 1 << 6, 2)]      # AAAA, AAAC, AACC; AAAA, AAAC
    e.close()


@pytest.mark.parametrize("name", ["ones", "twice"])
@pytest.mark.parametrize("slots,per", [(0, 0), (64, 30)])
def test_contention_from_the_first_set_and_from_a_rehashed_one(name, slots, per):
    e, got, before, (table, _) = checked(name, slots, per)
    assert (before[5] >= 5) == bool(slots)
    cl = e.cluster()
    assert cl[0][DC.GRAY_FEATURE] == 1 and before[2][DC.GRAY_FEATURE] == DC.GRAY_N
    assert got[0][DC.GRAY_FEATURE] == (DC.GRAY_N // 2 if name == "twice" else 1)
    # the pairs with their reads are a Counter of the valid pairs: the rehash has carried every count
    lib, fq, run, umi = DC.shape(name)
    index = {s.encode(): f for f, s in enumerate(lib)}
    seen = collections.Counter((index[s[:20]], s[20:28]) for s, _ in UC.records(fq))
    assert sorted((f, sum(b"ACGT".index(ch) << (2 * j) for j, ch in enumerate(u)), n) for (f, u), n in seen.items()) == table
    e.close()


def test_count_collapse_count_more_and_reset():
    lib, fq, run, umi = DC.shape("ones")
    parts = CC.pieces(fq, 16000)
    assert len(parts) >= 3
    e = DEmu(lib, umi, **run)
    zeros = ([0] * len(lib), 0, 0, 0, 0)
    assert e.directional() == zeros
    seen = []
    for part in parts:
        e.count(part)
        seen.append(e.directional())
    assert seen[-1] == DC.expected("ones") and seen[0] != seen[-1]
    first = DC.expect(lib, parts[0], umi, **run)
    assert seen[0] == first
    e.reset()
    assert e.directional() == zeros and e.pairs()[0] == []
    e.count(parts[0])
    assert e.directional() == first
    e.close()


def test_the_restatement_disagrees_with_itself_nowhere_and_knows_the_small_cases():
    """umitools_directional on hand-made counts, under every tie order"""
    cases = [({b"AAAA": 10, b"AAAC": 1, b"AACC": 1}, 1), ({b"AAAA": 3, b"AAAC": 3}, 2), ({b"AAAA": 2, b"AAAC": 2}, 2),
             ({b"AAAA": 2, b"AAAC": 1}, 1), ({b"AAAA": 3, b"AAAC": 2}, 1), ({b"AAAA": 1, b"AAAC": 1, b"AACC": 1}, 1),
             ({b"AAAA": 1, b"AAAC": 1, b"AACC": 5}, 1), ({b"G": 5, b"A": 1, b"C": 1, b"T": 1}, 1), ({b"A": 2, b"C": 2, b"G": 2, b"T": 2}, 4)]
    for counts, want in cases:
        for tie in DC.TIE_ORDERS:
            for seed in range(3):
                assert DC.umitools_directional(counts, DC.ordered(counts, tie, seed)) == want


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE_ARGV = ["-c", "--s", "x", "--g", "y", "--o", "z"]


@pytest.mark.parametrize("argv", [["--mur", "directional"], ["--umi", "20,8", "--mur", "directional"], ["--umi", "20,8", "--mu", "0", "--mur", "directional"],
                                  ["--umi", "20,8", "--mu", "1", "--mur", "adjacency"], ["--umi", "20,8", "--mu", "1", "--mur", ""],
                                  ["--mu", "1", "--mur", "cluster"], ["--umi", "20,8", "--mur", "cluster"]])
def test_command_line_refusals(argv, capsys):
    with pytest.raises(SystemExit):
        fast2q.input_parser(BASE_ARGV + argv)
    said = capsys.readouterr().out
    assert ("--mur" in said or "--mu" in said) and "FATAL" in said


@pytest.mark.parametrize("argv", [["--mo", "EC"], ["--pe", "--st2", "0"]])
def test_the_refusals_of_umi_hold(argv, capsys):
    with pytest.raises(SystemExit):
        fast2q.input_parser(BASE_ARGV + ["--umi", "20,8", "--mu", "1", "--mur", "directional"] + argv)
    said = capsys.readouterr().out
    assert "--umi" in said and "FATAL" in said


def test_command_line_takes_the_flag(tmp_path, capsys):
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path), "--umi", "20,8", "--mu", "1"]
    plain = fast2q.input_parser(argv)
    cluster = fast2q.input_parser(argv + ["--mur", "cluster"])
    directional = fast2q.input_parser(argv + ["--mur", "directional"])
    assert "umi_rule" not in plain and "umi_rule" not in cluster and directional["umi_rule"] == "directional"
    assert directional["used_cmd"].endswith("--umi 20,8 --mu 1 --mur directional")
    strip = lambda p: {k: v for k, v in p.items() if k not in ("umi_rule", "used_cmd")}
    assert strip(cluster) == strip(plain) == strip(directional)
    # --mur cluster is a run of today; directional is another context (reads are kept), the rest of its key is the same
    assert fast2q._counter_kwargs(cluster) == fast2q._counter_kwargs(plain) and "umi_reads" not in fast2q._counter_kwargs(plain)
    assert fast2q._counter_kwargs(directional) == dict(fast2q._counter_kwargs(plain), umi_reads=True)
    headers = lambda p: [h for h in fast2q.run_headers(fast2q.initializer(dict(p))) if not h.startswith("#cmd used")]
    assert headers(plain) == headers(cluster)
    assert [h for h in headers(directional) if h != "#UMI collapse rule: directional"] == headers(plain)
    assert "#UMI collapse rule: directional" in headers(directional)
    capsys.readouterr()
    fast2q.initializer(directional)
    assert "--mur directional" in capsys.readouterr().out
    assert fast2q.UMI_DIRECTIONAL_STATS_HEAD[0].startswith("#") and len(fast2q.UMI_DIRECTIONAL_STATS_HEAD) == 6
    assert fast2q.UMI_DIRECTIONAL_STATS_HEAD not in (fast2q.UMI_COLLAPSE_STATS_HEAD, fast2q.UMI_STATS_HEAD)
    assert fast2q.umi_text(0b11100100, 4) == "ACGT" and fast2q.umi_text(0, 16) == "A" * 16


def test_header_declares_the_calls_and_the_binding_exports_them():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    assert re.search(r"\bint\s+f2q_set_umi_reads\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int32_t\s+on\s*\)", text)
    assert re.search(r"\bint\s+f2q_umi_collapse_directional\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int64_t\s*\*\s*molecules\s*,\s*int64_t\s+extra\[4\]\s*\)", text)
    assert re.search(r"\bint\s+f2q_umi_pairs\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*uint64_t\s+cap\s*,\s*uint64_t\s*\*\s*n\s*,\s*uint32_t\s*\*\s*feature\s*,"
                     r"\s*uint32_t\s*\*\s*codes\s*,\s*uint32_t\s*\*\s*reads\s*\)", text)
    for name in ("f2q_set_umi_reads", "f2q_umi_collapse_directional", "f2q_umi_pairs"):
        assert name in binding.EXPORTS
    assert hasattr(binding.Counter, "umi_pairs") and hasattr(binding.Counter, "set_umi_reads")
    assert "F2Q_EUNSUPPORTED" in text[text.index("f2q_set_umi_reads(ctx, on"):] and re.search(r"#define\s+F2Q_ABI_VERSION\s+1\b", text)
    if os.path.exists(binding.LIB_PATH):
        L = binding.load()
        assert all(hasattr(L, n) for n in ("f2q_set_umi_reads", "f2q_umi_collapse_directional", "f2q_umi_pairs"))
