"""--umi1 / --umi2 with --pe without a GPU: the paired hook and record walk of k_count_umi_pair (umi_codes_paired /
UmiPairHook of f2q_device.h on the merged records pack_pairs writes) compiled for the host by
tests/emu/f2q_umi_pair_emu.cpp, against the yardstick of tests/umi_pair_cases.py -- the inputs of the GPU list in
tests/test_umi_pair_gpu.py; the command line's flags, refusals, parameter dictionary, cache key, print-out and header
lines; the header against the binding's export list.  The ABI's state errors need the library: tests/test_umi_pair_gpu.py."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import paired_cases as PC
import umi_pair_cases as UP
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_umi_pair_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_umi_pair_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
_L = []


def _lib():
    if _L:
        return _L[0]
    deps = [SRC, os.path.join(TESTS, "emu", "f2q_pair_emu.cpp"), os.path.join(CSRC, "f2q_device.h"), os.path.join(CSRC, "f2q_host.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-o", LIB, SRC])
    L = C.CDLL(LIB)
    vp, i64p, u64p = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)
    L.upemu_create.restype = vp
    L.upemu_create.argtypes = [C.POINTER(binding.Params), C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int]
    L.upemu_destroy.argtypes = [vp]
    L.upemu_set_features.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32]
    L.upemu_count_block.restype = C.c_uint64
    L.upemu_count_block.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.upemu_read.restype = C.c_longlong
    L.upemu_read.argtypes = [vp, i64p, i64p, i64p, i64p]
    L.upemu_pairs.restype = C.c_uint64
    L.upemu_pairs.argtypes = [vp, C.c_uint64, u64p, C.POINTER(C.c_uint32), u64p, u64p]
    L.upemu_reset.argtypes = [vp]
    _L.append(L)
    return L


class UPEmu:
    def __init__(self, lib, parts, rc2, slots=0, keep=True, st1=UP.ST1, st2=UP.ST2, length=UP.LEN, **run):
        self.L, self.n = _lib(), len(lib)
        p, self._keep = binding.make_params(mode="C", start=",".join(str(s) for s in tuple(st1) + tuple(st2)), length=length, **run)
        p1, p2 = [part or (0, 0) for part in parts]
        self.h = C.c_void_p(self.L.upemu_create(C.byref(p), len(st1), 1 if rc2 else 0, p1[0], p1[1], p2[0], p2[1], slots, 1 if keep else 0))
        assert self.h
        enc = [s.encode() for s in lib]
        offs = np.zeros(len(enc) + 1, dtype=np.uint32)
        offs[1:] = np.cumsum([len(b) for b in enc])
        self.L.upemu_set_features(self.h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc))

    def count(self, fq1, fq2):
        n = self.L.upemu_count_block(self.h, fq1, len(fq1), fq2, len(fq2))
        assert n != 2 ** 64 - 1, "a pair went into the tiles: the plan of a paired UMI context has no fast path"
        return n

    def read(self):
        """(counts, stats, umis, umi_reads, umi_failed), the pair table sorted by (feature, codes), rehashes"""
        counts, umis = (C.c_int64 * self.n)(), (C.c_int64 * self.n)()
        stats, extra = (C.c_int64 * 5)(), (C.c_int64 * 2)()
        rehashes = self.L.upemu_read(self.h, counts, stats, umis, extra)
        assert rehashes >= 0                                         # (-1: the overflow flag)
        cap = sum(umis) + 1
        words, reads, held, slots = (C.c_uint64 * cap)(), (C.c_uint32 * cap)(), C.c_uint64(), C.c_uint64()
        occupied = self.L.upemu_pairs(self.h, cap, words, reads, C.byref(held), C.byref(slots))
        assert held.value == occupied == sum(umis) and 2 * occupied <= max(slots.value, 1)
        table = sorted((w >> 32, w & 0xFFFFFFFF, r) for w, r in zip(words[:occupied], reads[:occupied]))
        return (list(counts), list(stats), list(umis), extra[0], extra[1]), table, rehashes

    def reset(self):
        self.L.upemu_reset(self.h)

    def close(self):
        self.L.upemu_destroy(self.h)


def pieces(fq1, fq2, per):
    """the two texts cut into pieces of `per` whole records"""
    l1, l2 = fq1.split(b"\n"), fq2.split(b"\n")
    for i in range(0, len(l1) - 1, 4 * per):
        yield b"\n".join(l1[i:i + 4 * per]) + b"\n", b"\n".join(l2[i:i + 4 * per]) + b"\n"


def emu_result(lib, fq1, fq2, parts, rc2, slots=0, per=0, **kw):
    e = UPEmu(lib, parts, rc2, slots, **kw)
    total = 0
    for a, b in (pieces(fq1, fq2, per) if per else [(fq1, fq2)]):
        total += e.count(a, b)
    got = e.read()
    e.close()
    return got + (total,)


def wanted(e):
    return (e.counts, e.stats, UP.umis_of(e), e.ok, e.bad)


@pytest.mark.parametrize("rc2", [False, True])
def test_base_shape_vs_yardstick(rc2):
    lib, fq1, fq2 = UP.base(rc2)
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, rc2, (None, UP.UMI2), miss=1)
    got, table, _, n = emu_result(lib, fq1, fq2, (None, UP.UMI2), rc2, miss=1)
    assert want.uncovered == 0 and n == 3000
    assert got == wanted(want) and table == UP.table_of(want)
    assert want.ok + want.bad == want.stats[1] + want.stats[2] and want.stats[2] > 0 and want.ok > 2000
    assert sum(got[2]) < want.ok - 100 and max(got[2]) <= 48        # many pairs repeat a (feature, UMI) pair


def test_orientation_the_umi_is_the_text_as_sequenced():
    lib, (fq1, fq2), table = UP.orientation()
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, True, (None, UP.UMI2), miss=1)
    got, got_table, _, _ = emu_result(lib, fq1, fq2, (None, UP.UMI2), True, miss=1)
    assert want.uncovered == 0 and UP.table_of(want) == table and want.bad == 0
    assert got == wanted(want) and got_table == table
    assert got[2][0] == 2                                            # AAAAAAAC and GTTTTTTT on feature 0: two pairs
    assert (0, UP.code_of(b"AAAAAAAC"), 1) in got_table and (0, UP.code_of(b"GTTTTTTT"), 1) in got_table


@pytest.mark.parametrize("rc2", [False, True])
def test_invalid_parts_kind_by_kind(rc2):
    lib, (fq1, fq2), kinds = UP.invalid(rc2)
    recs = list(pieces(fq1, fq2, 1))
    assert len(recs) == len(kinds) == 12 * len(UP.INVALID_KINDS)
    for phred, also in ((30, set()), (0, {"lowq_first", "lowq_last"})):
        e = UPEmu(lib, (None, UP.UMI2), rc2, miss=1, phred=phred)
        for kind in UP.INVALID_KINDS:
            a = b"".join(r[0] for r, k in zip(recs, kinds) if k == kind)
            b = b"".join(r[1] for r, k in zip(recs, kinds) if k == kind)
            want = UP.expect(lib, a, b, UP.ST1, UP.ST2, UP.LEN, rc2, (None, UP.UMI2), miss=1, phred=phred)
            e.reset()
            assert e.count(a, b) == 12
            got, table, _ = e.read()
            assert want.uncovered == 0 and got == wanted(want) and table == UP.table_of(want), kind
            valid = kind in UP.VALID_KINDS | also
            assert (want.ok, want.bad) == ((12, 0) if valid else (0, 12)), kind      # every pair is assigned
            assert sum(got[2]) == want.ok, kind                      # every UMI is distinct
        e.close()


@pytest.mark.parametrize("parts", [UP.TWO, (UP.TWO[0], None), (None, UP.TWO[1])])
def test_two_parts_fill_all_code_bits(parts):
    lib, (fq1, fq2) = UP.two_parts()
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, True, parts, miss=1)
    got, table, _, _ = emu_result(lib, fq1, fq2, parts, True, miss=1)
    assert want.uncovered == 0 and got == wanted(want) and table == UP.table_of(want)
    assert sum(got[2][:512]) == 0 and want.bad == {UP.TWO: 4, (UP.TWO[0], None): 2, (None, UP.TWO[1]): 2}[parts]
    if parts == UP.TWO:
        assert (550, 0xFFFFFFFF, 2) in table and (550, 0, 1) in table and UP.cluster_of(want)[2] >= 3
        assert want.per[599] and max(len(u) for u in want.per[599]) == 16


@pytest.mark.parametrize("shape", ["ragged", "dirty"])
def test_per_pair_split(shape):
    """mate-1 lengths of 0 .. 160 move r1 from pair to pair; dirty: CRLF, trailing blanks, quality bytes >= 128, quality
    lines of another length.  The UMIs are whatever the mates hold at the parts' positions"""
    lib = PC.pair_library(200, UP.LEN, 1, 1, 21)
    fq1, fq2 = PC.make_pairs(lib, UP.LEN, list(UP.ST1), list(UP.ST2), True, 2000, seed=31 if shape == "ragged" else 32,
                             ragged=True, dirty=shape == "dirty")
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, True, UP.TWO, miss=1)
    got, table, _, n = emu_result(lib, fq1, fq2, UP.TWO, True, miss=1)
    assert want.uncovered == 0 and n == 2000
    assert got == wanted(want) and table == UP.table_of(want)
    assert want.ok > 200 and want.bad > 200


def test_growth_pieces_and_reuse():
    lib, fq1, fq2 = UP.many()
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, True, (None, UP.UMI2), miss=1)
    got, table, rehashes, n = emu_result(lib, fq1, fq2, (None, UP.UMI2), True, slots=64, per=150, miss=1)
    assert want.uncovered == 0 and n == 6000 and rehashes >= 5
    assert got == wanted(want) and table == UP.table_of(want) and sum(got[2]) > 3000
    e = UPEmu(lib, (None, UP.UMI2), True, slots=64, keep=False, miss=1)
    e.count(fq1, fq2)
    assert e.read()[0] == wanted(want)
    e.reset()
    blib, b1, b2 = UP.base(True)
    assert blib == lib
    e.count(b1, b2)
    assert e.read()[0] == wanted(UP.expect(lib, b1, b2, UP.ST1, UP.ST2, UP.LEN, True, (None, UP.UMI2), miss=1))
    e.close()


def test_the_twin_under_sanitizers(tmp_path):
    """the same host code as a stand-alone program with -fsanitize=address,undefined over its built-in sample"""
    exe = str(tmp_path / "umi_pair_emu")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DF2Q_UMI_PAIR_EMU_MAIN",
                           "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", exe, SRC])
    done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE_ARGV = ["-c", "--s", "x", "--g", "y", "--o", "z"]
PE = ["--pe", "--st2", "0"]


@pytest.mark.parametrize("argv,words", [
    (["--umi1", "20,6"], ["--umi1", "--pe"]), (["--umi2", "12,8"], ["--umi2", "--pe"]),
    (["--umi1", "20,6", "--umi2", "12,8"], ["--umi1", "--umi2", "--pe"]),
    (PE + ["--umi2", "12,8", "--umi", "20,8"], ["--umi", "--pe"]),
    (PE + ["--umi1", "0,4", "--mo", "EC"], ["--umi1", "--mo EC"]), (PE + ["--umi2", "0,4", "--mo", "EC"], ["--umi2", "--mo EC"]),
    (PE + ["--umi1", "20,9", "--umi2", "12,8"], ["--umi1", "--umi2", "16"]),
    (PE + ["--umi1", "20"], ["--umi1", "S,L"]), (PE + ["--umi2", "20,0"], ["--umi2", "S,L"]), (PE + ["--umi2", "20,17"], ["--umi2", "S,L"]),
    (PE + ["--umi1=-1,8"], ["--umi1", "S,L"]), (PE + ["--umi2", "a,b"], ["--umi2", "S,L"]), (PE + ["--umi1", "1,2,3"], ["--umi1", "S,L"]),
    (PE + ["--umi", "20,8"], ["--umi", "--pe", "--umi1", "--umi2"]),
    (PE + ["--mu", "1"], ["--mu", "--umi"]), (PE + ["--umi2", "12,8", "--mur", "directional"], ["--mur", "--mu 1"])])
def test_command_line_refusals(argv, words, capsys):
    with pytest.raises(SystemExit):
        fast2q.input_parser(BASE_ARGV + argv)
    said = capsys.readouterr().out
    assert "FATAL" in said and all(w in said for w in words), said


def test_command_line_takes_the_flags(tmp_path, capsys, monkeypatch):
    for name in ("a_R1.fastq", "a_R2.fastq"):
        (tmp_path / name).write_bytes(b"@r\nACGT\n+\nIIII\n")
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path / "never")] + PE
    plain = fast2q.input_parser(argv)
    assert "umi_paired" not in plain and "umi" not in plain
    kw_plain = fast2q._counter_kwargs(plain)
    assert set(kw_plain) == {"mode", "miss", "phred", "length", "start", "upstream", "downstream", "miss_search_up", "miss_search_down",
                             "qual_up", "qual_down", "device", "start2", "rc2"}
    seen = {}
    for extra, parts in ((["--umi2", "12,8"], (None, (12, 8))), (["--umi1", "20,6"], ((20, 6), None)),
                         (["--umi1", "20,6", "--umi2", "12,10"], ((20, 6), (12, 10)))):
        p = fast2q.input_parser(argv + extra)
        assert p["umi_paired"] == parts and p["used_cmd"].endswith(" ".join(extra)) and fast2q.umi_length(p) == sum(x[1] for x in parts if x)
        # a run without the flags has the same parameter dictionary
        assert {k: v for k, v in p.items() if k not in ("umi_paired", "used_cmd")} == {k: v for k, v in plain.items() if k != "used_cmd"}
        kw = fast2q._counter_kwargs(p)
        assert kw["umi_paired"] == parts and {k: v for k, v in kw.items() if k != "umi_paired"} == kw_plain
        seen[parts] = tuple(sorted((k, str(v)) for k, v in kw.items()))
    assert len(set(seen.values())) == 3                             # two part layouts never share a context
    p = fast2q.input_parser(argv + ["--umi2", "12,8", "--mu", "1", "--mur", "directional"])
    assert p["umi_mismatch"] == 1 and p["umi_rule"] == "directional" and fast2q._counter_kwargs(p)["umi_reads"] is True
    assert "umi_reads" not in fast2q._counter_kwargs(fast2q.input_parser(argv + ["--umi2", "12,8", "--mu", "1"]))
    assert fast2q.umi_length(plain) == 0 and fast2q.umi_length(fast2q.input_parser(BASE_ARGV + ["--umi", "3,7"])) == 7
    # several ranks: refused before any output directory exists, and again where a sample would be counted
    p = fast2q.input_parser(argv + ["--umi2", "12,8"])
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(dict(p))
    said = capsys.readouterr().out
    assert "FATAL" in said and "--umi1 / --umi2" in said and "several ranks" in said
    p["Progress bar"] = False
    with pytest.raises(RuntimeError, match="--umi1 / --umi2.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a_R1.fastq"), {"ACGT": fast2q.Features("g", 0)}, p, {})
    assert not (tmp_path / "never").exists()


def test_parameter_print_out_and_run_header_name_the_parts(capsys, tmp_path):
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path)] + PE
    p = fast2q.initializer(fast2q.input_parser(argv + ["--umi1", "20,6", "--umi2", "12,10"]))
    said = capsys.readouterr().out
    assert "UMI part in mate 1, start position: 20, length: 6bp" in said and "UMI part in mate 2, start position: 12, length: 10bp" in said
    head = fast2q.run_headers(p)
    assert "#UMI in mate 1, start, length: 20,6" in head and "#UMI in mate 2, start, length: 12,10" in head
    assert head.index("#UMI in mate 1, start, length: 20,6") < head.index("#UMI in mate 2, start, length: 12,10")
    p = fast2q.initializer(fast2q.input_parser(argv + ["--umi2", "12,8"]))
    said = capsys.readouterr().out
    assert "UMI part in mate 2, start position: 12, length: 8bp" in said and "UMI part in mate 1" not in said
    head = fast2q.run_headers(p)
    assert "#UMI in mate 2, start, length: 12,8" in head and not any("UMI in mate 1" in line for line in head)
    plain = fast2q.initializer(fast2q.input_parser(argv))
    assert "UMI" not in capsys.readouterr().out and not any("UMI" in line for line in fast2q.run_headers(plain))


def test_header_declares_the_call_and_the_binding_exports_it():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    assert re.search(r"\bint\s+f2q_set_umi_paired\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int32_t\s+start1\s*,\s*int32_t\s+length1\s*,\s*int32_t\s+start2\s*,"
                     r"\s*int32_t\s+length2\s*\)\s*;", text)
    assert "f2q_set_umi_paired" in binding.EXPORTS
    declared = set(re.findall(r"\b(f2q_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(binding.EXPORTS)
    assert re.search(r"#define\s+F2Q_ABI_VERSION\s+1\b", text)
    if os.path.exists(binding.LIB_PATH):
        L = binding.load()
        assert all(hasattr(L, s) for s in binding.EXPORTS)
