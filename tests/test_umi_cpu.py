"""--umi without a GPU: the lane logic of k_count_umi (general_read with a UmiHook, umi_codes / umi_insert / umi_claim of
f2q_device.h) compiled for the host by tests/emu/f2q_umi_emu.cpp, against the plain-Python expectation of
tests/umi_cases.py -- the inputs of the GPU list in tests/test_umi_gpu.py; f2q_set_umi's argument and state errors
through the ABI (they need the library and a device: marked gpu); the command line's flag and refusals; the header
against the binding's export list."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import umi_cases as UC
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_umi_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_umi_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
_L = []


def _lib():
    if _L:
        return _L[0]
    deps = [SRC, os.path.join(TESTS, "emu", "f2q_emu.cpp")] + [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h", "f2q_synth.h", "f2q_reader.h")]
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
    _L.append(L)
    return L


class UEmu:
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

    def read(self):
        """(counts, stats, umis, umi_reads, umi_failed), rehashes"""
        counts, umis = (C.c_int64 * self.n)(), (C.c_int64 * self.n)()
        stats, extra = (C.c_int64 * 5)(), (C.c_int64 * 2)()
        rehashes = self.L.uemu_read(self.h, counts, stats, umis, extra)
        assert rehashes >= 0                                         # (-1: the overflow flag)
        held, occ, slots = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.L.uemu_set_info(self.h, C.byref(held), C.byref(occ), C.byref(slots))
        assert held.value == occ.value == sum(umis) and 2 * held.value <= max(slots.value, 1)
        return (list(counts), list(stats), list(umis), extra[0], extra[1]), rehashes

    def reset(self):
        self.L.uemu_reset(self.h)

    def close(self):
        self.L.uemu_destroy(self.h)


def emu_result(lib, fq, umi, slots=0, pieces=1, **run):
    e = UEmu(lib, umi, slots, **run)
    recs = fq.split(b"\n@r")                                          # (no quality line of the cases starts with "@r")
    recs = [recs[0]] + [b"@r" + r for r in recs[1:]]
    per = -(-len(recs) // pieces)
    for i in range(0, len(recs), per):
        e.count(b"\n".join(recs[i:i + per]) + (b"\n" if i + per < len(recs) else b""))
    got = e.read()
    e.close()
    return got


@pytest.mark.parametrize("miss", [0, 1])
def test_base_shape_vs_expectation(miss):
    lib, fq, run, umi = UC.base()
    want = UC.expect(lib, fq, umi, miss=miss, **run)
    got, _ = emu_result(lib, fq, umi, miss=miss, **run)
    assert got == want
    counts, stats, umis, ok, bad = want
    assert ok + bad == stats[1] + stats[2] and bad == 0 and (miss == 0 or stats[2] > 0)
    assert sum(umis) < ok - 100 and max(umis) <= 48                  # many reads repeat a (feature, UMI) pair


def test_invalid_umis_move_reads_between_the_two_counters():
    lib, fq, kinds = UC.invalid()
    valid_kinds = {"whole", "cut28", "lower", "q29_last", "lowq_outside"}
    for phred, also in ((30, set()), (0, {"lowq_first", "lowq_last"})):
        want = UC.expect(lib, fq, (UC.S, UC.L), miss=1, phred=phred, start="0", length=20)
        got, _ = emu_result(lib, fq, (UC.S, UC.L), miss=1, phred=phred, start="0", length=20)
        assert got == want
        n_ok = sum(k in valid_kinds | also for k in kinds)
        assert (want[3], want[4]) == (n_ok, len(kinds) - n_ok)       # every read is assigned: the window is whole and clean
        assert sum(want[2]) == n_ok                                  # every UMI is distinct


def test_imperfect_hits_share_the_feature_s_set():
    lib, fq, pairs = UC.imperfect()
    want = UC.expect(lib, fq, (UC.S, UC.L), miss=1, **UC.RUN)
    got, _ = emu_result(lib, fq, (UC.S, UC.L), miss=1, **UC.RUN)
    assert got == want
    assert {f: n for f, n in enumerate(got[2]) if n} == pairs and got[3] == 7 and got[1][2] == 5


def test_sixteen_base_umi_over_the_feature_window():
    lib, fq, run, umi = UC.wide()
    want = UC.expect(lib, fq, umi, miss=1, **run)
    got, _ = emu_result(lib, fq, umi, miss=1, **run)
    assert got == want
    assert sum(got[2][:512]) == 0 and got[2][600] >= 1 and got[2][601] >= 1 and max(got[2]) > 1


def test_anchored_run():
    lib, fq, run, umi = UC.anchored()
    want = UC.expect(lib, fq, umi, miss=1, **run)
    got, _ = emu_result(lib, fq, umi, miss=1, **run)
    assert got == want
    assert want[3] > 0 and want[4] > 0 and want[1][3] + want[1][4] > 0


def test_growth_from_a_small_set_changes_nothing():
    lib, fq, run, umi = UC.base()
    want = UC.expect(lib, fq, umi, miss=1, **run)
    got, rehashes = emu_result(lib, fq, umi, slots=64, pieces=140, miss=1, **run)
    assert got == want and rehashes >= 5


def test_reset_and_reuse():
    lib, fq, run, umi = UC.base()
    fq2 = UC.sample(0x5EC0, n_reads=1500)
    e = UEmu(lib, umi, miss=1, **run)
    e.count(fq)
    assert e.read()[0] == UC.expect(lib, fq, umi, miss=1, **run)
    e.reset()
    e.count(fq2)
    assert e.read()[0] == UC.expect(lib, fq2, umi, miss=1, **run)
    e.close()


# ---- the ABI's argument and state errors (they need the library and a device) ----------------------------------------
@pytest.mark.gpu
def test_set_umi_argument_and_state_errors():
    lib = UC.library()[:8]
    for bad in ((-1, 8), (0, 0), (0, 17), (5, -3)):
        with pytest.raises(binding.F2QError) as exc:
            binding.Counter(features=lib, umi=bad)
        assert exc.value.code == -1
    with pytest.raises(binding.F2QError) as exc:
        binding.Counter(mode="EC", umi=(0, 8))
    assert exc.value.code == -7
    with pytest.raises(binding.F2QError) as exc:
        binding.Counter(features=None, start="0", start2="0", umi=(0, 8))
    assert exc.value.code == -7
    with binding.Counter(features=lib, umi=(20, 8)) as c:
        with pytest.raises(binding.F2QError) as exc:
            c.set_umi(20, 8)
        assert exc.value.code == -7
        umis, ok, bad = c.read_umis()                                # nothing counted yet
        assert list(umis) == [0] * 8 and (ok, bad) == (0, 0)
    with binding.Counter(features=lib) as c:
        with pytest.raises(binding.F2QError) as exc:
            c.read_umis()
        assert exc.value.code == -7
        c.count_block(b"@r\nACGT\n+\nIIII\n")
        with pytest.raises(binding.F2QError) as exc:                 # after a counting call
            c.set_umi(20, 8)
        assert exc.value.code == -7


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE_ARGV = ["-c", "--s", "x", "--g", "y", "--o", "z"]


@pytest.mark.parametrize("argv,word", [(["--umi", "20,8", "--mo", "EC"], "--mo EC"), (["--umi", "20,8", "--pe", "--st2", "0"], "--pe"),
                                       (["--umi", "20"], "S,L"), (["--umi", "20,0"], "S,L"), (["--umi", "20,17"], "S,L"),
                                       (["--umi=-1,8"], "S,L"), (["--umi", "a,b"], "S,L"), (["--umi", "1,2,3"], "S,L")])
def test_command_line_refusals(argv, word, capsys):
    with pytest.raises(SystemExit):
        fast2q.input_parser(BASE_ARGV + argv)
    said = capsys.readouterr().out
    assert "--umi" in said and word in said and "FATAL" in said


def test_command_line_takes_the_flag_and_refuses_several_ranks(tmp_path, capsys, monkeypatch):
    (tmp_path / "a.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path)]
    p = fast2q.input_parser(argv + ["--umi", "20,8"])
    assert p["umi"] == (20, 8) and p["used_cmd"].endswith("--umi 20,8")
    plain = fast2q.input_parser(argv)
    assert "umi" not in plain and {k: v for k, v in p.items() if k not in ("umi", "used_cmd")} == {k: v for k, v in plain.items() if k != "used_cmd"}
    # the context cache key tells a UMI context from a plain one, and two windows from each other
    kw, kw_plain = fast2q._counter_kwargs(p), fast2q._counter_kwargs(plain)
    assert kw["umi"] == (20, 8) and "umi" not in kw_plain
    assert fast2q._counter_kwargs(dict(p, umi=(20, 9))) != kw
    p["test_mode"] = False
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(dict(p))
    said = capsys.readouterr().out
    assert "--umi" in said and "several ranks" in said
    p["Progress bar"] = False
    with pytest.raises(RuntimeError, match="--umi.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a.fastq"), {"ACGT": fast2q.Features("g", 0)}, p, {})


def test_parameter_print_out_and_stats_header_name_the_window(capsys, tmp_path):
    p = fast2q.input_parser(["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path), "--umi", "20,8"])
    p = fast2q.initializer(p)
    assert "UMI start position in the read: 20, length: 8bp" in capsys.readouterr().out
    assert "#UMI start position in the read, length: 20,8" in fast2q.run_headers(p)


def test_header_declares_the_umi_calls_and_the_binding_exports_them():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    for name in ("f2q_set_umi", "f2q_read_umis"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in binding.EXPORTS
    assert re.search(r"#define\s+F2Q_ABI_VERSION\s+1\b", text)
    if os.path.exists(binding.LIB_PATH):
        L = binding.load()
        assert all(hasattr(L, s) for s in binding.EXPORTS)
