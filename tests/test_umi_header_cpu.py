"""--umih without a GPU: the header parse of f2q_device.h (header_umi_codes), the host packer's array (frame_fastq +
header_umis of f2q_host.h) and the lane logic of the header instances of k_count_umi (general_read with a UmiHeaderHook),
compiled for the host by tests/emu/f2q_umi_header_emu.cpp, against the plain-Python rule and expectation of
tests/umi_header_cases.py -- the inputs of the GPU list in tests/test_umi_header_gpu.py; the command line's flag, refusals
and print-outs; the header against the binding's export list."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import umi_header_cases as HC
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_umi_header_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_umi_header_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
_L = []


def _lib():
    if _L:
        return _L[0]
    deps = [SRC] + [os.path.join(TESTS, "emu", f) for f in ("f2q_umi_emu.cpp", "f2q_emu.cpp")] + \
           [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h", "f2q_synth.h", "f2q_reader.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", LIB, SRC, "-lz", "-lpthread"])
    L = C.CDLL(LIB)
    vp, i64p, u32p = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    L.uemu_create.restype = vp
    L.uemu_create.argtypes = [C.POINTER(binding.Params), C.c_int32, C.c_int32, C.c_uint64]
    L.uemu_destroy.argtypes = [vp]
    L.uemu_set_features.argtypes = [vp, C.c_char_p, u32p, C.c_uint32]
    L.uemu_read.restype = C.c_longlong
    L.uemu_read.argtypes = [vp, i64p, i64p, i64p, i64p]
    L.hemu_parse.restype = C.c_int
    L.hemu_parse.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    L.hemu_array.restype = C.c_size_t
    L.hemu_array.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.c_size_t]
    L.hemu_count_block.restype = C.c_size_t
    L.hemu_count_block.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int]
    L.hemu_pairs.restype = C.c_size_t
    L.hemu_pairs.argtypes = [vp, u32p, u32p, u32p, C.c_size_t]
    _L.append(L)
    return L


def parse(line, sep, length):
    """header_umi_codes on one line: the codes, or None"""
    codes = C.c_uint32(0xDEADBEEF)
    return codes.value if _lib().hemu_parse(line, len(line), sep, length, C.byref(codes)) else None


def host_array(fq, sep, length):
    L = _lib()
    n = L.hemu_array(fq, len(fq), sep, length, None, 0)
    out = (C.c_uint64 * max(n, 1))()
    assert L.hemu_array(fq, len(fq), sep, length, out, n) == n
    return list(out)[:n]


def emu_result(lib, fq, umi, keep=False, slots=0, pieces=1, **run):
    """(counts, stats, umis, valid, invalid), the (feature, codes, reads) table, rehashes -- the text counted in `pieces` blocks"""
    L = _lib()
    p, _keep = binding.make_params(mode="C", **run)
    h = C.c_void_p(L.uemu_create(C.byref(p), 0, umi[1], slots))
    assert h
    enc = [s.encode() for s in lib]
    offs = np.zeros(len(enc) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(b) for b in enc])
    L.uemu_set_features(h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc))
    lines = fq.split(b"\n")
    n_rec = (len(lines) - 1) // 4
    per = -(-n_rec // pieces)
    for i in range(0, n_rec, per):
        piece = b"".join(line + b"\n" for line in lines[4 * i:4 * min(i + per, n_rec)])
        assert L.hemu_count_block(h, piece, len(piece), umi[0], umi[1], int(keep)) == len(piece)
    counts, umis = (C.c_int64 * len(lib))(), (C.c_int64 * len(lib))()
    stats, extra = (C.c_int64 * 5)(), (C.c_int64 * 2)()
    rehashes = L.uemu_read(h, counts, stats, umis, extra)
    assert rehashes >= 0
    cap = sum(umis) + 1
    f, codes, reads = ((C.c_uint32 * cap)() for _ in range(3))
    n = L.hemu_pairs(h, f, codes, reads, cap)
    assert n == sum(umis)
    L.uemu_destroy(h)
    return (list(counts), list(stats), list(umis), extra[0], extra[1]), sorted(zip(f[:n], codes[:n], reads[:n])), rehashes


# ---- the parse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sep,length", [(HC.SEP, 8), (ord(":"), 8), (HC.SEP, 16), (ord("|"), 1)])
def test_parse_function_against_the_rule_on_random_headers(sep, length):
    heads = HC.random_headers(0x20000 + sep + length, 20000 if (sep, length) == (HC.SEP, 8) else 4000, sep, length)
    valid = 0
    for h in heads:
        u = HC.header_umi(h, sep, length)
        assert parse(h, sep, length) == (None if u is None else HC.code_of(u)), h
        valid += u is not None
    assert len(heads) // 10 < valid < len(heads) * 9 // 10 or length != 8          # both verdicts are well covered


def test_parse_function_kind_by_kind():
    for kind, ok in HC.INVALID_KINDS.items():
        head, sep = HC.invalid_header(kind, 7, b"GATTACAG")
        assert (HC.header_umi(head, sep, 8) is not None) == ok, kind
        assert parse(head, sep, 8) == (HC.code_of(b"GATTACAG") if ok else None), kind
    assert parse(b"@x_" + b"T" * 16, HC.SEP, 16) == 0xFFFFFFFF and parse(b"@x_" + b"A" * 16, HC.SEP, 16) == 0
    assert parse(b"@x_" + b"A" * 17, HC.SEP, 16) is None and parse(b"", HC.SEP, 8) is None and parse(b"_", HC.SEP, 8) is None
    assert parse(b"@x_ACGTACGT_", HC.SEP, 8) is None and parse(b"@x_ACGT_ACGT", HC.SEP, 4) == HC.code_of(b"ACGT")


# ---- the host packer's array ---------------------------------------------------------------------------------------------
def test_host_packers_array_against_the_rule():
    lib, fq, run, (sep, length) = HC.base()
    assert host_array(fq, sep, length) == [HC.entry_of(h, sep, length) for h, _, _ in HC.records(fq)]
    for kind, (text, sep) in HC.invalid()[1].items():
        want = [HC.entry_of(h, sep, 8) for h, _, _ in HC.records(text)]
        assert host_array(text, sep, 8) == want and all(bool(w) == HC.INVALID_KINDS[kind] for w in want), kind
    # no final newline; an incomplete record at the end; an empty text
    lib, few, _, _ = HC.edge(3)
    assert len(host_array(few[:-1], HC.SEP, 8)) == 3 and host_array(few[:-1], HC.SEP, 8) == host_array(few, HC.SEP, 8)
    assert host_array(few + b"@r9_ACGTACGT\nACGT\n+\n", HC.SEP, 8) == host_array(few, HC.SEP, 8)
    assert host_array(b"", HC.SEP, 8) == []
    lib, wide, _, (sep, length) = HC.wide16()
    got = host_array(wide, sep, length)
    assert got[0] == (1 << 32) | 0xFFFFFFFF and got[1] == 1 << 32 and got == [HC.entry_of(h, sep, length) for h, _, _ in HC.records(wide)]


# ---- the lane logic of the header hook -----------------------------------------------------------------------------------
@pytest.mark.parametrize("miss", [0, 1])
def test_base_shape_vs_expectation(miss):
    lib, fq, run, umi = HC.base()
    want = HC.expect(lib, fq, umi, miss=miss, **run)
    got, table, _ = emu_result(lib, fq, umi, keep=True, miss=miss, **run)
    assert got == HC.wanted(want) and table == HC.table_of(want)
    assert want.ok + want.bad == want.stats[1] + want.stats[2] and want.bad == 0 and want.ok > 2000
    assert sum(len(c) for c in want.per) < want.ok - 100                           # many reads repeat a (feature, UMI) pair
    got, table, rehashes = emu_result(lib, fq, umi, slots=64, pieces=9, miss=miss, **run)   # the set rehashes across blocks
    assert got == HC.wanted(want) and [t[:2] for t in table] == [t[:2] for t in HC.table_of(want)] and rehashes >= 1


def test_invalid_kinds_and_sixteen_bases():
    lib, kinds = HC.invalid()
    for kind, (fq, sep) in kinds.items():
        want = HC.expect(lib, fq, (sep, 8), miss=1, **HC.UC.RUN)
        got, table, _ = emu_result(lib, fq, (sep, 8), keep=True, miss=1, **HC.UC.RUN)
        assert got == HC.wanted(want) and table == HC.table_of(want), kind
        assert (want.ok, want.bad) == ((12, 0) if HC.INVALID_KINDS[kind] else (0, 12)) and sum(len(c) for c in want.per) == want.ok, kind
    lib, fq, run, umi = HC.wide16()
    want = HC.expect(lib, fq, umi, miss=1, **run)
    got, table, _ = emu_result(lib, fq, umi, keep=True, miss=1, **run)
    assert got == HC.wanted(want) and table == HC.table_of(want)
    assert {c for f, c, n in table} >= {0, 0xFFFFFFFF} and min(f for f, c, n in table) >= 512


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "hemu_main")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DF2Q_UMI_HEADER_EMU_MAIN"] + FLAGS +
                          ["-o", exe, SRC, "-lz", "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 mismatches" in out.stdout, out.stdout + out.stderr


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE_ARGV = ["-c", "--s", "x", "--g", "y", "--o", "z"]


@pytest.mark.parametrize("argv,words", [
    (["--umih", "_,8", "--umi", "20,8"], ["--umih", "--umi", "one source"]),
    (["--umih", "_,8", "--pe", "--st2", "0", "--umi1", "0,8"], ["--umih", "--umi1", "one source"]),
    (["--umih", "_,8", "--pe", "--st2", "0", "--umi2", "0,8"], ["--umih", "--umi2", "one source"]),
    (["--umih", "_,8", "--mo", "EC"], ["--umih", "--mo EC"]),
    (["--umih", "_"], ["--umih", "SEP,L"]), (["--umih", "8"], ["--umih", "SEP,L"]), (["--umih", "_,"], ["--umih", "SEP,L"]),
    (["--umih", "__,8"], ["--umih", "SEP,L"]), (["--umih", ",8"], ["--umih", "SEP,L"]), (["--umih", "_,x"], ["--umih", "SEP,L"]),
    (["--umih", "_,-8"], ["--umih", "SEP,L"]),
    (["--umih", "a,8"], ["--umih", "separator"]), (["--umih", "7,8"], ["--umih", "separator"]), (["--umih", "+,8"], ["--umih", "separator"]),
    (["--umih", " ,8"], ["--umih", "separator"]), (["--umih", "é,8"], ["--umih", "separator"]),
    (["--umih", "_,0"], ["--umih", "between 1 and 16"]), (["--umih", "_,17"], ["--umih", "between 1 and 16"])])
def test_command_line_refusals(argv, words, capsys):
    with pytest.raises(SystemExit):
        fast2q.input_parser(BASE_ARGV + argv)
    said = capsys.readouterr().out
    assert "FATAL" in said and all(w in said for w in words), said


def test_command_line_takes_the_flag_and_refuses_several_ranks(tmp_path, capsys, monkeypatch):
    (tmp_path / "a.fastq").write_bytes(b"@r_ACGTACGT\nACGT\n+\nIIII\n")
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path / "never")]
    p = fast2q.input_parser(argv + ["--umih", "_,8"])
    assert p["umi_header"] == ("_", 8) and fast2q.umi_length(p) == 8
    assert fast2q.input_parser(argv + ["--umih", ":,16"])["umi_header"] == (":", 16)
    assert fast2q.input_parser(argv + ["--umih", ",,4"])["umi_header"] == (",", 4)                # split at the last comma
    plain = fast2q.input_parser(argv)
    assert "umi_header" not in plain and {k: v for k, v in p.items() if k not in ("umi_header", "used_cmd")} == {k: v for k, v in plain.items() if k != "used_cmd"}
    kw, kw_plain = fast2q._counter_kwargs(p), fast2q._counter_kwargs(plain)
    assert kw["umi_header"] == ("_", 8) and "umi_header" not in kw_plain and "umi" not in kw and "umi_reads" not in kw
    assert fast2q._counter_kwargs(dict(p, umi_header=("_", 9))) != kw and fast2q._counter_kwargs(dict(p, umi_header=(":", 8))) != kw
    # --mu 1 and --mur directional take it in place of --umi
    d = fast2q.input_parser(argv + ["--umih", "_,8", "--mu", "1", "--mur", "directional"])
    assert d["umi_mismatch"] == 1 and d["umi_rule"] == "directional" and fast2q._counter_kwargs(d)["umi_reads"] is True
    # with --pe: a paired context that takes the UMI from mate 1's header
    pe = fast2q.input_parser(argv + ["--pe", "--st2", "0", "--rc2", "--umih", "_,8", "--mu", "1", "--mur", "directional"])
    kw = fast2q._counter_kwargs(pe)
    assert kw["umi_header"] == ("_", 8) and kw["start2"] == "0" and kw["rc2"] is True and kw["umi_reads"] is True and "umi_paired" not in kw
    # several ranks: refused before any output directory exists, and again where a sample would be counted
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    for params in (p, pe):
        params["test_mode"] = False
        with pytest.raises(SystemExit):
            fast2q.file_sizer_split(dict(params))
        said = capsys.readouterr().out
        assert "FATAL" in said and "--umih" in said and "several ranks" in said
    p["Progress bar"] = False
    with pytest.raises(RuntimeError, match="--umih.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a.fastq"), {"ACGT": fast2q.Features("g", 0)}, p, {})
    assert not (tmp_path / "never").exists()


def test_parameter_print_out_and_run_header_name_the_source(capsys, tmp_path):
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path)]
    p = fast2q.initializer(fast2q.input_parser(argv + ["--umih", "_,8"]))
    said = capsys.readouterr().out
    assert "UMI in the read header" in said and "'_'" in said and "length: 8bp" in said
    head = fast2q.run_headers(p)
    assert "#UMI in read header, separator, length: _,8" in head and "#UMI start position" not in head
    p = fast2q.initializer(fast2q.input_parser(argv + ["--umih", ":,12", "--mu", "1"]))
    capsys.readouterr()
    head = fast2q.run_headers(p)
    assert "#UMI in read header, separator, length: :,12" in head and "#UMI mismatches collapsed: 1" in head
    assert "#UMI in read header" not in fast2q.run_headers(fast2q.initializer(fast2q.input_parser(argv)))


def test_header_declares_the_call_and_the_binding_exports_it():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    assert re.search(r"\bint\s+f2q_set_umi_header\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int32_t\s+sep\s*,\s*int32_t\s+length\s*\)\s*;", text)
    assert "f2q_set_umi_header" in binding.EXPORTS
    assert "def header_umi(header_line, sep, L):" in text                           # the rule is stated there
    if os.path.exists(binding.LIB_PATH):
        assert hasattr(binding.load(), "f2q_set_umi_header")
