"""--sb without a GPU: the barcode rule of f2q_device.h (demux_decide / demux_find), the host's table builder (demux_validate /
demux_build of f2q_host.h) and the lane logic of k_count_demux (general_read with a DemuxHook), compiled for the host by
tests/emu/f2q_demux_emu.cpp, against the plain-Python rule and expectation of tests/demux_cases.py -- the inputs of the GPU
list in tests/test_demux_gpu.py; the refusals that need no device; the command line's flags, refusals and print-outs; the
header against the binding's export list."""
import ctypes as C
import importlib
import itertools
import os
import random
import re
import subprocess

import numpy as np
import pytest

import demux_cases as DC
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_demux_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_demux_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
_L = []


def _lib():
    if _L:
        return _L[0]
    deps = [SRC, os.path.join(TESTS, "emu", "f2q_emu.cpp")] + [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h", "f2q_synth.h", "f2q_reader.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", LIB, SRC, "-lz", "-lpthread"])
    L = C.CDLL(LIB)
    vp, i64p, u32p, i32 = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.c_int32
    L.demu_validate.argtypes = [C.c_char_p, C.c_uint32, i32, i32, i32, C.c_char_p, C.c_size_t]
    L.demu_table.restype = vp
    L.demu_table.argtypes = [C.c_char_p, C.c_uint32, i32, i32, i32]
    L.demu_info.argtypes = [vp, C.POINTER(C.c_uint64), u32p, u32p]
    L.demu_slots.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.demu_decide.argtypes = [vp, i32, C.c_char_p, i32, C.c_char_p, i32, u32p]
    L.demu_create.restype = vp
    L.demu_create.argtypes = [C.POINTER(binding.Params), C.c_char_p, C.c_uint32, i32, i32, i32]
    L.demu_destroy.argtypes = [vp]
    L.demu_set_features.argtypes = [vp, C.c_char_p, u32p, C.c_uint32]
    L.demu_count_block.restype = C.c_size_t
    L.demu_count_block.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.demu_read.argtypes = [vp, i64p, i64p, i64p, i64p, i64p]
    L.demu_reset.argtypes = [vp]
    _L.append(L)
    return L


class Table:
    """the host-built table of a barcode set and the device rule on it"""

    def __init__(self, barcodes, start, miss):
        self.L, self.n = _lib(), len(barcodes)
        self.h = C.c_void_p(self.L.demu_table(b"".join(barcodes), len(barcodes), len(barcodes[0]), start, miss))
        assert self.h

    def decide(self, seq, qual, phred=30):
        sample = C.c_uint32(0xDEAD)
        v = self.L.demu_decide(self.h, phred, seq, len(seq), qual, len(qual), C.byref(sample))
        return sample.value, v

    def info(self):
        slots, entries, amb = C.c_uint64(), C.c_uint32(), C.c_uint32()
        self.L.demu_info(self.h, C.byref(slots), C.byref(entries), C.byref(amb))
        return slots.value, entries.value, amb.value

    def slots(self):
        out = (C.c_uint64 * self.info()[0])()
        self.L.demu_slots(self.h, out)
        return list(out)

    def close(self):
        self.L.demu_destroy(self.h)


def emu_result(lib, fq, barcodes, at, miss_bc, per=0, **run):
    """(counts, stats, matrix, sample_stats, verdicts) as lists -- the text counted in pieces of `per` records (0: one block)"""
    L = _lib()
    p, _keep = binding.make_params(mode="C", **run)
    h = C.c_void_p(L.demu_create(C.byref(p), b"".join(barcodes), len(barcodes), len(barcodes[0]), at, miss_bc))
    assert h
    enc = [s.encode() for s in lib]
    offs = np.zeros(len(enc) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(b) for b in enc])
    L.demu_set_features(h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc))
    for piece in (DC.pieces(fq, per) if per else [fq]):
        assert L.demu_count_block(h, piece, len(piece)) == len(piece)
    nf, rows = len(lib), len(barcodes) + 1
    counts, stats, matrix, sstats, verdicts = (C.c_int64 * nf)(), (C.c_int64 * 5)(), (C.c_int64 * (rows * nf))(), (C.c_int64 * (rows * 5))(), (C.c_int64 * 5)()
    L.demu_read(h, counts, stats, matrix, sstats, verdicts)
    L.demu_destroy(h)
    return (list(counts), list(stats), [list(matrix[b * nf:(b + 1) * nf]) for b in range(rows)],
            [list(sstats[b * 5:(b + 1) * 5]) for b in range(rows)], list(verdicts))


# ---- the rule ------------------------------------------------------------------------------------------------------------
def test_exhaustive_three_base_windows_against_every_subset_of_six_barcodes():
    pool = [b"ACG", b"ACT", b"AGT", b"TTT", b"AAA", b"CGA"]                      # one and two bases apart, A x 3 and T x 3
    windows = [bytes(w) for w in itertools.product(b"ACGTN", repeat=3)]
    assert len(windows) == 125
    checked = 0
    for k in range(1, 7):
        for subset in itertools.combinations(pool, k):
            for M in (0, 1):
                t = Table(subset, 2, M)
                for w in windows:
                    seq = b"GG" + w + b"C"
                    assert t.decide(seq, b"IIIIII") == DC.barcode_of(seq, b"IIIIII", 2, 3, 30, subset, M), (subset, M, w)
                    checked += 1
                t.close()
    assert checked == 63 * 2 * 125


def test_sixteen_base_barcodes_with_the_zero_and_the_all_ones_code():
    rng = random.Random(0x16)
    bcs = [b"A" * 16, b"T" * 16] + [DC.UC.rand_seq(rng, 16) for _ in range(10)]
    for M in (0, 1):
        t = Table(bcs, 0, M)
        windows = [b"A" * 16, b"T" * 16, b"a" * 16, b"A" * 15 + b"N", b"N" + b"T" * 15, b"C" * 16, b"G" * 16]
        for _ in range(400):
            w = bytearray(bcs[rng.randrange(len(bcs))])
            for _ in range(rng.choice((0, 0, 1, 1, 2))):
                w[rng.randrange(16)] = rng.choice(b"ACGTNacgt")
            windows.append(bytes(w))
        seen = set()
        for w in windows:
            got = t.decide(w, b"I" * 16)
            assert got == DC.barcode_of(w, b"I" * 16, 0, 16, 30, bcs, M), (M, w)
            seen.add(got[1])
        assert t.decide(b"A" * 16, b"I" * 16) == (0, DC.EXACT) and t.decide(b"T" * 16, b"I" * 16) == (1, DC.EXACT)
        assert t.decide(b"C" * 16, b"I" * 16) == (len(bcs), DC.NO_MATCH)
        assert seen >= ({DC.EXACT, DC.ONE_MISMATCH, DC.NO_MATCH} if M else {DC.EXACT, DC.NO_MATCH})
        codes = {s & 0xFFFFFFFF for s in t.slots() if s}
        assert {0, 0xFFFFFFFF} <= codes                                              # both live next to the empty mark (the word 0)
        t.close()


def test_unreadable_windows_and_the_phred_rule():
    bcs = DC.barcodes()
    t = Table(bcs, 20, 1)
    seq = b"C" * 20 + bcs[5] + b"GG"
    for qual, phred in ((b"I" * 30, 30), (b"I" * 27, 30), (b"I" * 28, 30), (b"I" * 27 + b"#II", 30), (b"I" * 27 + b"=II", 30), (b"I" * 27 + b">II", 30),
                        (b"I" * 27 + b"#II", 0), (b"I" * 19 + b"#" + b"I" * 10, 30), (b"I" * 28 + b"#I", 30), (b"I" * 27 + b" II", 30)):
        assert t.decide(seq, qual, phred) == DC.barcode_of(seq, qual, 20, 8, phred, bcs, 1), (qual, phred)
    assert t.decide(seq[:27], b"I" * 30) == (12, DC.UNREADABLE) and t.decide(seq[:28], b"I" * 28) == (5, DC.EXACT)
    assert t.decide(b"", b"") == (12, DC.UNREADABLE)
    t.close()


# ---- the table -----------------------------------------------------------------------------------------------------------
def _brute_neighbours(bcs):
    """{window: set of barcodes one base away} over every substitution neighbour"""
    near = {}
    for b, s in enumerate(bcs):
        for j in range(len(s)):
            for c in b"ACGT":
                if c != s[j]:
                    near.setdefault(s[:j] + bytes([c]) + s[j + 1:], set()).add(b)
    return near


def _code(w):
    return sum(b"ACGT".index(c) << (2 * j) for j, c in enumerate(w))


@pytest.mark.parametrize("shape", ["nb1", "nb1024", "l1", "l16"])
def test_table_load_and_ambiguous_marks_against_brute_force(shape):
    bcs, start, _ = DC.shapes()[shape]
    near = _brute_neighbours(bcs)
    exact = {s: b for b, s in enumerate(bcs)}
    for M in (0, 1):
        t = Table(bcs, start, M)
        slots, entries, amb = t.info()
        want = dict((_code(s), (b, 0, 0)) for s, b in exact.items())
        if M:
            for w, who in near.items():
                if w not in exact:
                    want[_code(w)] = (min(who) if len(who) == 1 else None, 1, int(len(who) > 1))
        assert slots & (slots - 1) == 0 and slots >= 2 * entries and entries == len(want)
        assert amb == sum(v[2] for v in want.values())
        held = {}
        for s in t.slots():
            if s:
                assert s >> 63 == 1
                held[s & 0xFFFFFFFF] = ((s >> 32) & 0x3FF, (s >> 48) & 1, (s >> 49) & 1)
        assert set(held) == set(want)
        for code, (b, dist, ambiguous) in want.items():
            assert held[code][1:] == (dist, ambiguous) and (ambiguous or held[code][0] == b), code
        t.close()


@pytest.mark.parametrize("shape", ["nb1", "nb1024", "l1", "l1_three", "l16"])
@pytest.mark.parametrize("miss_bc", [0, 1])
def test_shapes_vs_expectation(shape, miss_bc):
    bcs, start, fq = DC.shapes()[shape]
    lib = DC.library()
    want = DC.expect(lib, fq, bcs, start, miss_bc, miss=1, **DC.RUN)
    got = emu_result(lib, fq, bcs, start, miss_bc, miss=1, **DC.RUN)
    assert got == want
    DC.check_invariants(*got)
    assert want[4][DC.EXACT] > 50 and (miss_bc == 0 or want[4][DC.ONE_MISMATCH] + want[4][DC.AMBIGUOUS] > 10)


# ---- the lane logic of the hook ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("miss", [0, 1])
@pytest.mark.parametrize("miss_bc", [0, 1])
def test_base_shape_vs_expectation(miss, miss_bc):
    lib, fq, run, bcs, start = DC.base()
    want = DC.expect(lib, fq, bcs, start, miss_bc, miss=miss, **run)
    got = emu_result(lib, fq, bcs, start, miss_bc, miss=miss, **run)
    assert got == want
    DC.check_invariants(*want)
    assert got == emu_result(lib, fq, bcs, start, miss_bc, per=30, miss=miss, **run)            # the state lives across blocks
    assert sum(want[0]) > 1500 and sum(want[2][len(bcs)]) > 100 and min(sum(row) for row in want[2][:len(bcs)]) > 20


def test_long_reads_and_anchored_runs():
    for case in (DC.long_reads(), DC.anchored()):
        lib, fq, run, bcs, start = case
        want = DC.expect(lib, fq, bcs, start, 1, miss=1, **run)
        assert emu_result(lib, fq, bcs, start, 1, miss=1, **run) == want
        DC.check_invariants(*want)
        assert all(want[4][k] > 10 for k in (DC.EXACT, DC.ONE_MISMATCH, DC.UNREADABLE)), want[4]


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "demu_main")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DF2Q_DEMUX_EMU_MAIN"] + FLAGS +
                          ["-o", exe, SRC, "-lz", "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout + out.stderr


# ---- refusals that need no device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seqs,n,length,start,miss,words", [
    (b"ACGT", 0, 4, 0, 0, ["between 1 and 1024"]), (b"A" * 1025, 1025, 1, 0, 0, ["between 1 and 1024"]),
    (b"", 1, 0, 0, 0, ["1 .. 16"]), (b"A" * 17, 1, 17, 0, 0, ["1 .. 16"]),
    (b"ACGT", 1, 4, -1, 0, [">= 0"]), (b"ACGT", 1, 4, 0, 2, ["0 or 1"]), (b"ACGT", 1, 4, 0, -1, ["0 or 1"]),
    (b"ACGTACNT", 2, 4, 0, 0, ["barcode 1", "ACNT", "A/C/G/T"]), (b"AC-T", 1, 4, 0, 1, ["barcode 0", "AC-T"]),
    (b"ACGTTTTTacgt", 3, 4, 0, 0, ["barcode 2", "ACGT", "repeats barcode 0"])])
def test_argument_refusals_name_the_barcode(seqs, n, length, start, miss, words):
    msg = C.create_string_buffer(512)
    assert _lib().demu_validate(seqs, n, length, start, miss, msg, 512) == -1
    assert all(w in msg.value.decode() for w in words), msg.value
    assert _lib().demu_table(seqs, n, length, start, miss) is None


def test_arguments_taken():
    msg = C.create_string_buffer(512)
    assert _lib().demu_validate(b"acgtTTTT", 2, 4, 0x3FFFFFFF, 1, msg, 512) == 0 and msg.value == b""
    t = Table([b"acgt", b"TTTT"], 0, 0)
    assert t.decide(b"ACGT", b"IIII") == (0, DC.EXACT) and t.decide(b"tttt", b"IIII") == (1, DC.EXACT)
    t.close()


def test_null_context_is_refused_by_the_library():
    L = binding.load()                                               # (the built library, as tests/test_abi_and_host.py loads it)
    assert L.f2q_set_sample_barcodes(None, b"ACGT", 1, 4, 0, 0) == -1 and L.f2q_read_demux(None, None, None, None) == -1


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE_ARGV = ["-c", "--s", "x", "--g", "y", "--o", "z"]


@pytest.fixture()
def sb(tmp_path):
    path = tmp_path / "samples.csv"
    path.write_text("".join(f"s{i:02d},{b.decode()}\n" for i, b in enumerate(DC.barcodes())))
    return str(path)


@pytest.mark.parametrize("argv,words", [
    (["--sbs", "20"], ["--sbs", "--sb"]), (["--sbm", "1"], ["--sbm", "--sb"]),
    (["--sb", "SB", "--mo", "EC"], ["--sb", "--mo EC"]), (["--sb", "SB", "--pe", "--st2", "0"], ["--sb", "--pe"]),
    (["--sb", "SB", "--umi", "20,8"], ["--sb", "--umi"]), (["--sb", "SB", "--umih", "_,8"], ["--sb", "--umih"]),
    (["--sb", "SB", "--pe", "--st2", "0", "--umi1", "0,8"], ["--sb", "--umi1"]), (["--sb", "SB", "--pe", "--st2", "0", "--umi2", "0,8"], ["--sb", "--umi2"]),
    (["--sb", "SB", "--sbs", "-1"], ["--sbs", ">= 0"]), (["--sb", "SB", "--sbs", "x"], ["--sbs", ">= 0"]), (["--sb", "SB", "--sbs", "2.5"], ["--sbs", ">= 0"]),
    (["--sb", "SB", "--sbm", "2"], ["--sbm", "0 or 1"]), (["--sb", "SB", "--sbm", "x"], ["--sbm", "0 or 1"]),
    (["--sb", "/nowhere/samples.csv"], ["--sb", "no .csv file"])])
def test_command_line_refusals(argv, words, capsys, sb):
    with pytest.raises(SystemExit):
        fast2q.input_parser(BASE_ARGV + [sb if a == "SB" else a for a in argv])
    said = capsys.readouterr().out
    assert "FATAL" in said and all(w in said for w in words), said


@pytest.mark.parametrize("text,words", [
    ("a,ACGT\nunassigned,TTTT\n", ["unassigned"]), ("a,ACGT\na,TTTT\n", ["name a", "twice"]), ("a,ACGT\nb,acgt\n", ["ACGT", "twice", "a, b"]),
    ("a,ACGT\nb,TTT\n", ["one length"]), ("a,ACNT\n", ["A/C/G/T"]), ("a," + "A" * 17 + "\n", ["between 1 and 16"]), ("a,\n", ["between 1 and 16"]),
    ("nothing here\n", ["separated"]), ("", ["separated"]),
    ("".join(f"n{i},{''.join(w)}\n" for i, w in zip(range(1025), itertools.product("ACGT", repeat=6))), ["at most 1024"])])
def test_malformed_sample_files_are_refused(text, words, tmp_path, capsys):
    path = tmp_path / "bad.csv"
    path.write_text(text)
    with pytest.raises(SystemExit):
        fast2q.input_parser(BASE_ARGV + ["--sb", str(path)])
    said = capsys.readouterr().out
    assert "FATAL" in said and "--sb" in said and all(w in said for w in words), said


def test_command_line_takes_the_flags_and_refuses_several_ranks(tmp_path, capsys, monkeypatch, sb):
    (tmp_path / "a.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path / "never")]
    p = fast2q.input_parser(argv + ["--sb", sb, "--sbs", "20", "--sbm", "1"])
    want = dict(path=sb, names=[f"s{i:02d}" for i in range(12)], barcodes=[b.decode() for b in DC.barcodes()], start=20, miss=1)
    assert p["sample_barcodes"] == want
    d = fast2q.input_parser(argv + ["--sb", sb])["sample_barcodes"]
    assert (d["start"], d["miss"]) == (0, 0)
    plain = fast2q.input_parser(argv)
    assert "sample_barcodes" not in plain and {k: v for k, v in p.items() if k not in ("sample_barcodes", "used_cmd")} == {k: v for k, v in plain.items() if k != "used_cmd"}
    kw, kw_plain = fast2q._counter_kwargs(p), fast2q._counter_kwargs(plain)
    assert kw["sample_barcodes"] == (20, tuple(want["barcodes"])) and kw["barcode_mismatch"] == 1
    assert "sample_barcodes" not in kw_plain and "barcode_mismatch" not in kw_plain
    assert {k: v for k, v in kw.items() if k not in ("sample_barcodes", "barcode_mismatch")} == kw_plain
    # semicolons, tabs, lower case and blanks are read as --g's are
    for sep in (";", "\t"):
        other = tmp_path / "other.csv"
        other.write_text("".join(f"s{i:02d}{sep}{b.decode().lower()[:4]} {b.decode()[4:]}\n" for i, b in enumerate(DC.barcodes())))
        assert fast2q.input_parser(argv + ["--sb", str(other)])["sample_barcodes"]["barcodes"] == want["barcodes"]
    # several ranks: refused before any output directory exists, and again where a sample would be counted
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    p["test_mode"] = False
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(dict(p))
    said = capsys.readouterr().out
    assert "FATAL" in said and "--sb" in said and "several ranks" in said
    p["Progress bar"] = False
    with pytest.raises(RuntimeError, match="--sb.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a.fastq"), {"ACGT": fast2q.Features("g", 0)}, p, {})
    assert not (tmp_path / "never").exists()


def test_parameter_print_out_and_run_header(capsys, tmp_path, sb):
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path)]
    p = fast2q.initializer(fast2q.input_parser(argv + ["--sb", sb, "--sbs", "20", "--sbm", "1"]))
    said = capsys.readouterr().out
    assert "Sample barcodes, start, length, mismatches: 20,8,1" in said and "12 inline sample barcodes" in said
    assert fast2q.run_headers(p)[-1] == "#Sample barcodes, start, length, mismatches: 20,8,1"
    plain = fast2q.initializer(fast2q.input_parser(argv))
    assert "Sample barcodes" not in capsys.readouterr().out and not any("Sample barcodes" in line for line in fast2q.run_headers(plain))
    assert fast2q.run_headers(p)[2:-1] == fast2q.run_headers(plain)[2:] and fast2q.run_headers(p)[0] == fast2q.run_headers(plain)[0]   # (line 1: the command used)


def test_header_declares_the_calls_and_the_binding_exports_them():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    assert re.search(r"\bint\s+f2q_set_sample_barcodes\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*const\s+char\s*\*\s*seqs\s*,\s*uint32_t\s+n\s*,\s*int32_t\s+length\s*,"
                     r"\s*int32_t\s+start\s*,\s*int32_t\s+miss\s*\)\s*;", text)
    assert re.search(r"\bint\s+f2q_read_demux\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int64_t\s*\*\s*matrix[^,]*,\s*int64_t\s*\*\s*sample_stats[^,]*,\s*int64_t\s+verdicts\[5\]\s*\)\s*;", text)
    assert {"f2q_set_sample_barcodes", "f2q_read_demux"} <= set(binding.EXPORTS)
    assert "def barcode_of(seq, qual, S, L, phred, barcodes, M):" in text                  # the rule is stated there
    assert hasattr(binding.load(), "f2q_set_sample_barcodes") and hasattr(binding.load(), "f2q_read_demux")


def test_sample_file_is_split_by_one_separator_only(tmp_path):
    path = tmp_path / "two.csv"
    path.write_text("a;x,ACGT\n\nb;y,TTTT\n")                                       # ',' splits every line: ';' is part of the names
    assert fast2q.sample_barcodes_loader(str(path)) == (["a;x", "b;y"], ["ACGT", "TTTT"])
    path.write_text("a,ACGT\nb;TTTT\n")                                              # no separator splits every line
    assert isinstance(fast2q.sample_barcodes_loader(str(path)), str)
