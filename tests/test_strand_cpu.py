"""--strand without a GPU: the lane logic of k_count_strand (strand_read: the in-place mirror of a staged record, the mirroring
accessor of a record that is walked where it lies, the two-trip loop around general_read; f2q_device.h), compiled for the
host by tests/emu/f2q_strand_emu.cpp, against the plain-Python expectation of tests/strand_cases.py -- the inputs of the GPU
list in tests/test_strand_gpu.py; the refusals that need no device; the command line's flags, refusals and print-outs; the
header against the binding's export list; the mirror under a sanitizer in a stand-alone program."""
import ctypes as C
import importlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import strand_cases as SC
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_strand_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_strand_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
MODES = {SC.REV: 1, SC.BOTH: 2}
_L = []


def _lib():
    if _L:
        return _L[0]
    deps = [SRC, os.path.join(TESTS, "emu", "f2q_emu.cpp")] + [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h", "f2q_synth.h", "f2q_reader.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", LIB, SRC, "-lz", "-lpthread"])
    L = C.CDLL(LIB)
    vp, i64p, u32p, i32 = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.c_int32
    L.semu_create.restype = vp
    L.semu_create.argtypes = [C.POINTER(binding.Params), i32]
    L.semu_destroy.argtypes = [vp]
    L.semu_set_features.argtypes = [vp, C.c_char_p, u32p, C.c_uint32]
    L.semu_count_block.restype = C.c_size_t
    L.semu_count_block.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int]
    L.semu_read.argtypes = [vp, i64p, i64p, i64p, i64p, C.POINTER(C.c_uint64)]
    L.semu_mirror.restype = i32
    L.semu_mirror.argtypes = [C.c_char_p, C.c_uint32, i32, i32, C.c_char_p]
    _L.append(L)
    return L


def emu_result(lib, fq, mode, per=0, walk_all=False, used=None, **run):
    """((counts, stats, rev_counts, extra), (staged, walked)) -- the text counted in pieces of `per` records (0: one block)"""
    L = _lib()
    p, _keep = binding.make_params(mode="C", **run)
    h = C.c_void_p(L.semu_create(C.byref(p), MODES[mode]))
    assert h
    enc = [s.encode() for s in lib]
    offs = np.zeros(len(enc) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(b) for b in enc])
    L.semu_set_features(h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc))
    for piece in (SC.pieces(fq, per) if per else [fq]):
        n = L.semu_count_block(h, piece, len(piece), int(walk_all))
        assert n == (len(piece) if used is None else used)
    nf = len(lib)
    counts, stats, rev, extra, layout = (C.c_int64 * nf)(), (C.c_int64 * 5)(), (C.c_int64 * nf)(), (C.c_int64 * 4)(), (C.c_uint64 * 2)()
    L.semu_read(h, counts, stats, rev, extra, layout)
    L.semu_destroy(h)
    return (list(counts), list(stats), list(rev), list(extra)), tuple(layout)


def mirror(line, mis, comp):
    out = C.create_string_buffer(len(line) + 1)
    n = _lib().semu_mirror(line, mis, len(line), int(comp), out)
    return out.raw[:n]


# ---- the cases and the expectation themselves ------------------------------------------------------------------------------
def test_the_cases_cover_what_they_claim():
    SC.check_coverage()


def test_expectation_consequences_of_the_rule():
    lib, fq, run = SC.base()
    plain = SC.expect(lib, fq, SC.FWD, miss=1, **run)
    assert plain[2] == [0] * len(lib) and plain[3] == [sum(plain[0]), 0, 0, 0]
    assert plain[:2] == tuple(SC.RE.oracle_of(lib, fq, miss=1, **run)[:2])                    # fwd is the reference itself
    # rev on a text equals a plain run on the text with every record mirrored
    rev = SC.expect(lib, fq, SC.REV, miss=1, **run)
    assert rev[:2] == tuple(SC.RE.oracle_of(lib, SC.mirror_text(fq), miss=1, **run)[:2])
    # both on a sample with no reverse-strand reads gives the plain run
    fwd_only = SC.pieces(fq, 1)
    v = SC.UC._verdicts(tuple(lib), SC.UC.run_key(dict(run, miss=1))).of
    keep = b"".join(p for p, (s, q) in zip(fwd_only, SC.UC.records(fq)) if v(*SC.mirrored(s, q))[0] < 0)
    assert len(keep) > len(fq) // 4
    assert SC.expect(lib, keep, SC.BOTH, miss=1, **run)[:2] == SC.expect(lib, keep, SC.FWD, miss=1, **run)[:2]


# ---- the mirror in place -----------------------------------------------------------------------------------------------------
def test_mirror_line_against_the_rule_on_every_alignment_and_length():
    rng = random.Random(0x31220)
    alphabet = b"ACGTacgtNnRYK.-*" + bytes([0, 31, 127, 128, 200, 255]) + b"!#5=>I~"
    for n in list(range(0, 40)) + [61, 150, 187, 188, 189, 190, 191, 192]:
        for mis in range(4):
            if mis + n > 192:
                continue
            line = bytes(rng.choice(alphabet) for _ in range(n))
            if n and line[-1:] in b" \t\r\n\x0b\x0c":
                line = line[:-1] + b"A"
            for lead in (b"", b" ", b"\t ", b" \x0b\x0c "):
                text = (lead + line)[:n] if n else b""
                if text != text.rstrip():
                    continue                                         # (a framed line is rstrip()-ed)
                assert mirror(text, mis, True) == SC.mirrored(text, b"")[0], (n, mis, lead)
                assert mirror(text, mis, False) == SC.mirrored(b"", text)[1], (n, mis, lead)


def test_complement_of_every_byte_value():
    every = bytes(range(256)).replace(b"\n", b"A")
    every = every.rstrip() + b"A"
    for mis in range(4):
        for at in range(0, len(every), 150):
            part = every[at:at + 150].lstrip().rstrip() or b"A"
            assert mirror(part, mis, True) == part.translate(SC.COMP)[::-1].rstrip()


# ---- the lane logic -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("miss", [0, 1, 2])
@pytest.mark.parametrize("mode", [SC.REV, SC.BOTH])
def test_base_shape_vs_expectation(mode, miss):
    lib, fq, run = SC.base()
    want = SC.expect(lib, fq, mode, miss=miss, **run)
    got, (staged, walked) = emu_result(lib, fq, mode, miss=miss, **run)
    assert got == want and walked == 0
    SC.check_invariants(mode, *got)
    assert emu_result(lib, fq, mode, per=30, miss=miss, **run)[0] == want                     # the state lives across blocks
    assert emu_result(lib, fq, mode, walk_all=True, miss=miss, **run) == (want, (0, want[1][0]))      # the accessor gives the same


@pytest.mark.parametrize("phred", [1, 30, 41])
def test_base_shape_phred(phred):
    lib, fq, run = SC.base()
    run = dict(run, phred=phred, miss=1)
    for mode in (SC.REV, SC.BOTH):
        want = SC.expect(lib, fq, mode, **run)
        assert emu_result(lib, fq, mode, **run)[0] == want
        assert emu_result(lib, fq, mode, walk_all=True, **run)[0] == want
        SC.check_invariants(mode, *want)


def test_both_counts_at_least_what_forward_counts():
    lib, fq, run = SC.base()
    both = SC.expect(lib, fq, SC.BOTH, miss=1, **run)
    fwd = SC.expect(lib, fq, SC.FWD, miss=1, **run)
    assert all(b >= f for b, f in zip(both[0], fwd[0]))


@pytest.mark.parametrize("name", sorted(n for n in SC.CASES if n != "base"))
@pytest.mark.parametrize("mode", [SC.REV, SC.BOTH])
def test_cases_vs_expectation_in_both_layouts(name, mode):
    lib, fq, run = SC.CASES[name]()
    want = SC.expect(lib, fq, mode, **run)
    used = SC.RE.oracle_of(lib, fq, **run)[2]
    got, (staged, walked) = emu_result(lib, fq, mode, used=used, **run)
    assert got == want
    SC.check_invariants(mode, *got)
    assert emu_result(lib, fq, mode, walk_all=True, used=used, **run)[0] == want
    if name.startswith("edge") or name in ("long_reads", "pass_pool"):
        assert staged > 100 and walked > 30, (staged, walked)
    else:
        assert staged > 100


def test_stand_alone_mirror_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "semu_main")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DF2Q_STRAND_EMU_MAIN"] + FLAGS +
                          ["-o", exe, SRC, "-lz", "-lpthread"])
    paths = []
    for name in ["odd0", "odd1", "odd2"] + [f"edge{r}{a}" for r in SC.RE.EDGE_R for a in ("", "a")]:
        paths.append(str(tmp_path / (name + ".fastq")))
        with open(paths[-1], "wb") as h:
            h.write(SC.CASES[name]()[1])
    out = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout and "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stdout + out.stderr
    print(out.stdout)
    lines, blanks, skipped = (int(x) for x in re.search(r"(\d+) lines mirrored .*\((\d+) with leading blanks\), (\d+) too long", out.stdout).groups())
    assert lines > 10000 and blanks > 100 and skipped > 1000


# ---- refusals that need no device ------------------------------------------------------------------------------------------
def test_null_context_is_refused_by_the_library():
    L = binding.load()                                               # (the built library, as tests/test_abi_and_host.py loads it)
    assert L.f2q_set_strand(None, 1) == -1 and L.f2q_read_strands(None, None, None) == -1


def test_binding_names_the_three_modes_in_the_order_of_the_header():
    assert binding.STRANDS == ("fwd", "rev", "both")                 # F2Q_STRAND_FWD 0, _REV 1, _BOTH 2: set_strand passes the index
    assert callable(binding.Counter.set_strand) and callable(binding.Counter.read_strands)


def test_header_declares_the_calls_and_the_binding_exports_them():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    assert re.search(r"\bint\s+f2q_set_strand\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int32_t\s+mode\s*\)\s*;", text)
    assert re.search(r"\bint\s+f2q_read_strands\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int64_t\s*\*\s*rev_counts[^,]*,\s*int64_t\s+extra\[4\]\s*\)\s*;", text)
    for name, value in (("F2Q_STRAND_FWD", 0), ("F2Q_STRAND_REV", 1), ("F2Q_STRAND_BOTH", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text)
    assert {"f2q_set_strand", "f2q_read_strands"} <= set(binding.EXPORTS)
    assert "def mirrored(seq, qual):" in text and "def strand_verdict(seq, qual, mode):" in text      # the rule is stated there
    declared = set(re.findall(r"^\s*(?:int|void|const char \*|uint64_t|f2q_ctx \*)\s*\*?\s*(f2q_\w+)\s*\(", text, re.M))
    assert {"f2q_set_strand", "f2q_read_strands"} <= declared
    assert hasattr(binding.load(), "f2q_set_strand") and hasattr(binding.load(), "f2q_read_strands")


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE_ARGV = ["-c", "--s", "x", "--g", "y", "--o", "z"]


@pytest.mark.parametrize("argv,words", [
    (["--strand", "up"], ["--strand up", "fwd, rev or both"]), (["--strand", ""], ["--strand", "fwd, rev or both"]), (["--strand", "BOTH"], ["--strand BOTH"]),
    (["--strand", "rev", "--mo", "EC"], ["--strand", "--mo EC"]), (["--strand", "both", "--pe", "--st2", "0"], ["--strand", "--pe"]),
    (["--strand", "both", "--umi", "20,8"], ["--strand", "--umi"]), (["--strand", "rev", "--umih", "_,8"], ["--strand", "--umih"]),
    (["--strand", "both", "--pe", "--st2", "0", "--umi1", "0,8"], ["--strand", "--umi1"]),
    (["--strand", "both", "--pe", "--st2", "0", "--umi2", "0,8"], ["--strand", "--umi2"]),
    (["--strand", "both", "--sb", "SB"], ["--strand", "--sb"])])
def test_command_line_refusals(argv, words, capsys, tmp_path):
    sb = tmp_path / "samples.csv"
    sb.write_text("a,ACGT\nb,TTTT\n")
    with pytest.raises(SystemExit):
        fast2q.input_parser(BASE_ARGV + [str(sb) if a == "SB" else a for a in argv])
    said = capsys.readouterr().out
    assert "FATAL" in said and all(w in said for w in words), said
    assert not os.path.exists("z")


def test_command_line_takes_the_flag_and_refuses_several_ranks(tmp_path, capsys, monkeypatch):
    (tmp_path / "a.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path / "never")]
    plain = fast2q.input_parser(argv)
    strip = lambda p: {k: v for k, v in p.items() if k not in ("strand", "used_cmd")}
    for value in ("rev", "both"):
        p = fast2q.input_parser(argv + ["--strand", value])
        assert p["strand"] == value and strip(p) == strip(plain)
        kw, kw_plain = fast2q._counter_kwargs(p), fast2q._counter_kwargs(plain)
        assert kw["strand"] == value and "strand" not in kw_plain and {k: v for k, v in kw.items() if k != "strand"} == kw_plain
    # fwd is a run without the flag
    fwd = fast2q.input_parser(argv + ["--strand", "fwd"])
    assert "strand" not in fwd and strip(fwd) == strip(plain) and fast2q._counter_kwargs(fwd) == fast2q._counter_kwargs(plain)
    # the exact --st and --st2 still parse as they did, next to the new long option
    assert fast2q.input_parser(argv + ["--st", "7"])["start"] == fast2q.input_parser(argv + ["--st", "7", "--strand", "both"])["start"]
    assert fast2q.input_parser(argv + ["--st", "7"])["start"] != plain["start"]
    pe = fast2q.input_parser(argv + ["--pe", "--st2", "3"])
    assert pe.get("paired") and "strand" not in pe
    # several ranks: refused before any output directory exists, and again where a sample would be counted
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    p["test_mode"] = False
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(dict(p))
    said = capsys.readouterr().out
    assert "FATAL" in said and "--strand" in said and "several ranks" in said
    p["Progress bar"] = False
    with pytest.raises(RuntimeError, match="--strand.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a.fastq"), {"ACGT": fast2q.Features("g", 0)}, p, {})
    assert not (tmp_path / "never").exists()


def test_parameter_print_out_and_run_header(capsys, tmp_path):
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path)]
    plain = fast2q.initializer(fast2q.input_parser(argv))
    assert "Strand" not in capsys.readouterr().out and not any("Strand" in line for line in fast2q.run_headers(plain))
    for value in ("rev", "both"):
        p = fast2q.initializer(fast2q.input_parser(argv + ["--strand", value]))
        assert f"Strand: {value}" in capsys.readouterr().out
        assert fast2q.run_headers(p)[-1] == f"#Strand: {value}"
        assert fast2q.run_headers(p)[2:-1] == fast2q.run_headers(plain)[2:] and fast2q.run_headers(p)[0] == fast2q.run_headers(plain)[0]   # (line 1: the command used)
    fwd = fast2q.initializer(fast2q.input_parser(argv + ["--strand", "fwd"]))
    assert "Strand" not in capsys.readouterr().out and fast2q.run_headers(fwd)[2:] == fast2q.run_headers(plain)[2:]
