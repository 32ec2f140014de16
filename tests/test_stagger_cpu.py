"""--stagger without a GPU: the lane logic of k_count_stagger (stagger_read: the walk layout, the span layout with its
register-built codes and masks, the hand-over of clipped starts; f2q_device.h), compiled for the host by
tests/emu/f2q_stagger_emu.cpp, against the plain-Python expectation of tests/stagger_cases.py -- the inputs of the GPU list
in tests/test_stagger_gpu.py; span against walk record by record; the invariants; the refusals that need no device; the
command line's flags, refusals and print-outs; the header against the binding's export list; the span builder under a
sanitizer in a stand-alone program."""
import ctypes as C
import importlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import emu_helper
import stagger_cases as GC
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_stagger_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_stagger_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
SPAN, WALK, UNSTAGED = 0, 1, 2
_L = []


def _lib():
    if _L:
        return _L[0]
    deps = [SRC, os.path.join(TESTS, "emu", "f2q_emu.cpp")] + [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h", "f2q_synth.h", "f2q_reader.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", LIB, SRC, "-lz", "-lpthread"])
    L = C.CDLL(LIB)
    vp, i64p, u32p, i32 = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.c_int32
    L.gemu_create.restype = vp
    L.gemu_create.argtypes = [C.POINTER(binding.Params), i32]
    L.gemu_destroy.argtypes = [vp]
    L.gemu_set_features.argtypes = [vp, C.c_char_p, u32p, C.c_uint32]
    L.gemu_count_block.restype = C.c_size_t
    L.gemu_count_block.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_char_p]
    L.gemu_read.argtypes = [vp, i64p, i64p, i64p, i64p, C.POINTER(C.c_uint64)]
    _L.append(L)
    return L


def emu_result(lib, fq, n, layout=SPAN, per=0, used=None, **run):
    """((counts, stats, perfect, imperfect), (staged, walked), per-record bytes) -- the text counted in pieces of `per`
    records (0: one block)"""
    L = _lib()
    p, _keep = binding.make_params(mode="C", **run)
    h = C.c_void_p(L.gemu_create(C.byref(p), n))
    assert h
    enc = [s.encode() for s in lib]
    offs = np.zeros(len(enc) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(b) for b in enc])
    L.gemu_set_features(h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc))
    verdicts = b""
    for piece in (GC.pieces(fq, per) if per else [fq]):
        out = C.create_string_buffer(4 * (piece.count(b"\n") // 4 + 2))
        got = L.gemu_count_block(h, piece, len(piece), layout, out)
        assert got == (len(piece) if used is None else used)
        verdicts += out.raw
    nf = len(lib)
    counts, stats, perfect, imperfect, lay = (C.c_int64 * nf)(), (C.c_int64 * 5)(), (C.c_int64 * (n + 1))(), (C.c_int64 * (n + 1))(), (C.c_uint64 * 2)()
    L.gemu_read(h, counts, stats, perfect, imperfect, lay)
    L.gemu_destroy(h)
    return (list(counts), list(stats), list(perfect), list(imperfect)), tuple(lay), verdicts[:4 * stats[0]] if not per else None


def all_layouts(lib, fq, n, want, used=None, **run):
    """the three layouts against the expectation and, record by record, against each other"""
    span, (staged, walked), v_span = emu_result(lib, fq, n, SPAN, used=used, **run)
    assert span == want
    walk, _, v_walk = emu_result(lib, fq, n, WALK, used=used, **run)
    assert walk == want and v_walk == v_span
    plain, lay, v_plain = emu_result(lib, fq, n, UNSTAGED, used=used, **run)
    assert plain == want and v_plain == v_span and lay == (0, want[1][0])
    GC.check_invariants(*span)
    return staged, walked


# ---- the cases and the expectation themselves ------------------------------------------------------------------------------
def test_the_cases_cover_what_they_claim():
    GC.check_coverage()


def test_expectation_consequences_of_the_rule():
    lib, fq, run = GC.base()
    run = dict(run, miss=1)
    # n = 0 is the reference itself
    zero = GC.expect(lib, fq, 0, **run)
    assert zero[:2] == tuple(GC.RE.oracle_of(lib, fq, **run)[:2]) and zero[2] == [zero[1][1]] and zero[3] == [zero[1][2]]
    # more starts never lose a perfect read of fewer starts, and never assign fewer reads
    few, many = GC.expect(lib, fq, 3, **run), GC.expect(lib, fq, GC.N, **run)
    assert many[1][1] >= few[1][1] >= zero[1][1] and sum(many[0]) >= sum(few[0]) >= sum(zero[0])
    assert many[2][:4] == few[2] and many[2][0] == zero[2][0]      # the perfect reads of an offset do not depend on later offsets


# ---- the lane logic -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("miss", [0, 1, 2])
def test_base_shape_vs_expectation(miss):
    lib, fq, run = GC.base()
    want = GC.expect(lib, fq, GC.N, miss=miss, **run)
    staged, walked = all_layouts(lib, fq, GC.N, want, miss=miss, **run)
    assert walked == 0 and staged == want[1][0]
    assert emu_result(lib, fq, GC.N, per=30, miss=miss, **run)[0] == want                     # the state lives across blocks


@pytest.mark.parametrize("phred", [1, 30, 41])
def test_base_shape_phred(phred):
    lib, fq, run = GC.base()
    run = dict(run, phred=phred, miss=1)
    all_layouts(lib, fq, GC.N, GC.expect(lib, fq, GC.N, **run), **run)


@pytest.mark.parametrize("name", sorted(n for n in GC.CASES if n != "base"))
def test_cases_vs_expectation_in_every_layout(name):
    lib, fq, run, n = GC.CASES[name]()
    want = GC.expect(lib, fq, n, **run)
    used = GC.RE.oracle_of(lib, fq, **run)[2]
    staged, walked = all_layouts(lib, fq, n, want, used=used, **run)
    if name.startswith("edge") or name in ("long_reads", "pass_pool"):
        assert staged > 100 and walked > 30, (staged, walked)
    else:
        assert staged > 100


def test_span_equals_walk_on_random_short_records():
    """20 000 records of 0 .. 45 bytes over a small alphabet against a small library of 4-mers and 6-mers: clipped windows,
    quality lines of another length, every verdict; the two layouts agree record by record"""
    rng = random.Random(0x5BA9)
    lib = sorted({"".join(rng.choice("ACGT") for _ in range(k)) for k in (4, 6) for _ in range(40)})
    recs = []
    for _ in range(20000):
        n = rng.randrange(46)
        s = bytes(rng.choice(b"ACGTACGTACGTacgtN.") for _ in range(n))
        q = bytes(rng.choice(b"I" * 60 + b"#=>5~") for _ in range(max(n + rng.choice((0, 0, 0, -3, -1, 1, 2)), 0)))
        recs.append((s, q))
    fq = GC.UC.fastq_of(recs)
    for n, start, length, miss in ((8, 2, 6, 1), (32, 0, 6, 2), (5, 3, 4, 1), (8, 30, 6, 1)):
        run = dict(start=str(start), length=length, phred=30, miss=miss)
        span, _, v_span = emu_result(lib, fq, n, SPAN, **run)
        walk, _, v_walk = emu_result(lib, fq, n, WALK, **run)
        plain, _, v_plain = emu_result(lib, fq, n, UNSTAGED, **run)
        assert v_span == v_walk == v_plain and span == walk == plain
        GC.check_invariants(*span)
        if start < 10:
            assert all(span[1][1:]) and sum(span[2][1:]) > 200 and sum(span[3][1:]) > 100, (span[1], span[2], span[3])


def test_every_guide_at_offset_0_gives_the_plain_run():
    lib, fq, run = GC.all_at_zero()
    plain = emu_helper.Emu(features=lib, mode="C", **run)
    plain.count_block(fq)
    counts, stats, _, _ = plain.read()
    assert stats[1] == stats[0] == 600
    for n in (1, GC.N, 32):
        got = emu_result(lib, fq, n, **run)[0]
        assert got[:2] == (counts, stats) and got[2] == [600] + [0] * n and got[3] == [0] * (n + 1)


def test_no_perfect_read_of_the_plain_run_is_assigned_otherwise():
    lib, fq, run = GC.base()
    run = dict(run, miss=1)
    plain = GC.UC._verdicts(tuple(lib), GC.UC.run_key(run)).of
    _, _, verdicts = emu_result(lib, fq, GC.N, **run)
    checked = 0
    for i, (s, q) in enumerate(GC.UC.records(fq)):
        f, which, _ = plain(s, q)
        if which == 1:
            assert tuple(verdicts[4 * i:4 * i + 4]) == (1, 1, f & 255, f >> 8)
            checked += 1
    assert checked > 50


def test_stand_alone_span_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gemu_main")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DF2Q_STAGGER_EMU_MAIN"] + FLAGS +
                          ["-o", exe, SRC, "-lz", "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout and "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stdout + out.stderr
    print(out.stdout)
    spans, keys = (int(x) for x in re.search(r"(\d+) spans built .*, (\d+) window keys", out.stdout).groups())
    assert spans > 500000 and keys > 1000000


# ---- refusals that need no device ------------------------------------------------------------------------------------------
def test_null_context_is_refused_by_the_library():
    L = binding.load()                                               # (the built library, as tests/test_abi_and_host.py loads it)
    assert L.f2q_set_stagger(None, 8) == -1 and L.f2q_read_stagger(None, None, None, 9) == -1


def test_header_declares_the_calls_and_the_binding_exports_them():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    assert re.search(r"\bint\s+f2q_set_stagger\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int32_t\s+n\s*\)\s*;", text)
    assert re.search(r"\bint\s+f2q_read_stagger\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int64_t\s*\*\s*perfect[^,]*,\s*int64_t\s*\*\s*imperfect[^,]*,\s*int32_t\s+n_offsets\s*\)\s*;", text)
    assert {"f2q_set_stagger", "f2q_read_stagger"} <= set(binding.EXPORTS)
    assert "def stagger_verdict(V, n):" in text                      # the rule is stated there
    declared = set(re.findall(r"^\s*(?:int|void|const char \*|uint64_t|f2q_ctx \*)\s*\*?\s*(f2q_\w+)\s*\(", text, re.M))
    assert {"f2q_set_stagger", "f2q_read_stagger"} <= declared
    assert hasattr(binding.load(), "f2q_set_stagger") and hasattr(binding.load(), "f2q_read_stagger")
    assert callable(binding.Counter.set_stagger) and callable(binding.Counter.read_stagger)


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE_ARGV = ["-c", "--s", "x", "--g", "y", "--o", "z"]


@pytest.mark.parametrize("argv,words", [
    (["--stagger", "x"], ["--stagger x", "0 to 32"]), (["--stagger", ""], ["--stagger", "0 to 32"]), (["--stagger", "-1"], ["--stagger -1", "0 to 32"]),
    (["--stagger", "33"], ["--stagger 33", "0 to 32"]), (["--stagger", "8.0"], ["--stagger 8.0"]),
    (["--stagger", "8", "--mo", "EC"], ["--stagger", "--mo EC"]), (["--stagger", "8", "--pe", "--st2", "0"], ["--stagger", "--pe"]),
    (["--stagger", "8", "--us", "ACGT"], ["--stagger", "--us"]), (["--stagger", "8", "--ds", "ACGT"], ["--stagger", "--ds"]),
    (["--stagger", "8", "--st", "2,30"], ["--stagger", "--st 2,30"]),
    (["--stagger", "8", "--umi", "20,8"], ["--stagger", "--umi"]), (["--stagger", "8", "--umih", "_,8"], ["--stagger", "--umih"]),
    (["--stagger", "8", "--pe", "--st2", "0", "--umi1", "0,8"], ["--stagger", "--umi1"]),
    (["--stagger", "8", "--pe", "--st2", "0", "--umi2", "0,8"], ["--stagger", "--umi2"]),
    (["--stagger", "8", "--sb", "SB"], ["--stagger", "--sb"]),
    (["--stagger", "8", "--strand", "rev"], ["--stagger", "--strand rev"]), (["--stagger", "8", "--strand", "both"], ["--stagger", "--strand both"]),
    (["--stagger", "8", "--st", "0,30", "--parts"], ["--stagger", "--parts"])])
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
    strip = lambda p: {k: v for k, v in p.items() if k not in ("stagger", "used_cmd")}
    for value in (1, 8, 32):
        p = fast2q.input_parser(argv + ["--stagger", str(value)])
        assert p["stagger"] == value and strip(p) == strip(plain)
        kw, kw_plain = fast2q._counter_kwargs(p), fast2q._counter_kwargs(plain)
        assert kw["stagger"] == value and "stagger" not in kw_plain and {k: v for k, v in kw.items() if k != "stagger"} == kw_plain
    # 0 is a run without the flag, whatever else the command line holds
    zero = fast2q.input_parser(argv + ["--stagger", "0"])
    assert "stagger" not in zero and strip(zero) == strip(plain) and fast2q._counter_kwargs(zero) == fast2q._counter_kwargs(plain)
    assert "stagger" not in fast2q.input_parser(argv + ["--stagger", "0", "--strand", "both"])
    # --strand fwd is no strand mode; the exact --st, --st2 and --strand still parse as they did, next to the new long option
    assert fast2q.input_parser(argv + ["--stagger", "8", "--strand", "fwd"])["stagger"] == 8
    assert fast2q.input_parser(argv + ["--st", "7"])["start"] == fast2q.input_parser(argv + ["--st", "7", "--stagger", "8"])["start"] == "7"
    assert fast2q.input_parser(argv + ["--strand", "both"])["strand"] == "both"
    assert fast2q.input_parser(argv + ["--pe", "--st2", "3"]).get("paired")
    # several ranks: refused before any output directory exists, and again where a sample would be counted
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    p["test_mode"] = False
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(dict(p))
    said = capsys.readouterr().out
    assert "FATAL" in said and "--stagger" in said and "several ranks" in said
    p["Progress bar"] = False
    with pytest.raises(RuntimeError, match="--stagger.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a.fastq"), {"ACGT": fast2q.Features("g", 0)}, p, {})
    assert not (tmp_path / "never").exists()


def test_parameter_print_out_and_run_header(capsys, tmp_path):
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path)]
    plain = fast2q.initializer(fast2q.input_parser(argv))
    assert "Stagger" not in capsys.readouterr().out and not any("Stagger" in line for line in fast2q.run_headers(plain))
    for value in (1, 32):
        p = fast2q.initializer(fast2q.input_parser(argv + ["--stagger", str(value)]))
        assert f"Stagger: {value}" in capsys.readouterr().out
        assert fast2q.run_headers(p)[-1] == f"#Stagger: {value}"
        assert fast2q.run_headers(p)[2:-1] == fast2q.run_headers(plain)[2:] and fast2q.run_headers(p)[0] == fast2q.run_headers(plain)[0]   # (line 1: the command used)
    zero = fast2q.initializer(fast2q.input_parser(argv + ["--stagger", "0"]))
    assert "Stagger" not in capsys.readouterr().out and fast2q.run_headers(zero)[2:] == fast2q.run_headers(plain)[2:]
