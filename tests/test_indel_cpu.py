"""--indel without a GPU: the lane logic of k_count_indel (indel_read: general_read for the plain verdict, the three words
of [s, s + L + 1) built from staged words or byte by byte, indel_decide; f2q_device.h) and the host builder of the
deletion-variant table (indel_build, f2q_host.h), compiled for the host by tests/emu/f2q_indel_emu.cpp, against the
plain-Python expectation of tests/indel_cases.py -- the inputs of the GPU list in tests/test_indel_gpu.py; staged against
unstaged record by record; the invariants; the refusals that need no device; the command line's flag, refusals and
print-outs; the header against the binding's export list; the key and span builders under sanitizers in a stand-alone
program."""
import ctypes as C
import importlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import emu_helper
import indel_cases as IC
from conftest import ROOT, TESTS

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_indel_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_indel_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
STAGED, UNSTAGED = 0, 2
_L = []


def _lib():
    if _L:
        return _L[0]
    deps = [SRC, os.path.join(TESTS, "emu", "f2q_emu.cpp")] + [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h", "f2q_synth.h", "f2q_reader.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", LIB, SRC, "-lz", "-lpthread"])
    L = C.CDLL(LIB)
    vp, i64p, u64p, u32p = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.iemu_create.restype = vp
    L.iemu_create.argtypes = [C.POINTER(binding.Params)]
    L.iemu_destroy.argtypes = [vp]
    L.iemu_set_features.argtypes = [vp, C.c_char_p, u32p, C.c_uint32]
    L.iemu_count_block.restype = C.c_size_t
    L.iemu_count_block.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_char_p]
    L.iemu_read.argtypes = [vp, i64p, i64p, i64p, i64p, i64p, i64p, i64p, u64p]
    L.iemu_table_slots.restype = C.c_uint64
    L.iemu_table_slots.argtypes = [vp]
    L.iemu_table_info.argtypes = [vp, u64p]
    L.iemu_table_dump.argtypes = [vp, u64p, u64p]
    _L.append(L)
    return L


def _open(lib, **run):
    L = _lib()
    p, _keep = binding.make_params(mode="C", **run)
    h = C.c_void_p(L.iemu_create(C.byref(p)))
    assert h
    enc = [s.encode() for s in lib]
    offs = np.zeros(len(enc) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(b) for b in enc])
    L.iemu_set_features(h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc))
    return L, h


def emu_result(lib, fq, layout=STAGED, per=0, used=None, **run):
    """((counts, stats, del_counts, ins_counts, del_pos, ins_pos, totals), (staged, unstaged), per-record bytes) -- the text
    counted in pieces of `per` records (0: one block)"""
    L, h = _open(lib, **run)
    verdicts = b""
    for piece in (IC.pieces(fq, per) if per else [fq]):
        out = C.create_string_buffer(4 * (piece.count(b"\n") // 4 + 2))
        got = L.iemu_count_block(h, piece, len(piece), layout, out)
        assert got == (len(piece) if used is None else used)
        verdicts += out.raw
    nf, length = len(lib), int(run["length"])
    arrays = [(C.c_int64 * max(n, 1))() for n in (nf, 5, nf, nf, length, length, 4)]
    lay = (C.c_uint64 * 2)()
    L.iemu_read(h, *arrays, lay)
    L.iemu_destroy(h)
    got = tuple(list(a)[:n] for a, n in zip(arrays, (nf, 5, nf, nf, length, length, 4)))
    return got, tuple(lay), verdicts[:4 * got[1][0]] if not per else None


def both_layouts(lib, fq, want, used=None, **run):
    """the staged and the unstaged layout against the expectation and, record by record, against each other"""
    staged, (n_staged, n_walked), v_staged = emu_result(lib, fq, STAGED, used=used, **run)
    assert staged == tuple(want)
    plain, lay, v_plain = emu_result(lib, fq, UNSTAGED, used=used, **run)
    assert plain == tuple(want) and v_plain == v_staged and lay == (0, want[1][0])
    IC.check_invariants(*staged)
    return n_staged, n_walked


# ---- the cases and the expectation themselves ------------------------------------------------------------------------------
def test_the_cases_cover_what_they_claim():
    IC.check_coverage()


def test_expectation_changes_no_count():
    lib, fq, run = IC.CASES["base"]()
    for miss in (0, 1, 2):
        e = IC.expect(lib, fq, miss=miss, **run)
        assert (e[0], e[1]) == tuple(IC.RE.oracle_of(lib, fq, miss=miss, **run)[:2])
    # more mismatches allowed: fewer reads are left for the trial
    tried = [IC.expect(lib, fq, miss=miss, **run)[6][0] for miss in (0, 1, 2)]
    assert tried[0] > tried[1] > tried[2]


# ---- the lane logic -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("miss", [0, 1, 2])
def test_base_shape_vs_expectation(miss):
    lib, fq, run = IC.CASES["base"]()
    want = IC.expect(lib, fq, miss=miss, **run)
    staged, walked = both_layouts(lib, fq, want, miss=miss, **run)
    assert walked == 0 and staged == want[1][0]
    assert emu_result(lib, fq, per=30, miss=miss, **run)[0] == tuple(want)                    # the state lives across blocks


@pytest.mark.parametrize("phred", [1, 41])
def test_base_shape_phred(phred):
    lib, fq, run = IC.CASES["base"]()
    run = dict(run, phred=phred, miss=1)
    both_layouts(lib, fq, IC.expect(lib, fq, **run), **run)


@pytest.mark.parametrize("name", sorted(n for n in IC.CASES if n != "base"))
def test_cases_vs_expectation_in_both_layouts(name):
    lib, fq, run = IC.CASES[name]()
    want = IC.expect(lib, fq, **run)
    used = IC.RE.oracle_of(lib, fq, **run)[2]
    staged, walked = both_layouts(lib, fq, want, used=used, **run)
    if name.startswith("edge") or name in ("long_reads", "pass_pool"):
        assert staged > 100 and walked > 30, (staged, walked)
    else:
        assert staged > 100


def test_random_short_records_against_the_rule():
    """20 000 records of 0 .. 45 bytes over a small alphabet against a small library of 4-mers and 6-mers: clipped windows,
    quality lines of another length, every verdict; the two layouts agree record by record and with the rule"""
    rng = random.Random(0x1DE9)
    lib = sorted({"".join(rng.choice("ACGT") for _ in range(k)) for k in (4, 6) for _ in range(40)})
    recs = []
    for _ in range(20000):
        n = rng.randrange(46)
        s = bytes(rng.choice(b"ACGTACGTACGTacgtN.") for _ in range(n))
        q = bytes(rng.choice(b"I" * 60 + b"#=>5~") for _ in range(max(n + rng.choice((0, 0, 0, -3, -1, 1, 2)), 0)))
        recs.append((s, q))
    fq = IC.UC.fastq_of(recs)
    for start, length, miss in ((2, 6, 0), (0, 4, 0), (3, 4, 1), (30, 6, 0)):
        run = dict(start=str(start), length=length, phred=30, miss=miss)
        staged, _, v_staged = emu_result(lib, fq, STAGED, **run)
        plain, _, v_plain = emu_result(lib, fq, UNSTAGED, **run)
        assert v_staged == v_plain and staged == plain
        IC.check_invariants(*staged)
        want = IC.per_read(lib, fq, **run)
        for i, (v0, verdict) in enumerate(want):
            code, pos, f = v_staged[4 * i], v_staged[4 * i + 1], v_staged[4 * i + 2] | (v_staged[4 * i + 3] << 8)
            if v0[0] >= 0:
                assert code == 0, i
            elif verdict is None:
                assert code == 1, (i, recs[i])
            elif verdict == "ambiguous":
                assert code == 4, (i, recs[i])
            else:
                assert (code, f, pos) == (2 + ("del", "ins").index(verdict[0]), verdict[1], verdict[2]), (i, recs[i], verdict)
        if start < 10:
            assert staged[6][1] > 100 and staged[6][2] > 100 and staged[6][3] > 30, staged[6]


def test_flag_semantics_against_the_plain_emulation():
    lib, fq, run = IC.CASES["base"]()
    for miss in (0, 1):
        plain = emu_helper.Emu(features=lib, mode="C", miss=miss, **run)
        plain.count_block(fq)
        counts, stats, _, _ = plain.read()
        got = emu_result(lib, fq, miss=miss, **run)[0]
        assert (got[0], got[1]) == (counts, stats)                   # --indel leaves counts and stats what they are
        assert got[6][0] == stats[0] - stats[1] - stats[2] == stats[3] + stats[4]      # tried: the unassigned reads


def test_host_table_against_a_dict_of_the_variants():
    for name in ("base", "l2", "l31", "l30"):
        lib, _, run = IC.CASES[name]()
        length = int(run["length"])
        cand, variants = IC.candidates(tuple(lib), length)
        L, h = _open(lib, **run)
        slots = L.iemu_table_slots(h)
        info, keys, vals = (C.c_uint64 * 3)(), (C.c_uint64 * slots)(), (C.c_uint64 * slots)()
        L.iemu_table_info(h, info)
        L.iemu_table_dump(h, keys, vals)
        L.iemu_destroy(h)
        got = {}
        for k, v in zip(keys, vals):
            if k == 2 ** 64 - 1:
                continue
            text = bytes(b"ACGT"[(k >> (2 * j)) & 3] for j in range(length - 1))
            assert k >> (2 * (length - 1)) == 0 and text not in got
            got[text] = None if v == 2 ** 64 - 1 else (v >> 8, v & 255)
        want = {v: (None if len(fs) > 1 else next(iter(fs.items()))) for v, fs in variants.items()}
        assert got == want                                           # the exclusion, the smallest p, the shared marks
        assert list(info) == [len(cand), len(variants), sum(len(fs) > 1 for fs in variants.values())]
        assert slots >= 2 * len(variants) and slots & (slots - 1) == 0          # at most half full
    lib = IC.CASES["base"]()[0]
    assert sum(len(fs) > 1 for fs in IC.candidates(tuple(lib), 20)[1].values()) >= IC.N_PAIR


def test_a_repeated_feature_takes_part_once():
    lib = ["ACGTACGTAC", "TTGCATTGCA", "ACGTACGTAC"]
    recs = [(b"GG" + IC.delete(b"ACGTACGTAC", 3) + b"TTTT", b"I" * 15), (b"GG" + IC.insert(b"ACGTACGTAC", 4, ord("T")) + b"TT", b"I" * 15)]
    got = emu_result(lib, IC.UC.fastq_of(recs), start="2", length=10, phred=30, miss=0)[0]
    assert got[2] == [1, 0, 0] and got[3] == [1, 0, 0] and got[6] == [2, 1, 1, 0]


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "iemu_main")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DF2Q_INDEL_EMU_MAIN"] + FLAGS +
                          ["-o", exe, SRC, "-lz", "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout and "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stdout + out.stderr
    print(out.stdout)
    keys, spans = (int(x) for x in re.search(r"(\d+) removed-base keys, (\d+) spans built", out.stdout).groups())
    assert keys == 40 * 2 * sum(range(2, 32)) and spans > 500000


# ---- refusals that need no device ------------------------------------------------------------------------------------------
def test_null_context_is_refused_by_the_library():
    L = binding.load()                                               # (the built library, as tests/test_abi_and_host.py loads it)
    assert L.f2q_set_indel(None, 1) == -1 and L.f2q_set_indel(None, 0) == -1
    assert L.f2q_read_indels(None, None, None, None, None, 20, None) == -1


def test_header_declares_the_calls_and_the_binding_exports_them():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    assert re.search(r"\bint\s+f2q_set_indel\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int32_t\s+on\s*\)\s*;", text)
    assert re.search(r"\bint\s+f2q_read_indels\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int64_t\s*\*\s*del_counts[^,]*,\s*int64_t\s*\*\s*ins_counts[^,]*,\s*int64_t\s*\*\s*del_pos[^,]*,"
                     r"\s*int64_t\s*\*\s*ins_pos[^,]*,\s*int32_t\s+n_pos\s*,\s*int64_t\s+totals\[4\]\s*\)\s*;", text)
    assert {"f2q_set_indel", "f2q_read_indels"} <= set(binding.EXPORTS)
    assert "def indel_verdict(" in text                              # the rule is stated there
    declared = set(re.findall(r"^\s*(?:int|void|const char \*|uint64_t|f2q_ctx \*)\s*\*?\s*(f2q_\w+)\s*\(", text, re.M))
    assert {"f2q_set_indel", "f2q_read_indels"} <= declared
    assert hasattr(binding.load(), "f2q_set_indel") and hasattr(binding.load(), "f2q_read_indels")
    assert callable(binding.Counter.set_indel) and callable(binding.Counter.read_indels)


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE_ARGV = ["-c", "--s", "x", "--g", "y", "--o", "z"]


@pytest.mark.parametrize("argv,words", [
    (["--indel", "2"], ["--indel 2", "no value"]),
    (["--indel", "--mo", "EC"], ["--indel", "--mo EC"]), (["--indel", "--pe", "--st2", "0"], ["--indel", "--pe"]),
    (["--indel", "--us", "ACGT"], ["--indel", "--us"]), (["--indel", "--ds", "ACGT"], ["--indel", "--ds"]),
    (["--indel", "--st", "2,30"], ["--indel", "--st 2,30"]), (["--indel", "--st", "-3"], ["--indel", "--st -3"]),
    (["--indel", "--l", "1"], ["--indel", "--l 1", "2 to 31"]), (["--indel", "--l", "32"], ["--indel", "--l 32", "2 to 31"]),
    (["--indel", "--umi", "20,8"], ["--indel", "--umi"]), (["--indel", "--umih", "_,8"], ["--indel", "--umih"]),
    (["--indel", "--pe", "--st2", "0", "--umi1", "0,8"], ["--indel", "--umi1"]),
    (["--indel", "--pe", "--st2", "0", "--umi2", "0,8"], ["--indel", "--umi2"]),
    (["--indel", "--sb", "SB"], ["--indel", "--sb"]),
    (["--indel", "--strand", "rev"], ["--indel", "--strand rev"]), (["--indel", "--strand", "both"], ["--indel", "--strand both"]),
    (["--indel", "--st", "0,30", "--parts"], ["--indel", "--parts"]),
    (["--indel", "--stagger", "8"], ["--indel", "--stagger 8"])])
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
    strip = lambda p: {k: v for k, v in p.items() if k not in ("indel", "used_cmd")}
    p = fast2q.input_parser(argv + ["--indel"])
    assert p["indel"] is True and strip(p) == strip(plain)
    kw, kw_plain = fast2q._counter_kwargs(p), fast2q._counter_kwargs(plain)
    assert kw["indel"] is True and "indel" not in kw_plain and {k: v for k, v in kw.items() if k != "indel"} == kw_plain
    assert "indel" not in plain
    for extra in (["--l", "2"], ["--l", "31"], ["--st", "0"], ["--strand", "fwd"], ["--stagger", "0"], ["--m", "2"]):
        assert fast2q.input_parser(argv + ["--indel"] + extra)["indel"] is True
    # the exact --st, --st2 and --strand still parse as they did, next to the new long option
    assert fast2q.input_parser(argv + ["--st", "7"])["start"] == fast2q.input_parser(argv + ["--st", "7", "--indel"])["start"] == "7"
    assert fast2q.input_parser(argv + ["--strand", "both"])["strand"] == "both"
    assert fast2q.input_parser(argv + ["--pe", "--st2", "3"]).get("paired")
    # several ranks: refused before any output directory exists, and again where a sample would be counted
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    p["test_mode"] = False
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(dict(p))
    said = capsys.readouterr().out
    assert "FATAL" in said and "--indel" in said and "several ranks" in said
    p["Progress bar"] = False
    with pytest.raises(RuntimeError, match="--indel.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a.fastq"), {"ACGT": fast2q.Features("g", 0)}, p, {})
    assert not (tmp_path / "never").exists()


def test_parameter_print_out_and_run_header(capsys, tmp_path):
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path)]
    plain = fast2q.initializer(fast2q.input_parser(argv))
    assert "Indel" not in capsys.readouterr().out and not any("Indel" in line for line in fast2q.run_headers(plain))
    p = fast2q.initializer(fast2q.input_parser(argv + ["--indel"]))
    assert "Indel reads reported: 1" in capsys.readouterr().out
    assert fast2q.run_headers(p)[-1] == "#Indel reads reported: 1"
    assert fast2q.run_headers(p)[2:-1] == fast2q.run_headers(plain)[2:] and fast2q.run_headers(p)[0] == fast2q.run_headers(plain)[0]   # (line 1: the command used)
