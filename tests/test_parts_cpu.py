"""--parts without a GPU: the host's table builder (parts_validate / parts_build of f2q_host.h) and the lane logic of
k_count_parts, both instances (parts_read: general_read, part_verdict, parts_class, the pair table, the recombinant set),
compiled for the host by tests/emu/f2q_parts_emu.cpp, against the plain-Python expectation of tests/parts_cases.py -- the
inputs of the GPU list in tests/test_parts_gpu.py; the expectation itself against the oracle on joined keys at --m 0; the
refusals that need no device; the command line's flags, refusals and print-outs; the header against the binding's exports."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import paired_cases as PC
import parts_cases as PT
from conftest import ROOT, TESTS
from oracle import oracle as O

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_parts_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_parts_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
NONE = 0xFFFFFFFF
_L = []


def _lib():
    if _L:
        return _L[0]
    deps = [SRC, os.path.join(TESTS, "emu", "f2q_pair_emu.cpp")] + [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + ["-o", LIB, SRC])
    L = C.CDLL(LIB)
    vp, i64p, u32p, u64p = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.ptemu_validate.argtypes = [C.c_char_p, u32p, C.c_uint32, C.c_char_p, C.c_size_t]
    L.ptemu_table.restype = vp
    L.ptemu_table.argtypes = [C.c_char_p, u32p, C.c_uint32]
    L.ptemu_info.argtypes = [vp, u32p, u32p, u64p, u32p]
    L.ptemu_part.restype = C.c_uint32
    L.ptemu_part.argtypes = [vp, C.c_int, C.c_uint32, C.c_char_p, C.c_size_t]
    L.ptemu_pairs.argtypes = [vp, u32p, u32p]
    L.ptemu_find.restype = C.c_uint32
    L.ptemu_find.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.ptemu_create.restype = vp
    L.ptemu_create.argtypes = [C.POINTER(binding.Params), C.c_int, C.c_int, C.c_uint64]
    L.ptemu_destroy.argtypes = [vp]
    L.ptemu_set_features.argtypes = [vp, C.c_char_p, u32p, C.c_uint32, C.c_char_p, C.c_size_t]
    L.ptemu_count_block.restype = C.c_uint64
    L.ptemu_count_block.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.ptemu_read.restype = C.c_longlong
    L.ptemu_read.argtypes = [vp, i64p, i64p, i64p, i64p, i64p, i64p]
    L.ptemu_recombinants.restype = C.c_uint64
    L.ptemu_recombinants.argtypes = [vp, C.c_uint64, u32p, u32p, u32p, u64p, u64p]
    L.ptemu_reset.argtypes = [vp]
    _L.append(L)
    return L


def _blob(lib):
    enc = [s.encode() for s in lib]
    offs = np.zeros(len(enc) + 1, dtype=np.uint32)
    if enc:
        offs[1:] = np.cumsum([len(b) for b in enc])
    return b"".join(enc), offs, offs.ctypes.data_as(C.POINTER(C.c_uint32))


def _pieces(fq, per):
    lines = fq.split(b"\n")[:-1]
    return [b"".join(l + b"\n" for l in lines[i:i + 4 * per]) for i in range(0, len(lines), 4 * per)]


def emu_result(lib, fq1, fq2, st1, st2, rc2=False, miss=1, phred=30, per=0, slots=0):
    """(counts, stats, dict as parts_cases.expect gives it, rehashes) -- the text counted in pieces of `per` records"""
    L = _lib()
    p, _keep = binding.make_params(mode="C", miss=miss, phred=phred, length=PT.L, start=f"{st1},{st2}")
    h = C.c_void_p(L.ptemu_create(C.byref(p), 0 if fq2 is None else 1, 1 if rc2 else 0, slots))
    assert h
    blob, offs, offp = _blob(lib)
    msg = C.create_string_buffer(512)
    assert L.ptemu_set_features(h, blob, offp, len(lib), msg, 512) == 0, msg.value
    a = _pieces(fq1, per) if per else [fq1]
    b = [None] * len(a) if fq2 is None else (_pieces(fq2, per) if per else [fq2])
    for x, y in zip(a, b):
        assert L.ptemu_count_block(h, x, len(x), y, len(y) if y else 0) == x.count(b"\n") // 4
    n1, n2, tslots, pairs = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
    L.ptemu_info(h, C.byref(n1), C.byref(n2), C.byref(tslots), C.byref(pairs))
    nf = len(lib)
    counts, stats, pc, m1, m2, cls = (C.c_int64 * nf)(), (C.c_int64 * 5)(), (C.c_int64 * nf)(), (C.c_int64 * n1.value)(), (C.c_int64 * n2.value)(), (C.c_int64 * 6)()
    rehashes = L.ptemu_read(h, counts, stats, pc, m1, m2, cls)
    cap = 1 << 16
    i1, i2, rd, held, sslots = (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), C.c_uint64(), C.c_uint64()
    n = L.ptemu_recombinants(h, cap, i1, i2, rd, C.byref(held), C.byref(sslots))
    assert n == held.value and (n == 0 or 2 * n <= sslots.value) and rehashes >= 0
    L.ptemu_destroy(h)
    got = dict(parts_counts=list(pc), part1=list(m1), part2=list(m2), classes=list(cls), recombinants={(i1[k], i2[k]): rd[k] for k in range(n)})
    return list(counts), list(stats), got, rehashes


def check_invariants(stats, got):
    c = got["classes"]
    assert sum(c) == stats[0]
    assert sum(got["parts_counts"]) == c[0] + c[1]
    assert sum(got["recombinants"].values()) == c[2]
    assert sum(got["part1"]) == c[0] + c[1] + c[2] + c[3] and sum(got["part2"]) == c[0] + c[1] + c[2] + c[4]


# ---- the tables ----------------------------------------------------------------------------------------------------------
def test_part_libraries_are_numbered_in_first_occurrence_order_and_the_pair_table_finds_every_feature():
    L = _lib()
    lib = list(PT.library()) + [PT.library()[3]]                    # a repeated feature: its pair stays with the first
    lib1, lib2, ids = PT.part_libraries(lib)
    blob, offs, offp = _blob(lib)
    h = C.c_void_p(L.ptemu_table(blob, offp, len(lib)))
    assert h
    n1, n2, slots, pairs = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
    L.ptemu_info(h, C.byref(n1), C.byref(n2), C.byref(slots), C.byref(pairs))
    assert (n1.value, n2.value, pairs.value) == (len(lib1), len(lib2), len(set(ids)))
    assert slots.value & (slots.value - 1) == 0 and slots.value >= 2 * pairs.value
    buf = C.create_string_buffer(64)

    def part(pos, i):
        n = L.ptemu_part(h, pos, i, buf, 64)
        return buf.raw[:n].decode()
    for pos, want in enumerate((lib1, lib2)):
        assert [part(pos, i) for i in range(len(want))] == want
    got_ids, found = (C.c_uint32 * (2 * len(lib)))(), (C.c_uint32 * len(lib))()
    L.ptemu_pairs(h, got_ids, found)
    assert [(got_ids[2 * f], got_ids[2 * f + 1]) for f in range(len(lib))] == ids
    first = {}
    for f, pair in enumerate(ids):
        first.setdefault(pair, f)
    assert list(found) == [first[pair] for pair in ids] and found[len(lib) - 1] == 3
    held = set(ids)
    missing = [(a, b) for a in range(len(lib1)) for b in range(len(lib2)) if (a, b) not in held]
    assert len(missing) > 1000 and all(L.ptemu_find(h, a, b) == NONE for a, b in missing)
    both = lib[0].split(":")[0]
    assert both in lib1 and both in lib2                             # one sequence, a part 1 and a part 2: two ids of separate spaces
    L.ptemu_destroy(h)


@pytest.mark.parametrize("lib", [PT.one_feature(), PT.star_library()])
def test_library_edges(lib):
    L = _lib()
    blob, offs, offp = _blob(lib)
    h = C.c_void_p(L.ptemu_table(blob, offp, len(lib)))
    n1, n2, slots, pairs = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
    L.ptemu_info(h, C.byref(n1), C.byref(n2), C.byref(slots), C.byref(pairs))
    assert (n1.value, n2.value, pairs.value) == (1, len(lib), len(lib)) and slots.value >= 2 * len(lib)
    assert [L.ptemu_find(h, 0, b) for b in range(len(lib))] == list(range(len(lib)))
    L.ptemu_destroy(h)
    fq, _ = PT.make_reads(lib, 0, 20, 300, 0xED6E)
    want = PT.expect(lib, fq, None, 0, 20, PT.L, miss=1)
    _, stats, got, _ = emu_result(lib, fq, None, 0, 20, miss=1)
    assert got == want and want["classes"][2] == 0 and want["classes"][0] > 50     # one part 1 pairs with every part 2: no recombinant
    check_invariants(stats, got)


@pytest.mark.parametrize("lib,words", [
    (["ACGT"], ["feature 0", "ACGT", "two non-empty parts"]), (["AC:GT", "ACGT:"], ["feature 1", "ACGT:"]), (["AC:GT", ":ACGT"], ["feature 1", ":ACGT"]),
    (["AC:GT", "A:C:G"], ["feature 1", "A:C:G"]), (["AC:GT", "TT:AA", ""], ["feature 2"]), (["AC:GT", ":"], ["feature 1"])])
def test_a_feature_that_is_not_two_parts_is_refused_by_name(lib, words):
    L = _lib()
    blob, offs, offp = _blob(lib)
    msg = C.create_string_buffer(512)
    assert L.ptemu_validate(blob, offp, len(lib), msg, 512) == -1
    assert all(w in msg.value.decode() for w in words), msg.value
    assert L.ptemu_table(blob, offp, len(lib)) is None
    p, _keep = binding.make_params(mode="C", miss=1, length=2, start="0,2")
    h = C.c_void_p(L.ptemu_create(C.byref(p), 0, 0, 0))
    assert L.ptemu_set_features(h, blob, offp, len(lib), msg, 512) == -1 and words[0] in msg.value.decode()
    L.ptemu_destroy(h)


def test_contexts_the_emulation_refuses():
    L = _lib()
    for kw in (dict(mode="EC", start="0,20"), dict(mode="C", start="0"), dict(mode="C", start="0,10,20"), dict(mode="C", upstream="ACGT", downstream="TTGA")):
        p, _keep = binding.make_params(length=10, **kw)
        assert L.ptemu_create(C.byref(p), 0, 0, 0) is None, kw


# ---- the lane logic against the expectation ------------------------------------------------------------------------------
@pytest.mark.parametrize("paired,rc2", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("miss", [0, 1, 2])
@pytest.mark.parametrize("phred", [30, 0])
def test_sample_vs_expectation(paired, rc2, miss, phred):
    lib, fq1, fq2, st1, st2 = PT.sample(paired, rc2)
    want = PT.expect(lib, fq1, fq2, st1, st2, PT.L, rc2, miss, phred)
    counts, stats, got, _ = emu_result(lib, fq1, fq2, st1, st2, rc2, miss, phred)
    assert got == want
    check_invariants(stats, got)
    assert len(want["recombinants"]) > 100
    if miss == 0:
        assert got["parts_counts"] == counts                          # the identity that guards the rule: no mismatches, one verdict
        assert want["classes"][1] == 0 and all(n >= 10 for k, n in enumerate(want["classes"]) if k != 1), want["classes"]      # (nothing is imperfect at --m 0)
    else:
        assert all(n >= 10 for n in want["classes"]), want["classes"] # every one of the six classes occurs


@pytest.mark.parametrize("paired,rc2", [(False, False), (True, True)])
def test_at_m0_the_expectation_equals_the_oracle_on_joined_keys(paired, rc2):
    lib, fq1, fq2, st1, st2 = PT.sample(paired, rc2)
    want = PT.expect(lib, fq1, fq2, st1, st2, PT.L, rc2, 0)
    if paired:
        counts, stats, uncovered = PC.pair_oracle(list(lib), fq1, fq2, [st1], [st2], PT.L, rc2, 0)
        assert uncovered == 0
    else:
        o = O.Oracle(features=[(str(i), s) for i, s in enumerate(lib)], miss=0, phred=30, length=PT.L, start=f"{st1},{st2}")
        o.count_fastq(fq1)
        counts, stats = o.counts(), o.stats()
        o.close()
    assert want["parts_counts"] == list(counts) and sum(counts) > 400
    assert want["classes"][1] == 0 and want["classes"][0] == stats[1]


def test_one_error_in_each_part_is_a_pair_here_and_lost_to_the_joined_rule():
    lib = PT.library()
    a, b = lib[7].split(":")
    a1, b1 = a[:2] + ("A" if a[2] != "A" else "C") + a[3:], b[:6] + ("G" if b[6] != "G" else "T") + b[7:]
    amb = PT.ambiguous_part1(lib)
    recs = [((a1 + "TTTTTTTTTT" + b1 + "CC").encode(), b"I" * 32), ((amb + "TTTTTTTTTT" + b + "CC").encode(), b"I" * 32)]
    fq = PC.fastq_of(recs)
    want = PT.expect(lib, fq, None, 0, 20, PT.L, miss=1)
    counts, stats, got, _ = emu_result(lib, fq, None, 0, 20, miss=1)
    assert got == want
    assert got["parts_counts"][7] == 1 and got["classes"] == [0, 1, 0, 0, 1, 0]      # the ambiguous part 1 is non-aligned: part 2 only
    assert sum(counts) == 0 and stats[3] == 2


@pytest.mark.parametrize("paired,rc2", [(False, False), (True, True)])
def test_pieces_and_a_set_grown_from_64_slots_give_the_one_block_result(paired, rc2):
    lib, fq1, fq2, st1, st2 = PT.sample(paired, rc2)
    whole = emu_result(lib, fq1, fq2, st1, st2, rc2)
    grown = emu_result(lib, fq1, fq2, st1, st2, rc2, per=30, slots=64)
    assert grown[:3] == whole[:3] and grown[3] >= 3 and whole[3] == 0


def test_long_reads():
    lib, fq = PT.long_reads()
    want = PT.expect(lib, fq, None, 0, 20, PT.L, miss=1)
    _, stats, got, _ = emu_result(lib, fq, None, 0, 20)
    assert got == want and want["classes"][2] > 40
    check_invariants(stats, got)


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ptemu_main")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DF2Q_PARTS_EMU_MAIN"] + FLAGS + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "single:" in out.stdout and "paired:" in out.stdout, out.stdout + out.stderr


# ---- refusals that need no device ------------------------------------------------------------------------------------------
def test_null_context_is_refused_by_the_library():
    L = binding.load()                                               # (the built library, as tests/test_abi_and_host.py loads it)
    n = C.c_uint64(0)
    assert L.f2q_set_parts(None) == -1 and L.f2q_parts_info(None, None, None) == -1
    assert L.f2q_read_parts(None, None, None, None, None) == -1 and L.f2q_parts_recombinants(None, 0, C.byref(n), None, None, None) == -1


# ---- the command line ----------------------------------------------------------------------------------------------------
BASE_ARGV = ["-c", "--s", "x", "--g", "y", "--o", "z"]


@pytest.mark.parametrize("argv,words", [
    (["--parts", "--st", "0,20", "--mo", "EC"], ["--parts", "--mo EC"]),
    (["--parts", "--us", "ACGT"], ["--parts", "--us"]), (["--parts", "--ds", "ACGT"], ["--parts", "--ds"]),
    (["--parts", "--st", "0,20", "--umi", "30,8"], ["--parts", "--umi"]), (["--parts", "--st", "0,20", "--umih", "_,8"], ["--parts", "--umih"]),
    (["--parts", "--pe", "--st2", "0", "--umi1", "30,8"], ["--parts", "--umi1"]), (["--parts", "--pe", "--st2", "0", "--umi2", "30,8"], ["--parts", "--umi2"]),
    (["--parts", "--st", "0,20", "--sb", "SB"], ["--parts", "--sb"]),
    (["--parts", "--st", "0,20", "--strand", "rev"], ["--parts", "--strand rev"]), (["--parts", "--st", "0,20", "--strand", "both"], ["--parts", "--strand both"]),
    (["--parts"], ["--parts", "exactly two windows", "--st 0"]), (["--parts", "--st", "0,10,20"], ["--parts", "exactly two windows"]),
    (["--parts", "--pe", "--st", "0,20", "--st2", "0"], ["--parts", "exactly two windows", "--st2 0"]),
    (["--parts", "--pe", "--st", "0", "--st2", "0,20"], ["--parts", "exactly two windows"])])
def test_command_line_refusals(argv, words, capsys, tmp_path):
    sb = tmp_path / "samples.csv"
    sb.write_text("a,ACGT\nb,TTGA\n")
    with pytest.raises(SystemExit):
        fast2q.input_parser(BASE_ARGV + [str(sb) if a == "SB" else a for a in argv])
    said = capsys.readouterr().out
    assert "FATAL" in said and all(w in said for w in words), said


def test_command_line_takes_the_flag_and_refuses_several_ranks_and_odd_libraries(tmp_path, capsys, monkeypatch):
    (tmp_path / "a.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    out = tmp_path / "never"
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(out), "--st", "0,20", "--l", "10"]
    p = fast2q.input_parser(argv + ["--parts"])
    plain = fast2q.input_parser(argv)
    assert p["parts"] is True and "parts" not in plain
    assert {k: v for k, v in p.items() if k not in ("parts", "used_cmd")} == {k: v for k, v in plain.items() if k != "used_cmd"}
    kw, kw_plain = fast2q._counter_kwargs(p), fast2q._counter_kwargs(plain)
    assert kw["parts"] is True and "parts" not in kw_plain and {k: v for k, v in kw.items() if k != "parts"} == kw_plain
    assert fast2q.input_parser(argv + ["--parts", "--strand", "fwd"])["parts"] is True          # (fwd is a run without --strand)
    pe = fast2q.input_parser(["-c", "--s", str(tmp_path), "--g", "y", "--o", str(out), "--parts", "--pe", "--st", "5", "--st2", "3", "--rc2"])
    assert pe["parts"] is True and fast2q._counter_kwargs(pe)["parts"] is True and fast2q._counter_kwargs(pe)["start2"] == "3"
    # a library row that is not two parts: refused by name, before an output directory exists
    assert fast2q.check_parts_library({"ACGT:TTGA": fast2q.Features("g1", 0)}) is None
    for seq in ("ACGTTTGA", "ACGT:", ":TTGA", "A:C:G"):
        assert "g2" in fast2q.check_parts_library({"ACGT:TTGA": fast2q.Features("g1", 0), seq: fast2q.Features("g2", 0)})
    guides = tmp_path / "guides.csv"
    guides.write_text("g1,ACGTACGTAC:TTGATTGATT\ng2,ACGTACGTACTTGATTGATT\n")
    with pytest.raises(SystemExit):
        fast2q.main(["-c", "--s", str(tmp_path), "--g", str(guides), "--o", str(out), "--st", "0,20", "--l", "10", "--parts", "--pb"])
    said = capsys.readouterr().out
    assert "FATAL" in said and "--parts" in said and "g2" in said and not out.exists()
    assert fast2q.part_libraries(["AA:CC", "GG:CC", "AA:TT", "CC:AA"]) == (["AA", "GG", "CC"], ["CC", "TT", "AA"])
    # several ranks: refused before any output directory exists, and again where a sample would be counted
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    p["test_mode"] = False
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(dict(p))
    said = capsys.readouterr().out
    assert "FATAL" in said and "--parts" in said and "several ranks" in said
    p["Progress bar"] = False
    with pytest.raises(RuntimeError, match="--parts.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a.fastq"), {"ACGT:ACGT": fast2q.Features("g", 0)}, p, {})
    assert not out.exists()


def test_parameter_print_out_and_run_header(capsys, tmp_path):
    argv = ["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path), "--st", "0,20", "--l", "10"]
    p = fast2q.initializer(fast2q.input_parser(argv + ["--parts"]))
    said = capsys.readouterr().out
    assert "Parts matched independently: 2" in said and "recombinant" in said
    assert fast2q.run_headers(p)[-1] == "#Parts matched independently: 2"
    plain = fast2q.initializer(fast2q.input_parser(argv))
    assert "Parts matched" not in capsys.readouterr().out and not any("Parts matched" in line for line in fast2q.run_headers(plain))
    assert fast2q.run_headers(p)[2:-1] == fast2q.run_headers(plain)[2:] and fast2q.run_headers(p)[0] == fast2q.run_headers(plain)[0]   # (line 1: the command used)


def test_header_declares_the_calls_and_the_binding_exports_them():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    assert re.search(r"\bint\s+f2q_set_parts\s*\(\s*f2q_ctx\s*\*\s*ctx\s*\)\s*;", text)
    assert re.search(r"\bint\s+f2q_parts_info\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*uint32_t\s*\*\s*n1\s*,\s*uint32_t\s*\*\s*n2\s*\)\s*;", text)
    assert re.search(r"\bint\s+f2q_read_parts\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*int64_t\s*\*\s*parts_counts[^,]*,\s*int64_t\s*\*\s*part1_reads[^,]*,\s*int64_t\s*\*\s*part2_reads[^,]*,"
                     r"\s*int64_t\s+classes\[6\]\s*\)\s*;", text)
    assert re.search(r"\bint\s+f2q_parts_recombinants\s*\(\s*f2q_ctx\s*\*\s*ctx\s*,\s*uint64_t\s+cap\s*,\s*uint64_t\s*\*\s*n\s*,\s*uint32_t\s*\*\s*part1\s*,\s*uint32_t\s*\*\s*part2\s*,"
                     r"\s*uint32_t\s*\*\s*reads\s*\)\s*;", text)
    calls = {"f2q_set_parts", "f2q_parts_info", "f2q_read_parts", "f2q_parts_recombinants"}
    assert calls <= set(binding.EXPORTS) and all(hasattr(binding.load(), c) for c in calls)
    assert "def part_verdicts(read, run):" in text and "def parts_class(v1, v2, features):" in text      # the rule is stated there
    for k, name in enumerate(binding.PARTS_CLASSES):
        assert re.search(rf"#define\s+F2Q_PARTS_{name.upper()}\s+{k}\b", text), name
