"""Paired-end samples without a GPU: the host twin of the device packer (frame_fastq twice + pack_pairs) and the
byte-exact routine on merged pairs (general_read<.., PAIRED>), compiled from the product's headers by
tests/emu/f2q_pair_emu.cpp, against the oracle on merged reads (tests/paired_cases.py); pairing files by name; the
command line's refusals; the header's new declarations against the binding's export list."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import paired_cases as PC
from conftest import ROOT, TESTS
from oracle import oracle as O

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
SRC = os.path.join(TESTS, "emu", "f2q_pair_emu.cpp")
LIB = os.path.join(TESTS, "emu", "libf2q_pair_emu.so")
CSRC = os.path.join(ROOT, "2fast2q_amd", "csrc")


def _lib():
    deps = [SRC, os.path.join(CSRC, "f2q_device.h"), os.path.join(CSRC, "f2q_host.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                               "-o", LIB, SRC])
    L = C.CDLL(LIB)
    vp = C.c_void_p
    L.pemu_create.restype = vp
    L.pemu_create.argtypes = [C.POINTER(binding.Params), C.c_int, C.c_int]
    for name in ("pemu_destroy", "pemu_force_general", "pemu_count_raw"):
        getattr(L, name).argtypes = [vp]
    L.pemu_set_features.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32]
    L.pemu_plan_multi.argtypes = [vp]
    L.pemu_pack.restype = C.c_uint64
    L.pemu_pack.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.pemu_packed_info.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.pemu_packed_get.argtypes = [vp, vp, vp, vp, vp, vp]
    L.pemu_read_counts.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.pemu_ec_n.restype = C.c_uint64
    L.pemu_ec_n.argtypes = [vp]
    L.pemu_ec_get.argtypes = [vp, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
    return L


class PEmu:
    def __init__(self, lib, starts, n_mate1, rc2, **kw):
        self.L = _lib()
        p, self._keep = binding.make_params(start=",".join(str(s) for s in starts), **kw)
        self.h = C.c_void_p(self.L.pemu_create(C.byref(p), n_mate1, 1 if rc2 else 0))
        assert self.h
        self.n = 0
        if lib is not None:
            enc = [s.encode() for s in lib]
            offs = np.zeros(len(enc) + 1, dtype=np.uint32)
            offs[1:] = np.cumsum([len(b) for b in enc])
            self.L.pemu_set_features(self.h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc))
            self.n = len(enc)

    def pack(self, fq1, fq2=None):
        n = self.L.pemu_pack(self.h, fq1, len(fq1), fq2, len(fq2) if fq2 is not None else 0)
        info = (C.c_uint64 * 6)()
        self.L.pemu_packed_info(self.h, info)
        tiles, wb, wq, rmax, clean, general = [int(x) for x in info]
        arrs = [np.zeros(max(tiles * wb * 256, 1), np.uint32), np.zeros(max(tiles * wq * 256, 1), np.uint32),
                np.zeros(max(tiles * 256, 1), np.uint16), np.zeros(max(tiles * 256, 1), np.uint32), np.zeros(max(general, 1), np.uint32)]
        self.L.pemu_packed_get(self.h, *[a.ctypes.data for a in arrs])
        return dict(n=n, tiles=tiles, wb=wb, wq=wq, rmax=rmax, clean=clean, general=general, bases=arrs[0], qual=arrs[1], len=arrs[2],
                    c_index=arrs[3], g_index=arrs[4][:general])

    def count_all_byte_exact(self, fq1, fq2):
        self.L.pemu_force_general(self.h)
        self.pack(fq1, fq2)
        self.L.pemu_count_raw(self.h)
        counts, stats = (C.c_int64 * max(self.n, 1))(), (C.c_int64 * 5)()
        self.L.pemu_read_counts(self.h, counts, stats)
        return list(counts)[:self.n], list(stats)

    def ec_rows(self):
        rows = []
        for e in range(self.L.pemu_ec_n(self.h)):
            key, ln, cnt, first = C.create_string_buffer(4096), C.c_uint32(), C.c_int64(), C.c_uint64()
            self.L.pemu_ec_get(self.h, e, key, C.byref(ln), C.byref(cnt), C.byref(first))
            rows.append((key.raw[:ln.value].decode("latin-1"), cnt.value, first.value))
        return sorted(rows, key=lambda r: r[2])

    def close(self):
        self.L.pemu_destroy(self.h)


GEOMS = [([5], [30], 10), ([0, 40], [12], 7), ([100], [3, 60], 9), ([20], [110], 13)]


@pytest.mark.parametrize("rc2", [False, True])
@pytest.mark.parametrize("st1,st2,length", GEOMS)
def test_clean_pairs_get_the_merged_reads_tile_slot(st1, st2, length, rc2):
    """pack_pairs lays a clean pair into exactly the words pack_records gives the merged read r1 + m2 of the single-end run
    --st a.., L1+b..: same tiles, same flag bits, same reads set aside.  The counting kernels' lane logic on such tiles is
    the single-end multi-window logic that tests/test_lane_logic_cpu.py emulates."""
    lib = PC.pair_library(200, length, len(st1), len(st2), 3)
    fq1, fq2 = PC.make_pairs(lib, length, st1, st2, rc2, 3000, seed=11, len1=150, len2=150)
    # N and lower-case bases, inside and outside the windows (uniform lengths: the two packers agree on who is clean)
    from conftest import sprinkle_symbols
    fq1, fq2 = sprinkle_symbols(fq1, 5, rate=0.01, symbols=b"NnacgtR"), sprinkle_symbols(fq2, 6, rate=0.01, symbols=b"NnacgtR")
    groups, uncovered = PC.merged_groups(fq1, fq2, st1, st2, length, rc2)
    assert uncovered == 0 and len(groups) == 1
    (start, merged), = groups.items()
    pe = PEmu(lib, st1 + st2, len(st1), rc2, miss=1, length=length)
    se = PEmu(lib, [int(x) for x in start.split(",")], 0, False, miss=1, length=length)
    assert pe.L.pemu_plan_multi(pe.h) == 1 and se.L.pemu_plan_multi(se.h) == 1
    a, b = pe.pack(fq1, fq2), se.pack(merged)
    assert a["n"] == b["n"] == 3000 and a["clean"] == b["clean"] > 0 and a["general"] == b["general"]
    assert ((a["len"] & 0x8000) != 0).sum() > 50                     # windows with odd symbols travel as flag bits
    for k in ("tiles", "wb", "wq", "rmax"):
        assert a[k] == b[k], k
    for k in ("bases", "qual", "len", "c_index", "g_index"):
        assert np.array_equal(a[k], b[k]), k
    pe.close(); se.close()


@pytest.mark.parametrize("rc2", [False, True])
@pytest.mark.parametrize("miss", [0, 1, 2])
@pytest.mark.parametrize("st1,st2,length", GEOMS[:3])
def test_byte_exact_routine_on_pairs_vs_oracle(st1, st2, length, miss, rc2):
    """every pair through general_read<.., PAIRED> on the merged raw record the host packer writes: ragged mates (some
    ending inside a window), odd symbols, quality lines of another length, bytes >= 128, CRLF -- against the oracle by the
    group-by-length construction; the generator leaves no pair uncovered (asserted)"""
    lib = PC.pair_library(150, length, len(st1), len(st2), 4, combinatorial=True)
    fq1, fq2 = PC.make_pairs(lib, length, st1, st2, rc2, 4000, seed=21 + miss, ragged=True, dirty=True)
    counts, stats, uncovered = PC.pair_oracle(lib, fq1, fq2, st1, st2, length, rc2, miss)
    assert uncovered == 0 and stats[0] == 4000 and stats[1] > 0 and stats[3] > 0
    pe = PEmu(lib, st1 + st2, len(st1), rc2, miss=miss, length=length)
    got = pe.count_all_byte_exact(fq1, fq2)
    pe.close()
    assert got[1] == stats and got[0] == counts


def test_both_mates_cut_short_exact_keys():
    """pairs in which BOTH mates end inside a window (no merged read stands for them): --m 0 against an irregular library
    that holds the clipped keys; expected counts from a dictionary of the ':'-joined keys (fast2q.py:362-367)"""
    length, st1, st2 = 10, [4], [6]
    recs1 = [(b"ACGTACGTACGTAC", b"I" * 14), (b"TTTTGGGGCC", b"I" * 10), (b"ACG", b"III"), (b"ACGTACGTACGTACGG", b"I" * 16)]
    recs2 = [(b"GGGGGGCATCA", b"I" * 11), (b"AAAAAACCC", b"I" * 9), (b"TTTTTTTTTTTTTTTTTTTT", b"I" * 20), (b"CCCCCCAT", b"I" * 8)]
    for rc2 in (False, True):
        keys = {}
        for (s1, _), (s2, _) in zip(recs1, recs2):
            m2 = PC.revcomp(s2) if rc2 else s2
            k = (s1[4:14] + b":" + m2[6:16]).decode()
            keys[k] = keys.get(k, 0) + 1
        lib = list(keys) + ["ACGTACGTAC:GGGGGGGGGG"]
        pe = PEmu(lib, st1 + st2, 1, rc2, miss=0, length=length)
        counts, stats = pe.count_all_byte_exact(PC.fastq_of(recs1), PC.fastq_of(recs2))
        pe.close()
        assert counts == [keys[k] for k in keys] + [0] and stats == [4, 4, 0, 0, 0]


@pytest.mark.parametrize("rc2", [False, True])
def test_extract_count_on_pairs_vs_oracle(rc2):
    length, st1, st2 = 8, [3], [20, 40]
    lib = PC.pair_library(40, length, 1, 2, 9)
    fq1, fq2 = PC.make_pairs(lib, length, st1, st2, rc2, 2500, seed=2, len1=70, len2=90, p_lowq=0.4)
    (start, merged), = PC.merged_groups(fq1, fq2, st1, st2, length, rc2)[0].items()
    o = O.Oracle(mode="EC", length=length, start=start)
    o.count_fastq(merged)
    pe = PEmu(None, st1 + st2, 1, rc2, mode="EC", length=length)
    _, stats = pe.count_all_byte_exact(fq1, fq2)
    rows = pe.ec_rows()
    pe.close()
    assert stats == o.stats() and [r[0] for r in rows] == o.keys() and [r[1] for r in rows] == o.counts()


def test_pairing_by_name():
    t = fast2q.mate_token
    assert t("x_S1_L001_R1_001.fastq.gz") == ("x_S1_L001_R*_001.fastq.gz", 1)
    assert t("/d/x_S1_L001_R2_001.fastq.gz") == ("x_S1_L001_R*_001.fastq.gz", 2)
    assert t("a_1.fq") == ("a_*.fq", 1) and t("a_2.fq") == ("a_*.fq", 2)
    assert t("s_R1_x_R2.fastq") == ("s_R1_x_R*.fastq", 2)              # the LAST token decides
    assert t("s_R1.fastq.gz")[1] == 1 and t("plain.fastq") == (None, 0) and t("b_R12.fastq") == (None, 0)
    files = ["d/s_R1_x_R2.fastq", "d/b_2.fastq.gz", "d/s_R1_x_R1.fastq", "d/b_1.fastq.gz"]
    assert fast2q.pair_files(files) == [("d/s_R1_x_R1.fastq", "d/s_R1_x_R2.fastq"), ("d/b_1.fastq.gz", "d/b_2.fastq.gz")]
    assert fast2q._sample_name("d/x_S1_L001_R1_001.fastq.gz") == "x_S1_L001_R1_001"
    with pytest.raises(ValueError, match="lonely_R1.fastq"):
        fast2q.pair_files(["d/lonely_R1.fastq", "d/b_1.fastq.gz", "d/b_2.fastq.gz"])
    with pytest.raises(ValueError, match="plain.fastq"):
        fast2q.pair_files(["d/plain.fastq"])


@pytest.mark.parametrize("argv,word", [(["--pe", "--st2", "3", "--us", "ACGT"], "--us"), (["--st2", "3"], "--st2"), (["--rc2"], "--rc2"),
                                       (["--pe"], "--st2"), (["-t", "--pe", "--st2", "3"], "-t")])
def test_command_line_refusals(argv, word, capsys):
    with pytest.raises(SystemExit):
        fast2q.input_parser(["-c", "--s", "x", "--g", "y", "--o", "z"] + argv)
    assert word in capsys.readouterr().out


def test_command_line_refuses_a_file_without_its_mate_and_several_ranks(tmp_path, capsys, monkeypatch):
    (tmp_path / "a_R1.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    p = fast2q.input_parser(["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path), "--pe", "--st2", "0", "--rc2"])
    assert p["paired"] and p["start2"] == "0" and p["rc2"] is True
    p["test_mode"] = False
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(p)
    assert "a_R1.fastq has no mate file" in capsys.readouterr().out
    (tmp_path / "a_R2.fastq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    q = fast2q.file_sizer_split(dict(p))
    assert q["sequencing_files"]["files"] == [str(tmp_path / "a_R1.fastq")] and q["mates"] == {str(tmp_path / "a_R1.fastq"): str(tmp_path / "a_R2.fastq")}
    # several ranks: refused where the samples are listed, and by reads_counter itself for a caller that gets past that
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    with pytest.raises(SystemExit):
        fast2q.file_sizer_split(dict(p))
    said = capsys.readouterr().out
    assert "--pe" in said and "several ranks" in said
    q["Running Mode"], q["Progress bar"] = "EC", False
    monkeypatch.setattr(fast2q, "_context_for", lambda seqs, kwargs: object())
    monkeypatch.setattr(fast2q, "_drop_context", lambda ctx: None)
    with pytest.raises(RuntimeError, match="--pe.*several ranks"):
        fast2q.reads_counter(0, str(tmp_path / "a_R1.fastq"), {}, q, {})
    monkeypatch.undo()
    # without --pe the listing is what it was
    plain = fast2q.input_parser(["-c", "--s", str(tmp_path), "--g", "y", "--o", str(tmp_path)])
    assert "paired" not in plain and "mates" not in plain


def test_header_declares_the_paired_calls_and_the_binding_exports_them():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    for name in ("f2q_set_mate2", "f2q_count_block_paired", "f2q_block_from_fastq_paired", "f2q_count_file_paired"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in binding.EXPORTS
    assert re.search(r"F2Q_EPAIRING\s*=\s*-9", text) and binding.F2Q_EPAIRING == -9 and binding.ERRORS[-9] == "EPAIRING"
    assert re.search(r"#define\s+F2Q_ABI_VERSION\s+1\b", text)
    if os.path.exists(binding.LIB_PATH):
        L = binding.load()
        assert all(hasattr(L, s) for s in binding.EXPORTS)
