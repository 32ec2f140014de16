"""Paired-end samples on the device: f2q_set_mate2 + the *_paired calls against the oracle on merged reads
(tests/paired_cases.py), bit-exact on the counts and all five counters."""
import csv
import functools
import gzip
import importlib
import os

import pytest

import paired_cases as PC
from conftest import bgzf_bytes, pkg
from oracle import oracle as O

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
PATH_MULTI_LDS = 10


@pytest.fixture(scope="module")
def P():
    return pkg()


GEOMS = {"1+1x10": ([5], [30], 10), "2+1x7": ([0, 40], [12], 7), "1+2x6": ([100], [3, 60], 6), "far9": ([120], [135], 9)}


@functools.lru_cache(maxsize=4)
def uniform_case(geom, rc2, combo, n=100000):
    st1, st2, length = GEOMS[geom]
    lib = PC.pair_library(2000, length, len(st1), len(st2), 7, combinatorial=combo)
    fq1, fq2 = PC.make_pairs_uniform(lib, length, st1, st2, rc2, n, seed=len(geom) + 2 * rc2 + combo)
    return lib, fq1, fq2


def counter(P, lib, st1, st2, length, rc2, **kw):
    return P.Counter(features=lib, start=",".join(map(str, st1)), start2=",".join(map(str, st2)), rc2=rc2, length=length, **kw)


@pytest.mark.parametrize("combo", [False, True], ids=["pairs", "combinatorial"])
@pytest.mark.parametrize("rc2", [False, True], ids=["fwd", "rc2"])
@pytest.mark.parametrize("miss", [0, 1, 2])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_uniform_pairs_vs_oracle(P, geom, miss, rc2, combo):
    """100 k pairs of 150 + 150 bases: counts and the five counters against the oracle on the merged reads; an A:B library
    with a 14..21-base joined key and --m <= 1 runs on the library-in-LDS kernel with no pair on the byte-exact road
    (the 'N's travel as flag bits)"""
    st1, st2, length = GEOMS[geom]
    lib, fq1, fq2 = uniform_case(geom, rc2, combo)
    counts, stats, uncovered = PC.pair_oracle(lib, fq1, fq2, st1, st2, length, rc2, miss)
    assert uncovered == 0 and stats[0] == 100000 and stats[1] > 10000
    with counter(P, lib, st1, st2, length, rc2, miss=miss) as c:
        used, t = c.count_block_paired(fq1, fq2, want_timing=True)
        got, gstats = c.read_counts()
    assert used == (len(fq1), len(fq2))
    assert list(gstats) == stats and list(got) == counts
    joined = (len(st1) + len(st2)) * length
    if 14 <= joined <= 21 and miss <= 1:
        assert t["path"] == PATH_MULTI_LDS and t["general_reads"] == 0 and t["fast_reads"] == 100000


@pytest.mark.parametrize("rc2", [False, True], ids=["fwd", "rc2"])
def test_every_road_gives_the_same(P, monkeypatch, rc2):
    """f2q_count_block_paired, f2q_block_from_fastq_paired + f2q_count_resident, and the same under F2Q_HOST_PACK=1,
    F2Q_FORCE_GENERAL=1, F2Q_NO_LT=1"""
    st1, st2, length = GEOMS["1+1x10"]
    lib, fq1, fq2 = uniform_case("1+1x10", rc2, False)
    counts, stats, _ = PC.pair_oracle(lib, fq1, fq2, st1, st2, length, rc2, 1)
    seen = {}
    for env in ({}, {"F2Q_HOST_PACK": "1"}, {"F2Q_FORCE_GENERAL": "1"}, {"F2Q_NO_LT": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with counter(P, lib, st1, st2, length, rc2, miss=1) as c:
            _, t = c.count_block_paired(fq1, fq2, want_timing=True)
            a = c.read_counts()
            c.reset()
            blk = c.block_from_fastq_paired(fq1, fq2)
            info = blk.info()
            t2 = c.count_resident(blk)
            b = c.read_counts()
            blk.free()
        for k in env:
            monkeypatch.delenv(k)
        assert list(a[1]) == stats and list(a[0]) == counts, env
        assert list(b[1]) == stats and list(b[0]) == counts, env
        assert info["n_reads"] == 100000 and t2["reads"] == 100000
        seen[tuple(env)] = (t["path"], t["general_reads"])
    assert seen[()] == (PATH_MULTI_LDS, 0) and seen[("F2Q_HOST_PACK",)] == (PATH_MULTI_LDS, 0)
    assert seen[("F2Q_FORCE_GENERAL",)][1] == 100000 and seen[("F2Q_NO_LT",)][0] == 5


@pytest.mark.parametrize("rc2", [False, True], ids=["fwd", "rc2"])
@pytest.mark.parametrize("miss", [0, 1, 2])
@pytest.mark.parametrize("geom", ["1+1x10", "2+1x7", "1+2x6"])
def test_ragged_and_dirty_pairs_vs_oracle(P, geom, miss, rc2):
    """mates of 0 .. 160 bases (some ending inside a window), N / IUPAC / lower-case bases, quality lines of another length,
    quality bytes >= 128, CRLF and trailing blanks: by the group-by-length construction.  No pair has BOTH mates cut short
    (a property of the generator, asserted: uncovered == 0); those have a test of their own below."""
    st1, st2, length = GEOMS[geom]
    lib = PC.pair_library(300, length, len(st1), len(st2), 5, combinatorial=True)
    fq1, fq2 = PC.make_pairs(lib, length, st1, st2, rc2, 6000, seed=40 + miss, ragged=True, dirty=True)
    counts, stats, uncovered = PC.pair_oracle(lib, fq1, fq2, st1, st2, length, rc2, miss)
    assert uncovered == 0 and stats[0] == 6000
    with counter(P, lib, st1, st2, length, rc2, miss=miss) as c:
        used, t = c.count_block_paired(fq1, fq2, want_timing=True)
        got, gstats = c.read_counts()
    assert used == (len(fq1), len(fq2))
    assert list(gstats) == stats and list(got) == counts
    assert t["fast_reads"] > 0 and t["general_reads"] > 0


def test_both_mates_cut_short_exact_keys(P):
    """both mates end inside a window: --m 0 against an irregular library holding the clipped keys; expected counts from a
    dictionary of the ':'-joined keys (the reference's exact hit, fast2q.py:362-367)"""
    recs1 = [(b"ACGTACGTACGTAC", b"I" * 14), (b"TTTTGGGGCC", b"I" * 10), (b"ACG", b"III"), (b"ACGTACGTACGTACGG", b"I" * 16)]
    recs2 = [(b"GGGGGGCATCA", b"I" * 11), (b"AAAAAACCC", b"I" * 9), (b"TTTTTTTTTTTTTTTTTTTT", b"I" * 20), (b"CCCCCCAT", b"I" * 8)]
    for rc2 in (False, True):
        keys = {}
        for (s1, _), (s2, _) in zip(recs1, recs2):
            m2 = PC.revcomp(s2) if rc2 else s2
            k = (s1[4:14] + b":" + m2[6:16]).decode()
            keys[k] = keys.get(k, 0) + 1
        lib = list(keys) + ["ACGTACGTAC:GGGGGGGGGG"]
        with counter(P, lib, [4], [6], 10, rc2, miss=0) as c:
            c.count_block_paired(PC.fastq_of(recs1), PC.fastq_of(recs2))
            got, stats = c.read_counts()
        assert list(got) == [keys[k] for k in keys] + [0] and list(stats) == [4, 4, 0, 0, 0]


@pytest.mark.parametrize("rc2", [False, True], ids=["fwd", "rc2"])
def test_extract_count_on_pairs(P, rc2):
    """keys, counts and first-seen order against the oracle on the merged reads"""
    length, st1, st2 = 8, [3], [20, 40]
    lib = PC.pair_library(60, length, 1, 2, 9)
    fq1, fq2 = PC.make_pairs_uniform(lib, length, st1, st2, rc2, 30000, seed=2, len1=70, len2=90, p_lowq=0.02)
    (start, merged), = PC.merged_groups(fq1, fq2, st1, st2, length, rc2)[0].items()
    o = O.Oracle(mode="EC", length=length, start=start)
    o.count_fastq(merged)
    with P.Counter(mode="EC", length=length, start="3", start2="20,40", rc2=rc2) as c:
        c.count_block_paired(fq1[:len(fq1) // 2], fq2[:len(fq2) // 2])           # (whole records: every record is as long)
        c.count_block_paired(fq1[len(fq1) // 2:], fq2[len(fq2) // 2:])
        _, stats = c.read_counts()
        rows = c.ec_results()
    assert list(stats) == o.stats() and [r[0] for r in rows] == o.keys() and [r[1] for r in rows] == o.counts()


def _drifting_case(rc2=True, n=20000):
    st1, st2, length = [5], [30], 10
    lib = PC.pair_library(400, length, 1, 1, 12)
    fq1, fq2 = PC.make_pairs_uniform(lib, length, st1, st2, rc2, n, seed=77, len1=60, len2=250)   # the files drift apart by many pieces
    return lib, st1, st2, length, fq1, fq2


def _in_memory(P, lib, st1, st2, length, rc2, fq1, fq2):
    with counter(P, lib, st1, st2, length, rc2, miss=1) as c:
        c.count_block_paired(fq1, fq2)
        counts, stats = c.read_counts()
    return list(counts), list(stats)


@pytest.mark.parametrize("chunk", ["4096", "65536", "1000000"])
@pytest.mark.parametrize("kinds", [("plain", "plain"), ("gzip", "bgzf"), ("bgzf", "plain")], ids=lambda k: "+".join(k))
def test_paired_files_equal_the_in_memory_call(P, tmp_path, monkeypatch, kinds, chunk):
    lib, st1, st2, length, fq1, fq2 = _drifting_case()
    want = _in_memory(P, lib, st1, st2, length, True, fq1, fq2)
    paths = []
    for k, (kind, data) in enumerate(zip(kinds, (fq1, fq2))):
        p = tmp_path / f"s_R{k + 1}.fastq{'' if kind == 'plain' else '.gz'}"
        p.write_bytes(data if kind == "plain" else gzip.compress(data, 1) if kind == "gzip" else bgzf_bytes(data))
        paths.append(str(p))
    monkeypatch.setenv("F2Q_FILE_CHUNK", chunk)
    with counter(P, lib, st1, st2, length, True, miss=1) as c:
        t, truncated = c.count_file_paired(*paths)
        counts, stats = c.read_counts()
    assert not truncated and t["reads"] == 20000
    assert (list(counts), list(stats)) == want


@pytest.mark.parametrize("longer", [0, 1])
def test_one_file_a_record_longer(P, tmp_path, monkeypatch, longer):
    lib, st1, st2, length, fq1, fq2 = _drifting_case(n=3000)
    want = _in_memory(P, lib, st1, st2, length, True, fq1, fq2)
    data = [fq1, fq2]
    data[longer] += b"@extra\nACGTACGTAC\n+\nIIIIIIIIII\n"
    for k in range(2):
        (tmp_path / f"x_{k + 1}.fastq").write_bytes(data[k])
    monkeypatch.setenv("F2Q_FILE_CHUNK", "8192")
    with counter(P, lib, st1, st2, length, True, miss=1) as c:
        with pytest.raises(P.binding.F2QError) as err:
            c.count_file_paired(str(tmp_path / "x_1.fastq"), str(tmp_path / "x_2.fastq"))
        assert err.value.code == P.binding.F2Q_EPAIRING and f"x_{longer + 1}.fastq" in str(err.value)
        counts, stats = c.read_counts()
    assert (list(counts), list(stats)) == want


@pytest.mark.parametrize("side", [0, 1])
def test_cut_off_archive_counts_the_pairs_before_the_cut(P, tmp_path, monkeypatch, side):
    lib, st1, st2, length, fq1, fq2 = _drifting_case(n=6000)
    data = [fq1, fq2]
    z = gzip.compress(data[side], 1)
    cut = z[:len(z) * 2 // 3]
    import zlib
    readable = zlib.decompressobj(31).decompress(cut)
    readable = readable[:readable.rfind(b"\n") + 1]                      # every complete line before the damage
    prefix = [fq1, fq2]
    prefix[side] = readable
    want = _in_memory(P, lib, st1, st2, length, True, *prefix)
    assert 0 < want[1][0] < 6000
    paths = [str(tmp_path / "c_R1.fastq.gz"), str(tmp_path / "c_R2.fastq.gz")]
    for k in range(2):
        open(paths[k], "wb").write(cut if k == side else gzip.compress(data[k], 1))
    monkeypatch.setenv("F2Q_FILE_CHUNK", "16384")
    with counter(P, lib, st1, st2, length, True, miss=1) as c:
        _, truncated = c.count_file_paired(*paths)
        counts, stats = c.read_counts()
    assert truncated and (list(counts), list(stats)) == want


def test_state_errors(P, tmp_path):
    lib = PC.pair_library(20, 10, 1, 1, 1)
    fq = b"@r\n" + b"A" * 50 + b"\n+\n" + b"I" * 50 + b"\n"
    (tmp_path / "f.fastq").write_bytes(fq)
    E = P.binding.F2QError
    with counter(P, lib, [5], [30], 10, False) as c:
        for call in (lambda: c.count_block(fq), lambda: c.block_from_fastq(fq), lambda: c.count_file(str(tmp_path / "f.fastq")),
                     lambda: c.synth_create(seed=1, n_reads=10, read_len=50), lambda: c.set_mate2("3")):
            with pytest.raises(E) as err:
                call()
            assert err.value.code == -7
        assert c.count_block_paired(fq, fq) == (len(fq), len(fq))
    with P.Counter(features=lib, length=10, start="5,30") as c:
        for call in (lambda: c.count_block_paired(fq, fq), lambda: c.block_from_fastq_paired(fq, fq),
                     lambda: c.count_file_paired(str(tmp_path / "f.fastq"), str(tmp_path / "f.fastq")), lambda: c.set_mate2("3")):
            with pytest.raises(E) as err:
                call()
            assert err.value.code == -7
    with P.Counter(length=10, upstream="ACGT", mode="EC") as c:
        with pytest.raises(E) as err:
            c.set_mate2("3")
        assert err.value.code == -1
    with P.Counter(length=10, start="5", mode="EC") as c:
        for bad in ([], [-1], list(range(16))):
            with pytest.raises(E) as err:
                c.set_mate2(bad)
            assert err.value.code == -1


class _Clock:
    """a scripted perf_counter, as tests/test_gpu_cli.py scripts it: the samples take 0.5 s, 0.75 s, ... whoever asks"""

    def __init__(self):
        self.t = 100.0

    def __call__(self):
        self.t += 0.25
        return self.t


def test_command_line_end_to_end(P, tmp_path, monkeypatch):
    """-c --pe --st .. --st2 .. --rc2 on a directory with two paired samples: the feature rows of compiled.csv and the
    per-sample rows of compiled_stats.csv equal those of the same command line run single-end on merged files named like
    the R1 files; the parameter header lines say what the flags say"""
    st1, st2, length = [5], [30], 10
    lib = PC.pair_library(80, length, 1, 1, 31)
    csvp = tmp_path / "lib.csv"
    csvp.write_text("".join(f"f{i},{s}\n" for i, s in enumerate(lib)))
    pe, se = tmp_path / "pe", tmp_path / "se"
    pe.mkdir(); se.mkdir()
    for k, (name, n) in enumerate((("alpha_S1_L001_R1_001", 3000), ("beta_R1", 1200))):
        fq1, fq2 = PC.make_pairs_uniform(lib, length, st1, st2, True, n, seed=50 + k, len1=75, len2=75)
        (pe / f"{name}.fastq.gz").write_bytes(gzip.compress(fq1, 1))
        (pe / f"{name.replace('R1', 'R2')}.fastq.gz").write_bytes(gzip.compress(fq2, 1))
        (start, merged), = PC.merged_groups(fq1, fq2, st1, st2, length, True)[0].items()
        assert start == "5,105"
        (se / f"{name}.fastq.gz").write_bytes(gzip.compress(merged, 1))
    outs = {}
    for tag, argv in (("pe", ["--s", str(pe), "--pe", "--st", "5", "--st2", "30", "--rc2"]), ("se", ["--s", str(se), "--st", "5,105"])):
        monkeypatch.setattr(fast2q.time, "perf_counter", _Clock())
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--g", str(csvp), "--o", str(out), "--l", str(length), "--m", "1", "--pb", "--cp", "1"] + argv)
        d = [x for x in out.iterdir() if x.is_dir()][0]
        outs[tag] = (list(csv.reader(open(d / "compiled.csv", newline=""))), list(csv.reader(open(d / "compiled_stats.csv", newline=""))))
    assert outs["pe"][0] == outs["se"][0] and outs["pe"][0][0] == ["#Feature", "alpha_S1_L001_R1_001", "beta_R1"]
    assert sum(int(r[1]) for r in outs["pe"][0][1:]) > 1500
    rows = lambda stats: [r for r in stats if r and not r[0].startswith("#")]
    assert rows(outs["pe"][1]) == rows(outs["se"][1]) and len(rows(outs["pe"][1])) == 2
    head = [r[0] for r in outs["pe"][1] if r and r[0].startswith("#") and r[0] != "#Sample name"]
    assert "#Feature start position in the read: 5" in head
    assert "#Paired-end, feature start position in mate 2: 30" in head and "#Mate 2 reverse-complemented: yes" in head
    assert any(h.startswith("#cmd used:") and "--pe" in h and "--st2 30" in h and "--rc2" in h for h in head)
    se_head = [r[0] for r in outs["se"][1] if r and r[0].startswith("#")]
    assert "#Feature start position in the read: 5,105" in se_head and not any("Paired-end" in h for h in se_head)
