"""--stagger on the device: f2q_set_stagger / k_count_stagger / f2q_read_stagger against the plain-Python expectation of
tests/stagger_cases.py (the oracle's Counter-mode verdict at every start, combined by the rule of include/f2q.h), in both
layouts, through every single-process counting entry point, and the command line's outputs."""
import csv
import gzip
import importlib

import numpy as np
import pytest

import stagger_cases as GC
from conftest import bgzf_bytes, pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")
ESTATE, EINVAL = -7, -1


@pytest.fixture(scope="module")
def P():
    return pkg()


def result(c):
    counts, stats = c.read_counts()
    perfect, imperfect = c.read_stagger()
    return list(counts), list(stats), list(perfect), list(imperfect)


def counted(P, lib, fq, n, used=None, **run):
    with P.Counter(features=lib, stagger=n, **run) as c:
        assert c.count_block(fq) == (len(fq) if used is None else used)
        return result(c)


def plain(P, lib, fq, **run):
    with P.Counter(features=lib, **run) as c:
        c.count_block(fq)
        counts, stats = c.read_counts()
    return list(counts), list(stats)


_WANT = {}


def want_base(miss=1, phred=30):
    """the base shape's expectation, computed once per (--m, --ph) and shared"""
    key = (miss, phred)
    if key not in _WANT:
        lib, fq, run = GC.base()
        _WANT[key] = GC.expect(lib, fq, GC.N, **dict(run, miss=miss, phred=phred))
    return _WANT[key]


# 1
@pytest.mark.parametrize("layout", ["span", "walk"])
@pytest.mark.parametrize("miss,phred", [(0, 30), (1, 30), (2, 30), (1, 1), (1, 41)])
def test_base_shape(P, monkeypatch, miss, phred, layout):
    lib, fq, run = GC.base()
    if layout == "walk":
        monkeypatch.setenv("F2Q_STAGGER_WALK", "1")
    got = counted(P, lib, fq, GC.N, **dict(run, miss=miss, phred=phred))
    assert tuple(got) == tuple(want_base(miss, phred))
    GC.check_invariants(*got)


# 2 .. 6, and the pool of 7 counted once
@pytest.mark.parametrize("layout", ["span", "walk"])
@pytest.mark.parametrize("name", sorted(n for n in GC.CASES if n != "base"))
def test_cases_vs_expectation(P, monkeypatch, name, layout):
    lib, fq, run, n = GC.CASES[name]()
    used = GC.RE.oracle_of(lib, fq, **run)[2]
    if layout == "walk":
        monkeypatch.setenv("F2Q_STAGGER_WALK", "1")
    got = counted(P, lib, fq, n, used=used, **run)
    assert tuple(got) == tuple(GC.expect(lib, fq, n, **run))
    GC.check_invariants(*got)


# 7
def test_second_pass(P):
    import subprocess
    import sys
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                           capture_output=True, text=True, check=True)
    fq, reps = GC.second_pass(int(probe.stdout.split()[-1]))
    lib = GC.UC.library()
    run = dict(GC.RUN, miss=1)
    want = GC.scaled(GC.expect(lib, GC.pass_pool(), GC.N, **run), reps)
    with P.Counter(features=lib, stagger=GC.N, **run) as c:
        blk = c.block_from_fastq(fq)
        assert blk.info()["n_reads"] == reps * GC.POOL
        for _ in range(2):                                               # (and the launch repeated on the resident block)
            c.reset()
            c.count_resident(blk)
            assert tuple(result(c)) == tuple(want)
        blk.free()


# 8
def test_no_oracle_two_hundred_thousand_reads(P, monkeypatch):
    guides = binding.synth_library(0x57A66, 500, 20)
    run = dict(miss=1, phred=30, length=20, start="0")
    with P.Counter(features=guides, **run) as c:
        fq = bytes(c.synth_fastq(seed=12, n_reads=200000, read_len=60))
        c.count_block(fq)
        at0 = [list(x) for x in c.read_counts()]
    # every read gets i % 9 bases in front of it: its feature now sits at offset i % 9
    rng = np.random.default_rng(5)
    pad = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(200000, 8)).tobytes()
    lines = fq.split(b"\n")
    for i in range(200000):
        d = i % 9
        lines[4 * i + 1] = pad[8 * i:8 * i + d] + lines[4 * i + 1]
        lines[4 * i + 3] = b"I" * d + lines[4 * i + 3]
    shifted = b"\n".join(lines)
    got = {}
    for layout in ("span", "walk"):
        if layout == "walk":
            monkeypatch.setenv("F2Q_STAGGER_WALK", "1")
        with P.Counter(features=guides, stagger=8, **run) as c:
            c.count_block(shifted)
            got[layout] = result(c)
    assert got["span"] == got["walk"]
    counts, stats, perfect, imperfect = got["span"]
    GC.check_invariants(*got["span"])
    assert stats[0] == 200000 and stats[1] >= at0[1][1]                  # an exact window is found wherever it was moved to
    assert all(p >= at0[1][1] // 9 - 2000 for p in perfect) and sum(counts) >= sum(at0[0])
    with P.Counter(features=guides, stagger=8, **run) as c:              # with every feature at offset 0: the plain run's perfect reads, all at 0
        c.count_block(fq)
        zero = result(c)
    assert zero[2][0] == at0[1][1] and sum(zero[2][1:]) <= 0.01 * at0[1][1]
    assert zero[1][1] >= at0[1][1] and zero[1][0] == 200000


# ---- every entry point, on case 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [7, 500])
def test_pieces_equal_one_block(P, per):
    lib, fq, run = GC.base()
    with P.Counter(features=lib, stagger=GC.N, miss=1, **run) as c:
        for piece in GC.pieces(fq, per):
            assert c.count_block(piece) == len(piece)
        assert tuple(result(c)) == tuple(want_base())


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf", "bgzf_device_inflate"])
def test_streamed_files_equal_the_one_block_result(P, tmp_path, monkeypatch, kind):
    lib, fq, run = GC.base()
    monkeypatch.setenv("F2Q_FILE_CHUNK", "4096")
    if kind == "bgzf_device_inflate":
        monkeypatch.setenv("F2Q_DEVICE_INFLATE", "1")
    path = tmp_path / {"plain": "s.fastq", "gzip": "s.fastq.gz"}.get(kind, "s.bgzf.fastq.gz")
    path.write_bytes(fq if kind == "plain" else gzip.compress(fq) if kind == "gzip" else bgzf_bytes(fq, block=3000))
    with P.Counter(features=lib, stagger=GC.N, miss=1, **run) as c:
        _, truncated = c.count_file(str(path))
        got = result(c)
    assert not truncated and tuple(got) == tuple(want_base())


def test_resident_blocks_device_text_and_host_pack(P, monkeypatch, capfd):
    lib, fq, run = GC.base()
    want = tuple(want_base())
    monkeypatch.setenv("F2Q_TRACE", "1")
    with P.Counter(features=lib, stagger=GC.N, miss=1, **run) as c:
        assert "k_count_stagger (span layout)" in capfd.readouterr().err     # F2Q_TRACE=1 names the kernel and the layout
        blk = c.block_from_fastq(fq)
        assert blk.info()["n_general"] == blk.info()["n_reads"] == want[1][0]      # every read takes the raw-record road
        t = c.count_resident(blk)
        assert t["general_reads"] == want[1][0] and tuple(result(c)) == want
        c.reset()
        c.count_resident_queued(blk)
        c.queued_times()
        assert tuple(result(c)) == want
        blk.free()
        c.reset()
        text = c.text_upload(fq)
        assert c.count_text(text) == len(fq) and tuple(result(c)) == want
        text.free()
    monkeypatch.delenv("F2Q_TRACE")
    monkeypatch.setenv("F2Q_HOST_PACK", "1")
    assert tuple(counted(P, lib, fq, GC.N, miss=1, **run)) == want


def test_reset_and_a_second_library_start_afresh(P):
    lib, fq, run = GC.base()
    fq2 = b"".join(GC.pieces(fq, 400)[1:3])
    zero = ([0] * len(lib), [0] * 5, [0] * (GC.N + 1), [0] * (GC.N + 1))
    with P.Counter(features=lib, stagger=GC.N, miss=1, **run) as c:
        assert tuple(result(c)) == zero                                  # nothing counted yet
        assert c.count_block(fq) == len(fq)
        first = result(c)
        c.reset()
        assert tuple(result(c)) == zero
        assert c.count_block(fq2) == len(fq2)
        second = result(c)
        c.set_features(lib[:100])                                        # a new library starts afresh
        perfect, imperfect = c.read_stagger()
        assert perfect.shape == (GC.N + 1,) and not perfect.any() and not imperfect.any()
        assert c.count_block(fq) == len(fq)
        assert tuple(result(c)) == tuple(GC.expect(lib[:100], fq, GC.N, miss=1, **run))
    assert tuple(first) == tuple(want_base())
    assert tuple(second) == tuple(GC.expect(lib, fq2, GC.N, miss=1, **run))


def test_setter_before_or_after_the_library_and_cleared(P):
    lib, fq, run = GC.base()
    with P.Counter(stagger=GC.N, miss=1, **run) as c:                   # before the library
        assert [list(x) for x in c.read_stagger()] == [[0] * (GC.N + 1)] * 2
        c.set_features(lib)
        assert c.count_block(fq) == len(fq) and tuple(result(c)) == tuple(want_base())
    with P.Counter(features=lib, miss=1, **run) as c:                   # after it, and set again with another n
        c.set_stagger(0)                                                 # accepted on a plain context, changes nothing
        c.set_stagger(3)
        c.set_stagger(GC.N)
        assert c.stagger == GC.N
        assert c.count_block(fq) == len(fq) and tuple(result(c)) == tuple(want_base())
        i64p = binding.C.POINTER(binding.C.c_int64)
        assert c._L.f2q_read_stagger(c._h, None, None, GC.N + 1) == 0    # either pointer may be NULL
        only = np.zeros(GC.N + 1, dtype=np.int64)
        assert c._L.f2q_read_stagger(c._h, None, only.ctypes.data_as(i64p), GC.N + 1) == 0 and list(only) == want_base()[3]
    # n = 0 clears it: the context counts what a context without the call counts, on the kernels it launched before
    want = plain(P, lib, fq, miss=1, **run)
    with P.Counter(features=lib, miss=1, **run) as c:
        blk = c.block_from_fastq(fq)
        before = {k: blk.info()[k] for k in ("n_reads", "n_general")}
        blk.free()
    for first in (True, False):
        with P.Counter(features=lib if first else None, stagger=GC.N, miss=1, **run) as c:
            c.set_stagger(0)
            if not first:
                c.set_features(lib)
            blk = c.block_from_fastq(fq)
            assert {k: blk.info()[k] for k in before} == before and before["n_general"] < before["n_reads"]      # the packed tiles again
            c.count_resident(blk)
            counts, stats = c.read_counts()
            assert (list(counts), list(stats)) == want
            _refused(ESTATE, ["f2q_set_stagger"], c.read_stagger)
            blk.free()


def _refused(code, words, call):
    with pytest.raises(binding.F2QError) as exc:
        call()
    assert exc.value.code == code and all(w in str(exc.value) for w in words), str(exc.value)


def test_state_and_argument_refusals_in_both_orders(P, tmp_path):
    lib, fq, run = GC.base()
    bcs = [b"ACGTACGT", b"TTGCAAGC"]
    pairs = ["ACGTACGTAC:TTGCATTGCA", "CCCCAAAATT:GGGGTTTTAA"]
    # the stagger second
    with P.Counter(mode="EC", **run) as c:
        _refused(ESTATE, ["Extract+Count"], lambda: c.set_stagger(8))
        c.set_stagger(0)
    with P.Counter(start2="0", **run) as c:
        _refused(ESTATE, ["paired"], lambda: c.set_stagger(8))
    with P.Counter(upstream="ACGTAC", downstream="TTGCAT", length=20) as c:
        _refused(ESTATE, ["--us/--ds"], lambda: c.set_stagger(8))
    with P.Counter(start="0,30", length=10) as c:
        _refused(ESTATE, ["one window"], lambda: c.set_stagger(8))
    with P.Counter(features=lib, umi=(30, 8), **run) as c:
        _refused(ESTATE, ["UMI"], lambda: c.set_stagger(8))
    with P.Counter(features=lib, umi_header=("_", 8), **run) as c:
        _refused(ESTATE, ["UMI"], lambda: c.set_stagger(8))
    with P.Counter(features=lib, sample_barcodes=(30, bcs), **run) as c:
        _refused(ESTATE, ["f2q_set_sample_barcodes"], lambda: c.set_stagger(8))
    with P.Counter(features=lib, strand="both", **run) as c:
        _refused(ESTATE, ["f2q_set_strand"], lambda: c.set_stagger(8))
    with P.Counter(features=lib, **run) as c:
        for n in (33, -1, 1000):
            assert c._L.f2q_set_stagger(c._h, n) == EINVAL and str(n) in c._L.f2q_last_error(c._h).decode()
        _refused(ESTATE, ["f2q_set_stagger"], c.read_stagger)
        assert c.count_block(fq[:4000]) > 0
        _refused(ESTATE, ["before counting"], lambda: c.set_stagger(8))
        c.set_stagger(0)                                                 # 0 on a plain context even now
    # the stagger first: the message names it
    path = tmp_path / "s.fastq"
    path.write_bytes(fq[:20000])
    with P.Counter(features=lib, stagger=8, **run) as c:
        assert c._L.f2q_read_stagger(c._h, None, None, 8) == EINVAL and "n + 1" in c._L.f2q_last_error(c._h).decode()
        _refused(ESTATE, ["stagger"], lambda: c.set_umi(30, 8))
        _refused(ESTATE, ["stagger"], lambda: c.set_umi_header("_", 8))
        _refused(ESTATE, [], lambda: c.set_umi_paired((0, 8), None))
        _refused(ESTATE, ["stagger"], lambda: c.set_sample_barcodes(30, bcs))
        _refused(ESTATE, ["stagger"], lambda: c.set_strand("both"))
        _refused(ESTATE, [], lambda: c.set_parts())
        _refused(ESTATE, [], lambda: c.set_mate2("0"))                   # (after f2q_set_features it is refused anyway)
        _refused(ESTATE, ["stagger", "ranks"], lambda: c.count_file_shard(str(path), 0, 2))
        n, _ = c.file_pieces(str(path), 1 << 16)
        _refused(ESTATE, ["stagger", "ranks"], lambda: c.count_pieces(str(path), 0, 2, 1 << 16, c.census_pieces(str(path), 0, 2, 1 << 16, n)))
        _, truncated = c.count_file_shard(str(path), 0, 1)               # one rank is a whole file
        assert not truncated and sum(c.read_stagger()[0]) > 0
        _refused(ESTATE, ["before counting"], lambda: c.set_stagger(0))  # counted: it stays a stagger context
    with P.Counter(stagger=8, **run) as c:                               # before the library: f2q_set_mate2 and the paired UMIs name it
        _refused(ESTATE, ["stagger"], lambda: c.set_mate2("0"))
        _refused(ESTATE, ["stagger"], lambda: c.set_umi_paired((0, 8), None))
    _refused(ESTATE, ["stagger"], lambda: P.Counter(stagger=8, umi=(30, 8), **run))
    _refused(ESTATE, ["Extract+Count"], lambda: P.Counter(mode="EC", stagger=8, **run))
    _refused(ESTATE, ["one window"], lambda: P.Counter(features=pairs, parts=True, stagger=8, start="0,30", length=10))


# ---- the command line ----------------------------------------------------------------------------------------------------
def _table(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


def test_cli_outputs(P, tmp_path, capsys):
    lib = GC.base()[0]
    base_fq = GC.base()[1]
    samples = {"s1": b"".join(GC.pieces(base_fq, 900)[:1]), "s2": b"".join(GC.pieces(base_fq, 500)[2:3])}
    indir = tmp_path / "in"
    indir.mkdir()
    for name, fq in samples.items():
        (indir / (name + ".fastq")).write_bytes(fq)
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    outs = {}
    for tag, extra in (("stagger", ["--stagger", "8"]), ("zero", ["--stagger", "0"]), ("plain", [])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(out), "--st", str(GC.S), "--l", "20", "--m", "1", "--pb"] + extra)
        (outs[tag],) = [d for d in out.iterdir() if d.is_dir()]
    capsys.readouterr()
    strip = lambda t: [r[:1] + r[3:] if r and not r[0].startswith("#") else r for r in t if not (r and r[0].startswith("#cmd used"))]    # (not the running times, not the command)
    # --stagger 0 is a run without the flag, byte for byte (but for the command line and the running times the files quote)
    assert (outs["zero"] / "compiled.csv").read_bytes() == (outs["plain"] / "compiled.csv").read_bytes()
    assert sorted(p.name for p in outs["zero"].iterdir()) == sorted(p.name for p in outs["plain"].iterdir())
    assert strip(_table(outs["zero"] / "compiled_stats.csv")) == strip(_table(outs["plain"] / "compiled_stats.csv"))
    assert not (outs["plain"] / "compiled_stagger.csv").exists() and not (outs["zero"] / "compiled_stagger.csv").exists()
    names = [f"g{i:03d}" for i in range(len(lib))]
    assert sorted(p.name for p in outs["stagger"].iterdir() if p.suffix == ".csv") == ["compiled.csv", "compiled_stagger.csv", "compiled_stats.csv"]
    want = {name: GC.expect(lib, fq, 8, miss=1, **GC.RUN) for name, fq in samples.items()}
    reads, stag = _table(outs["stagger"] / "compiled.csv"), _table(outs["stagger"] / "compiled_stagger.csv")
    assert reads[0] == ["#Feature", "s1", "s2"]
    for row in reads[1:]:
        f = names.index(row[0])
        assert [int(x) for x in row[1:]] == [want["s1"][0][f], want["s2"][0][f]]
    assert stag[0] == ["#Offset", "Start", "s1:perfect", "s1:imperfect", "s2:perfect", "s2:imperfect"]
    assert [[int(x) for x in r] for r in stag[1:]] == [[d, GC.S + d, want["s1"][2][d], want["s1"][3][d], want["s2"][2][d], want["s2"][3][d]] for d in range(9)]
    stats, plain_stats = _table(outs["stagger"] / "compiled_stats.csv"), _table(outs["plain"] / "compiled_stats.csv")
    header = ["#Stagger: 8"]
    at = stats.index(fast2q.STAGGER_STATS_HEAD)
    assert header in stats
    assert [r[0] for r in strip([r for r in stats[:at] if r != header])] == [r[0] for r in strip(plain_stats)]
    both = {s: [a + b for a, b in zip(want[s][2], want[s][3])] for s in samples}
    assert stats[at + 1:] == [[s, str(both[s][0]), str(sum(both[s][1:])), str(both[s].index(max(both[s])))] for s in ("s1", "s2")]
    # the counters of the run's own table are the rule's, and the columns of the offsets add up to them
    rows = {r[0]: r for r in stats[:at] if r and r[0] in samples}
    for s in samples:
        assert [int(x) for x in rows[s][3:]] == [want[s][1][0], want[s][1][1] + want[s][1][2], want[s][1][1], want[s][1][2], want[s][1][3], want[s][1][4]]
        assert sum(want[s][2]) == want[s][1][1] and sum(want[s][3]) == want[s][1][2]
