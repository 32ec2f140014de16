"""--indel on the device: f2q_set_indel / k_count_indel / f2q_read_indels against the plain-Python expectation of
tests/indel_cases.py (the oracle's Counter-mode verdict, then the rule of include/f2q.h for the reads it leaves unassigned),
through every single-process counting entry point, and the command line's outputs."""
import csv
import gzip
import importlib

import numpy as np
import pytest

import indel_cases as IC
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
    return (list(counts), list(stats)) + tuple(list(x) for x in c.read_indels())


def counted(P, lib, fq, used=None, **run):
    with P.Counter(features=lib, indel=True, **run) as c:
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
        lib, fq, run = IC.CASES["base"]()
        _WANT[key] = tuple(IC.expect(lib, fq, **dict(run, miss=miss, phred=phred)))
    return _WANT[key]


# 1
@pytest.mark.parametrize("miss,phred", [(0, 30), (1, 30), (2, 30), (1, 1), (1, 41)])
def test_base_shape(P, miss, phred):
    lib, fq, run = IC.CASES["base"]()
    got = counted(P, lib, fq, **dict(run, miss=miss, phred=phred))
    assert tuple(got) == want_base(miss, phred)
    IC.check_invariants(*got)


# the extremes, odd records, the staging edge, long reads, and the pool of the second pass counted once
@pytest.mark.parametrize("name", sorted(n for n in IC.CASES if n != "base"))
def test_cases_vs_expectation(P, name):
    lib, fq, run = IC.CASES[name]()
    used = IC.RE.oracle_of(lib, fq, **run)[2]
    got = counted(P, lib, fq, used=used, **run)
    assert tuple(got) == tuple(IC.expect(lib, fq, **run))
    IC.check_invariants(*got)


def test_second_pass(P):
    import subprocess
    import sys
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                           capture_output=True, text=True, check=True)
    fq, reps = IC.second_pass(int(probe.stdout.split()[-1]))
    lib = IC.UC.library()
    run = dict(IC.RUN, miss=1)
    want = IC.scaled(IC.expect(lib, IC.pass_pool(), **run), reps)
    with P.Counter(features=lib, indel=True, **run) as c:
        blk = c.block_from_fastq(fq)
        assert blk.info()["n_reads"] == reps * IC.POOL
        for _ in range(2):                                               # (and the launch repeated on the resident block)
            c.reset()
            c.count_resident(blk)
            assert tuple(result(c)) == tuple(want)
        blk.free()


def test_no_oracle_two_hundred_thousand_reads(P):
    guides = binding.synth_library(0x1DE15, 500, 20)
    run = dict(miss=1, phred=30, length=20, start="0")
    with P.Counter(features=guides, **run) as c:
        fq = bytes(c.synth_fastq(seed=13, n_reads=200000, read_len=60))
    # every fifth read loses one base of its window, every seventh gains one; the lines keep their 60 bytes
    rng = np.random.default_rng(6)
    where = rng.integers(0, 20, size=200000)
    base = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=200000).tobytes()
    lines = fq.split(b"\n")
    edited = 0
    for i in range(200000):
        s, p = lines[4 * i + 1], int(where[i])
        if i % 5 == 0:
            lines[4 * i + 1] = s[:p] + s[p + 1:] + base[i:i + 1]
            edited += 1
        elif i % 7 == 0:
            lines[4 * i + 1] = (s[:p] + base[i:i + 1] + s[p:])[:60]
            edited += 1
    text = b"\n".join(lines)
    with P.Counter(features=guides, **run) as c:
        c.count_block(text)
        without = [list(x) for x in c.read_counts()]
    with P.Counter(features=guides, indel=True, **run) as c:
        c.count_block(text)
        got = result(c)
    IC.check_invariants(*got)
    assert got[:2] == tuple(without) and got[1][0] == 200000         # counts and stats equal a context without the flag
    # the CPU expectation on the first 5 000 reads of this text (IC.expect) reports 714 deletion and 427 insertion reads of
    # its 1 572 edited reads (0.726; no ambiguous read): the others had a random, 'N' or low-quality window before the edit,
    # or the edit sits so near the 3' end that --m 1 takes the read.  The bounds leave a tenth of that for the sampling
    # error of 1 572 reads
    assert got[6][1] + got[6][2] >= 0.65 * edited, (got[6], edited)
    assert got[6][1] >= 0.40 * edited and got[6][2] >= 0.24 * edited and got[6][3] <= 0.01 * edited


# ---- every entry point, on case 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [7, 500])
def test_pieces_equal_one_block(P, per):
    lib, fq, run = IC.CASES["base"]()
    with P.Counter(features=lib, indel=True, miss=1, **run) as c:
        for piece in IC.pieces(fq, per):
            assert c.count_block(piece) == len(piece)
        assert tuple(result(c)) == want_base()


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf", "bgzf_device_inflate"])
def test_streamed_files_equal_the_one_block_result(P, tmp_path, monkeypatch, kind):
    lib, fq, run = IC.CASES["base"]()
    monkeypatch.setenv("F2Q_FILE_CHUNK", "4096")
    if kind == "bgzf_device_inflate":
        monkeypatch.setenv("F2Q_DEVICE_INFLATE", "1")
    path = tmp_path / {"plain": "s.fastq", "gzip": "s.fastq.gz"}.get(kind, "s.bgzf.fastq.gz")
    path.write_bytes(fq if kind == "plain" else gzip.compress(fq) if kind == "gzip" else bgzf_bytes(fq, block=3000))
    with P.Counter(features=lib, indel=True, miss=1, **run) as c:
        _, truncated = c.count_file(str(path))
        got = result(c)
    assert not truncated and tuple(got) == want_base()


def test_resident_blocks_device_text_and_host_pack(P, monkeypatch, capfd):
    lib, fq, run = IC.CASES["base"]()
    want = want_base()
    monkeypatch.setenv("F2Q_TRACE", "1")
    with P.Counter(features=lib, indel=True, miss=1, **run) as c:
        said = capfd.readouterr().err
        assert "k_count_indel" in said and "deletion-variant table" in said and " slots" in said      # F2Q_TRACE=1 names the kernel and the table's size
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
    assert tuple(counted(P, lib, fq, miss=1, **run)) == want


def test_reset_and_a_second_library_start_afresh(P):
    lib, fq, run = IC.CASES["base"]()
    fq2 = b"".join(IC.pieces(fq, 400)[1:3])
    zero = ([0] * len(lib), [0] * 5, [0] * len(lib), [0] * len(lib), [0] * IC.L, [0] * IC.L, [0] * 4)
    with P.Counter(features=lib, indel=True, miss=1, **run) as c:
        assert tuple(result(c)) == zero                                  # nothing counted yet
        assert c.count_block(fq) == len(fq)
        first = result(c)
        c.reset()
        assert tuple(result(c)) == zero
        assert c.count_block(fq2) == len(fq2)
        second = result(c)
        c.set_features(lib[:100])                                        # a new library starts afresh, with a table of its own
        again = c.read_indels()
        assert again[0].shape == (100,) and again[2].shape == (IC.L,) and not any(x.any() for x in again)
        assert c.count_block(fq) == len(fq)
        assert tuple(result(c)) == tuple(IC.expect(lib[:100], fq, miss=1, **run))
    assert tuple(first) == want_base()
    assert tuple(second) == tuple(IC.expect(lib, fq2, miss=1, **run))


def _refused(code, words, call):
    with pytest.raises(binding.F2QError) as exc:
        call()
    assert exc.value.code == code and all(w in str(exc.value) for w in words), str(exc.value)


def test_setter_before_or_after_the_library_and_cleared(P):
    lib, fq, run = IC.CASES["base"]()
    with P.Counter(indel=True, miss=1, **run) as c:                      # before the library
        assert [list(x) for x in c.read_indels()] == [[], [], [0] * IC.L, [0] * IC.L, [0] * 4]
        c.set_features(lib)
        assert c.count_block(fq) == len(fq) and tuple(result(c)) == want_base()
    with P.Counter(features=lib, miss=1, **run) as c:                    # after it, and set again
        c.set_indel(False)                                               # accepted on a plain context, changes nothing
        c.set_indel(True)
        c.set_indel(True)
        assert c.indel is True
        assert c.count_block(fq) == len(fq) and tuple(result(c)) == want_base()
        i64p = binding.C.POINTER(binding.C.c_int64)
        assert c._L.f2q_read_indels(c._h, None, None, None, None, IC.L, None) == 0      # any pointer may be NULL
        only = np.zeros(IC.L, dtype=np.int64)
        assert c._L.f2q_read_indels(c._h, None, None, None, only.ctypes.data_as(i64p), IC.L, None) == 0 and list(only) == want_base()[5]
    # 0 clears it: the context counts what a context without the call counts, on the kernels it launched before
    want = plain(P, lib, fq, miss=1, **run)
    assert tuple(want) == want_base()[:2]                                # (the flag changed no count)
    with P.Counter(features=lib, miss=1, **run) as c:
        blk = c.block_from_fastq(fq)
        before = {k: blk.info()[k] for k in ("n_reads", "n_general")}
        blk.free()
    for first in (True, False):
        with P.Counter(features=lib if first else None, indel=True, miss=1, **run) as c:
            c.set_indel(False)
            if not first:
                c.set_features(lib)
            blk = c.block_from_fastq(fq)
            assert {k: blk.info()[k] for k in before} == before and before["n_general"] < before["n_reads"]      # the packed tiles again
            c.count_resident(blk)
            counts, stats = c.read_counts()
            assert (list(counts), list(stats)) == want
            _refused(ESTATE, ["f2q_set_indel"], c.read_indels)
            blk.free()


def test_state_and_argument_refusals_in_both_orders(P, tmp_path):
    lib, fq, run = IC.CASES["base"]()
    lib = lib[:600]
    bcs = [b"ACGTACGT", b"TTGCAAGC"]
    pairs = ["ACGTACGTAC:TTGCATTGCA", "CCCCAAAATT:GGGGTTTTAA"]
    # the flag second
    with P.Counter(mode="EC", **run) as c:
        _refused(ESTATE, ["Extract+Count"], lambda: c.set_indel(True))
        c.set_indel(False)
    with P.Counter(start2="0", **run) as c:
        _refused(ESTATE, ["paired"], lambda: c.set_indel(True))
    with P.Counter(upstream="ACGTAC", downstream="TTGCAT", length=20) as c:
        _refused(ESTATE, ["--us/--ds"], lambda: c.set_indel(True))
    with P.Counter(start="0,30", length=10) as c:
        _refused(ESTATE, ["one window"], lambda: c.set_indel(True))
    for length in (1, 32):
        with P.Counter(start="2", length=length) as c:
            _refused(ESTATE, ["2 .. 31", str(length)], lambda: c.set_indel(True))
    with P.Counter(features=lib, umi=(30, 8), **run) as c:
        _refused(ESTATE, ["UMI"], lambda: c.set_indel(True))
    with P.Counter(features=lib, umi_header=("_", 8), **run) as c:
        _refused(ESTATE, ["UMI"], lambda: c.set_indel(True))
    with P.Counter(features=lib, sample_barcodes=(30, bcs), **run) as c:
        _refused(ESTATE, ["f2q_set_sample_barcodes"], lambda: c.set_indel(True))
    with P.Counter(features=lib, strand="both", **run) as c:
        _refused(ESTATE, ["f2q_set_strand"], lambda: c.set_indel(True))
    with P.Counter(features=lib, stagger=8, **run) as c:
        _refused(ESTATE, ["f2q_set_stagger"], lambda: c.set_indel(True))
    with P.Counter(features=pairs, parts=True, start="0,11", length=10) as c:
        _refused(ESTATE, [], lambda: c.set_indel(True))
    with P.Counter(features=lib, **run) as c:
        _refused(ESTATE, ["f2q_set_indel"], c.read_indels)
        assert c.count_block(fq[:4000]) > 0
        _refused(ESTATE, ["before counting"], lambda: c.set_indel(True))
        c.set_indel(False)                                               # 0 on a plain context even now
    # the flag first: the message names it
    path = tmp_path / "s.fastq"
    path.write_bytes(fq[:20000])
    with P.Counter(features=lib, indel=True, **run) as c:
        for n in (IC.L - 1, IC.L + 1, 0):
            assert c._L.f2q_read_indels(c._h, None, None, None, None, n, None) == EINVAL and "n_pos = L" in c._L.f2q_last_error(c._h).decode()
        _refused(ESTATE, ["indel"], lambda: c.set_umi(30, 8))
        _refused(ESTATE, ["indel"], lambda: c.set_umi_header("_", 8))
        _refused(ESTATE, [], lambda: c.set_umi_paired((0, 8), None))
        _refused(ESTATE, ["indel"], lambda: c.set_sample_barcodes(30, bcs))
        _refused(ESTATE, ["indel"], lambda: c.set_strand("both"))
        _refused(ESTATE, ["indel"], lambda: c.set_stagger(8))
        c.set_stagger(0)
        _refused(ESTATE, [], lambda: c.set_parts())
        _refused(ESTATE, [], lambda: c.set_mate2("0"))                   # (after f2q_set_features it is refused anyway)
        _refused(ESTATE, ["indel", "ranks"], lambda: c.count_file_shard(str(path), 0, 2))
        n, _ = c.file_pieces(str(path), 1 << 16)
        _refused(ESTATE, ["indel", "ranks"], lambda: c.count_pieces(str(path), 0, 2, 1 << 16, c.census_pieces(str(path), 0, 2, 1 << 16, n)))
        _, truncated = c.count_file_shard(str(path), 0, 1)               # one rank is a whole file
        assert not truncated and c.read_indels()[4][0] > 0
        _refused(ESTATE, ["before counting"], lambda: c.set_indel(False))  # counted: it stays an indel context
    with P.Counter(indel=True, **run) as c:                              # before the library: f2q_set_mate2, the paired UMIs and f2q_set_parts name it
        _refused(ESTATE, ["indel"], lambda: c.set_mate2("0"))
        _refused(ESTATE, ["indel"], lambda: c.set_umi_paired((0, 8), None))
    _refused(ESTATE, ["indel"], lambda: P.Counter(indel=True, umi=(30, 8), **run))
    _refused(ESTATE, ["Extract+Count"], lambda: P.Counter(mode="EC", indel=True, **run))
    _refused(ESTATE, [], lambda: P.Counter(features=pairs, parts=True, indel=True, start="0,11", length=10))


# ---- the command line ----------------------------------------------------------------------------------------------------
def _table(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


def test_cli_outputs(P, tmp_path, capsys):
    lib, base_fq, _ = IC.CASES["base"]()
    lib = lib[:600]                                                      # (the guides file holds plain 20-mers)
    samples = {"s1": b"".join(IC.pieces(base_fq, 900)[:1]), "s2": b"".join(IC.pieces(base_fq, 500)[2:3])}
    indir = tmp_path / "in"
    indir.mkdir()
    for name, fq in samples.items():
        (indir / (name + ".fastq")).write_bytes(fq)
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    outs = {}
    for tag, extra in (("indel", ["--indel"]), ("plain", [])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(out), "--st", str(IC.S), "--l", "20", "--m", "1", "--pb"] + extra)
        (outs[tag],) = [d for d in out.iterdir() if d.is_dir()]
    capsys.readouterr()
    strip = lambda t: [r[:1] + r[3:] if r and not r[0].startswith("#") else r for r in t if not (r and r[0].startswith("#cmd used"))]    # (not the running times, not the command)
    # everything that existed before is what the run without the flag writes, byte for byte
    assert (outs["indel"] / "compiled.csv").read_bytes() == (outs["plain"] / "compiled.csv").read_bytes()
    new = ["compiled_indel.csv", "compiled_indel_positions.csv"]
    assert sorted(p.name for p in outs["indel"].iterdir() if p.name not in new) == sorted(p.name for p in outs["plain"].iterdir())
    assert all((outs["indel"] / name).exists() and not (outs["plain"] / name).exists() for name in new)
    stats, plain_stats = _table(outs["indel"] / "compiled_stats.csv"), _table(outs["plain"] / "compiled_stats.csv")
    header = ["#Indel reads reported: 1"]
    at = stats.index(fast2q.INDEL_STATS_HEAD)
    assert header in stats
    assert strip([r for r in stats[:at] if r != header]) == strip(plain_stats)
    # the three new outputs, by value
    names = [f"g{i:03d}" for i in range(len(lib))]
    want = {name: IC.expect(lib, fq, miss=1, **IC.RUN) for name, fq in samples.items()}
    reads, ind, pos = _table(outs["indel"] / "compiled.csv"), _table(outs["indel"] / "compiled_indel.csv"), _table(outs["indel"] / "compiled_indel_positions.csv")
    assert ind[0] == ["#Feature", "s1:del", "s1:ins", "s2:del", "s2:ins"] and [r[0] for r in ind] == [r[0] for r in reads]
    for row in ind[1:]:
        f = names.index(row[0])
        assert [int(x) for x in row[1:]] == [want["s1"][2][f], want["s1"][3][f], want["s2"][2][f], want["s2"][3][f]]
    assert pos[0] == ["#Position", "s1:del", "s1:ins", "s2:del", "s2:ins"]
    assert [[int(x) for x in r] for r in pos[1:]] == [[p, want["s1"][4][p], want["s1"][5][p], want["s2"][4][p], want["s2"][5][p]] for p in range(20)]
    assert stats[at + 1:] == [[s] + [str(x) for x in want[s][6]] for s in ("s1", "s2")]
    for s in samples:
        IC.check_invariants(*want[s])
        assert want[s][6][1] > 50 and want[s][6][2] > 50
