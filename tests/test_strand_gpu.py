"""--strand on the device: f2q_set_strand / k_count_strand / f2q_read_strands against the plain-Python expectation of
tests/strand_cases.py (the oracle's Counter-mode verdict on a record and on its mirror image, combined by the rule of
include/f2q.h), through every single-process counting entry point, and the command line's outputs."""
import csv
import gzip
import importlib

import numpy as np
import pytest

import strand_cases as SC
from conftest import bgzf_bytes, pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")
MODES = (SC.REV, SC.BOTH)


@pytest.fixture(scope="module")
def P():
    return pkg()


def result(c):
    counts, stats = c.read_counts()
    rev, extra = c.read_strands()
    return list(counts), list(stats), list(rev), list(extra)


def counted(P, lib, fq, mode, used=None, **run):
    with P.Counter(features=lib, strand=mode, **run) as c:
        assert c.count_block(fq) == (len(fq) if used is None else used)
        return result(c)


def plain(P, lib, fq, **run):
    with P.Counter(features=lib, **run) as c:
        c.count_block(fq)
        counts, stats = c.read_counts()
    return list(counts), list(stats)


_WANT = {}


def want_base(mode, miss=1, phred=30):
    """the base shape's expectation, computed once per (mode, --m, --ph) and shared"""
    key = (mode, miss, phred)
    if key not in _WANT:
        lib, fq, run = SC.base()
        _WANT[key] = SC.expect(lib, fq, mode, **dict(run, miss=miss, phred=phred))
    return _WANT[key]


# 1
@pytest.mark.parametrize("miss", [0, 1, 2])
@pytest.mark.parametrize("mode", [SC.FWD, SC.REV, SC.BOTH])
def test_base_shape_in_all_three_modes(P, mode, miss):
    lib, fq, run = SC.base()
    if mode == SC.FWD:                                                   # mode 0: the counts of a context without the call; f2q_read_strands refuses
        with P.Counter(features=lib, strand="fwd", miss=miss, **run) as c:
            assert c.count_block(fq) == len(fq)
            counts, stats = c.read_counts()
            with pytest.raises(binding.F2QError) as exc:
                c.read_strands()
            assert exc.value.code == ESTATE and "f2q_set_strand" in str(exc.value)
        assert (list(counts), list(stats)) == plain(P, lib, fq, miss=miss, **run) == tuple(want_base(SC.FWD, miss)[:2])
        return
    got = counted(P, lib, fq, mode, miss=miss, **run)
    assert tuple(got) == tuple(want_base(mode, miss))
    SC.check_invariants(mode, *got)
    if mode == SC.BOTH:
        assert all(b >= f for b, f in zip(got[0], want_base(SC.FWD, miss)[0]))


@pytest.mark.parametrize("phred", [1, 41])
@pytest.mark.parametrize("mode", MODES)
def test_base_shape_phred(P, mode, phred):
    lib, fq, run = SC.base()
    assert tuple(counted(P, lib, fq, mode, **dict(run, miss=1, phred=phred))) == tuple(want_base(mode, 1, phred))


# 2 .. 6, and the pool of 7 counted once
@pytest.mark.parametrize("name", sorted(n for n in SC.CASES if n != "base"))
@pytest.mark.parametrize("mode", MODES)
def test_cases_vs_expectation(P, name, mode):
    lib, fq, run = SC.CASES[name]()
    used = SC.RE.oracle_of(lib, fq, **run)[2]
    got = counted(P, lib, fq, mode, used=used, **run)
    assert tuple(got) == tuple(SC.expect(lib, fq, mode, **run))
    SC.check_invariants(mode, *got)


# 7
@pytest.mark.parametrize("mode", MODES)
def test_second_pass(P, mode):
    import subprocess
    import sys
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                           capture_output=True, text=True, check=True)
    fq, reps = SC.second_pass(int(probe.stdout.split()[-1]))
    lib = SC.library()
    want = SC.scaled(SC.expect(lib, SC.pass_pool(), mode, **SC.PASS_RUN), reps)
    with P.Counter(features=lib, strand=mode, **SC.PASS_RUN) as c:
        blk = c.block_from_fastq(fq)
        assert blk.info()["n_reads"] == reps * SC.POOL
        for _ in range(2):                                               # (and the launch repeated on the resident block)
            c.reset()
            c.count_resident(blk)
            assert tuple(result(c)) == tuple(want)
        blk.free()


# 8
def test_no_oracle_two_hundred_thousand_reads(P):
    guides = binding.synth_library(0x57A4D, 500, 20)
    with P.Counter(features=guides, miss=1, phred=30, length=20, start="0") as c:
        fq = bytes(c.synth_fastq(seed=11, n_reads=200000, read_len=60))
        c.count_block(fq)
        fwd = [list(x) for x in c.read_counts()]
        mirrored = SC.mirror_text(fq)
        c.reset()
        c.count_block(mirrored)
        on_mirrored = [list(x) for x in c.read_counts()]
    mixed = SC.mirror_text(fq, lambda i: i % 2 == 1)
    with P.Counter(features=guides, strand="rev", miss=1, phred=30, length=20, start="0") as c:
        c.count_block(fq)
        got = result(c)
        assert list(got[:2]) == on_mirrored                                  # rev on the text == a plain context on the mirrored text
        SC.check_invariants(SC.REV, *got)
        c.reset()
        c.count_block(mirrored)
        assert list(result(c)[:2]) == fwd
    with P.Counter(features=guides, strand="both", miss=1, phred=30, length=20, start="0") as c:
        c.count_block(mixed)
        got = result(c)
        SC.check_invariants(SC.BOTH, *got)
        assert got[1][0] == 200000 and got[3][1] + got[3][2] > 60000 and got[3][0] > 60000
        assert sum(got[0]) >= sum(fwd[0])                                # a read the plain text assigns is assigned on one strand or the other


# ---- every entry point, on case 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [7, 500])
@pytest.mark.parametrize("mode", MODES)
def test_pieces_equal_one_block(P, mode, per):
    lib, fq, run = SC.base()
    with P.Counter(features=lib, strand=mode, miss=1, **run) as c:
        for piece in SC.pieces(fq, per):
            assert c.count_block(piece) == len(piece)
        assert tuple(result(c)) == tuple(want_base(mode))


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf", "bgzf_device_inflate"])
@pytest.mark.parametrize("mode", MODES)
def test_streamed_files_equal_the_one_block_result(P, tmp_path, monkeypatch, mode, kind):
    lib, fq, run = SC.base()
    monkeypatch.setenv("F2Q_FILE_CHUNK", "4096")
    if kind == "bgzf_device_inflate":
        monkeypatch.setenv("F2Q_DEVICE_INFLATE", "1")
    path = tmp_path / {"plain": "s.fastq", "gzip": "s.fastq.gz"}.get(kind, "s.bgzf.fastq.gz")
    path.write_bytes(fq if kind == "plain" else gzip.compress(fq) if kind == "gzip" else bgzf_bytes(fq, block=3000))
    with P.Counter(features=lib, strand=mode, miss=1, **run) as c:
        _, truncated = c.count_file(str(path))
        got = result(c)
    assert not truncated and tuple(got) == tuple(want_base(mode))


@pytest.mark.parametrize("mode", MODES)
def test_resident_blocks_device_text_and_host_pack(P, monkeypatch, capfd, mode):
    lib, fq, run = SC.base()
    want = tuple(want_base(mode))
    monkeypatch.setenv("F2Q_TRACE", "1")
    with P.Counter(features=lib, strand=mode, miss=1, **run) as c:
        assert f"k_count_strand<{'true' if mode == SC.BOTH else 'false'}>" in capfd.readouterr().err      # F2Q_TRACE=1 names the kernel
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
    assert tuple(counted(P, lib, fq, mode, miss=1, **run)) == want


def test_reset_and_a_second_library_start_afresh(P):
    lib, fq, run = SC.base()
    fq2 = SC.mirror_text(fq, lambda i: i % 3 == 0)
    zero = ([0] * len(lib), [0] * 5, [0] * len(lib), [0] * 4)
    with P.Counter(features=lib, strand="both", miss=1, **run) as c:
        assert tuple(result(c)) == zero                                  # nothing counted yet
        assert c.count_block(fq) == len(fq)
        first = result(c)
        c.reset()
        assert tuple(result(c)) == zero
        assert c.count_block(fq2) == len(fq2)
        second = result(c)
        c.set_features(lib[:100])                                        # a new library starts afresh
        rev, extra = c.read_strands()
        assert rev.shape == (100,) and not rev.any() and not extra.any()
        assert c.count_block(fq) == len(fq)
        assert tuple(result(c)) == tuple(SC.expect(lib[:100], fq, SC.BOTH, miss=1, **run))
    assert tuple(first) == tuple(want_base(SC.BOTH))
    assert tuple(second) == tuple(SC.expect(lib, fq2, SC.BOTH, miss=1, **run))


def test_mode_before_or_after_the_library(P):
    lib, fq, run = SC.base()
    with P.Counter(strand="both", miss=1, **run) as c:
        rev, extra = c.read_strands()
        assert rev.shape == (0,) and list(extra) == [0] * 4
        c.set_features(lib)
        assert c.count_block(fq) == len(fq) and tuple(result(c)) == tuple(want_base(SC.BOTH))
    with P.Counter(features=lib, miss=1, **run) as c:
        c.set_strand("fwd")                                              # accepted, changes nothing
        c.set_strand("rev")
        assert c.strand == "rev"
        assert c.count_block(fq) == len(fq) and tuple(result(c)) == tuple(want_base(SC.REV))
        rev, extra = c.read_strands()
        i64p = binding.C.POINTER(binding.C.c_int64)
        assert c._L.f2q_read_strands(c._h, None, None) == 0              # either pointer may be NULL
        only = np.zeros(4, dtype=np.int64)
        assert c._L.f2q_read_strands(c._h, None, only.ctypes.data_as(i64p)) == 0 and list(only) == list(extra)
        c.set_strand("fwd")                                              # mode 0 stays accepted, and the context stays what it is
        assert c.strand == "rev" and list(c.read_strands()[1]) == list(extra)


ESTATE, EINVAL = -7, -1


def _refused(code, words, call):
    with pytest.raises(binding.F2QError) as exc:
        call()
    assert exc.value.code == code and all(w in str(exc.value) for w in words), str(exc.value)


def test_state_and_argument_refusals_in_both_orders(P, tmp_path):
    lib, fq, run = SC.base()
    bcs = [b"ACGTACGT", b"TTGCAAGC"]
    # the strand mode second
    with P.Counter(mode="EC", **run) as c:
        _refused(ESTATE, ["Extract+Count"], lambda: c.set_strand("rev"))
        c.set_strand("fwd")
    with P.Counter(start2="0", **run) as c:
        _refused(ESTATE, ["paired"], lambda: c.set_strand("both"))
    with P.Counter(features=lib, umi=(30, 8), **run) as c:
        _refused(ESTATE, ["UMI"], lambda: c.set_strand("both"))
    with P.Counter(features=lib, umi_header=("_", 8), **run) as c:
        _refused(ESTATE, ["UMI"], lambda: c.set_strand("rev"))
    with P.Counter(features=lib, start2="0", umi_paired=((0, 8), None), **run) as c:
        _refused(ESTATE, [], lambda: c.set_strand("rev"))
    with P.Counter(features=lib, sample_barcodes=(20, bcs), **run) as c:
        _refused(ESTATE, ["f2q_set_sample_barcodes"], lambda: c.set_strand("both"))
    with P.Counter(features=lib, **run) as c:
        for mode in (3, -1, 17):
            assert c._L.f2q_set_strand(c._h, mode) == EINVAL and str(mode) in c._L.f2q_last_error(c._h).decode()
        with pytest.raises(ValueError):
            c.set_strand("sideways")
        _refused(ESTATE, ["f2q_set_strand"], c.read_strands)
        assert c.count_block(fq[:4000]) > 0
        _refused(ESTATE, ["before counting"], lambda: c.set_strand("both"))
        c.set_strand("fwd")                                              # mode 0 even now
    # the strand mode first: the message names it
    path = tmp_path / "s.fastq"
    path.write_bytes(fq[:20000])
    with P.Counter(features=lib, strand="both", **run) as c:
        _refused(ESTATE, ["once"], lambda: c.set_strand("rev"))
        _refused(ESTATE, ["once"], lambda: c.set_strand("both"))
        _refused(ESTATE, ["strand mode"], lambda: c.set_umi(30, 8))
        _refused(ESTATE, ["strand mode"], lambda: c.set_umi_header("_", 8))
        _refused(ESTATE, [], lambda: c.set_umi_paired((0, 8), None))
        _refused(ESTATE, ["strand mode"], lambda: c.set_sample_barcodes(20, bcs))
        _refused(ESTATE, [], lambda: c.set_mate2("0"))                   # (after f2q_set_features it is refused anyway)
        _refused(ESTATE, ["strand mode", "ranks"], lambda: c.count_file_shard(str(path), 0, 2))
        n, _ = c.file_pieces(str(path), 1 << 16)
        _refused(ESTATE, ["strand mode", "ranks"], lambda: c.count_pieces(str(path), 0, 2, 1 << 16, c.census_pieces(str(path), 0, 2, 1 << 16, n)))
        _, truncated = c.count_file_shard(str(path), 0, 1)               # one rank is a whole file
        assert not truncated and c.read_strands()[1][3] > 0
    with P.Counter(strand="rev", **run) as c:                            # before the library: f2q_set_mate2 and the paired UMIs name the mode
        _refused(ESTATE, ["strand mode"], lambda: c.set_mate2("0"))
        _refused(ESTATE, ["strand mode"], lambda: c.set_umi_paired((0, 8), None))
    _refused(ESTATE, ["strand mode"], lambda: P.Counter(strand="rev", umi=(30, 8), **run))
    _refused(ESTATE, ["Extract+Count"], lambda: P.Counter(mode="EC", strand="rev", **run))


# ---- the command line ----------------------------------------------------------------------------------------------------
def _table(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


def test_cli_outputs(P, tmp_path, capsys):
    lib = SC.library()
    base_fq = SC.base()[1]
    samples = {"s1": b"".join(SC.pieces(base_fq, 1200)[:1]), "s2": b"".join(SC.pieces(base_fq, 800)[2:3])}
    indir = tmp_path / "in"
    indir.mkdir()
    for name, fq in samples.items():
        (indir / (name + ".fastq")).write_bytes(fq)
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    outs = {}
    for tag, extra in (("both", ["--strand", "both"]), ("rev", ["--strand", "rev"]), ("fwd", ["--strand", "fwd"]), ("plain", [])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(out), "--st", "0", "--l", "20", "--m", "1", "--pb"] + extra)
        (outs[tag],) = [d for d in out.iterdir() if d.is_dir()]
    capsys.readouterr()
    strip = lambda t: [r[:1] + r[3:] if r and not r[0].startswith("#") else r for r in t if not (r and r[0].startswith("#cmd used"))]    # (not the running times, not the command)
    # --strand fwd is a run without the flag, byte for byte (but for the command line and the running times the files quote)
    assert (outs["fwd"] / "compiled.csv").read_bytes() == (outs["plain"] / "compiled.csv").read_bytes()
    assert sorted(p.name for p in outs["fwd"].iterdir()) == sorted(p.name for p in outs["plain"].iterdir())
    assert strip(_table(outs["fwd"] / "compiled_stats.csv")) == strip(_table(outs["plain"] / "compiled_stats.csv"))
    assert not (outs["plain"] / "compiled_strand.csv").exists() and not (outs["fwd"] / "compiled_strand.csv").exists()
    names = [f"g{i:03d}" for i in range(len(lib))]
    for mode in ("both", "rev"):
        assert sorted(p.name for p in outs[mode].iterdir() if p.suffix == ".csv") == ["compiled.csv", "compiled_stats.csv", "compiled_strand.csv"]
        want = {name: SC.expect(lib, fq, mode, miss=1, **SC.RUN) for name, fq in samples.items()}
        reads, strand = _table(outs[mode] / "compiled.csv"), _table(outs[mode] / "compiled_strand.csv")
        assert reads[0] == ["#Feature", "s1", "s2"] and [r[0] for r in strand] == [r[0] for r in reads]
        assert strand[0] == ["#Feature", "s1:fwd", "s1:rev", "s2:fwd", "s2:rev"]
        for row, rrow in zip(strand[1:], reads[1:]):
            f = names.index(row[0])
            for k, s in enumerate(("s1", "s2")):
                fwd, rev = int(row[1 + 2 * k]), int(row[2 + 2 * k])
                assert int(rrow[1 + k]) == want[s][0][f] == fwd + rev and rev == want[s][2][f]
        stats, plain_stats = _table(outs[mode] / "compiled_stats.csv"), _table(outs["plain"] / "compiled_stats.csv")
        header = [f"#Strand: {mode}"]
        at = stats.index(fast2q.STRAND_STATS_HEAD)
        assert header in stats
        assert [r[0] for r in strip([r for r in stats[:at] if r != header])] == [r[0] for r in strip(plain_stats)]
        assert stats[at + 1:] == [[s] + [str(n) for n in want[s][3]] for s in ("s1", "s2")]
        # the counters of the run's own table are the rule's
        rows = {r[0]: r for r in stats[:at] if r and r[0] in samples}
        for s in samples:
            assert [int(x) for x in rows[s][3:]] == [want[s][1][0], want[s][1][1] + want[s][1][2], want[s][1][1], want[s][1][2], want[s][1][3], want[s][1][4]]
