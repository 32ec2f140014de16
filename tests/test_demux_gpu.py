"""--sb on the device: f2q_set_sample_barcodes / k_count_demux / f2q_read_demux against the plain-Python expectation of
tests/demux_cases.py (the oracle's Counter-mode verdict per read, the barcode rule, additive counters), through every
single-process counting entry point, and the command line's outputs."""
import csv
import gzip
import importlib

import pytest

import demux_cases as DC
from conftest import bgzf_bytes, pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")


@pytest.fixture(scope="module")
def P():
    return pkg()


def result(c):
    counts, stats = c.read_counts()
    matrix, sstats, verdicts = c.read_demux()
    return list(counts), list(stats), matrix.tolist(), sstats.tolist(), list(verdicts)


def counted(P, lib, fq, bcs, at, miss_bc, **run):
    with P.Counter(features=lib, sample_barcodes=(at, bcs), barcode_mismatch=miss_bc, **run) as c:
        assert c.count_block(fq) == len(fq)
        return result(c)


def plain(P, lib, fq, **run):
    with P.Counter(features=lib, **run) as c:
        assert c.count_block(fq) == len(fq)
        counts, stats = c.read_counts()
    return list(counts), list(stats)


_WANT = {}


def want_base(miss_bc, miss):
    """the base shape's expectation, computed once per (M, --m) and shared"""
    key = (miss_bc, miss)
    if key not in _WANT:
        lib, fq, run, bcs, at = DC.base()
        _WANT[key] = DC.expect(lib, fq, bcs, at, miss_bc, miss=miss, **run)
    return _WANT[key]


# 1
@pytest.mark.parametrize("miss", [0, 1])
@pytest.mark.parametrize("miss_bc", [0, 1])
def test_parity_with_the_expectation_and_with_a_plain_context(P, miss_bc, miss):
    lib, fq, run, bcs, at = DC.base()
    got = counted(P, lib, fq, bcs, at, miss_bc, miss=miss, **run)
    assert got == tuple(want_base(miss_bc, miss))
    assert tuple(got[:2]) == plain(P, lib, fq, miss=miss, **run)
    DC.check_invariants(*got)


# 2
@pytest.mark.parametrize("miss_bc", [0, 1])
def test_both_table_placements_give_the_same(P, monkeypatch, capfd, miss_bc):
    lib, fq, run, bcs, at = DC.base()
    monkeypatch.setenv("F2Q_TRACE", "1")
    said = {}
    for where in ("lds", "global"):
        monkeypatch.setenv("F2Q_DEMUX_TABLE", where)
        assert counted(P, lib, fq, bcs, at, miss_bc, miss=1, **run) == tuple(want_base(miss_bc, 1)), where
        said[where] = capfd.readouterr().err
    # 12 barcodes of 8 bases: 12 entries (32 slots) or 12 * 25 - 4 = at most 300 (1024 slots) -- both fit the 32 KiB of the LDS instance
    assert "sample barcodes: 12 of 8 bases at 20" in said["lds"] and ", LDS" in said["lds"] and ", global" in said["global"]


def test_a_table_too_large_for_lds_is_read_from_global_memory(P, monkeypatch, capfd):
    bcs, at, fq = DC.shapes()["nb1024"]
    lib = DC.library()
    monkeypatch.setenv("F2Q_TRACE", "1")
    monkeypatch.setenv("F2Q_DEMUX_TABLE", "lds")
    got = counted(P, lib, fq, bcs, at, 1, miss=1, **DC.RUN)
    assert ", global" in capfd.readouterr().err
    assert got == tuple(DC.expect(lib, fq, bcs, at, 1, miss=1, **DC.RUN))


# 3
@pytest.mark.parametrize("shape", ["l16", "l1", "l1_three", "nb1", "nb1024"])
def test_table_edges(P, shape):
    bcs, at, fq = DC.shapes()[shape]
    lib = DC.library()
    for miss_bc in (0, 1):
        got = counted(P, lib, fq, bcs, at, miss_bc, miss=1, **DC.RUN)
        assert got == tuple(DC.expect(lib, fq, bcs, at, miss_bc, miss=1, **DC.RUN)), miss_bc
        DC.check_invariants(*got)


# 4, 5
@pytest.mark.parametrize("case", ["long_reads", "anchored"])
def test_long_reads_and_anchored_runs(P, case):
    lib, fq, run, bcs, at = getattr(DC, case)()
    want = DC.expect(lib, fq, bcs, at, 1, miss=1, **run)
    got = counted(P, lib, fq, bcs, at, 1, miss=1, **run)
    assert got == tuple(want)
    assert tuple(got[:2]) == plain(P, lib, fq, miss=1, **run)
    assert want[4][DC.UNREADABLE] > 10 and want[4][DC.ONE_MISMATCH] > 10


# 6
def test_pieces_of_thirty_records_equal_one_block(P):
    lib, fq, run, bcs, at = DC.base()
    with P.Counter(features=lib, sample_barcodes=(at, bcs), barcode_mismatch=1, miss=1, **run) as c:
        for piece in DC.pieces(fq, 30):
            assert c.count_block(piece) == len(piece)
        assert result(c) == tuple(want_base(1, 1))


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf", "bgzf_device_inflate"])
def test_streamed_files_equal_the_one_block_result(P, tmp_path, monkeypatch, kind):
    lib, fq, run, bcs, at = DC.base()
    monkeypatch.setenv("F2Q_FILE_CHUNK", "4096")
    if kind == "bgzf_device_inflate":
        monkeypatch.setenv("F2Q_DEVICE_INFLATE", "1")
    path = tmp_path / {"plain": "s.fastq", "gzip": "s.fastq.gz"}.get(kind, "s.bgzf.fastq.gz")
    path.write_bytes(fq if kind == "plain" else gzip.compress(fq) if kind == "gzip" else bgzf_bytes(fq, block=3000))
    with P.Counter(features=lib, sample_barcodes=(at, bcs), barcode_mismatch=1, miss=1, **run) as c:
        _, truncated = c.count_file(str(path))
        got = result(c)
    assert not truncated and got == tuple(want_base(1, 1))


def test_resident_blocks_device_text_and_host_pack(P, monkeypatch):
    lib, fq, run, bcs, at = DC.base()
    want = tuple(want_base(1, 1))
    with P.Counter(features=lib, sample_barcodes=(at, bcs), barcode_mismatch=1, miss=1, **run) as c:
        blk = c.block_from_fastq(fq)
        assert blk.info()["n_general"] == blk.info()["n_reads"] == want[1][0]      # every read takes the raw-record road
        t = c.count_resident(blk)
        assert t["general_reads"] == want[1][0] and result(c) == want
        c.reset()
        c.count_resident_queued(blk)
        c.queued_times()
        assert result(c) == want
        blk.free()
        c.reset()
        text = c.text_upload(fq)
        assert c.count_text(text) == len(fq) and result(c) == want
        text.free()
    monkeypatch.setenv("F2Q_HOST_PACK", "1")
    assert counted(P, lib, fq, bcs, at, 1, miss=1, **run) == want


# 7
def test_reset_and_reuse_match_fresh_contexts(P):
    lib, fq, run, bcs, at = DC.base()
    fq2, _ = DC.sample(0x5EC0, n_reads=1000)
    nb = len(bcs)
    with P.Counter(features=lib, sample_barcodes=(at, bcs), barcode_mismatch=1, miss=1, **run) as c:
        assert result(c) == ([0] * len(lib), [0] * 5, [[0] * len(lib)] * (nb + 1), [[0] * 5] * (nb + 1), [0] * 5)      # nothing counted yet
        assert c.count_block(fq) == len(fq)
        first = result(c)
        c.reset()
        assert result(c) == ([0] * len(lib), [0] * 5, [[0] * len(lib)] * (nb + 1), [[0] * 5] * (nb + 1), [0] * 5)
        assert c.count_block(fq2) == len(fq2)
        second = result(c)
        c.set_features(lib[:100])                                                    # a new library starts a new matrix
        assert c.read_demux()[0].shape == (nb + 1, 100) and not c.read_demux()[0].any()
    assert first == tuple(want_base(1, 1))
    assert second == counted(P, lib, fq2, bcs, at, 1, miss=1, **run) == tuple(DC.expect(lib, fq2, bcs, at, 1, miss=1, **run))


def test_barcodes_before_or_after_the_library(P):
    lib, fq, run, bcs, at = DC.base()
    with P.Counter(sample_barcodes=(at, bcs), barcode_mismatch=1, miss=1, **run) as c:
        assert c.read_demux()[0].shape == (len(bcs) + 1, 0)
        c.set_features(lib)
        assert c.count_block(fq) == len(fq) and result(c) == tuple(want_base(1, 1))
    with P.Counter(features=lib, miss=1, **run) as c:
        c.set_sample_barcodes(at, [b.lower() for b in bcs], 1)                       # upper-cased on the way in
        assert c.count_block(fq) == len(fq) and result(c) == tuple(want_base(1, 1))
        matrix, sstats, verdicts = c.read_demux()
        i64p = binding.C.POINTER(binding.C.c_int64)
        assert c._L.f2q_read_demux(c._h, None, None, None) == 0                      # any pointer may be NULL
        only = binding.np.zeros(5, dtype=binding.np.int64)
        assert c._L.f2q_read_demux(c._h, None, None, only.ctypes.data_as(i64p)) == 0 and list(only) == list(verdicts)


ESTATE, EINVAL = -7, -1


def _refused(code, words, call):
    with pytest.raises(binding.F2QError) as exc:
        call()
    assert exc.value.code == code and all(w in str(exc.value) for w in words), str(exc.value)


def test_state_refusals(P, tmp_path):
    lib, fq, run, bcs, at = DC.base()
    sb = dict(sample_barcodes=(at, bcs))
    _refused(ESTATE, ["Extract+Count"], lambda: P.Counter(mode="EC", **sb, **run))
    _refused(ESTATE, ["single reads"], lambda: P.Counter(start2="0", **sb, **run))
    with P.Counter(start2="0", **run) as c:
        _refused(ESTATE, ["paired"], lambda: c.set_sample_barcodes(at, bcs))
    _refused(ESTATE, ["UMI"], lambda: P.Counter(umi=(30, 8), **sb, **run))
    with P.Counter(features=lib, start2="0", umi_paired=((0, 8), None), **run) as c:
        _refused(ESTATE, [], lambda: c.set_sample_barcodes(at, bcs))
    with P.Counter(features=lib, umi_header=("_", 8), **run) as c:
        _refused(ESTATE, ["UMI"], lambda: c.set_sample_barcodes(at, bcs))
    with P.Counter(features=lib, **run) as c:
        _refused(ESTATE, ["f2q_set_sample_barcodes first"], c.read_demux)
        assert c.count_block(fq[:4000]) > 0
        _refused(ESTATE, ["before counting"], lambda: c.set_sample_barcodes(at, bcs))
    path = tmp_path / "s.fastq"
    path.write_bytes(fq[:20000])
    with P.Counter(features=lib, **sb, **run) as c:
        _refused(ESTATE, ["once"], lambda: c.set_sample_barcodes(at, bcs))
        _refused(ESTATE, ["UMI"], lambda: c.set_umi(30, 8))
        _refused(ESTATE, ["UMI"], lambda: c.set_umi_header("_", 8))
        _refused(ESTATE, ["UMI"], lambda: c.set_umi_paired((0, 8), None))
        _refused(ESTATE, [], lambda: c.set_mate2("0"))                               # (after f2q_set_features it is refused anyway)
        _refused(ESTATE, ["ranks"], lambda: c.count_file_shard(str(path), 0, 2))
        n, _ = c.file_pieces(str(path), 1 << 16)
        _refused(ESTATE, ["ranks"], lambda: c.count_pieces(str(path), 0, 2, 1 << 16, c.census_pieces(str(path), 0, 2, 1 << 16, n)))
        _, truncated = c.count_file_shard(str(path), 0, 1)                           # one rank is a whole file
        assert not truncated and c.read_demux()[2].sum() == c.read_counts()[1][0] > 0


def test_argument_refusals_name_the_barcode(P):
    lib, fq, run, bcs, at = DC.base()
    with P.Counter(features=lib, **run) as c:
        L, h = c._L, c._h
        for args, words in (((b"ACGT", 0, 4, 0, 0), ["between 1 and 1024"]), ((b"A" * 1025, 1025, 1, 0, 0), ["between 1 and 1024"]),
                            ((b"", 1, 0, 0, 0), ["1 .. 16"]), ((b"A" * 17, 1, 17, 0, 0), ["1 .. 16"]), ((b"ACGT", 1, 4, -1, 0), [">= 0"]),
                            ((b"ACGT", 1, 4, 0, 2), ["0 or 1"]), ((b"ACGTACNT", 2, 4, 0, 0), ["barcode 1", "ACNT"]),
                            ((b"ACGTTTTTacgt", 3, 4, 0, 0), ["barcode 2", "repeats barcode 0"])):
            assert L.f2q_set_sample_barcodes(h, *args) == EINVAL
            assert all(w in L.f2q_last_error(h).decode() for w in words), (args, L.f2q_last_error(h))
        with pytest.raises(ValueError):
            c.set_sample_barcodes(0, [b"ACGT", b"ACG"])
        c.set_sample_barcodes(at, bcs)                                               # the refusals left the context as it was
        assert c.count_block(fq) == len(fq) and result(c) == tuple(want_base(0, 1))
    with pytest.raises(ValueError):
        P.Counter(features=lib, barcode_mismatch=1, **run)


# 8 ---- the command line ----------------------------------------------------------------------------------------------
def _table(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


def test_cli_outputs(P, tmp_path, capsys):
    lib, bcs = DC.library(), DC.barcodes()
    samples = {"s1": DC.sample(0x51, n_reads=1200)[0], "s2": DC.sample(0x52, n_reads=800)[0]}
    indir = tmp_path / "in"
    indir.mkdir()
    for name, fq in samples.items():
        (indir / (name + ".fastq")).write_bytes(fq)
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    bnames = [f"bc{i:02d}" for i in range(len(bcs))]
    sb = tmp_path / "samples.csv"
    sb.write_text("".join(f"{n},{b.decode()}\n" for n, b in zip(bnames, bcs)))
    outs = {}
    for tag, extra in (("sb", ["--sb", str(sb), "--sbs", "20", "--sbm", "1"]), ("plain", [])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(out), "--st", "0", "--l", "20", "--m", "1", "--pb"] + extra)
        (outs[tag],) = [d for d in out.iterdir() if d.is_dir()]
    capsys.readouterr()
    # what the run wrote before stays as it was
    assert (outs["sb"] / "compiled.csv").read_bytes() == (outs["plain"] / "compiled.csv").read_bytes()
    assert not (outs["plain"] / "compiled_demux.csv").exists()
    assert sorted(p.name for p in outs["sb"].iterdir() if p.suffix == ".csv") == ["compiled.csv", "compiled_demux.csv", "compiled_stats.csv"]
    stats, plain_stats = _table(outs["sb"] / "compiled_stats.csv"), _table(outs["plain"] / "compiled_stats.csv")
    header = ["#Sample barcodes, start, length, mismatches: 20,8,1"]
    at_v, at_s = stats.index(fast2q.DEMUX_VERDICT_STATS_HEAD), stats.index(fast2q.DEMUX_SAMPLE_STATS_HEAD)
    strip = lambda t: [r[:1] + r[3:] if r and not r[0].startswith("#") else r for r in t if not (r and r[0].startswith("#cmd used"))]    # (not the running times, not the command)
    assert header in stats and strip([r for r in stats[:at_v] if r != header]) == strip(plain_stats)
    # the demultiplexed table: <name>.csv's layout and row order, a column per barcode in CSV order and the unassigned reads, per file
    reads, demux = _table(outs["sb"] / "compiled.csv"), _table(outs["sb"] / "compiled_demux.csv")
    assert reads[0] == ["#Feature", "s1", "s2"] and [r[0] for r in demux] == [r[0] for r in reads]
    assert demux[0] == ["#Feature"] + [f"{s}:{b}" for s in ("s1", "s2") for b in bnames + ["unassigned"]]
    want = {name: DC.expect(lib, fq, bcs, 20, 1, miss=1, **DC.RUN) for name, fq in samples.items()}
    names = [f"g{i:03d}" for i in range(len(lib))]
    per = len(bcs) + 1
    for row, rrow in zip(demux[1:], reads[1:]):
        f = names.index(row[0])
        for k, s in enumerate(("s1", "s2")):
            cols = [int(x) for x in row[1 + k * per:1 + (k + 1) * per]]
            assert cols == [want[s][2][b][f] for b in range(per)] and sum(cols) == int(rrow[1 + k])
    # both blocks of <name>_stats.csv
    assert stats[at_v + 1:at_s] == [[s] + [str(n) for n in want[s][4]] for s in ("s1", "s2")]
    assert stats[at_s + 1:] == [[f"{s}:{b}"] + [str(n) for n in (r[0], r[1] + r[2], r[1], r[2], r[3], r[4])]
                                for s in ("s1", "s2") for b, r in zip(bnames + ["unassigned"], want[s][3])]
