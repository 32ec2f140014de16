"""GPU: from file to counts on a low-complexity sample (tests/low_complexity_cases.py): a few records make up most of the
8 MB, gzip shrinks them 240 : 1, and with a small F2Q_GZ_SYM_KB the parallel gzip decoder's speculative chunk inside that
stretch reaches its symbol cap.  Every source, every mode, paired files, a cut-off archive and the command line must give
what the oracle gives on the text."""
import csv
import gzip
import importlib

import pytest

import assign_cases as AC
import low_complexity_cases as LC
import umi_cases as UC
import umi_collapse_cases as CC
import umi_dir_cases as DC
from conftest import bgzf_bytes, pkg
from oracle import oracle as O

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")

SOURCES = ["plain", "gzip", "gzip_seq", "bgzf", "bgzf_device"]
M1 = dict(miss=1, **LC.FIXED)
ANCHORED = dict(miss=1, upstream=LC.UP, downstream=LC.DOWN)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the sample as a plain file, one gzip member (level 6) and BGZF (members of 64 KiB of text)"""
    d = tmp_path_factory.mktemp("low_complexity")
    text = LC.file_sample()[1]
    raw = gzip.compress(text, 6)
    (d / "s.fastq").write_bytes(text)
    (d / "s.fastq.gz").write_bytes(raw)
    (d / "b.fastq.gz").write_bytes(bgzf_bytes(text))
    return {"plain": str(d / "s.fastq"), "gzip": str(d / "s.fastq.gz"), "bgzf": str(d / "b.fastq.gz"), "raw": raw, "dir": d}


def oracle_of(text, mode="C", **kw):
    lib = LC.library()
    o = O.Oracle(features=[(str(i), g) for i, g in enumerate(lib)] if mode == "C" else None, mode=mode, **kw)
    o.count_fastq(text)
    out = (o.counts(), o.stats(), o.keys() if mode == "EC" else None)
    o.close()
    return out


@pytest.fixture(scope="module")
def want_m1():
    return oracle_of(LC.file_sample()[1], **M1)


def set_source(monkeypatch, source, chunk=None):
    """the environment of one road; returns the key of `files` it reads"""
    for k in ("F2Q_GZ_PAR", "F2Q_DEVICE_INFLATE", "F2Q_FILE_CHUNK", "F2Q_TRACE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in LC.GZ_ENV.items():
        monkeypatch.setenv(k, v)
    if chunk: monkeypatch.setenv("F2Q_FILE_CHUNK", chunk)
    if source == "gzip_seq": monkeypatch.setenv("F2Q_GZ_PAR", "0")
    if source == "bgzf_device": monkeypatch.setenv("F2Q_DEVICE_INFLATE", "1")
    if source.startswith("bgzf"): monkeypatch.setenv("F2Q_TRACE", "1")
    return source.split("_")[0]


def capped(capfd):
    return LC.capped_chunks(capfd.readouterr().err)


@pytest.mark.parametrize("chunk", ["65536", None])
@pytest.mark.parametrize("source", SOURCES)
def test_count_file_every_source(files, want_m1, monkeypatch, capfd, source, chunk):
    """plain, gzip through the pool (a chunk capped), gzip on one thread, BGZF inflated on the host and on the device
    (members of 64 KiB of text in a few hundred bytes): the oracle's counts and counters, every record, nothing truncated"""
    lib, text, records = LC.file_sample()
    key = set_source(monkeypatch, source, chunk)
    capfd.readouterr()
    with pkg().Counter(features=lib, **M1) as c:
        t, truncated = c.count_file(files[key])
        counts, stats = c.read_counts()
    said = capfd.readouterr().err
    assert not truncated and t["reads"] == records == want_m1[1][0]
    assert list(stats) == want_m1[1] and list(counts) == want_m1[0]
    assert (LC.capped_chunks(said) >= 1) == (source == "gzip"), said[-2000:]
    if key == "bgzf":
        assert ("(bgzf-device," in said) == (source == "bgzf_device") and ("(bgzf," in said) == (source == "bgzf"), said[-2000:]


def test_counter_anchored_on_the_capped_file(files, monkeypatch, capfd):
    lib, text, records = LC.file_sample()
    want = oracle_of(text, **ANCHORED)
    assert want[0][7] == 25000 and want[0][9] > 4000                 # the hot stretch is what the anchors find
    set_source(monkeypatch, "gzip")
    with pkg().Counter(features=lib, **ANCHORED) as c:
        t, truncated = c.count_file(files["gzip"])
        counts, stats = c.read_counts()
    assert capped(capfd) >= 1
    assert not truncated and t["reads"] == records and (list(counts), list(stats)) == want[:2]


def test_extract_count_one_hot_key_on_the_capped_file(files, monkeypatch, capfd):
    """Extract+Count: the key of feature 5 carries 25 000 of the 36 100 reads"""
    lib, text, records = LC.file_sample()
    counts, stats, keys = oracle_of(text, mode="EC", **LC.FIXED)
    assert max(counts) == 25000 and keys[counts.index(25000)] == lib[5]
    set_source(monkeypatch, "gzip")
    with pkg().Counter(mode="EC", **LC.FIXED) as c:
        t, truncated = c.count_file(files["gzip"])
        _, gstats = c.read_counts()
        rows = c.ec_results()
    assert capped(capfd) >= 1
    assert not truncated and t["reads"] == records and list(gstats) == stats
    assert [(k, n) for k, n, _ in rows] == list(zip(keys, counts))


def test_extract_count_assigned_on_the_capped_file(files, want_m1, monkeypatch, capfd):
    """--mo EC --as: the extracted keys matched against the library give what Counter mode gives on the same reads"""
    lib, text, records = LC.file_sample()
    assert AC.aggregate(lib, text, 1, **LC.FIXED) == want_m1[:2]
    set_source(monkeypatch, "gzip")
    with pkg().Counter(mode="EC", miss=1, **LC.FIXED) as c:
        c.set_assign_library(lib)
        t, truncated = c.count_file(files["gzip"])
        counts, stats = c.ec_assign()
        rows = c.ec_assigned()
    assert capped(capfd) >= 1
    assert not truncated and t["reads"] == records and (list(counts), list(stats)) == want_m1[:2]
    AC.check_rows(lib, rows, list(counts), list(stats), 1)


def test_umis_directional_on_the_capped_file(files, want_m1, monkeypatch, capfd):
    """--umi 20,8 --mu 1 --mur directional: a handful of (feature, UMI) pairs with thousands of reads each.  Feature 5:
    25 000 and 3 000 reads one base apart, one molecule under both rules; feature 40: 2 500 and 2 000 reads one base
    apart, one cluster but two directional molecules"""
    lib, text, records = LC.file_sample()
    run = dict(M1)
    base = UC.expect(lib, text, LC.UMI, **run)
    clus = CC.expect(lib, text, LC.UMI, **run)
    want = DC.expect(lib, text, LC.UMI, **run)
    assert (base[0], base[1]) == want_m1[:2]
    assert want[0][5] == clus[0][5] >= 2 and want[0][40] == clus[0][40] + 1    # (the ordinary reads add the same to both rules)
    set_source(monkeypatch, "gzip")
    with pkg().Counter(features=lib, umi=LC.UMI, umi_reads=True, **run) as c:
        t, truncated = c.count_file(files["gzip"])
        counts, stats = c.read_counts()
        umis, ok, bad = c.read_umis()
        molecules, pairs, edges = c.collapse_umis(1)
        got = c.collapse_umis_directional()
        table = c.umi_pairs()
    assert capped(capfd) >= 1
    assert not truncated and t["reads"] == records
    assert (list(counts), list(stats), list(umis), ok, bad) == base
    assert (list(molecules), pairs, edges) == clus
    assert (list(got[0]),) + tuple(got[1:]) == want
    assert list(zip(table[0].tolist(), table[1].tolist(), table[2].tolist())) == DC.pair_table(lib, text, LC.UMI, **run)


@pytest.mark.parametrize("zipped", [0, 1], ids=["R1_gzip", "R2_gzip"])
def test_paired_one_mate_capped(tmp_path, monkeypatch, capfd, zipped):
    """count_file_paired with one mate the capped gzip and the other plain: what count_block_paired gives on the texts"""
    lib, st1, st2, length, fq1, fq2, pairs = LC.paired_sample()
    kw = dict(features=lib, start=",".join(map(str, st1)), start2=",".join(map(str, st2)), rc2=True, length=length, miss=1)
    with pkg().Counter(**kw) as c:
        assert c.count_block_paired(fq1, fq2) == (len(fq1), len(fq2))
        want = tuple(list(x) for x in c.read_counts())
    assert want[1][0] == pairs and want[1][1] > 1100                 # more perfect pairs than there are ordinary ones: the runs count
    paths = []
    for k, data in enumerate((fq1, fq2)):
        p = tmp_path / (f"s_R{k + 1}.fastq" + (".gz" if k == zipped else ""))
        p.write_bytes(gzip.compress(data, 6) if k == zipped else data)
        paths.append(str(p))
    set_source(monkeypatch, "gzip")
    capfd.readouterr()
    with pkg().Counter(**kw) as c:
        t, truncated = c.count_file_paired(*paths)
        got = tuple(list(x) for x in c.read_counts())
    assert capped(capfd) >= 1
    assert not truncated and t["reads"] == pairs and got == want


def test_cut_off_archive(files, tmp_path, monkeypatch, capfd):
    """the gzip file cut at half: truncation is reported and the reads counted are the complete records zlib delivers
    before the error.  (Half of this archive lies in the ordinary reads in front of the hot stretch, where no chunk is
    capped; damage while chunks are being capped is tests/test_reader_cpu.py's.)"""
    lib, text, records = LC.file_sample()
    cut = files["raw"][: len(files["raw"]) // 2]
    readable = LC.zlib_prefix(cut)
    assert text.startswith(readable) and 0 < len(readable) < len(text)
    whole = readable.count(b"\n") // 4
    want = oracle_of(b"\n".join(readable.split(b"\n")[: 4 * whole]) + b"\n", **M1)
    assert want[1][0] == whole
    path = tmp_path / "cut.fastq.gz"
    path.write_bytes(cut)
    set_source(monkeypatch, "gzip")
    with pkg().Counter(features=lib, **M1) as c:
        t, truncated = c.count_file(str(path))
        counts, stats = c.read_counts()
    assert truncated and t["reads"] == whole and (list(counts), list(stats)) == want[:2]


def test_command_line_plain_and_gzip_columns_agree(files, want_m1, tmp_path, monkeypatch, capfd):
    """`2fast2q -c` on a directory that holds the sample plain and gzipped: two equal columns, the oracle's counts, and
    no word of an incomplete archive"""
    lib = LC.library()
    indir = tmp_path / "in"
    indir.mkdir()
    (indir / "a_plain.fastq").write_bytes(LC.file_sample()[1])
    (indir / "b_zipped.fastq.gz").write_bytes(files["raw"])
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    set_source(monkeypatch, "gzip")
    capfd.readouterr()
    fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(tmp_path), "--st", "0", "--l", "20", "--m", "1", "--pb"])
    said = capfd.readouterr()
    fast2q.close_contexts()
    assert "incomplete or corrupted" not in said.err and "incomplete or corrupted" not in said.out
    assert LC.capped_chunks(said.err) >= 1
    (out,) = [d for d in tmp_path.iterdir() if d.is_dir() and d.name.startswith("2FAST2Q_output_")]
    rows = list(csv.reader(open(out / "compiled.csv", newline="")))
    assert rows[0] == ["#Feature", "a_plain", "b_zipped"]
    assert [r[1] for r in rows[1:]] == [r[2] for r in rows[1:]]
    assert {r[0]: int(r[1]) for r in rows[1:]} == {f"g{i:03d}": n for i, n in enumerate(want_m1[0])}
