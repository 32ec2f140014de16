"""--umih on the device: f2q_set_umi_header, k_header_umi at ingest and the header instances of k_count_umi /
k_count_umi_pair, through every entry point that takes FASTQ text or files, against the plain-Python expectation of
tests/umi_header_cases.py; and everything after the hook against the inline path (f2q_set_umi / f2q_set_umi_paired) on
reads that carry the same UMI in both places.  The inputs are those of tests/test_umi_header_cpu.py."""
import csv
import gzip
import importlib
import re

import pytest

import paired_cases as PC
import umi_cases as UC
import umi_header_cases as HC
import umi_pair_cases as UP
from conftest import bgzf_bytes, pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")
PAIR = dict(start=",".join(map(str, UP.ST1)), start2=",".join(map(str, UP.ST2)), length=UP.LEN, rc2=True)


@pytest.fixture(scope="module")
def P():
    return pkg()


def ctx(P, lib, umi, keep=True, miss=1, **run):
    return P.Counter(features=lib, umi_header=(chr(umi[0]), umi[1]), umi_reads=keep, miss=miss, **run)


def result(c):
    counts, stats = c.read_counts()
    umis, ok, bad = c.read_umis()
    return list(counts), list(stats), list(umis), ok, bad


def table(c):
    f, codes, reads = c.umi_pairs()
    return list(zip(f.tolist(), codes.tolist(), reads.tolist()))


def downstream(c):
    """the four outputs everything after the hook makes: f2q_read_umis, f2q_umi_collapse(1), the directional rule, the pairs"""
    umis, ok, bad = c.read_umis()
    molecules, pairs, edges = c.collapse_umis(1)
    d = c.collapse_umis_directional()
    return (list(umis), ok, bad), (list(molecules), pairs, edges), (list(d[0]),) + tuple(d[1:]), table(c)


def check(c, want):
    assert result(c) == HC.wanted(want)
    assert want.ok + want.bad == want.stats[1] + want.stats[2]
    assert table(c) == HC.table_of(want)
    molecules, pairs, edges = c.collapse_umis(1)
    assert (list(molecules), pairs, edges) == HC.cluster_of(want)


# ---- 1. the base shape through every entry point ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_want():
    lib, fq, run, umi = HC.base()
    want = HC.expect(lib, fq, umi, miss=1, **run)
    assert want.stats[0] == 4000 and want.stats[2] > 0 and want.ok > 2000 and want.bad == 0
    assert sum(len(c) for c in want.per) < want.ok - 100
    return want


def test_base_count_block(P, base_want):
    lib, fq, run, umi = HC.base()
    with ctx(P, lib, umi, **run) as c:
        assert c.umi_length == 8 and c.umi_header == ("_", 8) and c.umi is None and c.umi_paired is None
        assert c.count_block(fq) == len(fq)
        check(c, base_want)
    with ctx(P, lib, umi, keep=False, **run) as c:                   # the instance without reads per pair
        c.count_block(fq)
        assert result(c) == HC.wanted(base_want)
    with P.Counter(features=lib, miss=1, **run) as c:                # every read is decided exactly as without the call
        c.count_block(fq)
        counts, stats = c.read_counts()
        assert (list(counts), list(stats)) == (base_want.counts, base_want.stats)


def test_base_resident_block_and_device_text(P, base_want):
    lib, fq, run, umi = HC.base()
    with ctx(P, lib, umi, **run) as c:
        blk = c.block_from_fastq(fq)
        assert blk.info()["n_general"] == blk.info()["n_reads"] == 4000          # every read is a raw record
        c.count_resident(blk)
        check(c, base_want)
        c.reset()                                                    # the block carries its header UMIs: counted again
        c.count_resident(blk)
        blk.free()
        check(c, base_want)
        c.reset()
        text = c.text_upload(fq)
        assert c.count_text(text) == len(fq)
        text.free()
        check(c, base_want)


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf", "bgzf_device_inflate"])
def test_base_file_in_small_pieces(P, base_want, tmp_path, monkeypatch, kind):
    lib, fq, run, umi = HC.base()
    monkeypatch.setenv("F2Q_FILE_CHUNK", "4096")                     # ~80 pieces: the set lives across them, headers fall at their borders
    if kind == "bgzf_device_inflate":                                # (it ends in the same block_from_text_device)
        monkeypatch.setenv("F2Q_DEVICE_INFLATE", "1")
    path = tmp_path / {"plain": "s.fastq", "gzip": "s.fastq.gz"}.get(kind, "s.bgzf.fastq.gz")
    path.write_bytes(fq if kind == "plain" else gzip.compress(fq, 1) if kind == "gzip" else bgzf_bytes(fq, block=3000))
    with ctx(P, lib, umi, **run) as c:
        _, truncated = c.count_file(str(path))
        assert not truncated
        check(c, base_want)


def test_base_set_rehashes(P, base_want, monkeypatch, capfd):
    lib, fq, run, umi = HC.base()
    monkeypatch.setenv("F2Q_UMI_SLOTS", "64")
    monkeypatch.setenv("F2Q_TRACE", "1")
    lines = fq.split(b"\n")
    with ctx(P, lib, umi, **run) as c:
        for i in range(0, 16000, 4 * 445):
            piece = b"".join(x + b"\n" for x in lines[i:min(i + 4 * 445, 16000)])
            assert c.count_block(piece) == len(piece)
        check(c, base_want)
    assert len(re.findall(r"\[f2q trace\] UMI set rehash \d+:", capfd.readouterr().err)) >= 1


# ---- 2. invalid kinds ------------------------------------------------------------------------------------------------------
def test_invalid_kinds(P):
    lib, kinds = HC.invalid()
    ctxs = {}
    try:
        for kind, (fq, sep) in kinds.items():
            want = HC.expect(lib, fq, (sep, 8), miss=1, **UC.RUN)
            c = ctxs.get(sep) or ctxs.setdefault(sep, ctx(P, lib, (sep, 8), **UC.RUN))
            c.reset()
            assert c.count_block(fq) == len(fq), kind
            assert result(c) == HC.wanted(want) and table(c) == HC.table_of(want), kind
            assert (want.ok, want.bad) == ((12, 0) if HC.INVALID_KINDS[kind] else (0, 12)), kind
            assert sum(len(u) for u in want.per) == want.ok and want.stats[1] == 12, kind
    finally:
        for c in ctxs.values():
            c.close()
    assert set(ctxs) == {ord("_"), ord(":")}


# ---- 3. wave and staging edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_wave_edges(P, n):
    lib, fq, run, umi = HC.edge(n)
    want = HC.expect(lib, fq, umi, miss=1, **run)
    assert want.stats[0] == n
    with ctx(P, lib, umi, **run) as c:
        assert c.count_block(fq) == len(fq)
        check(c, want)
        c.reset()
        assert c.count_block(fq[:-1]) == len(fq) - 1                 # no final newline: the last record is complete all the same
        check(c, want)
        c.reset()
        tail = b"@r9999_ACGTACGT\n" + fq.split(b"\n")[1] + b"\n+\n"    # an incomplete record is not counted
        assert c.count_block(fq + tail) == len(fq)
        check(c, want)


@pytest.mark.parametrize("all_long", [True, False])
def test_headers_longer_than_the_staging_area(P, all_long):
    lib, fq, run, umi = HC.long_headers(all_long)
    heads = [len(h) for h, _, _ in HC.records(fq)]
    assert len(heads) == 200 and max(heads) == 420 and (min(heads) == 420) == all_long
    if all_long:                                                     # 64 records: 63 whole ones and a header, > 40 KiB
        assert 63 * (420 + 150 + 2 + 150 + 4) + 420 > 40 * 1024
    want = HC.expect(lib, fq, umi, miss=1, **run)
    assert want.ok > 100 and want.bad > 5
    with ctx(P, lib, umi, **run) as c:
        assert c.count_block(fq) == len(fq)
        check(c, want)


# ---- 4. sixteen bases ------------------------------------------------------------------------------------------------------
def test_sixteen_bases_all_t_and_all_a(P):
    lib, fq, run, umi = HC.wide16()
    want = HC.expect(lib, fq, umi, miss=1, **run)
    with ctx(P, lib, umi, **run) as c:
        assert c.umi_length == 16
        c.count_block(fq)
        check(c, want)
        got = table(c)
    assert {code for f, code, n in got} >= {0, 0xFFFFFFFF} and min(f for f, code, n in got) >= 512
    assert sum(n for f, code, n in got if code in (0, 0xFFFFFFFF)) >= 2 and want.bad == 0


# ---- 5. equivalence with the inline path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["fixed", "anchored"])
def test_equals_the_inline_path(P, shape):
    lib, fq, run, inline, header = HC.twin() if shape == "fixed" else HC.twin_anchored()
    seen = []
    for kwargs in (dict(umi=inline), dict(umi_header=(chr(header[0]), header[1]))):
        with P.Counter(features=lib, umi_reads=True, miss=1, **run, **kwargs) as c:
            assert c.count_block(fq) == len(fq)
            seen.append((result(c), downstream(c)))
    assert seen[0] == seen[1]
    (counts, stats, umis, ok, bad), (_, cluster, directional, pairs) = seen[1]
    assert ok > 500 and bad > 10
    if shape == "fixed":                                             # its pool has neighbours at distance 1: they are joined
        assert cluster[2] > 10 and sum(cluster[0]) < cluster[1]
    assert sum(directional[0]) >= sum(cluster[0]) and len(pairs) == cluster[1]
    want = HC.expect(lib, fq, header, miss=1, **run)                 # and both are the Python expectation
    assert seen[1][0] == HC.wanted(want) and pairs == HC.table_of(want) and cluster == HC.cluster_of(want)


# ---- 6. paired -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_inline(P):
    lib, fq1, fq2 = HC.twin_paired()
    with P.Counter(features=lib, umi_paired=((0, 8), None), umi_reads=True, miss=1, **PAIR) as c:
        assert c.count_block_paired(fq1, fq2) == (len(fq1), len(fq2))
        got = (result(c), downstream(c))
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, True, ((0, 8), None), miss=1)
    assert want.uncovered == 0 and got[0] == (want.counts, want.stats, UP.umis_of(want), want.ok, want.bad) and got[1][3] == UP.table_of(want)
    assert want.stats[0] == 2000 and want.ok > 1000 and got[1][1][2] > 10
    return got


def test_paired_header_of_mate_1(P, pair_inline):
    lib, fq1, fq2 = HC.twin_paired()
    h1, h2 = [h for h, _, _ in HC.records(fq1)], [h for h, _, _ in HC.records(fq2)]
    assert sum(HC.header_umi(a, HC.SEP, 8) != HC.header_umi(b, HC.SEP, 8) for a, b in zip(h1, h2)) > 1900    # R2's header says otherwise
    with P.Counter(features=lib, umi_header=("_", 8), umi_reads=True, miss=1, **PAIR) as c:
        assert c.paired and c.umi_length == 8
        assert c.count_block_paired(fq1, fq2) == (len(fq1), len(fq2))
        assert (result(c), downstream(c)) == pair_inline
        c.reset()
        blk = c.block_from_fastq_paired(fq1, fq2)
        assert blk.info()["n_general"] == blk.info()["n_reads"] == 2000
        c.count_resident(blk)
        blk.free()
        assert (result(c), downstream(c)) == pair_inline
    with P.Counter(features=lib, umi_header=("_", 8), miss=1, **PAIR) as c:         # without reads per pair
        c.count_block_paired(fq1, fq2)
        assert result(c) == pair_inline[0]


def test_paired_files(P, pair_inline, tmp_path, monkeypatch):
    lib, fq1, fq2 = HC.twin_paired()
    monkeypatch.setenv("F2Q_FILE_CHUNK", "4096")
    paths = [tmp_path / "s_R1.fastq", tmp_path / "s_R2.fastq.gz"]
    paths[0].write_bytes(fq1)
    paths[1].write_bytes(gzip.compress(fq2, 1))
    with P.Counter(features=lib, umi_header=("_", 8), umi_reads=True, miss=1, **PAIR) as c:
        _, truncated = c.count_file_paired(str(paths[0]), str(paths[1]))
        assert not truncated
        assert (result(c), downstream(c)) == pair_inline


# ---- 7. the host-pack twin -------------------------------------------------------------------------------------------------
def test_host_pack_twin(P, base_want, pair_inline, monkeypatch, tmp_path):
    monkeypatch.setenv("F2Q_HOST_PACK", "1")
    lib, fq, run, umi = HC.base()
    with ctx(P, lib, umi, **run) as c:
        assert c.count_block(fq) == len(fq)
        check(c, base_want)
        c.reset()
        blk = c.block_from_fastq(fq)
        c.count_resident(blk)
        blk.free()
        check(c, base_want)
    lib, kinds = HC.invalid()
    for sep in (ord("_"), ord(":")):
        with ctx(P, lib, (sep, 8), **UC.RUN) as c:
            for kind, (text, s) in kinds.items():
                if s == sep:
                    c.reset()
                    want = HC.expect(lib, text, (sep, 8), miss=1, **UC.RUN)
                    assert c.count_block(text) == len(text), kind
                    assert result(c) == HC.wanted(want) and table(c) == HC.table_of(want), kind
    lib, fq1, fq2 = HC.twin_paired()
    with P.Counter(features=lib, umi_header=("_", 8), umi_reads=True, miss=1, **PAIR) as c:
        assert c.count_block_paired(fq1, fq2) == (len(fq1), len(fq2))
        assert (result(c), downstream(c)) == pair_inline


# ---- 8. a context without the call launches what it launched before --------------------------------------------------------
def test_existing_launches_are_unchanged(P, monkeypatch, capfd):
    lib, fq, run, umi = UC.base()
    want = UC.expect(lib, fq, umi, miss=1, **run)
    monkeypatch.setenv("F2Q_TRACE_SYNC", "1")                        # names every counting step on stderr
    with P.Counter(features=lib, umi=umi, miss=1, **run) as c:       # the inline context: k_count_umi, nothing of the header road
        _, t = c.count_block(fq, want_timing=True)
        assert result(c) == want and t["launches"] == 1
    said = capfd.readouterr().err
    assert "k_count_umi done" in said and "header" not in said
    with P.Counter(features=lib, miss=1, **run) as c:                # a plain context: no UMI kernel at all
        c.count_block(fq)
        counts, stats = c.read_counts()
        assert (list(counts), list(stats)) == (want[0], want[1])
    said = capfd.readouterr().err
    assert "k_count_umi" not in said and "k_header_umi" not in said
    hlib, hfq, hrun, humi = HC.base()
    with ctx(P, hlib, humi, **hrun) as c:                            # the header context: its own two kernels
        _, t = c.count_block(hfq, want_timing=True)
        assert t["launches"] == 1
    said = capfd.readouterr().err
    assert "k_header_umi done" in said and "k_count_umi (header) done" in said and "k_count_umi done" not in said


# ---- 9. the ABI's errors ---------------------------------------------------------------------------------------------------
def test_abi_argument_and_state_errors(P, tmp_path):
    lib = UC.library()[:8]

    def code_of(call):
        with pytest.raises(binding.F2QError) as exc:
            call()
        return exc.value.code
    for bad in ((ord("a"), 8), (ord("Z"), 8), (ord("0"), 8), (ord("+"), 8), (32, 8), (127, 8), (0, 8), (-1, 8), (9, 8), (300, 8),
                (ord("_"), 0), (ord("_"), 17), (ord("_"), -1)):
        assert code_of(lambda: P.Counter(features=lib, umi_header=bad)) == -1, bad
    for sep in "!_:|~#.-/":
        with P.Counter(features=lib, umi_header=(sep, 16)) as c:
            assert c.umi_header == (sep, 16)
    assert code_of(lambda: P.Counter(mode="EC", umi_header=("_", 8))) == -7                                           # Extract+Count
    assert code_of(lambda: P.Counter(features=lib, umi=(20, 8), umi_header=("_", 8))) == -7                           # a UMI context already
    assert code_of(lambda: P.Counter(features=lib, umi_paired=((0, 8), None), umi_header=("_", 8), **PAIR)) == -7
    a = b"@a_ACGTACGT\n" + lib[0].encode() + b"\n+\n" + b"I" * 20 + b"\n"
    with P.Counter(features=lib, umi_header=("_", 8)) as c:
        assert code_of(lambda: c.set_umi_header("_", 8)) == -7                                                         # twice
        assert code_of(lambda: c.set_umi(0, 8)) == -7
        assert code_of(lambda: c.set_mate2("0")) == -7
        umis, ok, bad = c.read_umis()                                                                                  # nothing counted yet
        assert list(umis) == [0] * 8 and (ok, bad) == (0, 0)
        assert code_of(lambda: c.synth_create(seed=7, n_reads=100, read_len=60)) == -7                                 # no headers
        c.set_umi_reads(True)
        assert c.count_block(a) == len(a)
        assert c.read_umis()[1:] == (1, 0) and table(c) == [(0, HC.code_of(b"ACGTACGT"), 1)]
        assert code_of(lambda: c.set_umi_reads(False)) == -7                                                           # after a counting call
        path = tmp_path / "s.fastq"
        path.write_bytes(a)
        assert code_of(lambda: c.count_file_shard(str(path), 0, 2)) == -7                                              # several ranks
        n, _ = c.file_pieces(str(path), 4096)
        census = c.census_pieces(str(path), 0, 2, 4096, n)
        assert code_of(lambda: c.count_pieces(str(path), 0, 2, 4096, census)) == -7
    with P.Counter(features=lib) as c:
        blk = c.block_from_fastq(a)                                                                                    # a block made before the call
        c.set_umi_header("_", 8)
        assert code_of(lambda: c.count_resident(blk)) == -7
        blk.free()
        assert c.count_block(a) == len(a) and c.read_umis()[1:] == (1, 0)
    with P.Counter(features=lib) as c:
        c.count_block(a)
        assert code_of(lambda: c.set_umi_header("_", 8)) == -7                                                         # after a counting call
    with P.Counter(features=PC.pair_library(8, UP.LEN, 1, 1, 21), umi_header=("_", 8), **PAIR) as c:                  # paired: the single-read calls stay refused
        assert c.paired and c.umi_length == 8 and code_of(lambda: c.count_block(a)) == -7


# ---- 10. the command line --------------------------------------------------------------------------------------------------
def _table(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


def test_command_line_end_to_end(P, tmp_path, capsys):
    lib, fq, run, inline, header = HC.twin()
    lines = fq.split(b"\n")
    samples = {"s1": fq, "s2": b"".join(x + b"\n" for x in lines[4 * 1000:4 * 2500])}
    indir = tmp_path / "in"
    indir.mkdir()
    for name, text in samples.items():
        (indir / (name + ".fastq")).write_bytes(text)
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    outs = {}
    for tag, source in (("header", ["--umih", "_,8"]), ("inline", ["--umi", "20,8"])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(out), "--st", "0", "--l", "20", "--m", "1", "--pb"] + source +
                    ["--mu", "1", "--mur", "directional", "--k"])
        (outs[tag],) = [d for d in out.iterdir() if d.is_dir()]
    capsys.readouterr()
    names = {p.name for p in outs["inline"].iterdir()}
    assert names == {p.name for p in outs["header"].iterdir()}
    assert names >= {"compiled_umi.csv", "compiled_umi_collapsed.csv", "compiled_umi_directional.csv", "s1_umi_reads.csv", "s2_umi_pairs.csv"}
    source_row = {"header": ["#UMI in read header, separator, length: _,8"], "inline": ["#UMI start position in the read, length: 20,8"]}
    for path in outs["inline"].iterdir():
        other = outs["header"] / path.name
        if path.name == "compiled_stats.csv":                        # running times and the command line aside
            rows = {tag: _table(outs[tag] / path.name) for tag in outs}
            for tag in outs:
                assert rows[tag].count(source_row[tag]) == 1 and source_row["inline" if tag == "header" else "header"] not in rows[tag]
            at = rows["inline"].index(source_row["inline"])
            assert rows["header"].index(source_row["header"]) == at
            numbers = lambda t: [r[:1] + r[3:] for i, r in enumerate(t) if r and i != at and not r[0].startswith("#cmd used")]
            assert numbers(rows["header"]) == numbers(rows["inline"])
        elif path.name.endswith("_reads.csv") and not path.name.endswith("_umi_reads.csv"):      # (its first line holds the running time)
            assert _table(other)[1:] == _table(path)[1:]
        elif path.suffix == ".csv":
            assert other.read_bytes() == path.read_bytes(), path.name
    pairs = _table(outs["header"] / "s1_umi_pairs.csv")
    want = HC.expect(lib, fq, header, miss=1, **run)
    assert pairs[0] == ["#Feature", "UMI", "Reads"] and len(pairs) - 1 == sum(len(c) for c in want.per) > 500
    # the refusals leave no output directory
    base = ["-c", "--s", str(indir), "--g", str(guides), "--o", str(tmp_path / "never")]
    for extra, words in ((["--umih", "_,8", "--umi", "20,8"], ["--umih", "--umi"]), (["--umih", "_,8", "--mo", "EC"], ["--umih", "--mo EC"]),
                         (["--umih", "a,8"], ["--umih", "separator"]), (["--umih", "_,17"], ["--umih", "16"]), (["--umih", "_8"], ["--umih", "SEP,L"])):
        with pytest.raises(SystemExit):
            fast2q.main(base + extra)
        said = capsys.readouterr().out
        assert "FATAL" in said and all(w in said for w in words)
    assert not (tmp_path / "never").exists()
