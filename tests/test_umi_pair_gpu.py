"""--umi1 / --umi2 with --pe on the device: f2q_set_umi_paired / k_count_umi_pair (both layouts of F2Q_UMI_PAIR_STAGE) and
everything downstream of the (feature, UMI) set, against the yardstick of tests/umi_pair_cases.py: the oracle's verdict on
every pair's merged record, the UMI from the two original mates, the collapse rules as tests/umi_collapse_cases.py and
tests/umi_dir_cases.py state them.  The inputs are those of tests/test_umi_pair_cpu.py."""
import csv
import gzip
import importlib
import re

import pytest

import paired_cases as PC
import umi_collapse_cases as CC
import umi_pair_cases as UP
from conftest import pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")
START = dict(start=",".join(map(str, UP.ST1)), start2=",".join(map(str, UP.ST2)), length=UP.LEN)
STAGE_WORDS = 48                               # F2Q_GEN_WORDS: the default layout stages nothing wider
PAIR_STAGE_WORDS = 76                          # F2Q_UMI_PAIR_WORDS: the staged layout's area (F2Q_UMI_PAIR_STAGE=1)


@pytest.fixture(scope="module")
def P():
    return pkg()


def ctx(P, lib, parts, rc2, keep=True, miss=1, phred=30):
    return P.Counter(features=lib, rc2=rc2, umi_paired=parts, umi_reads=keep, miss=miss, phred=phred, **START)


def result(c):
    counts, stats = c.read_counts()
    umis, ok, bad = c.read_umis()
    return list(counts), list(stats), list(umis), ok, bad


def table(c):
    f, codes, reads = c.umi_pairs()
    return list(zip(f.tolist(), codes.tolist(), reads.tolist()))


def wanted(e):
    return (e.counts, e.stats, UP.umis_of(e), e.ok, e.bad)


def cluster(c):
    molecules, pairs, edges = c.collapse_umis(1)
    return list(molecules), pairs, edges


def directional(c):
    got = c.collapse_umis_directional()
    return (list(got[0]),) + tuple(got[1:])


def check_all(c, want):
    """everything the set gives, against the yardstick's (feature, UMI, reads) table"""
    assert want.uncovered == 0
    assert result(c) == wanted(want)
    assert want.ok + want.bad == want.stats[1] + want.stats[2]
    assert cluster(c) == UP.cluster_of(want)
    assert directional(c) == UP.directional_of(want)
    assert table(c) == UP.table_of(want)


# ---- 1. base ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc2", [False, True])
def test_base_shape(P, rc2):
    lib, fq1, fq2 = UP.base(rc2)
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, rc2, (None, UP.UMI2), miss=1)
    with ctx(P, lib, (None, UP.UMI2), rc2) as c:
        assert c.umi_length == 8 and c.umi_paired == (None, UP.UMI2) and c.umi is None
        assert c.count_block_paired(fq1, fq2) == (len(fq1), len(fq2))
        check_all(c, want)
    assert want.stats[0] == 3000 and want.stats[2] > 0 and want.ok > 2000 and sum(UP.umis_of(want)) < want.ok - 100
    with ctx(P, lib, (None, UP.UMI2), rc2, keep=False) as c:        # the instance without reads per pair
        c.count_block_paired(fq1, fq2)
        assert result(c) == wanted(want) and cluster(c) == UP.cluster_of(want)
    with P.Counter(features=lib, rc2=rc2, miss=1, **START) as c:    # counts and the five counters are those of the plain context
        c.count_block_paired(fq1, fq2)
        counts, stats = c.read_counts()
        assert (list(counts), list(stats)) == (want.counts, want.stats)


# ---- 2. orientation --------------------------------------------------------------------------------------------------------
def test_orientation_the_umi_is_the_text_as_sequenced(P):
    lib, (fq1, fq2), rows = UP.orientation()
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, True, (None, UP.UMI2), miss=1)
    assert UP.table_of(want) == rows and want.bad == 0
    with ctx(P, lib, (None, UP.UMI2), True) as c:
        c.count_block_paired(fq1, fq2)
        check_all(c, want)
        got = table(c)
    texts = {(f, CC.text_of(code, 8)) for f, code, _ in got}
    assert {u for _, u in texts} == set(UP.ORIENT_UMIS)
    assert (0, b"AAAAAAAC") in texts and (0, b"GTTTTTTT") in texts and want.per[0] == {b"AAAAAAAC": 1, b"GTTTTTTT": 1}


# ---- 3. invalid parts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc2", [False, True])
def test_invalid_parts_kind_by_kind(P, rc2):
    lib, (fq1, fq2), kinds = UP.invalid(rc2)
    l1, l2 = fq1.split(b"\n"), fq2.split(b"\n")
    assert len(kinds) == 12 * len(UP.INVALID_KINDS) == (len(l1) - 1) // 4
    for phred, also in ((30, set()), (0, {"lowq_first", "lowq_last"})):
        with ctx(P, lib, (None, UP.UMI2), rc2, phred=phred) as c:
            for kind in UP.INVALID_KINDS:
                a = b"".join(b"\n".join(l1[4 * i:4 * i + 4]) + b"\n" for i, k in enumerate(kinds) if k == kind)
                b = b"".join(b"\n".join(l2[4 * i:4 * i + 4]) + b"\n" for i, k in enumerate(kinds) if k == kind)
                want = UP.expect(lib, a, b, UP.ST1, UP.ST2, UP.LEN, rc2, (None, UP.UMI2), miss=1, phred=phred)
                c.reset()
                assert c.count_block_paired(a, b) == (len(a), len(b))
                assert want.uncovered == 0 and result(c) == wanted(want) and table(c) == UP.table_of(want), kind
                valid = kind in UP.VALID_KINDS | also
                assert (want.ok, want.bad) == ((12, 0) if valid else (0, 12)) and sum(UP.umis_of(want)) == want.ok, kind


# ---- 4. two parts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [UP.TWO, (UP.TWO[0], None)])
def test_two_parts(P, parts):
    lib, (fq1, fq2) = UP.two_parts()
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, True, parts, miss=1)
    with ctx(P, lib, parts, True) as c:
        assert c.umi_length == sum(p[1] for p in parts if p)
        c.count_block_paired(fq1, fq2)
        check_all(c, want)
        got = table(c)
    assert sum(UP.umis_of(want)[:512]) == 0 and want.bad == (4 if parts == UP.TWO else 2)
    if parts == UP.TWO:
        assert (550, 0xFFFFFFFF, 2) in got and (550, 0, 1) in got and UP.cluster_of(want)[2] >= 3


# ---- 5. the per-pair split -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["ragged", "dirty"])
def test_per_pair_split(P, shape):
    lib = PC.pair_library(200, UP.LEN, 1, 1, 21)
    fq1, fq2 = PC.make_pairs(lib, UP.LEN, list(UP.ST1), list(UP.ST2), True, 2000, seed=31 if shape == "ragged" else 32,
                             ragged=True, dirty=shape == "dirty")
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, True, UP.TWO, miss=1)
    assert want.stats[0] == 2000 and want.ok > 200 and want.bad > 200
    with ctx(P, lib, UP.TWO, True) as c:
        assert c.count_block_paired(fq1, fq2) == (len(fq1), len(fq2))
        check_all(c, want)


# ---- 6. the staging edge ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [STAGE_WORDS, PAIR_STAGE_WORDS])
def test_staging_edge_both_layouts(P, monkeypatch, words):
    lib, (fq1, fq2) = UP.staging_edge(words)
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, True, UP.TWO, miss=1)
    assert want.ok > 30 and want.bad > 3
    lens = {len(a[0]) + len(b[0]) for a, b in zip(PC.records(fq1), PC.records(fq2))}
    assert lens == set(range(4 * words - 4, 4 * words + 5)) | {600}
    seen = {}
    for stage in ("0", "1", None):
        if stage is None:
            monkeypatch.delenv("F2Q_UMI_PAIR_STAGE", raising=False)
        else:
            monkeypatch.setenv("F2Q_UMI_PAIR_STAGE", stage)
        with ctx(P, lib, UP.TWO, True) as c:
            blk = c.block_from_fastq_paired(fq1, fq2)
            assert blk.info()["n_general"] == blk.info()["n_reads"] == want.stats[0]     # every pair is a merged raw record
            c.count_resident(blk)
            blk.free()
            check_all(c, want)
            seen[stage] = (result(c), table(c))
    assert seen["0"] == seen["1"] == seen[None]


# ---- 7. growth and pieces --------------------------------------------------------------------------------------------------
def test_growth_files_host_pack_and_reuse(P, tmp_path, monkeypatch, capfd):
    lib, fq1, fq2 = UP.many()
    want = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, True, (None, UP.UMI2), miss=1)
    assert sum(UP.umis_of(want)) > 3000
    monkeypatch.setenv("F2Q_UMI_SLOTS", "64")
    monkeypatch.setenv("F2Q_TRACE", "1")
    l1, l2 = fq1.split(b"\n"), fq2.split(b"\n")
    with ctx(P, lib, (None, UP.UMI2), True) as c:                    # rehashes with reads kept
        for i in range(0, len(l1) - 1, 4 * 500):
            a, b = b"\n".join(l1[i:i + 2000]) + b"\n", b"\n".join(l2[i:i + 2000]) + b"\n"
            assert c.count_block_paired(a, b) == (len(a), len(b))
        check_all(c, want)
        c.reset()                                                    # a second sample on the same context
        blib, b1, b2 = UP.base(True)
        assert blib == lib and result(c) == ([0] * len(lib), [0] * 5, [0] * len(lib), 0, 0) and table(c) == []
        c.count_block_paired(b1, b2)
        check_all(c, UP.expect(lib, b1, b2, UP.ST1, UP.ST2, UP.LEN, True, (None, UP.UMI2), miss=1))
    assert len(re.findall(r"\[f2q trace\] UMI set rehash \d+:", capfd.readouterr().err)) >= 4
    monkeypatch.delenv("F2Q_TRACE")
    monkeypatch.setenv("F2Q_FILE_CHUNK", "4096")
    for kind in ("plain", "gzip"):
        paths = [tmp_path / f"s_R{k}.fastq{'.gz' if kind == 'gzip' else ''}" for k in (1, 2)]
        for path, fq in zip(paths, (fq1, fq2)):
            path.write_bytes(gzip.compress(fq, 1) if kind == "gzip" else fq)
        with ctx(P, lib, (None, UP.UMI2), True) as c:
            _, truncated = c.count_file_paired(str(paths[0]), str(paths[1]))
            assert not truncated
            check_all(c, want)
    monkeypatch.setenv("F2Q_HOST_PACK", "1")
    with ctx(P, lib, (None, UP.UMI2), True) as c:
        c.count_block_paired(fq1, fq2)
        check_all(c, want)


# ---- 8. the command line ---------------------------------------------------------------------------------------------------
def _table(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


def test_command_line_end_to_end(P, tmp_path, capsys):
    lib = PC.pair_library(200, UP.LEN, 1, 1, 21)
    samples = {"alpha_S1_L001_R1_001": UP.base(True)[1:], "beta_R1": UP.base(True, 1200, 0x5EC0)[1:]}
    indir = tmp_path / "in"
    indir.mkdir()
    for name, (fq1, fq2) in samples.items():
        (indir / (name + ".fastq")).write_bytes(fq1)
        (indir / (name.replace("R1", "R2") + ".fastq")).write_bytes(fq2)
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    outs = {}
    for tag, extra in (("umi", ["--umi2", "12,8", "--mu", "1", "--mur", "directional"]), ("plain", [])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(out), "--st", "5", "--l", "10", "--m", "1", "--pb", "--pe", "--st2", "0",
                     "--rc2", "--k"] + extra)
        (outs[tag],) = [d for d in out.iterdir() if d.is_dir()]
    capsys.readouterr()
    want = {n: UP.expect(lib, a, b, UP.ST1, UP.ST2, UP.LEN, True, (None, UP.UMI2), miss=1) for n, (a, b) in samples.items()}
    assert all(w.uncovered == 0 for w in want.values())
    clus, dirs = {n: UP.cluster_of(w) for n, w in want.items()}, {n: UP.directional_of(w) for n, w in want.items()}
    names = [f"g{i:03d}" for i in range(len(lib))]
    order = sorted(enumerate(names), key=lambda e: e[1])
    order_names = list(samples)
    # the outputs a run without the flags writes are there byte for byte (the running times and the command line aside)
    new_files = {"compiled_umi.csv", "compiled_umi_collapsed.csv", "compiled_umi_directional.csv"} | \
                {n + s for n in samples for s in ("_umi_reads.csv", "_umi_pairs.csv")}
    assert {p.name for p in outs["umi"].iterdir()} == {p.name for p in outs["plain"].iterdir()} | new_files
    stats, plain_stats = _table(outs["umi"] / "compiled_stats.csv"), _table(outs["plain"] / "compiled_stats.csv")
    at = stats.index(fast2q.UMI_STATS_HEAD)
    numbers = lambda t: [r[:1] + r[3:] for r in t if r and not r[0].startswith("#cmd used") and not r[0].startswith("#UMI")]
    assert numbers(stats[:at]) == numbers(plain_stats)
    for path in outs["plain"].iterdir():
        if path.name.endswith("_reads.csv"):                         # (its first line holds the running time)
            assert _table(outs["umi"] / path.name)[1:] == _table(path)[1:]
        elif path.suffix == ".csv" and path.name != "compiled_stats.csv":
            assert (outs["umi"] / path.name).read_bytes() == path.read_bytes(), path.name
    assert ["#UMI in mate 2, start, length: 12,8"] in stats and not any(r and r[0].startswith("#UMI in mate 1") for r in stats)
    assert ["#UMI mismatches collapsed: 1"] in stats and ["#UMI collapse rule: directional"] in stats
    # the three tables, in compiled.csv's layout and row order
    reads = _table(outs["umi"] / "compiled.csv")
    columns = {"_umi": {s: UP.umis_of(want[s]) for s in samples}, "_umi_collapsed": {s: clus[s][0] for s in samples},
               "_umi_directional": {s: dirs[s][0] for s in samples}}
    for suffix, column in columns.items():
        got = _table(outs["umi"] / f"compiled{suffix}.csv")
        assert got[0] == reads[0] == ["#Feature"] + order_names and [r[0] for r in got] == [r[0] for r in reads]
        assert got[1:] == [[n] + [str(column[s][i]) for s in order_names] for i, n in order], suffix
    # the stats blocks
    assert stats[at + 1:at + 3] == [[s, str(want[s].ok), str(want[s].bad)] for s in order_names]
    at = stats.index(fast2q.UMI_COLLAPSE_STATS_HEAD)
    assert stats[at + 1:at + 3] == [[s, str(clus[s][1]), str(clus[s][2]), str(sum(clus[s][0]))] for s in order_names]
    at = stats.index(fast2q.UMI_DIRECTIONAL_STATS_HEAD)
    rows = []
    for s in order_names:
        mol, pairs, edges, dominated, n = dirs[s]
        rows.append([s, str(pairs), str(edges), str(dominated), str(sum(mol)), str(n)])
    assert stats[at + 1:] == rows
    # --k: the per-sample tables, the UMI text the concatenation as sequenced
    for s in order_names:
        kept = _table(outs["umi"] / (s + "_umi_reads.csv"))
        assert kept[0] == ["#Feature", "Reads", "UMIs", "Molecules", "Directional"]
        cols = [want[s].counts, UP.umis_of(want[s]), clus[s][0], dirs[s][0]]
        assert kept[1:] == [[n] + [str(col[i]) for col in cols] for i, n in order]
        dump = _table(outs["umi"] / (s + "_umi_pairs.csv"))
        assert dump[0] == ["#Feature", "UMI", "Reads"]
        assert dump[1:] == [[names[f], CC.text_of(code, 8).decode(), str(n)] for f, code, n in UP.table_of(want[s])]
    # the refusals leave no output directory
    base = ["-c", "--s", str(indir), "--g", str(guides), "--o", str(tmp_path / "never")]
    for extra, words in ((["--umi2", "12,8"], ["--umi2", "--pe"]), (["--pe", "--st2", "0", "--umi", "12,8"], ["--umi", "--pe", "--umi2"]),
                         (["--pe", "--st2", "0", "--umi1", "0,9", "--umi2", "12,8"], ["--umi1", "--umi2", "16"])):
        with pytest.raises(SystemExit):
            fast2q.main(base + extra)
        said = capsys.readouterr().out
        assert "FATAL" in said and all(w in said for w in words)
    assert not (tmp_path / "never").exists()


# ---- 9. the ABI's errors ---------------------------------------------------------------------------------------------------
def test_abi_argument_and_state_errors(P, tmp_path):
    lib = PC.pair_library(8, UP.LEN, 1, 1, 21)

    def code_of(call):
        with pytest.raises(binding.F2QError) as exc:
            call()
        return exc.value.code
    for bad in (((0, 0), (0, 0)), (None, None), ((-1, 4), None), (None, (-1, 4)), ((0, -4), (0, 8)), ((0, 4), (0, -1)), ((0x40000000, 4), None),
                (None, (0x40000000, 4)), ((0, 9), (0, 8)), ((0, 17), None), (None, (3, 17))):
        assert code_of(lambda: P.Counter(features=lib, umi_paired=bad, **START)) == -1, bad
    assert code_of(lambda: P.Counter(features=lib, start="5", length=UP.LEN, umi_paired=(None, (12, 8)))) == -7      # not paired
    assert code_of(lambda: P.Counter(mode="EC", umi_paired=(None, (12, 8)), **START)) == -7                          # Extract+Count
    assert code_of(lambda: P.Counter(features=lib, umi=(0, 8), **START)) == -7                                       # f2q_set_umi on a paired context
    with P.Counter(features=lib, start="5", length=UP.LEN, umi=(20, 8)) as c:                                        # f2q_set_mate2 on a UMI context
        assert code_of(lambda: c.set_mate2("0")) == -7
    with P.Counter(features=lib, umi_paired=((0x3FFFFFFF, 8), (0, 8)), **START) as c:                                # the largest start, 16 bases
        assert c.umi_length == 16
        assert code_of(lambda: c.set_umi_paired(None, (12, 8))) == -7                                                # twice
        assert code_of(lambda: c.set_umi(0, 8)) == -7
        umis, ok, bad = c.read_umis()                                                                                # nothing counted yet
        assert list(umis) == [0] * 8 and (ok, bad) == (0, 0)
        c.set_umi_reads(True)
        a = b"@a\n" + b"A" * 30 + b"\n+\n" + b"I" * 30 + b"\n"
        assert c.count_block_paired(a, a) == (len(a), len(a))
        assert c.read_umis()[1:] == (0, 0) and list(c.read_counts()[1])[0] == 1
        assert code_of(lambda: c.set_umi_reads(False)) == -7                                                         # after a counting call
        path = tmp_path / "s_R1.fastq"
        path.write_bytes(a)
        assert code_of(lambda: c.count_file_shard(str(path), 0, 2)) == -7                                            # several ranks
    with P.Counter(features=lib, **START) as c:
        assert code_of(c.read_umis) == -7
        a = b"@a\nACGT\n+\nIIII\n"
        c.count_block_paired(a, a)
        assert code_of(lambda: c.set_umi_paired(None, (12, 8))) == -7                                                # after a counting call
