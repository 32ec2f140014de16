"""--parts on the device: f2q_set_parts / k_count_parts<false, true> / f2q_read_parts / f2q_parts_recombinants against the
plain-Python expectation of tests/parts_cases.py (one single-window oracle run per part, the class rule written out),
through every single-process counting entry point, and the command line's outputs."""
import csv
import gzip
import importlib

import pytest

import parts_cases as PT
from conftest import bgzf_bytes, pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")
ESTATE, EINVAL = -7, -1


@pytest.fixture(scope="module")
def P():
    return pkg()


def run_of(st1, st2, paired, rc2=False, miss=1):
    if paired:
        return dict(start=str(st1), start2=str(st2), rc2=rc2, length=PT.L, miss=miss, phred=30)
    return dict(start=f"{st1},{st2}", length=PT.L, miss=miss, phred=30)


def result(c):
    pc, m1, m2, cls = c.read_parts()
    i1, i2, reads = c.parts_recombinants()
    return dict(parts_counts=pc.tolist(), part1=m1.tolist(), part2=m2.tolist(), classes=cls.tolist(),
                recombinants={(int(a), int(b)): int(n) for a, b, n in zip(i1, i2, reads)})


def joined(c):
    counts, stats = c.read_counts()
    return list(counts), list(stats)


def count(c, fq1, fq2):
    if fq2 is None:
        assert c.count_block(fq1) == len(fq1)
    else:
        assert c.count_block_paired(fq1, fq2) == (len(fq1), len(fq2))


def counted(P, lib, fq1, fq2, **run):
    with P.Counter(features=lib, parts=True, **run) as c:
        count(c, fq1, fq2)
        return joined(c), result(c)


def plain(P, lib, fq1, fq2, **run):
    with P.Counter(features=lib, **run) as c:
        count(c, fq1, fq2)
        return joined(c)


def check_invariants(stats, got):
    c = got["classes"]
    assert sum(c) == stats[0]
    assert sum(got["parts_counts"]) == c[0] + c[1]
    assert sum(got["recombinants"].values()) == c[2]
    assert sum(got["part1"]) == c[0] + c[1] + c[2] + c[3] and sum(got["part2"]) == c[0] + c[1] + c[2] + c[4]


def pieces(fq, per):
    lines = fq.split(b"\n")[:-1]
    return [b"".join(l + b"\n" for l in lines[i:i + 4 * per]) for i in range(0, len(lines), 4 * per)]


_WANT = {}


def want_of(paired, rc2, miss):
    """the sample's expectation, computed once per shape and --m and shared"""
    key = (paired, rc2, miss)
    if key not in _WANT:
        lib, fq1, fq2, st1, st2 = PT.sample(paired, rc2)
        _WANT[key] = PT.expect(lib, fq1, fq2, st1, st2, PT.L, rc2, miss)
    return _WANT[key]


SHAPES = [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("paired,rc2", SHAPES)
@pytest.mark.parametrize("miss", [0, 1])
def test_parity_with_the_expectation_and_with_a_plain_context(P, paired, rc2, miss):
    lib, fq1, fq2, st1, st2 = PT.sample(paired, rc2)
    run = run_of(st1, st2, paired, rc2, miss)
    (counts, stats), got = counted(P, lib, fq1, fq2, **run)
    assert got == want_of(paired, rc2, miss)
    assert (counts, stats) == plain(P, lib, fq1, fq2, **run)          # everything written before is the joined rule's, unchanged
    check_invariants(stats, got)
    if miss == 0:
        assert got["parts_counts"] == counts and got["classes"][1] == 0
    else:
        assert all(n >= 10 for n in got["classes"]) and got["parts_counts"] != counts


@pytest.mark.parametrize("paired,rc2", [(False, False), (True, True)])
def test_a_set_grown_from_64_slots_in_pieces_of_thirty_records(P, monkeypatch, capfd, paired, rc2):
    lib, fq1, fq2, st1, st2 = PT.sample(paired, rc2)
    monkeypatch.setenv("F2Q_PARTS_SLOTS", "64")
    monkeypatch.setenv("F2Q_TRACE", "1")
    with P.Counter(features=lib, parts=True, **run_of(st1, st2, paired, rc2)) as c:
        a = pieces(fq1, 30)
        b = [None] * len(a) if fq2 is None else pieces(fq2, 30)
        for x, y in zip(a, b):
            count(c, x, y)
        got = result(c)
    said = capfd.readouterr().err
    assert got == want_of(paired, rc2, 1)
    n1, n2, _ = PT.part_libraries(lib)
    assert f"parts: n1 {len(n1)}, n2 {len(n2)}, pair table 256 slots" in said and said.count("[f2q trace] parts: n1") == 1
    assert said.count("recombinant set rehash") >= 3 and "64 -> 128 slots" in said


def test_records_longer_than_the_lds_staging_area(P):
    lib, fq = PT.long_reads()
    run = run_of(0, 20, False)
    (counts, stats), got = counted(P, lib, fq, None, **run)
    assert got == PT.expect(lib, fq, None, 0, 20, PT.L, miss=1)
    assert (counts, stats) == plain(P, lib, fq, None, **run)
    check_invariants(stats, got)


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf", "bgzf_device_inflate"])
@pytest.mark.parametrize("paired", [False, True])
def test_streamed_files_equal_the_one_block_result(P, tmp_path, monkeypatch, kind, paired):
    lib, fq1, fq2, st1, st2 = PT.sample(paired, paired)
    monkeypatch.setenv("F2Q_FILE_CHUNK", "4096")
    if kind == "bgzf_device_inflate":
        monkeypatch.setenv("F2Q_DEVICE_INFLATE", "1")
    paths = []
    for tag, fq in (("R1", fq1), ("R2", fq2)):
        if fq is not None:
            paths.append(tmp_path / {"plain": f"s_{tag}.fastq", "gzip": f"s_{tag}.fastq.gz"}.get(kind, f"s_{tag}.bgzf.fastq.gz"))
            paths[-1].write_bytes(fq if kind == "plain" else gzip.compress(fq) if kind == "gzip" else bgzf_bytes(fq, block=3000))
    with P.Counter(features=lib, parts=True, **run_of(st1, st2, paired, paired)) as c:
        _, truncated = c.count_file_paired(str(paths[0]), str(paths[1])) if paired else c.count_file(str(paths[0]))
        got = result(c)
    assert not truncated and got == want_of(paired, paired, 1)


def test_resident_blocks_device_text_and_host_pack(P, monkeypatch):
    lib, fq1, _, st1, st2 = PT.sample(False, False)
    want = want_of(False, False, 1)
    n = sum(want["classes"])
    with P.Counter(features=lib, parts=True, **run_of(st1, st2, False)) as c:
        blk = c.block_from_fastq(fq1)
        assert blk.info()["n_general"] == blk.info()["n_reads"] == n   # every read takes the raw-record road
        t = c.count_resident(blk)
        assert t["general_reads"] == n and result(c) == want
        c.reset()
        c.count_resident_queued(blk)
        c.queued_times()
        assert result(c) == want
        blk.free()
        c.reset()
        text = c.text_upload(fq1)
        assert c.count_text(text) == len(fq1) and result(c) == want
        text.free()
    lib, p1, p2, a, b = PT.sample(True, True)
    with P.Counter(features=lib, parts=True, **run_of(a, b, True, True)) as c:
        blk = c.block_from_fastq_paired(p1, p2)
        assert blk.info()["n_general"] == blk.info()["n_reads"]
        c.count_resident(blk)
        assert result(c) == want_of(True, True, 1)
        blk.free()
    monkeypatch.setenv("F2Q_HOST_PACK", "1")
    assert counted(P, lib, p1, p2, **run_of(a, b, True, True))[1] == want_of(True, True, 1)
    lib, fq1, _, st1, st2 = PT.sample(False, False)
    assert counted(P, lib, fq1, None, **run_of(st1, st2, False))[1] == want


def test_reset_reuse_and_a_new_library(P):
    lib, fq1, _, st1, st2 = PT.sample(False, False)
    other, _ = PT.make_reads(lib, st1, st2, 700, 0x5EC0)
    run = run_of(st1, st2, False)
    n1, n2, _ = PT.part_libraries(lib)
    empty = dict(parts_counts=[0] * len(lib), part1=[0] * len(n1), part2=[0] * len(n2), classes=[0] * 6, recombinants={})
    with P.Counter(features=lib, parts=True, **run) as c:
        assert c.parts_info() == (len(n1), len(n2)) and result(c) == empty           # nothing counted yet
        count(c, fq1, None)
        first = result(c)
        c.reset()
        assert result(c) == empty
        count(c, other, None)
        second = result(c)
        small = lib[:40]
        c.set_features(small)                                                        # a new library rebuilds the tables and starts afresh
        s1, s2, _ = PT.part_libraries(small)
        assert c.parts_info() == (len(s1), len(s2)) and result(c)["classes"] == [0] * 6 and result(c)["recombinants"] == {}
        count(c, fq1, None)
        third = result(c)
        _refused(EINVAL, ["feature 1", "ACGTACGT"], lambda: c.set_features(["AAAA:CCCC", "ACGTACGT"]))
        assert c.parts_info() == (len(s1), len(s2))                                  # the refusal left the context as it was
    assert first == want_of(False, False, 1)
    assert second == PT.expect(lib, other, None, st1, st2, PT.L, miss=1) == counted(P, lib, other, None, **run)[1]
    assert third == PT.expect(small, fq1, None, st1, st2, PT.L, miss=1)


def test_parts_before_the_library_and_null_pointers(P):
    lib, fq1, _, st1, st2 = PT.sample(False, False)
    with P.Counter(parts=True, **run_of(st1, st2, False)) as c:
        assert c.parts_info() == (0, 0) and result(c)["classes"] == [0] * 6
        c.set_features(lib)
        count(c, fq1, None)
        assert result(c) == want_of(False, False, 1)
        assert c._L.f2q_read_parts(c._h, None, None, None, None) == 0                # any pointer may be NULL
        n = binding.C.c_uint64(0)
        assert c._L.f2q_parts_recombinants(c._h, 0, binding.C.byref(n), None, None, None) == 0 and n.value == len(want_of(False, False, 1)["recombinants"])
        buf = (binding.C.c_uint32 * 4)()
        assert c._L.f2q_parts_recombinants(c._h, 4, binding.C.byref(n), buf, None, None) == EINVAL
    with P.Counter(features=lib, **run_of(st1, st2, False)) as c:
        c.set_parts()                                                                # after the library
        count(c, fq1, None)
        assert result(c) == want_of(False, False, 1)


@pytest.mark.parametrize("which", ["one_feature", "star"])
def test_library_edges(P, which):
    lib = PT.one_feature() if which == "one_feature" else PT.star_library()
    fq, _ = PT.make_reads(lib, 0, 20, 300, 0xED6E)
    run = run_of(0, 20, False)
    (counts, stats), got = counted(P, lib, fq, None, **run)
    assert got == PT.expect(lib, fq, None, 0, 20, PT.L, miss=1) and got["classes"][2] == 0 and got["recombinants"] == {}
    assert (counts, stats) == plain(P, lib, fq, None, **run)
    check_invariants(stats, got)


def _refused(code, words, call):
    with pytest.raises(binding.F2QError) as exc:
        call()
    assert exc.value.code == code and all(w in str(exc.value) for w in words), str(exc.value)


def test_state_and_argument_refusals(P, tmp_path):
    lib, fq1, _, st1, st2 = PT.sample(False, False)
    run = run_of(st1, st2, False)
    _refused(ESTATE, ["Extract+Count"], lambda: P.Counter(mode="EC", parts=True, start="0,20", length=10))
    _refused(ESTATE, ["--us/--ds"], lambda: P.Counter(parts=True, upstream="ACGTAC", downstream="TTGACA", length=10))
    _refused(ESTATE, ["exactly two windows", "not 1"], lambda: P.Counter(parts=True, start="0", length=10))
    _refused(ESTATE, ["exactly two windows", "not 3"], lambda: P.Counter(parts=True, start="0,10,20", length=10))
    _refused(ESTATE, ["one window per mate", "2 + 1"], lambda: P.Counter(parts=True, start="0,20", start2="0", length=10))
    _refused(ESTATE, ["one window per mate", "1 + 2"], lambda: P.Counter(parts=True, start="0", start2="0,20", length=10))
    _refused(ESTATE, ["UMI"], lambda: P.Counter(parts=True, umi=(30, 8), **run))
    _refused(ESTATE, ["UMI"], lambda: P.Counter(parts=True, umi_header=("_", 8), **run))
    _refused(ESTATE, ["UMI"], lambda: P.Counter(parts=True, start="0", start2="0", umi_paired=((12, 8), None), length=10))
    _refused(ESTATE, ["demultiplexing"], lambda: P.Counter(parts=True, sample_barcodes=(30, [b"ACGTACGT", b"TTGACATG"]), **run))
    _refused(ESTATE, ["strand"], lambda: P.Counter(parts=True, strand="both", **run))
    _refused(EINVAL, ["feature 2", "ACGTACGTACGTACGTACGTA", "two non-empty parts"], lambda: P.Counter(features=list(lib[:2]) + ["ACGTACGTACGTACGTACGTA"], parts=True, **run))
    with P.Counter(features=list(lib[:2]) + ["ACGTACGTACGTACGTACGTA"], **run) as c:
        _refused(EINVAL, ["feature 2"], c.set_parts)
        _refused(ESTATE, ["f2q_set_parts first"], c.read_parts)                      # ... and the context is no parts context
        _refused(ESTATE, ["f2q_set_parts first"], c.parts_recombinants)
        _refused(ESTATE, ["f2q_set_parts first"], c.parts_info)
    with P.Counter(features=lib, strand="fwd", **run) as c:
        count(c, fq1[:4000].rsplit(b"\n@", 1)[0] + b"\n", None)
        _refused(ESTATE, ["before counting"], c.set_parts)
    path = tmp_path / "s.fastq"
    path.write_bytes(fq1[:20000])
    with P.Counter(features=lib, parts=True, **run) as c:
        c.set_strand("fwd")                                                          # mode 0 changes nothing, anywhere
        _refused(ESTATE, ["once"], c.set_parts)
        _refused(ESTATE, ["parts"], lambda: c.set_umi(30, 8))
        _refused(ESTATE, ["parts"], lambda: c.set_umi_header("_", 8))
        _refused(ESTATE, [], lambda: c.set_umi_paired((0, 8), None))
        _refused(ESTATE, ["parts"], lambda: c.set_sample_barcodes(30, [b"ACGTACGT"]))
        _refused(ESTATE, ["parts"], lambda: c.set_strand("rev"))
        _refused(ESTATE, [], lambda: c.set_mate2("0"))
        _refused(ESTATE, ["ranks"], lambda: c.count_file_shard(str(path), 0, 2))
        n, _ = c.file_pieces(str(path), 1 << 16)
        _refused(ESTATE, ["ranks"], lambda: c.count_pieces(str(path), 0, 2, 1 << 16, c.census_pieces(str(path), 0, 2, 1 << 16, n)))
        _, truncated = c.count_file_shard(str(path), 0, 1)                           # one rank is a whole file
        assert not truncated and sum(result(c)["classes"]) == joined(c)[1][0] > 0
    with P.Counter(parts=True, **run) as c:                                          # set_mate2 comes before set_parts, never after
        _refused(ESTATE, ["f2q_set_mate2 comes first"], lambda: c.set_mate2("0"))
    with P.Counter(features=lib, **run) as c, P.Counter(features=lib, parts=True, **run) as d:
        blk = c.block_from_fastq(fq1)                                                # packed tiles of a plain context
        if blk.info()["n_general"] != blk.info()["n_reads"]:
            assert d._L.f2q_count_resident(d._h, blk._h, None) == ESTATE and b"f2q_set_parts" in d._L.f2q_last_error(d._h)
        blk.free()


# ---- the command line ----------------------------------------------------------------------------------------------------
def _table(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


@pytest.mark.parametrize("paired", [False, True])
def test_cli_outputs(P, tmp_path, capsys, paired):
    lib = PT.library()
    shape = PT.PAIRED if paired else PT.SINGLE
    st1, st2 = shape["st1"], shape["st2"]
    samples = {name: PT.make_reads(lib, st1, st2, n, seed, paired=paired, rc2=paired) for name, n, seed in (("s1", 900, 0xC11), ("s2", 600, 0xC12))}
    indir = tmp_path / "in"
    indir.mkdir()
    for name, (fq1, fq2) in samples.items():
        if paired:
            (indir / (name + "_R1.fastq")).write_bytes(fq1)
            (indir / (name + "_R2.fastq")).write_bytes(fq2)
        else:
            (indir / (name + ".fastq")).write_bytes(fq1)
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    where = ["--pe", "--st", str(st1), "--st2", str(st2), "--rc2"] if paired else ["--st", f"{st1},{st2}"]
    outs = {}
    for tag, extra in (("parts", ["--parts", "--k"]), ("plain", ["--k"])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(out), "--l", str(PT.L), "--m", "1", "--pb"] + where + extra)
        (outs[tag],) = [d for d in out.iterdir() if d.is_dir()]
    capsys.readouterr()
    snames = [n + "_R1" for n in samples] if paired else list(samples)
    # what the run wrote before stays as it was; the exact list of new files
    assert (outs["parts"] / "compiled.csv").read_bytes() == (outs["plain"] / "compiled.csv").read_bytes()
    new = sorted(set(p.name for p in outs["parts"].iterdir() if p.suffix == ".csv") - set(p.name for p in outs["plain"].iterdir()))
    assert new == sorted(["compiled_parts.csv", "compiled_recombinants.csv"] + [s + "_parts_marginals.csv" for s in snames])
    stats, plain_stats = _table(outs["parts"] / "compiled_stats.csv"), _table(outs["plain"] / "compiled_stats.csv")
    header = ["#Parts matched independently: 2"]
    at = stats.index(fast2q.PARTS_STATS_HEAD)
    strip = lambda t: [r[:1] + r[3:] if r and not r[0].startswith("#") else r for r in t if not (r and r[0].startswith("#cmd used"))]    # (not the running times, not the command)
    assert header in stats and strip([r for r in stats[:at] if r != header]) == strip(plain_stats)
    want = {s: PT.expect(lib, fq1, fq2, st1, st2, PT.L, paired, 1) for s, (fq1, fq2) in zip(snames, samples.values())}
    # <name>_parts.csv: <name>.csv's layout and row order, holding parts_counts
    reads, parts = _table(outs["parts"] / "compiled.csv"), _table(outs["parts"] / "compiled_parts.csv")
    assert parts[0] == reads[0] == ["#Feature"] + snames and [r[0] for r in parts] == [r[0] for r in reads]
    names = [f"g{i:03d}" for i in range(len(lib))]
    for row in parts[1:]:
        assert [int(x) for x in row[1:]] == [want[s]["parts_counts"][names.index(row[0])] for s in snames]
    # <name>_recombinants.csv: a row per pair of part texts seen in any sample, by total reads, then by the texts
    lib1, lib2, _ = PT.part_libraries(lib)
    rec = _table(outs["parts"] / "compiled_recombinants.csv")
    assert rec[0] == ["#Part1", "Part2"] + snames
    rows = {}
    for k, s in enumerate(snames):
        for (i1, i2), n in want[s]["recombinants"].items():
            rows.setdefault((lib1[i1], lib2[i2]), [0] * len(snames))[k] = n
    assert rec[1:] == [[a, b] + [str(n) for n in ns] for (a, b), ns in sorted(rows.items(), key=lambda kv: (-sum(kv[1]), kv[0]))] and len(rows) > 100
    # the block of <name>_stats.csv and the marginals
    assert stats[at + 1:] == [[s] + [str(n) for n in (c[0], c[1], c[2], len(want[s]["recombinants"]), c[3], c[4], c[5])] for s in snames for c in [want[s]["classes"]]]
    for s in snames:
        assert _table(outs["parts"] / (s + "_parts_marginals.csv")) == [["#position", "part", "reads"]] + \
            [["1", p, str(n)] for p, n in zip(lib1, want[s]["part1"])] + [["2", p, str(n)] for p, n in zip(lib2, want[s]["part2"])]
