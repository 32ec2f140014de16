"""--mur directional on the device: reads per (feature, UMI) pair (f2q_set_umi_reads: k_count_umi<true>, k_umi_rehash<true>,
f2q_umi_pairs) and f2q_umi_collapse_directional (k_umi_uf_init / k_umi_link<true> / k_umi_dir_spread / k_umi_dir_roots)
against the literal restatement of UMI-tools in tests/umi_dir_cases.py, computed under three tie orders; what the calls
leave untouched, their state errors, and the command line's outputs."""
import collections
import csv
import importlib
import re

import pytest

import umi_cases as UC
import umi_collapse_cases as CC
import umi_dir_cases as DC
from conftest import pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")


@pytest.fixture(scope="module")
def P():
    return pkg()


def directional(c):
    got = c.collapse_umis_directional()
    assert (list(got[0]),) + got[1:3] == cluster(c, rule="directional")          # collapse_umis' tuple of three
    return (list(got[0]),) + got[1:]


def cluster(c, dist=1, **kw):
    molecules, pairs, edges = c.collapse_umis(dist, **kw)
    return list(molecules), pairs, edges


def pairs(c):
    f, codes, reads = c.umi_pairs()
    return list(zip(f.tolist(), codes.tolist(), reads.tolist()))


def state(c):
    counts, stats = c.read_counts()
    umis, ok, bad = c.read_umis()
    return list(counts), list(stats), list(umis), ok, bad, cluster(c)


def checked(P, name, per=0):
    """the shape counted with reads kept (in pieces of `per` records), collapsed twice, the invariants of every shape"""
    lib, fq, run, umi = DC.shape(name)
    assert DC.separates(name)                                        # the expectation itself tells the rules apart
    with P.Counter(features=lib, umi=umi, umi_reads=True, **run) as c:
        for piece in (CC.pieces(fq, per) if per else [fq]):
            assert c.count_block(piece) == len(piece)
        before = state(c)
        got = directional(c)
        assert directional(c) == got                                 # calling twice
        table = pairs(c)
        assert state(c) == before                                    # nothing another call reads has changed
    want = DC.expected(name)
    assert got == want
    (wcl, wpairs, wedges), wumis = DC.expected_cluster(name)
    cl = before[5]
    assert cl == (wcl, wpairs, wedges) and before[2] == wumis
    assert all(a <= b <= u for a, b, u in zip(cl[0], got[0], before[2]))
    assert got[1] == cl[1] and got[2] == cl[2] and got[4] == before[3] == sum(r for _, _, r in table)
    assert table == DC.expected_pairs(name)
    return got, before


def test_known_answers(P):
    """features 6 .. 21 hold the case "two single reads X - Y, five reads next to Y" with random UMIs, so that the dominated
    Y lies below its tree's root in some and is the root in others.  The slots of the device set cannot be read through
    the ABI; that both sides occur is asserted in tests/test_umi_dir_cpu.py::test_known_answers on the emulated set, which
    has the device's hash, probe sequence and first size (65 536 slots, no rehash for these 62 pairs), so the same slots.
    Here the pair dump shows that all sixteen X, Y, Z triples are in the set with their reads, and every answer is 1"""
    got, before = checked(P, "known")
    code = lambda u: sum(b"ACGT".index(ch) << (2 * j) for j, ch in enumerate(u))
    table = {(f, c): n for f, c, n in DC.expected_pairs("known")}    # (checked() has compared the device's dump with it)
    for f, (x, y, z) in enumerate(DC.known()[5], 6):
        assert (table[(f, code(x))], table[(f, code(y))], table[(f, code(z))]) == (1, 1, 5)
    dirw, clw, umiw = DC.known()[4]
    assert got[0] == dirw and before[5][0] == clw and before[2] == umiw
    assert got[0][:6] == [1, 2, 2, 1, 1, 1] and got[0][6:6 + DC.N_SPREAD] == [1] * DC.N_SPREAD


def test_one_base_umis(P):
    got, before = checked(P, "known1")
    assert got[0][:2] == [1, 4] and before[5][0][:2] == [1, 1] and before[2][:2] == [4, 4]


def test_sixteen_base_umis_next_to_wide_feature_indices(P):
    got, _ = checked(P, "wide")
    assert sum(got[0][:512]) == 0 and got[2] > 0


# F2Q_UMI_LINK_WG, F2Q_UMI_LINK_GRID -> the workgroup size the linking launch must take (None: unset; 96 is no whole
# number of waves and 0 no grid: the default for both)
GEOMETRIES = [(None, None, 256), ("64", "1", 64), ("128", "2", 128), ("96", "0", 256)]


def set_geometry(monkeypatch, wg, grid):
    monkeypatch.setenv("F2Q_TRACE", "1")
    for key, value in (("F2Q_UMI_LINK_WG", wg), ("F2Q_UMI_LINK_GRID", grid)):
        if value is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, value)


@pytest.mark.parametrize("wg,grid,used", GEOMETRIES)
@pytest.mark.parametrize("name", ["known1", "wide"])
def test_launch_geometry(P, monkeypatch, capfd, name, wg, grid, used):
    """both linking launches under every geometry the switches can give, on the shapes that bound 3L: one-base UMIs (3L = 3:
    21 groups a round, lane 63 idle) and sixteen-base ones (3L = 48: one group, 16 lanes idle).  The first set has
    65 536 slots: 64 x 1 strides over it many times"""
    set_geometry(monkeypatch, wg, grid)
    got, before = checked(P, name)                                   # (asserts the expectation of both rules)
    said = capfd.readouterr().err
    tails = re.findall(r"\[f2q trace\] UMI collapse directional: (\d+) pairs, (\d+) edges, (\d+) dominated, (\d+) molecules, (\d+) reads, [\d.]+ ms "
                       r"\([^;]*; wave, (\d+) x (\d+)\)", said)
    assert tails and all(tuple(map(int, t[:5])) == (got[1], got[2], got[3], sum(got[0]), got[4]) for t in tails)
    cl = before[5]
    ctails = re.findall(r"\[f2q trace\] UMI collapse: (\d+) pairs, (\d+) edges, (\d+) molecules, [\d.]+ ms \([^;]*; wave, (\d+) x (\d+)\)", said)
    assert ctails and all(tuple(map(int, t[:3])) == (cl[1], cl[2], sum(cl[0])) for t in ctails)
    for t in tails + ctails:
        glink, wgsize = int(t[-2]), int(t[-1])
        assert wgsize == used and 1 <= glink and glink * used <= 65536 and (glink * used < 65536) == (wg == "64")


def test_a_set_smaller_than_one_wave(P, monkeypatch, capfd):
    """a dozen records from a first set of 2 slots leave 32 slots: `base + lane < slots` cuts the one wave that has work,
    the other waves of the workgroup find none; the two rules give different answers on these records"""
    monkeypatch.setenv("F2Q_TRACE", "1")
    monkeypatch.setenv("F2Q_UMI_SLOTS", "2")
    got, before = checked(P, "tiny")
    assert got == DC.TINY_WANT and before[5] == CC.TINY_WANT and before[2] == DC.TINY_UMIS
    said = capfd.readouterr().err
    assert re.findall(r"\[f2q trace\] UMI set: (\d+) slots, (\d+) rehashes", said) == [("32", "0")], said      # the smallest power of two >= 2 x 11
    assert set(re.findall(r"; wave, (\d+) x (\d+)\)", said)) == {("1", "256")}


@pytest.mark.parametrize("layout", ["first_set", "rehashed"])
@pytest.mark.parametrize("name", ["ones", "twice"])
def test_contention(P, monkeypatch, capfd, name, layout):
    """dom[] and the union-find under heavy traffic together; 'rehashed': a first set of 64 slots fed in pieces of 30
    records, so every count has travelled through several rehashes"""
    want = DC.expected(name)
    assert want[0][DC.GRAY_FEATURE] == (DC.GRAY_N // 2 if name == "twice" else 1)
    assert DC.expected_cluster(name)[0][0][DC.GRAY_FEATURE] == 1
    monkeypatch.setenv("F2Q_TRACE", "1")
    if layout == "rehashed":
        monkeypatch.setenv("F2Q_UMI_SLOTS", "64")
    got, _ = checked(P, name, 30 if layout == "rehashed" else 0)
    assert got == want
    said = capfd.readouterr().err
    lines = re.findall(r"\[f2q trace\] UMI collapse directional: (\d+) pairs, (\d+) edges, (\d+) dominated, (\d+) molecules, (\d+) reads, [\d.]+ ms", said)
    assert lines[0] == (str(want[1]), str(want[2]), str(want[3]), str(sum(want[0])), str(want[4])), said
    assert (len(re.findall(r"\[f2q trace\] UMI set rehash \d+:", said)) >= 5) == (layout == "rehashed")
    # the pair dump is a Counter of the valid pairs (every read of these shapes is assigned and carries a valid UMI)
    lib, fq, run, umi = DC.shape(name)
    index = {s.encode(): f for f, s in enumerate(lib)}
    seen = collections.Counter((index[s[:20]], s[20:28]) for s, _ in UC.records(fq))
    code = lambda u: sum(b"ACGT".index(ch) << (2 * j) for j, ch in enumerate(u))
    assert sorted((f, code(u), n) for (f, u), n in seen.items()) == DC.expected_pairs(name)


def test_count_collapse_count_more_collapse_equals_a_fresh_context(P):
    lib, fq, run, umi = DC.shape("ones")
    parts = CC.pieces(fq, 16000)
    assert len(parts) >= 3
    zeros = ([0] * len(lib), 0, 0, 0, 0)
    with P.Counter(features=lib, umi=umi, umi_reads=True, **run) as c:
        assert directional(c) == zeros and pairs(c) == []            # nothing counted yet
        seen = []
        for part in parts:
            assert c.count_block(part) == len(part)
            seen.append(directional(c))
        assert seen[-1] == DC.expected("ones") and seen[0] != seen[-1]
        first = DC.expect(lib, parts[0], umi, **run)
        assert seen[0] == first
        c.reset()
        assert directional(c) == zeros and pairs(c) == [] and cluster(c) == zeros[:3]
        assert c.count_block(parts[0]) == len(parts[0])
        assert directional(c) == first
        assert pairs(c) == DC.pair_table(lib, parts[0], umi, **run)


def test_keeping_reads_changes_nothing_else(P):
    lib, fq, run, umi = DC.shape("twice")
    seen = []
    for keep in (False, True):
        with P.Counter(features=lib, umi=umi, umi_reads=keep, **run) as c:
            assert c.count_block(fq) == len(fq)
            seen.append(state(c))
    assert seen[0] == seen[1] and seen[0][3] == DC.expected("twice")[4]


def test_the_refusals(P):
    lib = DC.shape("known")[0][:8]
    with P.Counter(features=lib, umi=(20, 4)) as c:                  # reads not kept
        for call in (c.collapse_umis_directional, c.umi_pairs, lambda: c.collapse_umis(1, rule="directional")):
            with pytest.raises(binding.F2QError) as exc:
                call()
            assert exc.value.code == -7
        with pytest.raises(ValueError):
            c.collapse_umis(1, rule="adjacency")
        fq = DC.shape("known")[1]
        assert c.count_block(fq) == len(fq)
        with pytest.raises(binding.F2QError) as exc:                 # after counting
            c.set_umi_reads(True)
        assert exc.value.code == -7
    with P.Counter(features=lib) as c:                               # without f2q_set_umi
        for call in (lambda: c.set_umi_reads(True), c.collapse_umis_directional, c.umi_pairs):
            with pytest.raises(binding.F2QError) as exc:
                call()
            assert exc.value.code == -7
    with pytest.raises(binding.F2QError) as exc:
        P.Counter(features=lib, umi_reads=True)
    assert exc.value.code == -7


# ---- the command line ------------------------------------------------------------------------------------------------
def _table(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


def test_cli_outputs_and_refusals(P, tmp_path, capsys):
    lib = UC.library()
    samples = {"s1": DC.shape("known")[1], "s2": DC.shape("twice")[1][:600000]}
    samples["s2"] = samples["s2"][:samples["s2"].rindex(b"\n@r") + 1]
    indir = tmp_path / "in"
    indir.mkdir()
    for name, fq in samples.items():
        (indir / (name + ".fastq")).write_bytes(fq)
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    outs = {}
    for tag, extra in (("dir", ["--mur", "directional"]), ("mu", []), ("cluster", ["--mur", "cluster"])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(out), "--st", "0", "--l", "20", "--m", "1", "--pb",
                     "--umi", "20,8", "--mu", "1", "--k"] + extra)
        (outs[tag],) = [d for d in out.iterdir() if d.is_dir()]
    capsys.readouterr()
    run = dict(miss=1, **UC.RUN)
    want = {name: DC.expect(lib, fq, (20, 8), **run) for name, fq in samples.items()}
    clus = {name: CC.expect(lib, fq, (20, 8), **run) for name, fq in samples.items()}
    assert any(a != b for n in samples for a, b in zip(want[n][0], clus[n][0]))            # the two rules differ on this input
    # every file of the run without the flag is in the run with it, byte for byte; the running times aside
    numbers = lambda t: [r[:1] + r[3:] for r in t if r and not r[0].startswith("#cmd used")]
    new_files = {"compiled_umi_directional.csv", "s1_umi_pairs.csv", "s2_umi_pairs.csv"}
    assert {p.name for p in outs["dir"].iterdir()} == {p.name for p in outs["mu"].iterdir()} | new_files
    assert {p.name for p in outs["cluster"].iterdir()} == {p.name for p in outs["mu"].iterdir()}
    stats = {tag: _table(outs[tag] / "compiled_stats.csv") for tag in outs}
    for path in outs["mu"].iterdir():
        if path.name == "compiled_stats.csv":
            at = stats["dir"].index(fast2q.UMI_DIRECTIONAL_STATS_HEAD)
            kept = [r for r in stats["dir"][:at] if r != ["#UMI collapse rule: directional"]]
            assert numbers(kept) == numbers(stats["mu"]) == numbers(stats["cluster"])
        elif path.name.endswith("_umi_reads.csv"):
            assert [r[:4] for r in _table(outs["dir"] / path.name)] == _table(path) == _table(outs["cluster"] / path.name)
        elif path.name.endswith("_reads.csv"):                       # (its first line holds the running time)
            assert _table(outs["dir"] / path.name)[1:] == _table(path)[1:]
        elif path.suffix == ".csv":
            assert (outs["dir"] / path.name).read_bytes() == path.read_bytes() == (outs["cluster"] / path.name).read_bytes()
    names = [f"g{i:03d}" for i in range(len(lib))]
    order = sorted(enumerate(names), key=lambda e: e[1])
    table, plain = _table(outs["dir"] / "compiled_umi_directional.csv"), _table(outs["dir"] / "compiled_umi.csv")
    assert table[0] == plain[0] == ["#Feature", "s1", "s2"] and [r[0] for r in table] == [r[0] for r in plain]
    assert table[1:] == [[n, str(want["s1"][0][i]), str(want["s2"][0][i])] for i, n in order]
    at = stats["dir"].index(fast2q.UMI_DIRECTIONAL_STATS_HEAD)
    assert at > stats["dir"].index(fast2q.UMI_COLLAPSE_STATS_HEAD) and fast2q.UMI_DIRECTIONAL_STATS_HEAD not in stats["mu"]
    assert stats["dir"][at + 1:] == [[n, str(want[n][1]), str(want[n][2]), str(want[n][3]), str(sum(want[n][0])), str(want[n][4])] for n in ("s1", "s2")]
    assert ["#UMI collapse rule: directional"] in stats["dir"] and not any(r and r[0].startswith("#UMI collapse rule") for r in stats["mu"] + stats["cluster"])
    for name, fq in samples.items():
        kept = _table(outs["dir"] / (name + "_umi_reads.csv"))
        assert kept[0] == ["#Feature", "Reads", "UMIs", "Molecules", "Directional"]
        assert [r[4] for r in kept[1:]] == [str(want[name][0][i]) for i, n in order] and [r[3] for r in kept[1:]] == [str(clus[name][0][i]) for i, n in order]
        dump = _table(outs["dir"] / (name + "_umi_pairs.csv"))
        assert dump[0] == ["#Feature", "UMI", "Reads"]
        assert dump[1:] == [[names[f], CC.text_of(c, 8).decode(), str(n)] for f, c, n in DC.pair_table(lib, fq, (20, 8), **run)]
    # the refusals leave no output directory
    base = ["-c", "--s", str(indir), "--g", str(guides), "--o", str(tmp_path / "never")]
    for extra in (["--mur", "directional"], ["--umi", "20,8", "--mur", "directional"], ["--umi", "20,8", "--mu", "1", "--mur", "adjacency"],
                  ["--umi", "20,8", "--mu", "0", "--mur", "directional"]):
        with pytest.raises(SystemExit):
            fast2q.main(base + extra)
        said = capsys.readouterr().out
        assert "FATAL" in said and "--mur" in said
    assert not (tmp_path / "never").exists()
