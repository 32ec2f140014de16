"""--mu 1 on the device: f2q_umi_collapse (k_umi_uf_init / k_umi_link / k_umi_roots over the (feature, UMI) set) against
the plain-Python expectation of tests/umi_collapse_cases.py, its argument and state errors, what it leaves untouched,
and the command line's outputs."""
import csv
import importlib
import re

import pytest

import umi_collapse_cases as CC
from conftest import pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")


@pytest.fixture(scope="module")
def P():
    return pkg()


def collapse(c, dist=1):
    molecules, pairs, edges = c.collapse_umis(dist)
    return list(molecules), pairs, edges


def state(c):
    counts, stats = c.read_counts()
    umis, ok, bad = c.read_umis()
    return list(counts), list(stats), list(umis), ok, bad


def collapsed(P, name, per=0):
    """the shape counted (in pieces of `per` records) and collapsed twice; read_counts / read_umis around the collapse"""
    lib, fq, run, umi = CC.shape(name)
    with P.Counter(features=lib, umi=umi, **run) as c:
        for piece in (CC.pieces(fq, per) if per else [fq]):
            assert c.count_block(piece) == len(piece)
        before = state(c)
        got = collapse(c)
        assert collapse(c) == got                                    # calling twice
        assert state(c) == before                                    # nothing another call reads has changed
        assert collapse(c, 0) == (before[2], sum(before[2]), 0)      # the identity case: read_umis()
    return got, before[2]


def test_known_answers(P):
    got, umis = collapsed(P, "known")
    assert got == CC.known()[4] == CC.expected("known")
    assert got[1:] == (262, 1538) and got[0][:4] == [1, 2, 1, 1] and umis[:4] == [256, 3, 2, 1]


@pytest.mark.parametrize("length", [1, 2])
def test_one_and_two_base_umis(P, length):
    got, umis = collapsed(P, "short%d" % length)
    assert got == CC.expected("short%d" % length)
    if length == 1:
        assert got[0] == [min(n, 1) for n in umis] and max(umis) > 1


def test_sixteen_base_umis_next_to_wide_feature_indices(P):
    got, umis = collapsed(P, "wide")
    assert got == CC.expected("wide")
    assert sum(got[0][:512]) == 0 and got[2] > 0 and any(m < n for m, n in zip(got[0], umis))


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
@pytest.mark.parametrize("name", ["short1", "wide"])
def test_launch_geometry(P, monkeypatch, capfd, name, wg, grid, used):
    """the linking launch under every geometry the switches can give, on the shapes that bound 3L: one-base UMIs (3L = 3:
    21 groups a round, lane 63 idle) and sixteen-base ones (3L = 48: one group, 16 lanes idle).  The first set has
    65 536 slots: 64 x 1 strides over it many times (at most 1 024 workgroups of one wave would cover it once, and the
    grid is one per CU)"""
    set_geometry(monkeypatch, wg, grid)
    got, _ = collapsed(P, name)
    assert got == CC.expected(name)
    tails = re.findall(r"\[f2q trace\] UMI collapse: (\d+) pairs, (\d+) edges, (\d+) molecules, [\d.]+ ms \([^;]*; wave, (\d+) x (\d+)\)", capfd.readouterr().err)
    assert len(tails) == 3 and tails[2][3:] == ("0", str(used))      # (the third call is the identity case: no launch)
    for pairs, edges, molecules, glink, wgsize in tails[:2]:
        assert (int(pairs), int(edges), int(molecules), int(wgsize)) == (got[1], got[2], sum(got[0]), used)
        assert 1 <= int(glink) and int(glink) * used <= 65536 and (int(glink) * used < 65536) == (wg == "64")


def test_a_set_smaller_than_one_wave(P, monkeypatch, capfd):
    """a dozen records from a first set of 2 slots leave 32 slots: `base + lane < slots` cuts the one wave that has work,
    the other waves of the workgroup find none"""
    monkeypatch.setenv("F2Q_TRACE", "1")
    monkeypatch.setenv("F2Q_UMI_SLOTS", "2")
    got, umis = collapsed(P, "tiny")
    assert got == CC.TINY_WANT == CC.expected("tiny") and umis == [3, 2]
    said = capfd.readouterr().err
    assert re.findall(r"\[f2q trace\] UMI set: (\d+) slots, (\d+) rehashes", said) == [("32", "0")], said      # the smallest power of two >= 2 x 11
    assert re.findall(r"; wave, (\d+) x (\d+)\)", said)[:2] == [("1", "256")] * 2


@pytest.mark.parametrize("layout", ["first_set", "rehashed", "lane_per_slot"])
def test_contention(P, monkeypatch, capfd, layout):
    """every union of feature 7 lands in one tree; 'rehashed': a first set of 64 slots fed in pieces of 30 records"""
    want = CC.expected("contention")
    assert want[0][CC.GRAY_FEATURE] == 1 and want[2] > CC.CONTENTION_WANT[2] and want[1] > CC.CONTENTION_WANT[1]
    monkeypatch.setenv("F2Q_TRACE", "1")
    if layout == "rehashed":
        monkeypatch.setenv("F2Q_UMI_SLOTS", "64")
    if layout == "lane_per_slot":
        monkeypatch.setenv("F2Q_UMI_LINK", "lane")
    got, _ = collapsed(P, "contention", 30 if layout == "rehashed" else 0)
    assert got == want
    said = capfd.readouterr().err
    lines = re.findall(r"\[f2q trace\] UMI collapse: (\d+) pairs, (\d+) edges, (\d+) molecules, [\d.]+ ms", said)
    assert lines[:2] == [(str(want[1]), str(want[2]), str(sum(want[0])))] * 2, said
    assert (len(re.findall(r"\[f2q trace\] UMI set rehash \d+:", said)) >= 5) == (layout == "rehashed")
    assert ("lane," in said) == (layout == "lane_per_slot")


def test_count_collapse_count_more_collapse_equals_a_fresh_context(P):
    lib, fq, run, umi = CC.shape("contention")
    parts = CC.pieces(fq, 12000)
    assert len(parts) >= 3
    with P.Counter(features=lib, umi=umi, **run) as c:
        seen = []
        for part in parts:
            assert c.count_block(part) == len(part)
            seen.append(collapse(c))
        assert seen[-1] == collapsed(P, "contention")[0] == CC.expected("contention") and seen[0] != seen[-1]
        first = CC.expect(lib, parts[0], umi, **run)
        assert seen[0] == first
        c.reset()
        assert collapse(c) == ([0] * len(lib), 0, 0) and collapse(c, 0) == ([0] * len(lib), 0, 0)
        assert c.count_block(parts[0]) == len(parts[0])
        assert collapse(c) == first


def test_nothing_counted_and_the_refusals(P):
    lib = CC.shape("known")[0][:8]
    with P.Counter(features=lib, umi=(20, 8)) as c:
        assert collapse(c) == ([0] * 8, 0, 0) and collapse(c, 0) == ([0] * 8, 0, 0)
        for dist in (2, -1):
            with pytest.raises(binding.F2QError) as exc:
                c.collapse_umis(dist)
            assert exc.value.code == -1
    with P.Counter(features=lib) as c:
        with pytest.raises(binding.F2QError) as exc:
            c.collapse_umis()
        assert exc.value.code == -7


# ---- the command line ------------------------------------------------------------------------------------------------
def _table(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


def test_cli_outputs_and_refusals(P, tmp_path, capsys):
    import umi_cases as UC
    lib = UC.library()
    samples = {"s1": UC.base()[1], "s2": CC.shape("contention")[1][:600000]}
    samples["s2"] = samples["s2"][:samples["s2"].rindex(b"\n@r") + 1]
    indir = tmp_path / "in"
    indir.mkdir()
    for name, fq in samples.items():
        (indir / (name + ".fastq")).write_bytes(fq)
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    outs = {}
    for tag, extra in (("mu", ["--umi", "20,8", "--mu", "1", "--k"]), ("umi", ["--umi", "20,8", "--k"]), ("mu0", ["--umi", "20,8", "--mu", "0", "--k"])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(out), "--st", "0", "--l", "20", "--m", "1", "--pb"] + extra)
        (outs[tag],) = [d for d in out.iterdir() if d.is_dir()]
    capsys.readouterr()
    for name in ("compiled.csv", "compiled_umi.csv"):
        assert (outs["mu"] / name).read_bytes() == (outs["umi"] / name).read_bytes() == (outs["mu0"] / name).read_bytes()
    for tag in ("umi", "mu0"):                                       # --mu 0 is a run without the flag
        assert not (outs[tag] / "compiled_umi_collapsed.csv").exists()
        assert _table(outs[tag] / "s1_umi_reads.csv")[0] == ["#Feature", "Reads", "UMIs"]
        assert (outs[tag] / "s1_umi_reads.csv").read_bytes() == (outs["umi"] / "s1_umi_reads.csv").read_bytes()
    run = dict(miss=1, **UC.RUN)
    want = {name: CC.expect(lib, fq, (20, 8), **run) for name, fq in samples.items()}
    umis = {name: UC.expect(lib, fq, (20, 8), **run) for name, fq in samples.items()}
    assert any(m < n for m, n in zip(want["s1"][0], umis["s1"][2])) or any(m < n for m, n in zip(want["s2"][0], umis["s2"][2]))
    names = [f"g{i:03d}" for i in range(len(lib))]
    order = sorted(enumerate(names), key=lambda e: e[1])
    table, plain = _table(outs["mu"] / "compiled_umi_collapsed.csv"), _table(outs["mu"] / "compiled_umi.csv")
    assert table[0] == plain[0] == ["#Feature", "s1", "s2"] and [r[0] for r in table] == [r[0] for r in plain]
    assert table[1:] == [[n, str(want["s1"][0][i]), str(want["s2"][0][i])] for i, n in order]
    stats, ustats = _table(outs["mu"] / "compiled_stats.csv"), _table(outs["umi"] / "compiled_stats.csv")
    at = stats.index(fast2q.UMI_COLLAPSE_STATS_HEAD)
    assert at > stats.index(fast2q.UMI_STATS_HEAD) and fast2q.UMI_COLLAPSE_STATS_HEAD not in ustats
    assert stats[at + 1:] == [[n, str(want[n][1]), str(want[n][2]), str(sum(want[n][0]))] for n in ("s1", "s2")]
    assert ["#UMI mismatches collapsed: 1"] in stats and not any(r and r[0].startswith("#UMI mismatches") for r in ustats)
    numbers = lambda t: [r[:1] + r[3:] for r in t if r and not r[0].startswith("#")]      # (not the running times)
    assert numbers(stats[:at]) == numbers(ustats)
    for name in samples:
        kept = _table(outs["mu"] / (name + "_umi_reads.csv"))
        assert kept[0] == ["#Feature", "Reads", "UMIs", "Molecules"]
        assert kept[1:] == [[n, str(umis[name][0][i]), str(umis[name][2][i]), str(want[name][0][i])] for i, n in order]
        assert [r[:3] for r in kept] == _table(outs["umi"] / (name + "_umi_reads.csv"))
    # the two refusals leave no output directory
    base = ["-c", "--s", str(indir), "--g", str(guides), "--o", str(tmp_path / "never")]
    for extra in (["--mu", "1"], ["--umi", "20,8", "--mu", "2"]):
        with pytest.raises(SystemExit):
            fast2q.main(base + extra)
        said = capsys.readouterr().out
        assert "FATAL" in said and "--mu" in said
    assert not (tmp_path / "never").exists()
