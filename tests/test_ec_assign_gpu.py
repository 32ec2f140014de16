"""Extract+Count with a library on the device: f2q_set_assign_library / f2q_ec_assign / f2q_ec_fetch_assigned against
the oracle in Counter mode (tests/assign_cases.py): the count vector and the five counters over the same FASTQ bytes,
and every key's feature and distance."""
import csv
import importlib

import pytest

import assign_cases as AC
import paired_cases as PC
from conftest import pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")
ESTATE = -7


@pytest.fixture(scope="module")
def P():
    return pkg()


def assign(P, lib, fq, miss, **run):
    with P.Counter(mode="EC", miss=miss, **run) as c:
        c.set_assign_library(lib)
        assert c.count_block(fq) == len(fq)
        counts, stats, t = c.ec_assign(want_timing=True)
        rows = c.ec_assigned()
        plain = c.ec_results()
    assert [r[:3] for r in rows] == plain and t["launches"] >= 1 and t["kernel_ms"] > 0
    return list(counts), list(stats), rows


def check(P, lib, fq, miss, run):
    want = AC.aggregate(lib, fq, miss, **run)
    counts, stats, rows = assign(P, lib, fq, miss, **run)
    assert (counts, stats) == want
    AC.check_rows(lib, rows, counts, stats, miss)
    return counts, stats, rows


@pytest.mark.parametrize("miss", [0, 1, 2, 3])
def test_fixed_window_both_tables_every_key_form(P, miss):
    lib, fq, run, _ = AC.fixed_window()
    _, stats, rows = check(P, lib, fq, miss, run)
    keys = [r[0] for r in rows]
    plain = [k for k in keys if set(k) <= set("ACGT")]
    assert "" in keys and any(len(k) == 18 for k in plain) and any(len(k) == 20 for k in plain)          # single-word table
    assert any(1 <= k.count("N") <= 3 and set(k) <= set("ACGTN") for k in keys)
    assert any(k.count("N") >= 4 for k in keys) and any(set(k) & set("RY.") for k in keys)              # byte-string table
    assert stats[1] > 0 and stats[3] > 0 and stats[4] > 0 and (miss == 0 or stats[2] > 0)


@pytest.mark.parametrize("miss", [1, 2, 3])
def test_ties_are_unassigned_and_the_nearer_feature_wins(P, miss):
    lib, fq, run, _, mids, near = AC.ties()
    _, stats, rows = check(P, lib, fq, miss, run)
    got = {r[0]: (r[3], r[4]) for r in rows}
    for m in mids:
        assert got[m.decode()] == (-1, -1)
    for key, f in near:
        assert got[key.decode()] == (f, 1)
    assert stats[3] >= sum(r[1] for r in rows if r[0].encode() in mids) > 0


@pytest.mark.parametrize("miss", [0, 1, 2])
def test_irregular_library(P, miss):
    lib, fq, run, _ = AC.irregular()
    _, _, rows = check(P, lib, fq, miss, run)
    assert {len(lib[r[3]]) for r in rows if r[3] >= 0} == {18, 20, 24, 36}
    assert any(r[3] >= 0 and "N" in lib[r[3]] for r in rows)


@pytest.mark.parametrize("miss", [0, 1, 2])
def test_two_windows_joined_and_single_part_keys(P, miss):
    lib, fq, run, _ = AC.two_windows()
    _, _, rows = check(P, lib, fq, miss, run)
    assert any(":" in r[0] and r[3] >= 0 for r in rows) and any(":" not in r[0] and r[3] >= 0 for r in rows)
    assert any("N" in r[0] for r in rows)


@pytest.mark.parametrize("miss", [0, 1, 2])
def test_anchored_hot_keys_in_lds_and_without(P, monkeypatch, miss):
    lib, fq, run, _ = AC.anchored()
    monkeypatch.setenv("F2Q_HOT_LEARN", "4096")
    hot = check(P, lib, fq, miss, run)
    monkeypatch.setenv("F2Q_NO_HOT", "1")
    cold = assign(P, lib, fq, miss, **run)
    assert cold == hot


def test_growth_staleness_idempotence_and_reset(P, monkeypatch):
    lib, blocks, run = AC.growth()
    monkeypatch.setenv("F2Q_EC_STEP", "4096")
    with P.Counter(mode="EC", miss=1, **run) as c:
        c.set_assign_library(lib)
        c.count_block(blocks[0])
        first = c.ec_assign()
        assert (list(first[0]), list(first[1])) == AC.aggregate(lib, blocks[0], 1, **run)
        n1 = len(c.ec_assigned())
        c.count_block(blocks[1])
        with pytest.raises(binding.F2QError) as exc:
            c.ec_assigned()
        assert exc.value.code == ESTATE
        a = c.ec_assign()
        rows_a = c.ec_assigned()
        b = c.ec_assign()
        rows_b = c.ec_assigned()
        assert (list(a[0]), list(a[1])) == AC.aggregate(lib, blocks[0] + blocks[1], 1, **run)        # not doubled
        assert (list(b[0]), list(b[1])) == (list(a[0]), list(a[1])) and rows_a == rows_b
        assert len(rows_a) >= 20000 > n1 > 0
        by_feature = [0] * len(lib)
        for _key, n, _first, f, _d in rows_a:
            if f >= 0:
                by_feature[f] += n
        assert by_feature == list(a[0])
        c.reset()
        with pytest.raises(binding.F2QError) as exc:
            c.ec_assigned()
        assert exc.value.code == ESTATE
        c.count_block(blocks[2])
        third = c.ec_assign()
        assert (list(third[0]), list(third[1])) == AC.aggregate(lib, blocks[2], 1, **run)


@pytest.mark.parametrize("rc2", [False, True], ids=["fwd", "rc2"])
@pytest.mark.parametrize("miss", [0, 1, 2])
def test_paired_context(P, miss, rc2):
    st1, st2, length = [0, 40], [12], 7
    lib = PC.pair_library(300, length, len(st1), len(st2), 5, combinatorial=True)
    fq1, fq2 = PC.make_pairs(lib, length, st1, st2, rc2, 4000, seed=40 + miss, ragged=True, dirty=True)
    counts, stats, uncovered = PC.pair_oracle(lib, fq1, fq2, st1, st2, length, rc2, miss)
    assert uncovered == 0 and stats[0] == 4000
    with P.Counter(mode="EC", miss=miss, length=length, start=",".join(map(str, st1)), start2=",".join(map(str, st2)), rc2=rc2) as c:
        c.set_assign_library(lib)
        assert c.count_block_paired(fq1, fq2) == (len(fq1), len(fq2))
        got, gstats = c.ec_assign()
        rows = c.ec_assigned()
    assert list(gstats) == stats and list(got) == counts
    AC.check_rows(lib, rows, got, gstats, miss)


def test_state_errors(P):
    lib = ["ACGTACGTACGTACGTACGT", "TTTTACGTACGTACGTACGA"]
    with P.Counter(features=lib, miss=1) as c:
        for call in (lambda: c.set_assign_library(lib), c.ec_assign, c.ec_assigned):
            with pytest.raises(binding.F2QError) as exc:
                call()
            assert exc.value.code == ESTATE
    with P.Counter(mode="EC", miss=1) as c:
        for call in (c.ec_assign, c.ec_assigned):
            with pytest.raises(binding.F2QError) as exc:
                call()
            assert exc.value.code == ESTATE
        c.set_assign_library(lib)
        with pytest.raises(binding.F2QError) as exc:
            c.set_assign_library(lib)
        assert exc.value.code == ESTATE
        counts, stats = c.ec_assign()                           # nothing counted yet: all zero, and fetchable
        assert list(counts) == [0, 0] and list(stats) == [0] * 5 and c.ec_assigned() == []


def _run_cli(tmp_path, name, argv):
    out = tmp_path / name
    out.mkdir()
    fast2q.main(["-c", "--s", str(tmp_path / "in"), "--o", str(out), "--pb"] + argv)
    (run_dir,) = [d for d in out.iterdir() if d.is_dir()]
    return run_dir


def _files(d):
    return {p.name: p.read_bytes() for p in sorted(d.iterdir()) if p.suffix == ".csv" and not p.name.endswith("_stats.csv")}


def test_command_line(P, tmp_path, monkeypatch, capsys):
    lib, fq, run, _ = AC.fixed_window()
    (tmp_path / "in").mkdir()
    cut = fq.index(b"\n@r1500\n") + 1
    (tmp_path / "in" / "sampleA.fastq").write_bytes(fq[:cut])
    (tmp_path / "in" / "sampleB.fastq").write_bytes(fq[cut:])
    guides = tmp_path / "lib.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    common = ["--st", run["start"], "--l", str(run["length"]), "--m", "2"]
    c_dir = _run_cli(tmp_path, "c", common + ["--g", str(guides)])
    as_dir = _run_cli(tmp_path, "as", common + ["--mo", "EC", "--as", "--g", str(guides)])
    ec_dir = _run_cli(tmp_path, "ec", common + ["--mo", "EC", "--g", str(guides)])
    assert (as_dir / "compiled_features.csv").read_bytes() == (c_dir / "compiled.csv").read_bytes()
    # without --as: the files and bytes of an Extract+Count run; with it the same plus the three new files
    assert sorted(p.name for p in ec_dir.iterdir()) == sorted(p.name for p in as_dir.iterdir()
                                                             if not p.name.endswith(("_assigned.csv", "_features.csv")))
    assert _files(ec_dir) == {k: v for k, v in _files(as_dir).items() if not k.endswith(("_assigned.csv", "_features.csv"))}
    names = [f"g{i:03d}" for i in range(len(lib))]
    for sample, text in (("sampleA", fq[:cut]), ("sampleB", fq[cut:])):
        _, _, rows = assign(P, lib, text, 2, **run)
        with open(as_dir / f"{sample}_assigned.csv", newline="") as h:
            table = list(csv.reader(h))
        assert table[0] == ["#key", "reads", "feature_name", "mismatches"]
        assert table[1:] == [[k, str(n), names[f] if f >= 0 else "", str(d)] for k, n, _first, f, d in rows]
    # the stats block of the --as run holds the derived counters: those of the Counter run
    pick = lambda d: [r[3:] for r in csv.reader(open(d / "compiled_stats.csv", newline="")) if r and r[0].startswith("sample")]
    assert pick(as_dir) == pick(c_dir) and pick(as_dir) != pick(ec_dir)
    capsys.readouterr()
    for argv, ranks in ((["--mo", "EC", "--as"], 1), (["--as", "--g", str(guides)], 1), (["--mo", "EC", "--as", "--g", str(guides)], 2)):
        if ranks > 1:                                           # (what WORLD_SIZE=2 makes of sharding.world(), without a second process)
            monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
        with pytest.raises(SystemExit):
            fast2q.main(["-c", "--s", str(tmp_path / "in"), "--o", str(tmp_path), "--pb"] + common + argv)
        monkeypatch.undo()
        assert "--as" in capsys.readouterr().out
