"""Extract+Count keys one base apart collapsed on the device: f2q_ec_collapse / f2q_ec_fetch_collapsed against the
plain-Python rule of tests/ec_collapse_cases.py, key for key -- centroid text, cluster reads, the four counters -- in the
wave-cooperative layout and under F2Q_ECC_LINK=lane."""
import csv
import importlib

import pytest

import ec_collapse_cases as EC
from conftest import pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")
EINVAL, ESTATE = -1, -7
LAYOUTS = ("wave", "lane")


@pytest.fixture(scope="module")
def P():
    return pkg()


def collapse(P, monkeypatch, layout, run, fq, ratio, dist=1):
    """(rows, extra) of one context that counts fq and collapses it in the named layout"""
    monkeypatch.setenv("F2Q_ECC_LINK", layout)
    with P.Counter(mode="EC", **run) as c:
        assert c.count_block(fq) == len(fq)
        extra, t = c.ec_collapse(dist, ratio, want_timing=True)
        rows = c.ec_collapsed()
        plain = c.ec_results()
    assert [r[:3] for r in rows] == plain                      # f2q_ec_fetch's keys, reads and order
    return rows, extra, t


def both_layouts(P, monkeypatch, name):
    run, table, ratio, fq = EC.shapes()[name]
    got = {}
    for layout in LAYOUTS:
        rows, extra, t = collapse(P, monkeypatch, layout, run, fq, ratio)
        want = EC.check(rows, extra, table, ratio)
        got[layout] = (rows, extra)
    assert got["wave"] == got["lane"]
    return want, t


@pytest.mark.parametrize("name", ["len1", "len21", "len21_r2", "len22", "len22_r2", "len29", "len29_r2"])
def test_lengths(P, monkeypatch, name):
    (_cent, extra), t = both_layouts(P, monkeypatch, name)
    assert extra["absorbed_keys"] >= 3 and t["launches"] == 2 and t["kernel_ms"] > 0


def test_different_lengths_sharing_codes_do_not_join(P, monkeypatch):
    (cent, _extra), _t = both_layouts(P, monkeypatch, "lengths_share_codes")
    assert cent["ACGA"] == ("ACGC", 0) and cent["AAGA"] == ("AAGA", 1) and cent["ACG"] == ("ACG", 105)


@pytest.mark.parametrize("ratio", [2, 255])
def test_boundaries(P, monkeypatch, ratio):
    (cent, extra), _t = both_layouts(P, monkeypatch, "boundary_r%d" % ratio)
    assert extra["absorbed_keys"] == 1 and extra["absorbed_reads"] == 3
    assert sorted(v[1] for v in cent.values()) == [0, 2, 2 * ratio - 1, 3 * ratio + 3]


def test_ties(P, monkeypatch):
    (cent, _extra), _t = both_layouts(P, monkeypatch, "ties")
    assert cent["AAAAAAAA"][0] == "CAAAAAAA" and cent["GGGGGGGG"][0] == "GGGCGGGG"


def test_chains(P, monkeypatch):
    (cent, extra), _t = both_layouts(P, monkeypatch, "chains")
    assert extra["longest_chain"] == 6 and sorted(v[1] for v in cent.values() if v[1]) == [3, 7, 127]


def test_keys_that_are_not_eligible(P, monkeypatch):
    (cent, _extra), _t = both_layouts(P, monkeypatch, "n_keys")
    assert cent["ACGTNCGT"] == ("ACGTNCGT", 50) and cent["ACGTACGT"] == ("ACGTACGT", 3)
    run, table, ratio, fq = EC.shapes()["len30"]
    for layout in LAYOUTS:                                      # everything in the byte-string table: nothing to walk
        rows, extra, t = collapse(P, monkeypatch, layout, run, fq, ratio)
        EC.check(rows, extra, table, ratio)
        assert not any(extra.values()) and t["launches"] == 0 and all(r[3] == r[0] and r[4] == r[1] for r in rows)


def test_empty_table_dist_0_and_bad_arguments(P, monkeypatch):
    run, table, ratio, fq = EC.shapes()["len21"]
    with P.Counter(mode="EC", **run) as c:
        with pytest.raises(binding.F2QError) as exc:
            c.ec_collapsed()                                    # never called
        assert exc.value.code == ESTATE
        assert not any(c.ec_collapse().values()) and c.ec_collapsed() == []
        c.count_block(fq)
        for dist, r in ((2, 5), (-1, 5), (1, 1), (1, 256), (1, 0)):
            with pytest.raises(binding.F2QError) as exc:
                c.ec_collapse(dist, r)
            assert exc.value.code == EINVAL
        extra = c.ec_collapse(0, ratio)
        EC.check(c.ec_collapsed(), extra, table, ratio, dist=0)
        assert not any(extra.values())
    with P.Counter(features=["ACGTACGTACGTACGTACGT"], miss=1) as c:
        for call in (c.ec_collapse, c.ec_collapsed):
            with pytest.raises(binding.F2QError) as exc:
                call()
            assert exc.value.code == ESTATE


def test_a_table_that_has_grown_between_two_counting_calls(P, monkeypatch, capfd):
    run, blocks, tables, wants = EC.growth()
    monkeypatch.setenv("F2Q_TRACE", "1")
    for layout in LAYOUTS:
        monkeypatch.setenv("F2Q_ECC_LINK", layout)
        with P.Counter(mode="EC", **run) as c:
            c.count_block(blocks[0])
            capfd.readouterr()
            extra = c.ec_collapse()
            EC.check(c.ec_collapsed(), extra, tables[0], 5, want=wants[0])
            c.count_block(blocks[1])
            assert "tables grow (single-word" in capfd.readouterr().err
            with pytest.raises(binding.F2QError) as exc:
                c.ec_collapsed()                                # the arrays of the first call are stale
            assert exc.value.code == ESTATE
            extra = c.ec_collapse()
            _want, want_extra = EC.check(c.ec_collapsed(), extra, tables[1], 5, want=wants[1])
            assert want_extra["absorbed_keys"] >= 50 and len(tables[1]) > 98304 > len(tables[0])
            c.reset()
            with pytest.raises(binding.F2QError) as exc:
                c.ec_collapsed()
            assert exc.value.code == ESTATE


def test_both_counting_roads_into_the_same_table(P, monkeypatch):
    run, table, ratio, fq = EC.shapes()["roads"]
    monkeypatch.setenv("F2Q_HOT_LEARN", "2048")
    hot = collapse(P, monkeypatch, "wave", run, fq, ratio)[:2]
    EC.check(hot[0], hot[1], table, ratio)
    monkeypatch.setenv("F2Q_NO_HOT", "1")
    cold = collapse(P, monkeypatch, "wave", run, fq, ratio)[:2]
    monkeypatch.setenv("F2Q_FORCE_GENERAL", "1")
    general = collapse(P, monkeypatch, "lane", run, fq, ratio)[:2]
    assert hot == cold == general


def test_repeated_calls_change_nothing_another_call_reads(P, monkeypatch):
    run, table, ratio, fq = EC.shapes()["roads"]
    lib = sorted(table, key=table.get)[-8:]
    with P.Counter(mode="EC", miss=1, **run) as c:
        c.set_assign_library(lib)
        c.count_block(fq)
        plain = c.ec_results()
        counts, stats = c.ec_assign()
        assigned = c.ec_assigned()
        a = (c.ec_collapse(1, ratio), c.ec_collapsed())
        b = (c.ec_collapse(1, ratio), c.ec_collapsed())
        assert a == b
        EC.check(a[1], a[0], table, ratio)
        assert c.ec_results() == plain and c.ec_assigned() == assigned
        counts2, stats2 = c.ec_assign()
        assert list(counts2) == list(counts) and list(stats2) == list(stats) and c.ec_assigned() == assigned
        other = c.ec_collapse(1, 2)                             # afresh: another ratio is not added to the last result
        EC.check(c.ec_collapsed(), other, table, 2)


def _run_cli(tmp_path, name, argv):
    out = tmp_path / name
    out.mkdir()
    fast2q.main(["-c", "--s", str(tmp_path / "in"), "--o", str(out), "--pb", "--mo", "EC"] + argv)
    (run_dir,) = [d for d in out.iterdir() if d.is_dir()]
    return run_dir


def _csv(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


def test_command_line_two_samples(P, tmp_path):
    run, table_a, _ratio, fq_a = EC.shapes()["len21"]
    _run, table_b, _ratio, fq_b = EC.shapes()["len21_r2"]
    shared = dict(list(table_a.items())[:40])                   # sample B also holds keys of sample A, with their reads
    table_b = dict(table_b, **shared)
    fq_b = EC.fastq_of_table(table_b, seed=5)
    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "sampleA.fastq").write_bytes(fq_a)
    (tmp_path / "in" / "sampleB.fastq").write_bytes(fq_b)
    common = ["--st", "0", "--l", "21"]
    plain = _run_cli(tmp_path, "plain", common)
    zero = _run_cli(tmp_path, "zero", common + ["--ecm", "0"])
    coll = _run_cli(tmp_path, "coll", common + ["--ecm", "1", "--ecr", "3"])
    new = ("sampleA_clusters.csv", "sampleB_clusters.csv", "compiled_collapsed.csv")
    files = lambda d: {p.name: p.read_bytes() for p in d.iterdir() if p.suffix == ".csv"}
    timed = lambda rows: [r[:1] + r[3:] if r and r[0].startswith("sample") and len(r) == 9 else r for r in rows]   # (the running time of a sample)
    assert sorted(p.name for p in zero.iterdir()) == sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in coll.iterdir()) == sorted([p.name for p in plain.iterdir()] + list(new))
    for d in (zero, coll):
        assert {k: v for k, v in files(d).items() if k not in new + ("compiled_stats.csv",)} == \
               {k: v for k, v in files(plain).items() if k != "compiled_stats.csv"}
    line = ["#Extracted sequences collapsed, mismatches, ratio: 1,3"]
    # (the recorded command line names the output directory, a sample's row its running time)
    old = lambda rows: timed([r for r in rows if not r[0].startswith("#cmd used") and r != line])
    assert old(_csv(zero / "compiled_stats.csv")) == old(_csv(plain / "compiled_stats.csv"))
    assert "--ecm" not in (zero / "compiled_stats.csv").read_text()
    stats = _csv(coll / "compiled_stats.csv")
    head = stats.index(fast2q.EC_COLLAPSE_STATS_HEAD)
    assert line in stats[:head] and len(stats) == head + 3
    assert old(stats[:head]) == old(_csv(plain / "compiled_stats.csv"))
    compiled = {}
    for column, (sample, table, fq) in enumerate((("sampleA", table_a, fq_a), ("sampleB", table_b, fq_b))):
        want, extra = EC.ec_collapse(table, 3)
        with P.Counter(mode="EC", **run) as c:                  # the first-occurrence order of the sample's keys
            c.count_block(fq)
            order = [r[0] for r in c.ec_results()]
        rows = _csv(coll / f"{sample}_clusters.csv")
        assert rows[0] == ["#key", "reads", "centroid", "cluster_reads"]
        assert rows[1:] == [[k, str(table[k]), want[k][0], str(want[k][1])] for k in order]
        n_cent = sum(1 for k in table if want[k][0] == k)
        assert stats[head + 1 + column] == [sample] + [str(x) for x in (len(table), extra["eligible_keys"], extra["absorbed_keys"], n_cent,
                                                                       extra["absorbed_reads"], extra["longest_chain"])]
        for k in table:
            if want[k][0] == k:
                compiled.setdefault(k, [0, 0])[column] = want[k][1]
    got = _csv(coll / "compiled_collapsed.csv")
    assert got[0] == ["#Feature", "sampleA", "sampleB"]
    assert {r[0]: [int(r[1]), int(r[2])] for r in got[1:]} == compiled and len(got) - 1 == len(compiled)
    assert any(a and b for a, b in compiled.values()) and any(not a for a, b in compiled.values()) and any(not b for a, b in compiled.values())
    # the ordering rule of <fn>.csv: the samples in name order, a sequence where it is first met in a sample's sorted rows
    expected_order = []
    for table in (table_a, table_b):
        want, _ = EC.ec_collapse(table, 3)
        expected_order += [k for k in sorted(table) if want[k][0] == k and k not in expected_order]
    assert [r[0] for r in got[1:]] == expected_order
