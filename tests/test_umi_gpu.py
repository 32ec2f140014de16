"""--umi on the device: f2q_set_umi / k_count_umi / f2q_read_umis against the plain-Python expectation of
tests/umi_cases.py (the oracle's Counter-mode verdict per read, the UMI rule, a set() per feature), through every
counting entry point, and the command line's outputs."""
import csv
import gzip
import importlib
import re

import pytest

import umi_cases as UC
from conftest import bgzf_bytes, pkg

pytestmark = pytest.mark.gpu
fast2q = importlib.import_module("2fast2q_amd.fast2q")
binding = importlib.import_module("2fast2q_amd.binding")


@pytest.fixture(scope="module")
def P():
    return pkg()


def result(c):
    counts, stats = c.read_counts()
    umis, ok, bad = c.read_umis()
    return list(counts), list(stats), list(umis), ok, bad


def counted(P, lib, fq, umi, **run):
    with P.Counter(features=lib, umi=umi, **run) as c:
        assert c.count_block(fq) == len(fq)
        return result(c)


def plain(P, lib, fq, **run):
    with P.Counter(features=lib, **run) as c:
        assert c.count_block(fq) == len(fq)
        counts, stats = c.read_counts()
    return list(counts), list(stats)


@pytest.mark.parametrize("miss", [0, 1])
def test_parity_with_the_expectation_and_with_a_plain_context(P, miss):
    lib, fq, run, umi = UC.base()
    want = UC.expect(lib, fq, umi, miss=miss, **run)
    got = counted(P, lib, fq, umi, miss=miss, **run)
    assert got == want
    assert got[:2] == plain(P, lib, fq, miss=miss, **run)
    assert got[3] + got[4] == got[1][1] + got[1][2] and sum(got[2]) < got[3] - 100


def test_invalid_umis_move_reads_between_the_two_counters(P):
    lib, fq, kinds = UC.invalid()
    valid_kinds = {"whole", "cut28", "lower", "q29_last", "lowq_outside"}
    for phred, also in ((30, set()), (0, {"lowq_first", "lowq_last"})):
        run = dict(miss=1, phred=phred, start="0", length=20)
        want = UC.expect(lib, fq, (UC.S, UC.L), **run)
        assert counted(P, lib, fq, (UC.S, UC.L), **run) == want
        n_ok = sum(k in valid_kinds | also for k in kinds)
        assert (want[3], want[4]) == (n_ok, len(kinds) - n_ok) and sum(want[2]) == n_ok


def test_imperfect_hits_share_the_feature_s_set(P):
    lib, fq, pairs = UC.imperfect()
    got = counted(P, lib, fq, (UC.S, UC.L), miss=1, **UC.RUN)
    assert got == UC.expect(lib, fq, (UC.S, UC.L), miss=1, **UC.RUN)
    assert {f: n for f, n in enumerate(got[2]) if n} == pairs and got[3] == 7 and got[1][2] == 5


def test_sixteen_base_umi_over_the_feature_window(P):
    lib, fq, run, umi = UC.wide()
    got = counted(P, lib, fq, umi, miss=1, **run)
    assert got == UC.expect(lib, fq, umi, miss=1, **run)
    assert sum(got[2][:512]) == 0 and got[2][600] >= 1 and got[2][601] >= 1 and max(got[2]) > 1


def test_anchored_run(P):
    lib, fq, run, umi = UC.anchored()
    got = counted(P, lib, fq, umi, miss=1, **run)
    assert got == UC.expect(lib, fq, umi, miss=1, **run)
    assert got[:2] == plain(P, lib, fq, miss=1, **run) and got[3] > 0 and got[4] > 0


def test_growth_from_a_small_set_changes_nothing(P, monkeypatch, capfd):
    lib, fq, run, umi = UC.base()
    monkeypatch.setenv("F2Q_UMI_SLOTS", "64")
    monkeypatch.setenv("F2Q_TRACE", "1")
    recs = fq.split(b"\n@r")
    recs = [recs[0] + b"\n"] + [b"@r" + r + b"\n" for r in recs[1:-1]] + [b"@r" + recs[-1]]
    with P.Counter(features=lib, umi=umi, miss=1, **run) as c:
        for i in range(0, len(recs), 30):
            piece = b"".join(recs[i:i + 30])
            assert c.count_block(piece) == len(piece)
        got = result(c)
    said = capfd.readouterr().err
    assert got == UC.expect(lib, fq, umi, miss=1, **run)
    assert len(re.findall(r"\[f2q trace\] UMI set rehash \d+:", said)) >= 5, said


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf", "bgzf_device_inflate"])
def test_streamed_files_equal_the_one_block_result(P, tmp_path, monkeypatch, kind):
    lib, fq, run, umi = UC.base()
    monkeypatch.setenv("F2Q_FILE_CHUNK", "4096")
    if kind == "bgzf_device_inflate":
        monkeypatch.setenv("F2Q_DEVICE_INFLATE", "1")
    path = tmp_path / {"plain": "s.fastq", "gzip": "s.fastq.gz"}.get(kind, "s.bgzf.fastq.gz")
    path.write_bytes(fq if kind == "plain" else gzip.compress(fq) if kind == "gzip" else bgzf_bytes(fq, block=3000))
    with P.Counter(features=lib, umi=umi, miss=1, **run) as c:
        _, truncated = c.count_file(str(path))
        got = result(c)
    assert not truncated and got == UC.expect(lib, fq, umi, miss=1, **run)


def test_resident_blocks_and_device_text(P):
    lib, fq, run, umi = UC.base()
    want = UC.expect(lib, fq, umi, miss=1, **run)
    with P.Counter(features=lib, umi=umi, miss=1, **run) as c:
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


def test_reset_and_reuse_match_fresh_contexts(P):
    lib, fq, run, umi = UC.base()
    fq2 = UC.sample(0x5EC0, n_reads=1500)
    with P.Counter(features=lib, umi=umi, miss=1, **run) as c:
        assert c.count_block(fq) == len(fq)
        first = result(c)
        c.reset()
        assert result(c) == ([0] * len(lib), [0] * 5, [0] * len(lib), 0, 0)
        assert c.count_block(fq2) == len(fq2)
        second = result(c)
    assert first == counted(P, lib, fq, umi, miss=1, **run) == UC.expect(lib, fq, umi, miss=1, **run)
    assert second == counted(P, lib, fq2, umi, miss=1, **run) == UC.expect(lib, fq2, umi, miss=1, **run)


def test_sharded_calls_refuse_a_umi_context(P, tmp_path):
    lib, fq, run, umi = UC.base()
    path = tmp_path / "s.fastq"
    path.write_bytes(fq[:20000])
    with P.Counter(features=lib, umi=umi, **run) as c:
        with pytest.raises(binding.F2QError) as exc:
            c.count_file_shard(str(path), 0, 2)
        assert exc.value.code == -7 and "ranks" in str(exc.value)


# ---- the command line ------------------------------------------------------------------------------------------------
def _table(path):
    with open(path, newline="") as h:
        return list(csv.reader(h))


def test_cli_outputs_and_refusals(P, tmp_path, monkeypatch, capsys):
    lib = UC.library()
    samples = {"s1": UC.base()[1], "s2": UC.sample(0x5EC0, n_reads=1500)}
    indir = tmp_path / "in"
    indir.mkdir()
    for name, fq in samples.items():
        (indir / (name + ".fastq")).write_bytes(fq)
    guides = tmp_path / "guides.csv"
    guides.write_text("".join(f"g{i:03d},{s}\n" for i, s in enumerate(lib)))
    outs = {}
    for tag, extra in (("umi", ["--umi", "20,8", "--k"]), ("plain", [])):
        out = tmp_path / ("out_" + tag)
        out.mkdir()
        fast2q.main(["-c", "--s", str(indir), "--g", str(guides), "--o", str(out), "--st", "0", "--l", "20", "--m", "1", "--pb"] + extra)
        (outs[tag],) = [d for d in out.iterdir() if d.is_dir()]
    capsys.readouterr()
    assert (outs["umi"] / "compiled.csv").read_bytes() == (outs["plain"] / "compiled.csv").read_bytes()
    assert not (outs["plain"] / "compiled_umi.csv").exists()
    want = {name: UC.expect(lib, fq, (20, 8), miss=1, **UC.RUN) for name, fq in samples.items()}
    names = [f"g{i:03d}" for i in range(len(lib))]
    reads, umis = _table(outs["umi"] / "compiled.csv"), _table(outs["umi"] / "compiled_umi.csv")
    assert umis[0] == reads[0] == ["#Feature", "s1", "s2"] and [r[0] for r in umis] == [r[0] for r in reads]
    assert umis[1:] == [[n, str(want["s1"][2][i]), str(want["s2"][2][i])] for i, n in sorted(enumerate(names), key=lambda e: e[1])]
    stats = _table(outs["umi"] / "compiled_stats.csv")
    at = stats.index(fast2q.UMI_STATS_HEAD)
    assert stats[at + 1:] == [[n, str(want[n][3]), str(want[n][4])] for n in ("s1", "s2")]
    assert ["#UMI start position in the read, length: 20,8"] in stats
    plain_stats = _table(outs["plain"] / "compiled_stats.csv")
    numbers = lambda t: [r[:1] + r[3:] for r in t if r and not r[0].startswith("#")]      # (not the running times)
    assert numbers(stats[:at]) == numbers(plain_stats) and len(numbers(plain_stats)) == 2
    for name in samples:
        kept = _table(outs["umi"] / (name + "_umi_reads.csv"))
        assert kept[0] == ["#Feature", "Reads", "UMIs"]
        assert kept[1:] == [[n, str(want[name][0][i]), str(want[name][2][i])] for i, n in sorted(enumerate(names), key=lambda e: e[1])]
    # the three refusals
    base = ["-c", "--s", str(indir), "--g", str(guides), "--o", str(tmp_path / "never"), "--umi", "20,8"]
    for extra, word in ((["--mo", "EC"], "--mo EC"), (["--pe", "--st2", "0"], "--pe")):
        with pytest.raises(SystemExit):
            fast2q.main(base + extra)
        said = capsys.readouterr().out
        assert "FATAL" in said and "--umi" in said and word in said
    monkeypatch.setattr(fast2q.sharding, "world", lambda: fast2q.sharding.World(0, 2, None))
    with pytest.raises(SystemExit):
        fast2q.main(base)
    said = capsys.readouterr().out
    assert "FATAL" in said and "--umi" in said and "several ranks" in said
    assert not (tmp_path / "never").exists()
