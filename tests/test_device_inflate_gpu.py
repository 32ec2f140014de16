"""GPU: BGZF members inflated on the device (k_inflate_bgzf) -- f2q_text_from_bgzf against zlib, damaged members, and
f2q_count_file with F2Q_DEVICE_INFLATE=1 against the host inflater on the same files."""
import csv
import gzip
import os
import random
import subprocess
import sys
import zlib

import pytest

import inflate_cases as IC
import synth
from conftest import ROOT, bgzf_bytes, case_fastq, load_cases, loader_view, pkg, sprinkle_symbols

pytestmark = pytest.mark.gpu

GUIDES = synth.make_library(120, 20, 47)


def corpus_texts():
    rng = random.Random(5)
    fq = sprinkle_symbols(synth.make_fastq(synth.Spec(seed=9, n_reads=1500, read_len=151), GUIDES), 2)
    return [fq[:65536], fq[:1], b"", bytes(rng.getrandbits(8) for _ in range(40000)), b"A" * 65536, b"ACGTTGCA" * 8192, fq[:30011]]


def members_text(ms):
    return b"".join(zlib.decompress(m[:-8], -15) for m in ms)


def test_text_from_bgzf_equals_zlib():
    texts = corpus_texts()
    ms = [IC.member(t, lv) for t in texts for lv in (0, 1, 6, 9)]
    for strat in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
        for t in texts:
            co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strat)
            ms.append(co.compress(t) + co.flush() + IC.trailer(t))
    ms = [m for m in ms if len(m) + 18 <= 65536]         # (a BGZF member holds at most 64 KiB: stored 64 KiB texts do not fit)
    with pkg().Counter(features=GUIDES) as c:
        dt, trunc = c.text_from_bgzf(IC.bgzf_wrap(ms))
        assert not trunc and dt.read() == members_text(ms)
        dt.free()


def test_text_from_bgzf_many_members():
    """over 10 000 members: many workgroups per CU, every alignment of a member's text in the output"""
    fq = synth.make_fastq(synth.Spec(seed=11, n_reads=60000, read_len=101), GUIDES)
    rng = random.Random(3)
    parts, i = [], 0
    while len(parts) < 10500:
        k = rng.randrange(0, 700)
        parts.append(fq[i:i + k]); i = (i + k) % (len(fq) - 700)
    with pkg().Counter(features=GUIDES) as c:
        dt, trunc = c.text_from_bgzf(IC.bgzf_wrap([IC.member(p, 1) for p in parts]))
        assert not trunc and dt.read() == b"".join(parts)
        dt.free()


@pytest.mark.parametrize("name", list(IC.damaged(b"x" * 100)))
def test_damaged_member_truncates(name):
    text = sprinkle_symbols(synth.make_fastq(synth.Spec(seed=3, n_reads=300, read_len=100), GUIDES), 1)[:50000]
    bad, _ = IC.damaged(text)[name]
    good = [IC.member(text[k:k + 9000], 6) for k in range(0, 45000, 9000)]
    with pkg().Counter(features=GUIDES) as c:
        dt, trunc = c.text_from_bgzf(IC.bgzf_wrap(good[:3] + [bad] + good[3:]))
        assert trunc and dt.read() == members_text(good[:3])
        dt.free()


def test_text_from_bgzf_refuses_what_it_does_not_take():
    F = pkg().binding.F2QError
    with pkg().Counter(features=GUIDES) as c:
        for buf in (gzip.compress(b"@r\nACGT\n+\nIIII\n"), bgzf_bytes(b"A" * 70000, block=70000), IC.bgzf_wrap([IC.member(b"ACGT")])[:-3]):
            with pytest.raises(F) as e:
                c.text_from_bgzf(buf)
            assert e.value.code == -8


def test_counted_device_text_matches_oracle(cases):
    """a golden case written as BGZF, inflated on the device and counted from there"""
    from test_lane_logic_cpu import params_of
    case = next(cs for cs in cases if cs["name"] == "synth_fixed_m1")
    fq = case_fastq(case)
    feats = [s for _, s in loader_view(case["features"])]
    with pkg().Counter(features=feats, **params_of(case)) as c:
        dt, trunc = c.text_from_bgzf(bgzf_bytes(fq, block=7000))
        assert not trunc
        c.count_text(dt)
        counts, stats = c.read_counts()
        dt.free()
    assert list(stats) == case["expected"]["stats"] and list(counts) == [r[2] for r in case["expected"]["rows"]]


# ---- f2q_count_file: the device path against the host path on the same file ------------------------------------------
def file_fastq():
    fq = synth.make_fastq(synth.Spec(seed=80, n_reads=6000, read_len=151), GUIDES)
    fq = fq.replace(b"\n", b"\r\n", 2000)
    fq += b"@huge\n" + GUIDES[7].encode() + b"ACGT" * 20000 + b"\n+\n" + b"I" * 80020 + b"\n"   # one record over 64 KiB
    fq += synth.make_fastq(synth.Spec(seed=82, n_reads=2000, read_len=75, cassette=True, up="ACGTAC", down="TTGACA", max_offset=20), GUIDES)
    return fq + synth.make_fastq(synth.Spec(seed=81, n_reads=500, read_len=40), GUIDES)[:-1]      # no final newline


def count(path, kw, env, monkeypatch, capfd=None):
    for k in ("F2Q_DEVICE_INFLATE", "F2Q_TRACE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    feats = GUIDES if kw.get("mode", "C") == "C" else None
    with pkg().Counter(features=feats, **kw) as c:
        t, trunc = c.count_file(str(path))
        counts, stats = c.read_counts()
        table = c.ec_results() if feats is None else None
    trace = capfd.readouterr().err if capfd else ""
    return (list(counts), list(stats), table, t["reads"], trunc), trace


KWS = {"m0": dict(miss=0), "m1": dict(miss=1), "fixed": dict(miss=1, start="3"), "us_ds": dict(miss=1, upstream="ACGTAC", downstream="TTGACA"),
       "two_windows": dict(miss=1, start="0,5"), "ec": dict(mode="EC", upstream="ACGT", length=9)}


def check_same(path, kw, monkeypatch, capfd, extra=None, source="bgzf-device"):
    extra = extra or {}
    host, _ = count(path, kw, extra, monkeypatch)
    capfd.readouterr()
    dev, trace = count(path, kw, dict(extra, F2Q_DEVICE_INFLATE="1", F2Q_TRACE="1"), monkeypatch, capfd)
    assert "[f2q trace]" in trace and f"({source}," in trace, trace
    assert ("(bgzf-device," in trace) == (source == "bgzf-device"), trace
    assert dev == host
    return dev


@pytest.mark.parametrize("chunk", ["4096", "65536", str(1 << 20), None])
@pytest.mark.parametrize("staging", ["as_it_comes", "every_piece", "never"])
def test_count_file_device_inflate_chunks(tmp_path, monkeypatch, capfd, chunk, staging):
    path = tmp_path / "f.fastq.gz"
    path.write_bytes(bgzf_bytes(file_fastq(), block=20000, level=1))
    env = {"F2Q_FILE_CHUNK": chunk} if chunk else {}
    if staging == "every_piece": env["F2Q_FORCE_STAGING"] = "1"
    if staging == "never": env["F2Q_NO_STAGING"] = "1"
    for name in ("m1", "ec"):
        res = check_same(path, KWS[name], monkeypatch, capfd, env)
        assert not res[4] and res[3] == 8501


@pytest.mark.parametrize("name", list(KWS))
def test_count_file_device_inflate_modes(tmp_path, monkeypatch, capfd, name):
    path = tmp_path / "f.fastq.gz"
    path.write_bytes(bgzf_bytes(file_fastq(), block=0xFF00, level=6))
    check_same(path, KWS[name], monkeypatch, capfd, {"F2Q_FILE_CHUNK": "65536"})


@pytest.mark.parametrize("kind", ["gzip", "bgzf_then_gzip", "cut_off_member", "big_member", "plain"])
def test_files_the_device_path_does_not_take(tmp_path, monkeypatch, capfd, kind):
    fq = file_fastq()
    data = {"gzip": gzip.compress(fq, 1), "bgzf_then_gzip": bgzf_bytes(fq[:200000], eof_marker=False) + gzip.compress(fq[200000:]),
            "cut_off_member": bgzf_bytes(fq, eof_marker=False)[:-100], "big_member": bgzf_bytes(fq, block=70000), "plain": fq}[kind]
    path = tmp_path / ("f.fastq" if kind == "plain" else "f.fastq.gz")
    path.write_bytes(data)
    source = {"gzip": "gzip", "plain": "plain", "bgzf_then_gzip": "gzip"}.get(kind, "bgzf")    # (the source the file ended as)
    check_same(path, KWS["m1"], monkeypatch, capfd, {"F2Q_FILE_CHUNK": "65536"}, source=source)


@pytest.mark.parametrize("chunk", ["65536", None])
def test_damaged_member_in_a_file(tmp_path, monkeypatch, capfd, chunk):
    fq = file_fastq()
    ms = [IC.member(fq[k:k + 30000], 6) for k in range(0, len(fq), 30000)]
    j = len(ms) // 2
    bad = bytearray(ms[j]); bad[len(bad) // 3] ^= 0x21
    path = tmp_path / "f.fastq.gz"
    path.write_bytes(IC.bgzf_wrap(ms[:j] + [bytes(bad)] + ms[j + 1:]))
    for name in ("m1", "ec"):
        res = check_same(path, KWS[name], monkeypatch, capfd, {"F2Q_FILE_CHUNK": chunk} if chunk else {})
        assert res[4] and 0 < res[3] < 8501


def test_cli_directory_with_and_without_device_inflate(tmp_path):
    (tmp_path / "in").mkdir()
    csvp = tmp_path / "lib.csv"
    csvp.write_text("".join(f"g{i},{g}\n" for i, g in enumerate(GUIDES)))
    for k, n in (("s1", 3000), ("s2", 1200), ("s3", 700)):
        fq = synth.make_fastq(synth.Spec(seed=30 + n, n_reads=n, read_len=60), GUIDES)
        (tmp_path / "in" / f"{k}.fastq.gz").write_bytes(bgzf_bytes(fq, block=9000))
    outs = {}
    for on in ("0", "1"):
        od = tmp_path / f"out{on}"
        od.mkdir()
        env = dict(os.environ, F2Q_DEVICE_INFLATE=on, F2Q_TRACE="1")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "2fast2q"), "-c", "--s", str(tmp_path / "in"), "--g", str(csvp), "--o", str(od),
                            "--m", "1", "--pb"], env=env, check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        # every sample went through the path the switch selects
        assert r.stderr.count("(bgzf-device,") == (3 if on == "1" else 0) and r.stderr.count("(bgzf,") == (0 if on == "1" else 3), r.stderr[-3000:]
        d = [x for x in od.iterdir() if x.is_dir() and x.name.startswith("2FAST2Q_output_")][0]
        stats = [r for r in csv.reader(open(d / "compiled_stats.csv", newline=""))]
        keep = [r[:1] + r[3:] for r in stats if r and not r[0].startswith("#")]          # the running time differs
        outs[on] = ((d / "compiled.csv").read_bytes(), keep)
    assert outs["0"] == outs["1"]
    assert len(outs["0"][1]) == 3
