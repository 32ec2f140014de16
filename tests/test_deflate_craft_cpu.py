"""DEFLATE streams that zlib's encoder never writes (tests/deflate_craft.py) through the three inflaters, on the host:
the decoder core of k_inflate_bgzf under ASan + UBSan (tests/emu/inflate_dev_fuzz.cpp), f2qz::Inflater behind the file
reader, and the parallel gunzip.  zlib is the reference.  What each family is meant to exercise is asserted from the
members' own bytes (deflate_craft.scan), not assumed."""
import gzip
import random
import struct
import subprocess
import zlib

import pytest

import deflate_craft as DC
import inflate_cases as IC
from emu_helper import read_file
from test_inflate_dev_cpu import ENV, fuzz_bin  # noqa: F401  (the checker, built as that file builds it)

FAMILIES = ["ladder", "one_dist", "no_dist", "repeat_zero", "grid", "mixed", "ring_sweep", "foreign"]
SWEEP_HEADERS = set(range(2007, 2077)) | set(range(3031, 3101))


# ---- preconditions --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facts():
    """scan() of every crafted member (the foreign ones come as their encoder made them)"""
    out = {}
    for fam, members in DC.good_families().items():
        if fam != "foreign":
            for name, (m, text) in members.items():
                out[name] = DC.scan(m)
                assert out[name]["text"] == text, name
    return out


def test_ladder_members_use_15_bit_codes_on_both_sides_of_both_roots(facts):
    pairs = set()
    for name in DC.ladder_family():
        f = facts[name]
        assert f["types"] == [2]
        assert 15 in f["llens"] and 15 in f["dlens"], name
        assert min(f["llens"]) <= 10 < max(f["llens"]) and {10, 11} <= f["llens"], name         # F2Q_INF_LROOT; 11: the host's root
        assert min(f["dlens"]) <= 8 < max(f["dlens"]) and {8, 9} <= f["dlens"], name            # F2Q_INF_DROOT
        assert f["l284_31"] == name.endswith("p284_1"), name
        assert 64000 < len(f["text"]) <= 65536
        pairs |= f["pairs"]
    for order in (0, 1):                                                       # every length at every distance the order codes
        dl = DC.ladder_tables(order)[1]
        got = facts[f"ladder_order{order}_p284_0"]["pairs"] | facts[f"ladder_order{order}_p284_1"]["pairs"]
        assert {(d, L) for d in DC.LADDER_DISTANCES if dl[DC.dist_sym(d)[0]] for L in DC.LADDER_LENGTHS} <= got
    assert {d for d, _ in pairs} >= set(DC.LADDER_DISTANCES) and {L for _, L in pairs} >= set(DC.LADDER_LENGTHS)
    # each symbol of the two ladders lies behind the root in one of the two orders, but for the four middle literals and
    # one distance symbol (17 distance symbols share two ladders of 16)
    for t, root in ((0, 10), (1, 8)):
        a, b = DC.ladder_tables(0)[t], DC.ladder_tables(1)[t]
        never = [s for s in range(len(a)) if (a[s] or b[s]) and max(a[s], b[s]) <= root]
        assert never == ([10, 64, 70, 73] if t == 0 else [11]), never


def test_one_code_and_no_code_distance_tables(facts):
    for name in DC.one_dist():
        assert facts[name]["single_dist"] and facts[name]["dlens"] == {1} and facts[name]["pairs"], name
    assert {d for n in DC.one_dist() for d, _ in facts[n]["pairs"]} == {1, 4}
    f = facts["no_dist"]
    assert f["no_dist"] and not f["pairs"] and f["text"] == b"@r\nACGT\n+\nIIII\n"


def test_repeat_zero_headers(facts):
    for name in DC.repeat_zero():
        f = facts[name]
        if "18_16" in name or "18,16" in name:
            assert {17, 18} & f["rep16_after"], name                            # a 16 straight after a 17 or 18
        if "0_16" in name or "0,16" in name:
            assert 0 in f["rep16_after"], name
    assert {17, 18} <= facts["zero_run_18_16_order0"]["rep16_after"] and {17, 18} <= facts["zero_run_18_16_order1"]["rep16_after"]
    assert facts["zero_straddle_None"]["straddle"] == {18} and facts["zero_straddle_18,16"]["straddle"] == {16}
    assert 18 in facts["zero_straddle_18,16"]["rep16_after"] and facts["zero_straddle_18,16"]["single_dist"]
    assert facts["zero_straddle_0,16"]["straddle"] == {16} and 0 in facts["zero_straddle_0,16"]["rep16_after"]
    assert facts["nonzero_straddle"]["straddle"] == {16} and 4 in facts["nonzero_straddle"]["rep16_after"]


def test_grid_holds_every_pair(facts):
    pairs = set()
    for name in DC.grid():
        assert facts[name]["types"] == [1]
        pairs |= facts[name]["pairs"]
    assert pairs == {(d, L) for d in DC.GRID_D for L in DC.GRID_L}


def test_mixed_members_copy_across_block_borders(facts):
    for name, (_, text) in DC.mixed().items():
        f, slen = facts[name], int(name[len("mixed_stored"):])
        assert f["types"] == [1, 0, 1, 0, 0, 1], name
        assert any(d > slen + 7 for d, _ in f["pairs"]), name                   # from the third block into the first
        if slen > 300:                                                         # from the last block into both stored texts
            assert (slen + 100, 258) in f["pairs"] and (slen, 65) in f["pairs"], name


def test_ring_sweep_has_no_gap(facts):
    members = [m for m, _ in DC.ring_sweep().values()]
    assert all(facts[n]["types"] == [1, 0, 1] for n in DC.ring_sweep())
    assert sorted(facts[n]["header_bytes"][2] for n in DC.ring_sweep()) == sorted(SWEEP_HEADERS)
    # the edges of refill (2 KiB ring of 32-bit words, from the word that holds the payload's first byte): ring_advance
    # once the word after ip's reaches word 512, ring_reset once it reaches word 768
    for edge in (511 * 4, 767 * 4):
        for res in range(4):
            assert {edge - res + k for k in range(-8, 8)} <= SWEEP_HEADERS
    for res in range(4):
        pads = DC.sweep_pads(members, res)
        assert all(o % 4 == res for o in DC.payload_offsets(members, pads))


def test_bgzf_wrap_pad(tmp_path):
    ms = [IC.member(b"ACGT\n" * k) for k in (1, 50, 0, 7)]
    assert IC.bgzf_wrap(ms, None) == IC.bgzf_wrap(ms)
    assert IC.bgzf_wrap(ms)[:18] == b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(ms[0]) - 1)
    for pad in (0, 1, 2, 3, [3, 0, 2, 1]):
        p = tmp_path / "p.gz"
        p.write_bytes(IC.bgzf_wrap(ms, pad))
        assert gzip.open(p).read() == b"ACGT\n" * 58
        offs = DC.payload_offsets(ms, pad)
        assert all(p.read_bytes()[o:o + len(m)] == m for o, m in zip(offs, ms))
        assert read_file(p, 1 << 16, 2) == (b"ACGT\n" * 58, False, "bgzf")


# ---- the kernel core ------------------------------------------------------------------------------------------------
def core(fuzz_bin, tmp_path, members, seed):
    """statuses and texts of the members from the checker's `bytes` mode, every payload at an offset = seed mod 4"""
    src, dst = tmp_path / f"members{seed}.bin", tmp_path / f"texts{seed}.bin"
    src.write_bytes(b"".join(struct.pack("<I", len(m)) + m for m in members))
    res = subprocess.run([fuzz_bin, "bytes", str(src), str(seed), str(dst)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:]
    raw, texts, o = dst.read_bytes(), [], 0
    while o < len(raw):
        n = struct.unpack_from("<I", raw, o)[0]
        texts.append(raw[o + 4:o + 4 + n])
        o += 4 + n
    status = [int(x) for x in res.stdout.split()]
    assert len(status) == len(texts) == len(members)
    return status, texts


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("family", FAMILIES)
def test_core_decodes_family(fuzz_bin, tmp_path, family, seed):
    fam = DC.good_families()[family]
    status, texts = core(fuzz_bin, tmp_path, [m for m, _ in fam.values()], seed)
    for name, st, got in zip(fam, status, texts):
        assert st == IC.OK, (name, st)
        assert got == fam[name][1], name


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_core_names_crafted_damage(fuzz_bin, tmp_path, seed):
    cases = DC.crafted_damage()
    status, texts = core(fuzz_bin, tmp_path, [m for m, _ in cases.values()], seed)
    for (name, (_, want)), st, got in zip(cases.items(), status, texts):
        assert st != IC.OK and (want is None or st == want) and got == b"", (name, st, want)


# ---- the host reader ------------------------------------------------------------------------------------------------
END = IC.member(b"")


@pytest.mark.parametrize("decoder", ["f2qz", "zlib"])
@pytest.mark.parametrize("family", FAMILIES)
def test_host_reader_reads_family(tmp_path, monkeypatch, family, decoder):
    fam = DC.good_families()[family]
    want = b"".join(t for _, t in fam.values())
    p = tmp_path / "f.fastq.gz"
    p.write_bytes(IC.bgzf_wrap([m for m, _ in fam.values()] + [END]))
    assert gzip.open(p).read() == want
    if decoder == "zlib":
        monkeypatch.setenv("F2Q_ZLIB", "1")
    for threads in (1, 4):
        assert read_file(p, 1 << 16, threads) == (want, False, "bgzf"), threads


def test_host_reader_all_families_one_file(tmp_path):
    ms = list(DC.good_members().values())
    random.Random(6).shuffle(ms)
    want = b"".join(t for _, t in ms)
    p = tmp_path / "all.fastq.gz"
    p.write_bytes(IC.bgzf_wrap([m for m, _ in ms] + [END], pad=[None, 0, 1, 2, 3] * (len(ms) // 5 + 1)))
    for threads in (1, 4):
        assert read_file(p, 1 << 18, threads) == (want, False, "bgzf")


@pytest.mark.parametrize("name", list(DC.crafted_damage()))
def test_host_reader_truncates_at_crafted_damage(tmp_path, monkeypatch, name):
    good = [DC.grid()["grid_d64"], DC.one_dist()["one_dist_sym3"], DC.ladder_family()["ladder_order1_p284_1"], DC.mixed()["mixed_stored1025"]]
    bad = DC.crafted_damage()[name][0]
    p = tmp_path / "d.fastq.gz"
    p.write_bytes(IC.bgzf_wrap([m for m, _ in good[:3]] + [bad] + [m for m, _ in good[3:]] + [END]))
    want = b"".join(t for _, t in good[:3])
    for threads in (1, 4):
        assert read_file(p, 1 << 16, threads) == (want, True, "bgzf"), threads
    monkeypatch.setenv("F2Q_ZLIB", "1")
    assert read_file(p, 1 << 16, 4) == (want, True, "bgzf")


# ---- the parallel gunzip --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """one gzip member: about 6 MB of text in about 400 hand-built blocks"""
    raw, text, notes = DC.big_gzip(random.Random(5))
    p = tmp_path_factory.mktemp("big") / "big.fastq.gz"
    p.write_bytes(raw)
    assert gzip.open(p).read() == text and 300 <= notes["blocks"] <= 600 and 6_000_000 <= len(text) < 6_200_000
    assert notes["stored"] == {0, 1, 5, 700, 65535} and notes["reach_back"] > 1000 and notes["max_distance"] == 32768
    return p, raw, text


@pytest.fixture()
def par_env(monkeypatch):
    monkeypatch.setenv("F2Q_GZ_PAR_MIN_KB", "16")
    monkeypatch.setenv("F2Q_GZ_CHUNK_KB", "64")
    return monkeypatch


@pytest.mark.parametrize("threads", [1, 2, 5])
def test_parallel_gunzip_reads_hand_built_blocks(big, par_env, threads):
    p, _, text = big
    for piece in (1 << 16, 1 << 24):
        assert read_file(p, piece, threads, out_cap=1 << 25) == (text, False, "gzip"), piece


def test_sequential_gunzip_reads_hand_built_blocks(big, par_env):
    p, _, text = big
    par_env.setenv("F2Q_GZ_PAR", "0")
    assert read_file(p, 1 << 18, 2, out_cap=1 << 25) == (text, False, "gzip")


@pytest.mark.parametrize("cut", [0.97, 0.5, 0.13])
def test_parallel_gunzip_cut_off_hand_built_blocks(tmp_path, big, par_env, cut):
    """the cut-off file delivers exactly what zlib delivers of it, and reports truncation"""
    _, raw, text = big
    part = raw[:int(len(raw) * cut)]
    z = tmp_path / "c.fastq.gz"
    z.write_bytes(part)
    want = zlib.decompressobj(31).decompress(part)
    assert text.startswith(want) and len(want) > 0
    got = read_file(z, 1 << 18, 4, out_cap=1 << 25)
    par_env.setenv("F2Q_GZ_PAR", "0")
    seq = read_file(z, 1 << 18, 4, out_cap=1 << 25)
    assert got == seq == (want, True, "gzip")


# ---- a FASTQ file written by the craft writer (test_deflate_craft_gpu.py counts it on the device) --------------------
def test_host_reader_reads_crafted_fastq_file(tmp_path):
    import synth
    data, fq, members = DC.crafted_fastq_file(synth.make_library(120, 20, 47))
    assert fq.count(b"\n") == 4 * 3000 and len(members) >= 8
    types, deep = set(), 0
    for m in members:
        f = DC.scan(m)
        types |= set(f["types"])
        deep += 15 in f["llens"] and 15 in f["dlens"]
    assert types == {0, 1, 2} and deep >= 3
    ends, o = [], 0
    for m in members[:-1]:
        o += struct.unpack("<I", m[-4:])[0]
        ends.append(fq[o - 1:o])
    assert any(e != b"\n" for e in ends)                                    # members end in the middle of a record
    p = tmp_path / "crafted.fastq.gz"
    p.write_bytes(data)
    assert gzip.open(p).read() == fq
    for threads in (1, 4):
        assert read_file(p, 1 << 16, threads) == (fq, False, "bgzf")
