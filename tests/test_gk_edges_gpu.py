"""The byte-string feature index (GkDesc) at its edges, on the kernels: the cases of tests/gk_cases.py through
k_count_general, the packed kernels' stray-read road, k_count_anchor_pairs, k_count_strand and k_assign_entries against the
oracle on the same bytes.  Counts and the five counters are equal or the test fails; nothing here is a tolerance.  What
these inputs reach inside the index (bytes >= 64, the word / byte road, the piece counts, chains that wrap) is pinned by
tests/test_gk_edges_cpu.py on the same cases; the verdicts that follow from it are pinned here."""
import pytest

import gk_cases as G
import strand_cases as SC
from conftest import pkg

pytestmark = pytest.mark.gpu
F2Q_PATH_PAIRS = 8


@pytest.fixture(scope="module")
def P():
    return pkg()


def count(P, lib, fq, run, **ctx):
    """one context, one count_block: ((counts, stats), timing, read_strands() on a strand context)"""
    with P.Counter(features=lib, **run, **ctx) as c:
        used, t = c.count_block(fq, want_timing=True)
        counts, stats = c.read_counts()
        strands = c.read_strands() if "strand" in ctx else None
    assert used == len(fq) and t["reads"] == stats[0] == t["fast_reads"] + t["general_reads"]
    return (list(counts), list(stats)), t, strands


@pytest.mark.parametrize("L,miss", G.GPU_FIXED)
def test_fixed_window(P, monkeypatch, L, miss):
    """k_count_general<false>: general_read<.., WORDS = true> on the staged record (KeyViewT<const uint8_t *>) and, for
    L >= 96 with the 100-base tail, on the record in global memory (KeyViewT<gbytes>) -- gk_exact / gk_near on words up
    to L = 104, on bytes from 105, lib_scan where miss + 1 exceeds L or F2Q_GK_MAXP.  L <= 9: the irregular library sends
    the packed reads through k_count_fixed's decode and match_key<WORDS = false>; once more with every read on the general
    kernel."""
    lib, fq, run = G.fixed_case(L, miss)
    want = G.expect("fixed", L, miss)
    got, t, _ = count(P, lib, fq, run)
    assert got == want
    assert t["reads"] == G.N_READS
    if L > 31:
        assert t["general_reads"] == t["reads"] and t["fast_reads"] == 0
    if L >= 96:                                                      # both sides of the staging limit
        n = [len(s) for s, _ in G.records(fq)]
        assert min(n) + 3 <= G.STAGE < max(n)
    if L <= 9:
        assert t["fast_reads"] > 0 and t["general_reads"] > 0
        monkeypatch.setenv("F2Q_FORCE_GENERAL", "1")
        got, t, _ = count(P, lib, fq, run)
        assert got == want and t["general_reads"] == t["reads"]


@pytest.mark.parametrize("miss", [0, 1, 3])
def test_many_groups(P, miss):
    """k_count_general: gk_find over twelve length groups (keys of every group's length, in the gaps, below and above),
    groups of 1, 8 and 9 features, a chain that wraps a 16-slot table, both roads in one launch"""
    lib, fq, run = G.many_groups_case(miss)
    got, t, _ = count(P, lib, fq, run)
    assert got == G.expect("groups", miss)
    assert t["general_reads"] == t["reads"] == 2400


@pytest.mark.parametrize("miss", [0, 1, 2])
@pytest.mark.parametrize("kind", sorted(G.JOINED))
def test_joined_keys(P, kind, miss):
    """k_count_general with nseg > 1: KeyViewT::at over segments and separators under gk_key_words (3 x 34 + 2 = 104 bytes,
    2 x 40 + 1 = 81) and under gk_range_equal / key_dist (3 x 35 + 2 = 107).  No packed kernel takes windows of these
    lengths: the path is the general one as it comes."""
    lib, fq, run = G.joined_case(kind, miss)
    got, t, _ = count(P, lib, fq, run)
    assert got == G.expect("joined", kind, miss)
    assert t["general_reads"] == t["reads"] == G.N_READS


@pytest.mark.parametrize("plen", [31, 34])
def test_pair_kernel(P, monkeypatch, plen):
    """k_count_anchor_pairs, --m 1, a library of A:B with parts longer than 20 bases (no pair tables).  31 + 31: the 63-byte
    key is spelt into the lane's LDS buffer and matched there, match_key<true>.  34 + 34: the 69-byte key outgrows
    F2Q_PAIRS_KEYMAX and the lane hands the read to the byte-exact routine INSIDE the kernel (anchor_slow), so
    f2q_timing counts it with the packed reads: general_reads holds the reads the packer refuses, here those with an 'N'
    (the library is irregular, symbols do not travel as flags).  Under F2Q_FORCE_GENERAL every read is in general_reads
    and k_count_general searches both anchors itself; the result is the same."""
    lib, fq, run = G.pair_case(plen)
    want = G.expect("pairs", plen)
    refused = sum(b"N" in s for s, _ in G.records(fq))
    got, t, _ = count(P, lib, fq, run)
    assert got == want
    assert t["path"] == F2Q_PATH_PAIRS and t["general_reads"] == refused and t["fast_reads"] > 0.9 * t["reads"]
    monkeypatch.setenv("F2Q_FORCE_GENERAL", "1")
    got, t, _ = count(P, lib, fq, run)
    assert got == want and t["general_reads"] == t["reads"] == G.N_READS and t["fast_reads"] == 0


@pytest.mark.parametrize("miss", [1, 3])
@pytest.mark.parametrize("L", [65, 104])
def test_strand_both(P, L, miss):
    """k_count_strand<BOTH>: every second read of the fixed case mirrored in place, so its reverse trip builds the key
    through StrandBytes on the word road.  The expectation is strand_cases.expect: the oracle's verdict of a record and
    of its mirror image, combined by the rule of include/f2q.h."""
    lib, fq, run = G.fixed_case(L, miss)
    text = SC.mirror_text(fq, lambda i: i % 2 == 1)
    counts, stats, rev, extra = SC.expect(lib, text, SC.BOTH, **run)
    got, t, (grev, gextra) = count(P, lib, text, run, strand=SC.BOTH)
    assert got == (counts, stats) and (list(grev), list(gextra)) == (rev, extra)
    assert t["general_reads"] == t["reads"]
    assert extra[0] > 300 and extra[1] > 50 and extra[2] > 100


@pytest.mark.parametrize("miss", [0, 1, 3])
@pytest.mark.parametrize("name,arg", [("fixed", 64), ("fixed", 105), ("joined", "3x34")])
def test_assign(P, name, arg, miss):
    """Extract+Count on the case's bytes, then f2q_ec_assign against its library: k_assign_entries over the byte-string
    entries (match_key on 64- and 104-byte keys by words, on 105-byte keys by bytes) gives the Counter-mode oracle's counts
    and counters"""
    lib, fq, run = G.case(name, arg, miss)
    with P.Counter(mode="EC", **run) as c:
        c.set_assign_library(lib)
        assert c.count_block(fq) == len(fq)
        counts, stats, t = c.ec_assign(want_timing=True)
        keys = [k for k, _, _ in c.ec_results()]
    assert (list(counts), list(stats)) == G.expect(name, arg, miss)
    assert t["launches"] >= 1
    full = arg if name == "fixed" else 104
    assert sum(len(k) == full for k in keys) > 500 and all(len(k) <= full for k in keys)
