"""The anchored (--us/--ds) Counter kernels, every template instance pinned: k_count_anchor_lt (path 7), k_count_anchor
(path 6) and k_count_anchor_pairs (path 8) count the small blocks of tests/anchor_cases.py through the C ABI; counts and
the five statistics exactly equal to the oracle's, the kernel family that ran (`timing["path"]`) equal to what
choose_path must pick for the run, and no read outside the packed tiles.  Every block is 4352 + 37 reads or fewer except
the two skewed ones, which need 80 000 / 160 000 reads in ONE workgroup (F2Q_LT_WGS=1) so that a u16 counter passes
0x8000 twice."""
import pytest

import anchor_cases as AC
from conftest import pkg

pytestmark = pytest.mark.gpu

ENV = ("F2Q_LT_WGS", "F2Q_NO_LT", "F2Q_NO_PW", "F2Q_FORCE_GENERAL")


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def LIB(P):
    return tuple(P.binding.synth_library(AC.LIB_SEED, 2000, 20))


def _pair_lib(P, n):
    return AC.pair_library(P.binding.synth_library(AC.PAIR_SEEDS[0], n, 20), P.binding.synth_library(AC.PAIR_SEEDS[1], n, 20))


def _check(P, monkeypatch, case, run, path, env=None, general=0):
    """counts the block in a fresh context under `env`; everything a check here asserts"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    want_counts, want_stats = AC.expect(case, **run)
    with P.Counter(features=case.lib, **run) as c:
        _, t = c.count_block(case.fq, want_timing=True)
        counts, stats = c.read_counts()
    counts, stats = [int(x) for x in counts], [int(x) for x in stats]
    assert stats == want_stats
    assert counts == want_counts
    assert t["path"] == path                                     # the kernel under test counted the block, no other
    assert t["fast_reads"] + t["general_reads"] == case.n
    assert t["general_reads"] == general
    return counts, stats


def _check_general(P, monkeypatch, case, run, first):
    """the same block with every read a raw record (F2Q_FORCE_GENERAL=1): no packed tiles, the results of `first`"""
    got = _check(P, monkeypatch, case, run, 0, env={"F2Q_FORCE_GENERAL": "1"}, general=case.n)
    assert got == first


@pytest.mark.parametrize("miss,ms,anchors,max_len", AC.MATRIX7, ids=lambda v: str(v))
def test_lds_kernel_instances(P, LIB, monkeypatch, miss, ms, anchors, max_len):
    """k_count_anchor_lt<NW, KB, true, NEAR>: NW 5 and 3, --msu/--msd 0, 1, 2, --m 0 and 1, each anchor form"""
    case, run = AC.block(LIB, max_len=max_len), AC.run_kw(anchors, miss, ms)
    assert AC.expected_path(case, run) == AC.PATH_ANCHOR_LDS
    _check(P, monkeypatch, case, run, AC.PATH_ANCHOR_LDS)


@pytest.mark.parametrize("variant,miss,ms,anchors,max_len,extra", AC.MATRIX6, ids=lambda v: str(v))
def test_anchor_kernel_instances(P, LIB, monkeypatch, variant, miss, ms, anchors, max_len, extra):
    """k_count_anchor<NW, KB, false, true, SQ> on the same reads: F2Q_NO_LT=1, --qsu 20 (SQ = false) and --m 2"""
    case, run = AC.block(LIB, max_len=max_len), AC.run_kw(anchors, miss, ms, **extra)
    no_lt = variant == "no_lt"
    assert AC.expected_path(case, run, no_lt=no_lt) == AC.PATH_ANCHOR
    got = _check(P, monkeypatch, case, run, AC.PATH_ANCHOR, env={"F2Q_NO_LT": "1"} if no_lt else None)
    if no_lt:                                                    # ... and the library-in-LDS kernel on the same parameters
        assert got == _check(P, monkeypatch, case, run, AC.PATH_ANCHOR_LDS)


@pytest.mark.parametrize("wgs", [None, "1"], ids=["all_cus", "one_workgroup"])
@pytest.mark.parametrize("miss", [1, 0], ids=["m1", "m0"])
@pytest.mark.parametrize("which", range(4), ids=["1_tile", "2_tiles", "4_tiles", "17_tiles"])
def test_lds_kernel_tile_walk(P, LIB, monkeypatch, which, miss, wgs):
    """three groups of 256 threads per workgroup, two tiles in flight each: fewer tiles than groups (idle groups), a
    partial last tile, and, in one workgroup, a further round for some groups only (5 tiles) and for all (18)"""
    case, run = AC.tile_blocks(LIB)[which], AC.run_kw("both", miss, 1)
    _check(P, monkeypatch, case, run, AC.PATH_ANCHOR_LDS, env={"F2Q_LT_WGS": wgs} if wgs else None)


@pytest.mark.parametrize("miss", [1, 0], ids=["m1", "m0"])
def test_lds_kernel_counter_hand_off(P, LIB, monkeypatch, miss):
    """one feature takes 70 000 of 80 000 reads, a third of them at distance 1; one workgroup counts them all, so its u16
    counter passes 0x8000 twice (--m 0: once, through the exact hits alone)"""
    case, run = AC.skewed(LIB), AC.run_kw("both", miss, 0)
    counts, stats = _check(P, monkeypatch, case, run, AC.PATH_ANCHOR_LDS, env={"F2Q_LT_WGS": "1"})
    assert stats[0] == 80000
    assert counts[7] > (2 if miss else 1) * 0x8000               # what the input is for (the count itself is the oracle's, above)


@pytest.mark.parametrize("tables", [True, False], ids=["pair_tables", "string_index"])
def test_pairs_kernel_counter_hand_off(P, monkeypatch, tables):
    """k_count_anchor_pairs<.., USE_LDS = true> in one workgroup: features 6 and 7 share a histogram word and pass 0x8000
    twice and once, the last feature (even index, no partner half) once"""
    lib = _pair_lib(P, 2001)
    case, run = AC.skewed_pairs(lib), AC.run_kw(pairs=True, miss=1, ms=0)
    env = {"F2Q_LT_WGS": "1"} if tables else {"F2Q_LT_WGS": "1", "F2Q_NO_PW": "1"}
    counts, stats = _check(P, monkeypatch, case, run, AC.PATH_PAIRS, env=env, general=AC.general_reads(case, run, pair_tables=tables))
    assert stats[0] == case.n
    assert counts[6] > 2 * 0x8000 and counts[7] > 0x8000 and counts[2000] > 0x8000


def test_large_library_single_pair(P, monkeypatch):
    """F2Q_HIST_MAX + 1 features: k_count_anchor<.., USE_LDS = false> (global atomics); next to it the last size with an
    LDS histogram at --m 2: both sides of the boundary on k_count_anchor"""
    big = tuple(P.binding.synth_library(AC.LIB_SEED, AC.HIST_MAX + 1, 20))
    case, run = AC.block(big), AC.run_kw("both", 1, 1)
    first = _check(P, monkeypatch, case, run, AC.PATH_ANCHOR)
    assert first[0][AC.HIST_MAX] > 0
    _check_general(P, monkeypatch, case, run, first)
    edge, run2 = AC.block(big[:AC.HIST_MAX]), AC.run_kw("both", 2, 1)
    counts, _ = _check(P, monkeypatch, edge, run2, AC.PATH_ANCHOR)
    assert counts[AC.HIST_MAX - 1] > 0


def test_large_library_two_pairs(P, monkeypatch):
    """F2Q_HIST_MAX + 1 A:B features, two anchor pairs: k_count_anchor_pairs<.., USE_LDS = false>"""
    case, run = AC.block(_pair_lib(P, AC.HIST_MAX + 1)), AC.run_kw(pairs=True, miss=1, ms=1)
    first = _check(P, monkeypatch, case, run, AC.PATH_PAIRS, general=AC.general_reads(case, run))
    assert first[0][AC.HIST_MAX] > 0
    _check_general(P, monkeypatch, case, run, first)


def test_lds_kernel_accumulates(P, LIB):
    """two blocks counted without a reset add up (slab rows, k_reduce_slabs and the global hand-off share together);
    after a reset a block counts as on its own"""
    a, b = AC.block(LIB), AC.tile_blocks(LIB)[2]
    run = AC.run_kw("both", 1, 1)
    both, only_b = AC.expect((a, b), **run), AC.expect(b, **run)
    with P.Counter(features=a.lib, **run) as c:
        _, ta = c.count_block(a.fq, want_timing=True)
        _, tb = c.count_block(b.fq, want_timing=True)
        counts, stats = c.read_counts()
        assert ([int(x) for x in counts], [int(x) for x in stats]) == both
        c.reset()
        _, tb2 = c.count_block(b.fq, want_timing=True)
        counts, stats = c.read_counts()
        assert ([int(x) for x in counts], [int(x) for x in stats]) == only_b
    for t, n in ((ta, a.n), (tb, b.n), (tb2, b.n)):
        assert t["path"] == AC.PATH_ANCHOR_LDS and t["general_reads"] == 0 and t["fast_reads"] == n
