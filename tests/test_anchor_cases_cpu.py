"""The inputs of tests/test_anchor_kernels_gpu.py do what they are for: preconditions on tests/anchor_cases.py, checked
with the oracle alone (and, for what the packer and the host index decide, with the per-lane logic compiled for the host).
These are conditions on the input, not measurements of the kernels."""
import pytest

import anchor_cases as AC
import synth
from emu_helper import Emu
from oracle import oracle as O


@pytest.fixture(scope="module")
def LIB():
    return tuple(synth.make_library(2000, 20, AC.LIB_SEED))


def _pair_lib(n):
    return AC.pair_library(synth.make_library(n, 20, AC.PAIR_SEEDS[0]), synth.make_library(n, 20, AC.PAIR_SEEDS[1]))


def _emu(case, run, **emu_kw):
    """(counts, stats, fast, general) of the block through the host build of the lane logic"""
    e = Emu(features=case.lib, **emu_kw, **run)
    e.count_block(case.fq)
    out = e.read()
    e.close()
    return out


def _shape(case, longest=None):
    lens = [len(s) for s, _ in case.recs]
    assert max(lens) <= case.max_len <= 160 and (longest is None or max(lens) == longest)
    assert all(len(s) == len(q) for s, q in case.recs)
    assert not set("".join(s for s, _ in case.recs)) - set("ACGTN")
    assert set("".join(q for _, q in case.recs)) <= {"I", AC.LOWQ}


def _all_five(stats, n, miss):
    assert stats[0] == n and stats[1] > 0 and (stats[2] > 0) == (miss > 0) and stats[3] > 0 and stats[4] > 0, stats


@pytest.mark.parametrize("max_len", [150, 96])
def test_mixed_block_shape(LIB, max_len):
    case = AC.block(LIB, max_len=max_len)
    _shape(case, longest=max_len)                                # (96: at least one read of exactly 96 bases)
    assert case.n == AC.N17 and set(case.kinds) == set(AC.KINDS)
    for w in range(0, case.n, 64):                               # waves with and without a flagged read
        assert any("N" in s for s, _ in case.recs[w:w + 64]) == ((w // 64) % 2 == 0)
    assert AC.block(LIB, max_len=max_len) is case                # one object: the cached expectations key on it


@pytest.mark.parametrize("miss,ms,anchors,max_len", AC.MATRIX7, ids=lambda v: str(v))
def test_lds_matrix_inputs(LIB, miss, ms, anchors, max_len):
    case, run = AC.block(LIB, max_len=max_len), AC.run_kw(anchors, miss, ms)
    counts, stats = AC.expect(case, **run)
    _all_five(stats, case.n, miss)
    assert AC.expected_path(case, run) == AC.PATH_ANCHOR_LDS and AC.general_reads(case, run) == 0
    ecounts, estats, fast, gen = _emu(case, run)
    assert (ecounts, estats) == (counts, stats) and gen == 0 and fast == case.n


@pytest.mark.parametrize("variant,miss,ms,anchors,max_len,extra", AC.MATRIX6, ids=lambda v: str(v))
def test_anchor_matrix_inputs(LIB, variant, miss, ms, anchors, max_len, extra):
    case, run = AC.block(LIB, max_len=max_len), AC.run_kw(anchors, miss, ms, **extra)
    counts, stats = AC.expect(case, **run)
    _all_five(stats, case.n, miss)
    assert AC.expected_path(case, run, no_lt=variant == "no_lt") == AC.PATH_ANCHOR and AC.general_reads(case, run) == 0
    ecounts, estats, fast, gen = _emu(case, run, lt=variant != "no_lt")
    assert (ecounts, estats) == (counts, stats) and gen == 0


def test_matrices_reach_every_instance():
    kb = {0: 0, 1: 1, 2: 3}
    assert {(m > 0, kb[ms], ml) for m, ms, _, ml in AC.MATRIX7} == {(near, k, ml) for near in (False, True) for k in (0, 1, 3) for ml in (150, 96)}
    assert {a for _, _, a, _ in AC.MATRIX7} == {"both", "up", "down"}
    seen6 = {(ml, kb[ms], "qual_up" not in extra) for _, _, ms, _, ml, extra in AC.MATRIX6}
    assert seen6 == {(ml, k, sq) for ml in (150, 96) for k in (0, 1, 3) for sq in (False, True)}
    for variant in ("no_lt", "qual_up", "miss2"):
        assert {(ml, kb[ms]) for v, _, ms, _, ml, _ in AC.MATRIX6 if v == variant} == {(ml, k) for ml in (150, 96) for k in (0, 1, 3)}


def test_library_fits_the_lds_tables(LIB):
    e = Emu(features=list(LIB), **AC.run_kw("both", 1, 0))
    assert e.lt_ok()
    e.close()


@pytest.mark.parametrize("max_len", [150, 96])
def test_windows_of_another_length_pass_their_tests(LIB, max_len):
    """reads whose window between both anchors is 19 and 21 bases long and passes every Phred test: 'no match', without
    a lookup in the kernels"""
    case, run = AC.block(LIB, max_len=max_len), AC.run_kw("both", 1, 0)
    for kind, length in (("win19", 19), ("win21", 21)):
        found = 0
        for i in [i for i, k in enumerate(case.kinds) if k == kind][:20]:
            s, q = case.recs[i]
            a, b = O.sequence_tinder(s.encode(), q.encode(), upstream=AC.UP, downstream=AC.DOWN, qual_up=30, qual_down=30)
            if a is not None and b - a == length and set(q) == {"I"}:
                assert AC.verdict_of(case, i, **run) == [1, 0, 0, 1, 0]
                found += 1
        assert found > 0


def test_kinds_do_what_they_say(LIB):
    """one read of each kind alone, both anchors, --m 1, exact anchors: the verdict the kind is named for"""
    case, run = AC.block(LIB), AC.run_kw("both", 1, 0)
    want = {"exact": [1, 1, 0, 0, 0], "sub1": [1, 0, 1, 0, 0], "n1": [1, 0, 1, 0, 0], "q_past_down": [1, 1, 0, 0, 0],
            "q_win_first": [1, 0, 0, 0, 1], "q_win_last": [1, 0, 0, 0, 1], "q_up": [1, 0, 0, 0, 1], "q_down": [1, 0, 0, 0, 1],
            "n_up": [1, 0, 0, 0, 1], "up_mm1": [1, 0, 0, 0, 1], "end_in_win": [1, 0, 0, 0, 1], "end_in_down": [1, 0, 0, 0, 1],
            "no_up": [1, 0, 0, 0, 1], "win19": [1, 0, 0, 1, 0], "win21": [1, 0, 0, 1, 0], "n2": [1, 0, 0, 1, 0], "sub1_n1": [1, 0, 0, 1, 0]}
    for kind, st in want.items():
        i = case.kinds.index(kind, 1)
        assert AC.verdict_of(case, i, **run) == st, (kind, case.recs[i])
    # the quality byte in the upstream anchor passes --qsu 20; an anchor with one mismatch is found with --msu 1
    assert AC.verdict_of(case, case.kinds.index("q_up"), **AC.run_kw("both", 1, 0, qual_up=20)) == [1, 1, 0, 0, 0]
    assert AC.verdict_of(case, case.kinds.index("up_mm1"), **AC.run_kw("both", 1, 1)) == [1, 1, 0, 0, 0]
    assert AC.verdict_of(case, case.kinds.index("up_mm2"), **AC.run_kw("both", 1, 1)) == [1, 0, 0, 0, 1]
    assert AC.verdict_of(case, case.kinds.index("up_mm2"), **AC.run_kw("both", 1, 2)) == [1, 1, 0, 0, 0]
    # down-only: the window of a 'no_up' read would start before the read (the byte-exact slice routine)
    i = case.kinds.index("no_up")
    s, q = case.recs[i]
    a, b = O.sequence_tinder(s.encode(), q.encode(), downstream=AC.DOWN, qual_down=30)
    assert a < 0 < b and AC.verdict_of(case, i, **AC.run_kw("down", 1, 0)) == [1, 0, 0, 1, 0]


def test_tile_count_blocks(LIB):
    blocks = AC.tile_blocks(LIB)
    assert [b.n for b in blocks] == [256 + 37, 512 + 37, 1024 + 37, 4352 + 37]
    for case in blocks:
        _shape(case)
        for miss in (0, 1):
            run = AC.run_kw("both", miss, 1)
            _all_five(AC.expect(case, **run)[1], case.n, miss)
            assert AC.expected_path(case, run) == AC.PATH_ANCHOR_LDS and _emu(case, run)[3] == 0


def test_skewed_block(LIB):
    case = AC.skewed(LIB)
    _shape(case)
    assert case.n == 80000 and max(len(s) for s, _ in case.recs) > 96 and not any("N" in s for s, _ in case.recs)
    run = AC.run_kw("both", 1, 0)
    counts, stats = AC.expect(case, **run)
    assert stats[0] == 80000 and counts[7] > 2 * 0x8000 and stats[2] > 20000
    counts0, _ = AC.expect(case, **AC.run_kw("both", 0, 0))
    assert 0x8000 < counts0[7] < counts[7]                       # exact hits alone pass 0x8000 once
    assert AC.expected_path(case, run) == AC.PATH_ANCHOR_LDS and AC.general_reads(case, run) == 0


def test_skewed_pairs_block():
    lib = _pair_lib(2001)
    case = AC.skewed_pairs(lib)
    _shape(case)
    assert case.n == 160000 and len(lib) % 2 == 1 and not any("N" in s for s, _ in case.recs)
    run = AC.run_kw(pairs=True, miss=1, ms=0)
    counts, stats = AC.expect(case, **run)
    assert stats[0] == case.n and counts[6] > 2 * 0x8000 and counts[7] > 0x8000 and counts[2000] > 0x8000 and stats[2] > 20000
    assert 6 >> 1 == 7 >> 1 and 2000 % 2 == 0                    # one histogram word; a low half without a partner
    assert AC.expected_path(case, run) == AC.PATH_PAIRS
    assert AC.general_reads(case, run) == 0 and AC.general_reads(case, run, pair_tables=False) == 0
    e = Emu(features=list(lib), **run)
    assert e.pw_ok()
    e.close()


def test_large_libraries():
    """one feature more than the largest library with an LDS histogram, and that largest library at --m 2"""
    big = tuple(synth.make_library(AC.HIST_MAX + 1, 20, AC.LIB_SEED))
    case, run = AC.block(big), AC.run_kw("both", 1, 1)
    counts, stats = AC.expect(case, **run)
    _all_five(stats, case.n, 1)
    assert counts[AC.HIST_MAX] > 0 and AC.expected_path(case, run) == AC.PATH_ANCHOR and AC.general_reads(case, run) == 0
    ecounts, estats, _, gen = _emu(case, run)
    assert (ecounts, estats) == (counts, stats) and gen == 0

    edge, run2 = AC.block(big[:AC.HIST_MAX]), AC.run_kw("both", 2, 1)
    counts, stats = AC.expect(edge, **run2)
    _all_five(stats, edge.n, 2)
    assert counts[AC.HIST_MAX - 1] > 0 and AC.expected_path(edge, run2) == AC.PATH_ANCHOR

    plib = _pair_lib(AC.HIST_MAX + 1)
    pcase, prun = AC.block(plib), AC.run_kw(pairs=True, miss=1, ms=1)
    _shape(pcase)
    counts, stats = AC.expect(pcase, **prun)
    _all_five(stats, pcase.n, 1)
    assert counts[AC.HIST_MAX] > 0 and AC.expected_path(pcase, prun) == AC.PATH_PAIRS and AC.general_reads(pcase, prun) == 0
    e = Emu(features=list(plib), **prun)
    assert e.pw_ok()
    e.count_block(pcase.fq)
    ecounts, estats, _, gen = e.read()
    e.close()
    assert (ecounts, estats) == (counts, stats) and gen == 0
