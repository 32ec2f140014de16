"""The inputs of tests/test_ec_kernels_gpu.py do what they are for: preconditions on tests/ec_cases.py, checked with the
oracle alone and, for what the packer and the per-lane logic decide, with that logic compiled for the host (Emu).  These
are conditions on the input, not measurements of the kernels."""
import collections

import pytest

import anchor_cases as AC
import ec_cases as EC
from emu_helper import Emu
from oracle import oracle as O

BOTH = EC.run_kw("both", 0)


def _emu(cases, run):
    """(rows, stats, reads outside the packed tiles) of the blocks through the host build of the lane logic"""
    e = Emu(**run)
    for c in cases:
        e.count_block(c.fq)
    rows = e.ec_rows()
    _, stats, _, gen = e.read()
    e.close()
    return [(k, n) for k, n, _ in rows], stats, gen


def _window(s, q, run=BOTH):
    kw = {k: v for k, v in run.items() if k not in ("mode", "miss", "phred")}
    return O.sequence_tinder(s.encode(), q.encode(), **kw)


def test_single_word_rule():
    """ec64_word's edges as the issue states them"""
    fits = {(L, n) for L in range(0, 34) for n in range(0, 5) if EC.ec64_fits(L, n)}
    assert {(25, 1), (23, 2), (20, 3), (29, 0), (0, 0)} <= fits
    assert not {(26, 1), (24, 2), (21, 3), (20, 4), (1, 4), (29, 1), (30, 0)} & fits
    assert {e for e in EC.N_EDGES} == {(25, 1), (26, 1), (23, 2), (24, 2), (20, 3), (21, 3), (20, 4), (29, 1)}


@pytest.mark.parametrize("max_len", [150, 96])
def test_kinds_do_what_they_say(max_len):
    """one read of each Extract+Count kind alone, both anchors, exact anchors: the window the kind is named for, its key the
    oracle's, and the pass it must take"""
    case = EC.block(max_len)
    cl = EC.classify(case, BOTH)
    seen = set()
    for kind in EC.EC_KINDS:
        if kind not in case.kinds:
            assert kind in ("at:64", "at:65") and max_len == 96  # no room
            continue
        i = case.kinds.index(kind)
        s, q = case.recs[i]
        rows, stats = EC.rows_of(case, i, **BOTH)
        if kind == "odd":
            assert "R" in s and cl[i] == "raw" and stats == [1, 1, 0, 0, 0] and "R" in rows[0][0]
            continue
        a, b = _window(s, q)
        w = s[a:b]
        assert rows == [(w.upper(), 1)] and stats == [1, 1, 0, 0, 0]
        if kind.startswith("len:"):
            L = int(kind[4:])
            assert b - a == L and "N" not in w and cl[i] == ("inplace" if L <= 29 else "keys")
        elif kind.startswith("nn:"):
            _, L, K, where = kind.split(":")
            assert b - a == int(L) and w.count("N") == int(K) and w[0 if where == "first" else -1] == "N"
            assert cl[i] == ("inplace" if EC.ec64_fits(int(L), int(K)) else "keys")
        elif kind.startswith("at:"):
            assert a == int(kind[3:]) and b - a == 20 and cl[i] == "inplace"
        elif kind == "lower":
            assert w == w.lower() != w.upper() and "N" not in s and cl[i] == "inplace"      # the read stays packed, the key is upper case
        seen.add(cl[i])
    assert seen == {"inplace", "keys"}
    # down-only anchors: the window of a 'no_up' read starts before the read
    down = EC.run_kw("down", 0)
    i = case.kinds.index("no_up")
    a, b = _window(*case.recs[i], run=down)
    assert a < 0 < b and EC.classify(case, down)[i] == "slow"


def test_matrices_reach_every_instance():
    reached = set()
    for max_len, ms, extra, anchors in EC.HOT_MATRIX:
        case, run = EC.block(max_len), EC.run_kw(anchors, ms, **extra)
        got = EC.instances(case, run)
        assert len(got) == 2 and EC.stages(case, run)[:3] == [EC.S_LEARN, EC.S_BUILD, EC.S_HOT]
        reached |= got
    # k_extract_anchor_hot<NW, KB, SAMEQ, LEARN>: anchored_geom x learning; the stepped rows are the same 12 with F2Q_NO_HOT=1
    assert reached == {(nw, kb, sq, learn) for nw in (3, 5) for kb in (0, 1, 3) for sq in (True, False) for learn in (True, False)}
    assert {a for *_, a in EC.HOT_MATRIX} == set(EC.FORMS) and len(EC.HOT_MATRIX) == 12
    for ml in (150, 96):
        assert {a for m, *_, a in EC.HOT_MATRIX if m == ml} == set(EC.FORMS)
    assert EC.nw_of(EC.block(200)) == 10 and EC.nw_of(EC.pair_block(200)) == 10 and EC.nw_of(EC.pair_block(150)) == 5
    assert {ms for _, ms, _ in EC.PAIR_MATRIX} == {0, 1, 2} and any(e for _, _, e in EC.PAIR_MATRIX) and any(m == 200 for m, _, _ in EC.PAIR_MATRIX)
    assert {(0, 20), (16, 20), (3, 17), (5, 29), (2, 12)} == {(st, L) for st, L, _ in EC.FIXED_ROWS} and (0, 20, 1) in EC.FIXED_ROWS


def _packed(case, run):
    return [(c, rec) for c, rec in zip(EC.classify(case, run), case.recs) if c != "raw"]


@pytest.mark.parametrize("max_len,ms,extra,anchors", EC.HOT_MATRIX, ids=lambda v: str(v))
def test_hot_matrix_inputs(max_len, ms, extra, anchors):
    """every pass has reads inside the learning tiles and after them; a hot set forms; the lane logic agrees with the oracle"""
    case, run = EC.block(max_len), EC.run_kw(anchors, ms, **extra)
    assert max(len(s) for s, _ in case.recs) == max_len and case.n == EC.N17 and set(case.kinds) >= set(AC.KINDS)
    packed = _packed(case, run)
    want = {"inplace", "keys", "fail"} | ({"slow"} if anchors == "down" else set())
    assert {c for c, _ in packed[:EC.LEARN]} == want == {c for c, _ in packed[EC.LEARN:]}
    assert "raw" in EC.classify(case, run)[:EC.LEARN] and "raw" in EC.classify(case, run)[EC.LEARN:]
    for part in (packed[:EC.LEARN], packed[EC.LEARN:]):          # waves with flagged reads and waves without
        flags = {any("N" in s for _, (s, _) in part[w:w + 64]) for w in range(0, len(part), 64)}
        assert flags == {True, False}
    # the keys that reach F2Q_HOT_MINCOUNT among the learning reads come again after them
    early = EC.expect(EC.Plain([rec for _, rec in packed[:EC.LEARN]]), **run)[0]
    late = dict(EC.expect(EC.Plain([rec for _, rec in packed[EC.LEARN:]]), **run)[0])
    hot = [k for k, n in early if n >= EC.HOT_MINCOUNT]
    assert len(hot) >= 4 and all(late.get(k, 0) > 0 for k in hot[:4])
    rows, stats = EC.expect(case, **run)
    assert stats[0] == case.n and stats[1] > 0 and stats[4] > 0
    assert _emu([case], run) == (rows, stats, EC.general_reads(case, run))


def test_other_anchored_inputs():
    wide, run = EC.block(200), EC.run_kw("both", 1)
    assert _emu([wide], run) == (*EC.expect(wide, **run), EC.general_reads(wide, run))
    blocks = EC.tile_blocks()
    assert [b.n for b in blocks] == [256 + 37, 512 + 37, 1024 + 37, 4352 + 37]
    for b in blocks:
        tiles = -(-len(_packed(b, run)) // EC.TILE)
        assert tiles == -(-b.n // EC.TILE) and "keys" in EC.classify(b, run)          # the raw records do not cost a tile
        assert _emu([b], run) == (*EC.expect(b, **run), EC.general_reads(b, run))
    a, b = EC.block(150), EC.block(150, seed=2)
    assert a.recs != b.recs
    assert _emu([a, b], run)[:2] == EC.expect((a, b), **run)


@pytest.mark.parametrize("max_len,ms,extra", EC.PAIR_MATRIX, ids=lambda v: str(v))
def test_pair_matrix_inputs(max_len, ms, extra):
    case, run = EC.pair_block(max_len), EC.run_kw(ms=ms, pairs=True, **extra)
    rows, stats = EC.expect(case, **run)
    assert any(":" in k for k, _ in rows) and any(k and ":" not in k for k, _ in rows) and stats[4] > 0
    assert EC.general_reads(case, run) == 0
    assert _emu([case], run) == (rows, stats, 0)


@pytest.mark.parametrize("st,L,phred", EC.FIXED_ROWS, ids=lambda v: str(v))
def test_fixed_inputs(st, L, phred):
    case = EC.fixed_block(st, L, phred)
    run = EC.fixed_run(case)
    cl = EC.classify(case, run)
    count = collections.Counter(cl)
    assert count["inplace"] > 3000 and count["raw"] > 0 and (count["fail"] > 0) == (phred > 1)
    assert any(len(s) < st + L and c == "inplace" for c, (s, _) in zip(cl, case.recs))                       # a clipped window, packed
    assert any("N" in s[st:st + L] and c == "inplace" for c, (s, _) in zip(cl, case.recs)) == (L < 29)   # 'N's that fit the word
    assert any("N" in s[st:st + L] and c == "raw" for c, (s, _) in zip(cl, case.recs)) == (L == 29)      # 29 bases with an 'N' never do
    packed = [rec for c, rec in zip(cl, case.recs) if c != "raw"]
    early = EC.expect(EC.Plain(packed[:EC.LEARN]), **run)[0]
    assert sum(n >= EC.HOT_MINCOUNT for _, n in early) >= 1 and len(packed) > EC.LEARN + 8 * EC.TILE      # tiles after the learning ones
    assert _emu([case], run) == (*EC.expect(case, **run), count["raw"])


def test_fixed_tile_blocks():
    blocks = EC.fixed_tile_blocks()
    run = EC.fixed_run(blocks[0])
    tiles = [-(-sum(c != "raw" for c in EC.classify(b, run)) // EC.TILE) for b in blocks]
    assert tiles == list(EC.FC.TILE_COUNTS)
    for b in blocks:
        assert _emu([b], run) == (*EC.expect(b, **run), EC.general_reads(b, run))
    # after the designed block of the same library: the keys its learning reads make hot come again in the 17- and 33-tile blocks
    a = EC.fixed_block(0, 20)
    assert EC.fixed_run(a) == run and EC.stages(a, run) == [EC.S_LEARN, EC.S_BUILD, EC.S_HOT]
    packed = [rec for c, rec in zip(EC.classify(a, run), a.recs) if c != "raw"]
    hot = [k for k, n in EC.expect(EC.Plain(packed[:EC.LEARN]), **run)[0] if n >= EC.HOT_MINCOUNT]
    for b in blocks[3:]:
        later = dict(EC.expect(b, **run)[0])
        assert hot and all(later.get(k, 0) > 0 for k in hot)
        assert _emu([a, b], run)[:2] == EC.expect((a, b), **run)


@pytest.mark.parametrize("n_keys,limit", [(12000, EC.HOT_CAP), (33000, EC.HOT_CAND)])
def test_capacity_blocks(n_keys, limit):
    """the lane logic is run on the 12 000-key blocks only: it takes 24 s on the 33 000-key ones (where it agreed with the
    oracle when this test was written), and they are the same reads in kind"""
    a, b = EC.capacity_blocks(n_keys)
    if n_keys == 12000:
        assert _emu([a, b], EC.FIXED20)[:2] == EC.expect((a, b), **EC.FIXED20)
    seen = collections.Counter(s for s, _ in a.recs)
    assert sum(n >= EC.HOT_MINCOUNT for n in seen.values()) == n_keys > limit
    again = collections.Counter(s for s, _ in b.recs)
    assert all(again[k] == 2 for k in seen) and sum(k not in seen for k in again) == 2000
    assert not (set("".join(seen)) | set("".join(again))) - set("ACGT") and {len(k) for k in again} == {20}


def test_growth_blocks():
    """the restated arithmetic of ec_reserve: block A's table stays at the floor, block B's reserve must grow it.  (The lane
    logic on the host takes 148 s for these 130 240 reads, so it is not run here; run once, it gave the oracle's rows.)"""
    a, b, c, hot = EC.growth_blocks()
    slots, room = EC.first_reserve(a.n, EC.LEARN)
    assert (slots, room) == (1 << 17, 3 << 15) and a.n % EC.TILE == 0
    learning = collections.Counter(s for s, _ in a.recs[:EC.LEARN])
    keys = len(learning)
    assert keys == EC.GROW_HOT + EC.GROW_SINGLES and all(learning[k] == 8 >= EC.HOT_MINCOUNT for k in hot)
    assert {s for s, _ in a.recs[EC.LEARN:]} <= set(hot)
    assert not EC.grows_before_launch(a.n - EC.LEARN, keys, EC.LEARN, room)          # (the reserve after the learning launch)
    nb = -(-b.n // EC.TILE) * EC.TILE
    assert EC.grows_before_launch(nb, keys, EC.LEARN, room)
    new = {s for s, _ in b.recs} - set(learning)
    assert len(new) == EC.GROW_NEW and sum(s in hot for s, _ in b.recs) == EC.GROW_B_HOT
    # the grown table: the room doubled for the keys there, a quarter more than asked for
    keys64 = EC.expect_of(nb, keys, EC.LEARN) + EC.aside_of(nb)
    assert 3 * EC.slots_for(keys + keys64 + 16 + max(keys, keys64 // 4)) // 4 > keys + len(new)
    assert {s for s, _ in c.recs} <= set(hot)


def test_byte_string_blocks():
    a, b = EC.bytes_blocks()
    run = EC.run_kw("both", 0)
    for blk in (a, b):
        cl = EC.classify(blk, run)
        assert cl.count("keys") == EC.BYTES_KEYS and cl.count("inplace") == EC.LEARN and set(cl[:EC.LEARN]) == {"inplace"}
    aside = EC.aside_of(-(-a.n // EC.TILE) * EC.TILE)
    entries = max(aside + 16 + aside // 4, 1 << 12)                # ec_reserve's first byte-string table
    assert EC.BYTES_KEYS + 16 <= entries < EC.BYTES_KEYS + aside + 16 and 2 * EC.BYTES_KEYS > 4096
    rows, stats = EC.expect((a, b), **run)
    assert sum(len(k) == 31 for k, _ in rows) == 2 * EC.BYTES_KEYS
    assert _emu([a, b], run) == (rows, stats, 0)


@pytest.mark.parametrize("fixed", [False, True], ids=["anchored", "fixed_window"])
def test_full_table_blocks(fixed):
    """(the lane logic on the host takes 207 s for each of these 141 024-read blocks, so it is not run here; run once, it
    gave the oracle's rows for both)"""
    case = EC.full_block(fixed)
    run = EC.FIXED20 if fixed else EC.run_kw("both", 0)
    n_slots = -(-case.n // EC.TILE) * EC.TILE
    slots, room = EC.first_reserve(n_slots, EC.LEARN)
    assert slots == 1 << 17                                      # the floor: 2^16 keys of room
    assert not EC.grows_before_launch(n_slots - EC.LEARN, EC.FULL_HOT, EC.LEARN, room)
    rows, stats = EC.expect(case, **run)
    assert len(rows) == EC.FULL_HOT + EC.FULL_NEW > slots and stats == [case.n, case.n, 0, 0, 0]
    assert len({k for k, _ in rows[:EC.FULL_HOT]}) == EC.FULL_HOT and all(n == EC.LEARN // EC.FULL_HOT + (i < EC.LEARN % EC.FULL_HOT) for i, (_, n) in enumerate(rows[:EC.FULL_HOT]))
    assert sum("N" in k for k, _ in rows) == EC.FULL_NEW // 16
    if not fixed:
        assert set(EC.classify(case, run)) == {"inplace"} and EC.nw_of(case) == 3
