"""The byte-string feature index (GkDesc) at its edges, on the CPU emulation: tests/gk_cases.py through the product's
per-lane logic as g++ compiles it (tests/emu) against the oracle; what those inputs reach in the index, by the Python model
of gk_cases; and the model against the tables build_gk makes.  tests/test_gk_edges_gpu.py runs the same cases on the kernels."""
import pytest

import gk_cases as G
import strand_cases as SC
from emu_helper import Emu


def emulate(lib, fq, run, **kw):
    e = Emu(features=lib, **run, **kw)
    assert e.count_block(fq) == len(fq)
    counts, stats, fast, gen = e.read()
    return e, (counts, stats), fast, gen


# ---- emulation vs oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("miss", G.MISSES)
@pytest.mark.parametrize("L", G.LENS)
def test_fixed_window_emulation_vs_oracle(L, miss):
    """general_read<.., WORDS = true> on the raw records (every read where L > 31), and for L <= 9 fixed_lane's decode and
    match_key<WORDS = false> on the packed reads of the irregular library"""
    lib, fq, run = G.fixed_case(L, miss)
    _, got, fast, gen = emulate(lib, fq, run)
    assert got == G.expect("fixed", L, miss)
    assert fast + gen == got[1][0] == G.N_READS
    assert gen == G.N_READS if L > 31 else (fast > 0 and gen > 0)
    assert got[1][1] > 0 and got[1][3] > 0 and got[1][4] > 0 and (miss == 0 or got[1][2] > 0)


@pytest.mark.parametrize("miss", [0, 1, 3])
def test_many_groups_emulation_vs_oracle(miss):
    lib, fq, run = G.many_groups_case(miss)
    _, got, fast, gen = emulate(lib, fq, run)
    assert got == G.expect("groups", miss) and fast == 0 and gen == got[1][0]
    assert {len(s) for s in lib} == {n for n, _ in G.GROUPS} and len(G.GROUPS) == 12
    assert got[1][1] > 0 and got[1][3] > 0 and (miss == 0 or got[1][2] > 0)


@pytest.mark.parametrize("miss", [0, 1, 2])
@pytest.mark.parametrize("kind", sorted(G.JOINED))
def test_joined_keys_emulation_vs_oracle(kind, miss):
    lib, fq, run = G.joined_case(kind, miss)
    _, got, fast, gen = emulate(lib, fq, run)
    assert got == G.expect("joined", kind, miss) and fast == 0 and gen == got[1][0]
    assert all(got[1][1:]) if miss else (got[1][1] > 0 and got[1][3] > 0 and got[1][4] > 0)
    # the features that hold ':' where a key holds a base (and the other way round) are reached as soon as --m allows it
    _, combos, fresh, _, lone = G.joined_library(kind)
    hits = lambda f: got[0][lib.index(f.decode())]
    assert (hits(lone[:16] + b":" + lone[17:]) > 0) == (miss >= 1)
    assert (hits(G._shifted(list(fresh[0]), b"C")) > 0) == (miss >= 2)
    assert (hits(b"G".join(fresh[1])) > 0) == (miss >= len(fresh[1]) - 1)               # a base at every separator of the key
    assert any(len(s) == len(lib[0]) and s.count(":") == len(combos[0]) - 1 and got[0][i] for i, s in enumerate(lib))
    assert any(":" not in s and got[0][i] for i, s in enumerate(lib))                    # a one-part key: the other windows failed


@pytest.mark.parametrize("plen", [31, 34])
def test_pair_kernel_emulation_vs_oracle(plen):
    """pairs_lane's string road (no pair tables: the parts are longer than 20 bases): a 63-byte key is matched in place,
    match_key<true>; a 69-byte key outgrows F2Q_PAIRS_KEYMAX and the read goes to the byte-exact routine"""
    lib, fq, run = G.pair_case(plen)
    e, got, fast, gen = emulate(lib, fq, run)
    assert got == G.expect("pairs", plen) and not e.pw_ok()
    assert 2 * plen + 1 == (63 if plen == 31 else 69) and (2 * plen + 2 > G.PAIRS_KEYMAX) == (plen == 34)
    assert fast > 0.9 * G.N_READS and all(got[1][1:])
    assert gen == sum(b"N" in s for s, _ in G.records(fq))          # the irregular library: no symbol travels as a flag
    assert e.pairs_slow() == 0 if plen == 31 else e.pairs_slow() > 0.6 * fast


@pytest.mark.parametrize("miss", [1, 3])
@pytest.mark.parametrize("L", [65, 104])
def test_strand_both_emulation_vs_expectation(L, miss):
    """strand_read<BOTH>: every second read mirrored in place, its reverse trip reads the key through StrandBytes"""
    from test_strand_cpu import emu_result
    lib, fq, run = G.fixed_case(L, miss)
    text = SC.mirror_text(fq, lambda i: i % 2 == 1)
    want = SC.expect(lib, text, SC.BOTH, **run)
    got, _ = emu_result(lib, text, SC.BOTH, **run)
    assert got == want
    assert want[3][0] > 300 and want[3][1] > 50 and want[3][2] > 100, want[3]


@pytest.mark.parametrize("miss", [0, 1, 3])
@pytest.mark.parametrize("name,arg", [("fixed", 64), ("fixed", 105), ("joined", "3x34")])
def test_assign_emulation_vs_oracle(name, arg, miss):
    """Extract+Count, then every extracted key against the case's library: the Counter-mode oracle's counts and counters"""
    from test_ec_assign_cpu import emu_assign
    lib, fq, run = G.case(name, arg, miss)
    counts, stats, rows = emu_assign(lib, fq, **run)
    assert (counts, stats) == G.expect(name, arg, miss)
    full = arg if name == "fixed" else 104
    assert sum(len(r[0]) == full for r in rows) > 500 and all(len(r[0]) <= full for r in rows)


# ---- what the inputs reach -----------------------------------------------------------------------------------------------------
def reach_of(L, miss):
    lib, fq, run = G.fixed_case(L, miss)
    keys = G.fixed_keys(fq, run)
    return G.reach(lib, keys, miss), G.verdict_classes(lib, keys, miss)


@pytest.mark.parametrize("L", G.LENS)
def test_fixed_window_inputs_reach_the_edges(L):
    """over the cases the GPU test runs (gk_cases.GPU_FIXED), by the Python model of the index.  The conditions:
    (a) at each L >= 65 some key's exact probe compares a feature that differs from it at bytes >= 64 only, before its
        empty slot or its hit -- here in EVERY case of such an L;
    (b) a candidate is met through two pieces, the later one wholly at bytes >= 64 -- at L = 104 (the word road) and at
        L = 105 (the byte road), the lengths whose misses 2, 3 and 7 cut a piece off behind byte 64;
    (c) a candidate is met through a piece that straddles bytes 63 / 64 -- at every L >= 65 (miss 1);
    (e) see test_piece_counts;
    (f) perfect, imperfect, non-aligned by distance and non-aligned by a tie at every L >= 56 for every miss >= 1;
    and the road: keys of at most 104 bytes on words, longer ones on bytes; a scan wherever there are no piece tables."""
    seen = dict(dup_hi=0, straddle=0)
    for miss in [m for n, m in G.GPU_FIXED if n == L]:
        r, v = reach_of(L, miss)
        if L >= 65:
            assert r["hi_only"] > 0, (L, miss, r)                                        # (a)
        seen["dup_hi"] += r["dup_hi"]
        if miss == 1:
            seen["straddle"] += r["straddle"]
        if L >= 56 and miss >= 1:
            assert all(v[k] > 0 for k in ("perfect", "imperfect", "far", "tie")), (L, miss, v)   # (f)
        assert (r["word"] > 0 and r["byte"] == 0) if L <= G.GK_WORD_BYTES else r["byte"] > 0, (L, miss, r)
        assert (L in r["scan_lens"]) == (miss > 0 and (miss + 1 > L or miss + 1 > G.GK_MAXP)), (L, miss, r)
        assert r["no_group"] > 0                                                          # reads that end inside the window
    if L in (104, 105):
        assert seen["dup_hi"] > 0                                                         # (b)
    if L >= 65:
        assert seen["straddle"] > 0                                                       # (c)


@pytest.mark.parametrize("miss", [0, 1, 3])
def test_many_groups_inputs_reach_the_edges(miss):
    """(d) a probe chain goes round the end of a 16-slot table; keys of every group's length, in every gap, below the
    smallest and above the largest group; the groups of 1, 8 and 9 features"""
    lib, fq, run = G.many_groups_case(miss)
    keys = G.fixed_keys(fq, run)
    r = G.reach(lib, keys, miss)
    assert r["wrap16"] > 0, r                                                            # (d)
    m = G.Model(lib, miss)
    assert [(g.len, g.n) for g in m.groups] == list(G.GROUPS)
    assert {g.n: g.bits for g in m.groups if g.n in (1, 8, 9)} == {1: 4, 8: 4, 9: 5}
    lens = {len(k) for k in keys}
    assert lens >= {n for n, _ in G.GROUPS} | set(G.GAP_LENS) | set(G.BELOW) | set(G.ABOVE)
    assert min(lens) < G.GROUPS[0][0] and max(lens) > G.GROUPS[-1][0]
    assert r["word"] > 0 and r["byte"] > 0 and r["no_group"] > 0
    for n, count in G.GROUPS:                                                            # every group answers an exact hit
        assert any(k.decode() in lib for k in keys if len(k) == n), n


@pytest.mark.parametrize("miss", G.MISSES)
@pytest.mark.parametrize("L", G.LENS)
def test_piece_counts(L, miss):
    """(e) miss + 1 > L or miss + 1 > F2Q_GK_MAXP: no piece tables (the group is scanned); else miss + 1 of them for
    miss > 0 -- in the model and in the groups build_gk makes"""
    lib, fq, run = G.fixed_case(L, miss)
    want = 0 if miss == 0 or miss + 1 > L or miss + 1 > G.GK_MAXP else miss + 1
    g = G.Model(lib, miss).by_len[L]
    assert g.n_pieces == want and g.cut == [p * L // want for p in range(want)] + [L]
    e = Emu(features=lib, **run)
    (pg,) = [x for x in e.gk()[1] if x["len"] == L]
    assert pg["n_pieces"] == want and pg["maxp"] == G.GK_MAXP and 8 * pg["maxw"] == G.GK_WORD_BYTES


# ---- the model against build_gk -------------------------------------------------------------------------------------------------
def check_model(lib, run):
    e = Emu(features=lib, **run)
    tab, groups = e.gk()
    m = G.Model(lib, run["miss"])
    assert tab == m.tab
    assert [(g["len"], g["n"], g["bits"], g["n_pieces"], g["exact_off"], g["piece_off"], g["cut"]) for g in groups] == \
        [(g.len, g.n, g.bits, g.n_pieces, g.exact_off, g.piece_off, g.cut) for g in m.groups]


@pytest.mark.parametrize("L", G.LENS)
def test_model_agrees_with_build_gk_fixed(L):
    for miss in G.MISSES:
        lib, _, run = G.fixed_case(L, miss)
        check_model(lib, run)


def test_model_agrees_with_build_gk_other_cases():
    for miss in (0, 1, 3):
        lib, _, run = G.many_groups_case(miss)
        check_model(lib, run)
    for kind in G.JOINED:
        for miss in (0, 1, 2):
            lib, _, run = G.joined_case(kind, miss)
            check_model(lib, run)
    lib, _, run = G.pair_case(31)
    check_model(lib, run)
