"""The inputs of tests/test_fixed_kernels_gpu.py do what they are for: preconditions on tests/fixed_cases.py, checked
with the oracle alone and with the per-lane logic compiled for the host (tests/emu).  The matrices name every template
instance the launchers of the fixed-window Counter kernels can pick, and every row reaches the instance it names; the
designed constellations are what they claim; the host build of the lane logic equals the oracle on every block.  These
are conditions on the input, not measurements of the kernels."""
import pytest

import fixed_cases as FC
from emu_helper import Emu

LENGTHS = (14, 16, 17, 18, 20, 21)                               # every feature length of the matrices


def _emu(case, run, **emu_kw):
    """(counts, stats, fast, general) of the block through the host build of the lane logic, and the Emu's own account"""
    e = Emu(features=list(case.lib.feats), **emu_kw, **run)
    e.count_block(case.fq)
    out = e.read()
    acct = dict(lt_ok=e.lt_ok(), lt=e.lt_reads(), pt=e.pt_reads(), parts=e.pt_parts(), v2=e.v2_reads())
    e.close()
    return out, acct


def _lds_case(mw, st, L, phred):
    return FC.block(FC.pair_library(L) if mw else FC.library(L), st if mw else (st,), phred=phred)


def _all_five(stats, n, miss):
    assert stats[0] == n and stats[1] > 0 and (stats[2] > 0) == (miss > 0) and stats[3] > 0 and stats[4] > 0, stats


# ---- the matrices against the launchers --------------------------------------------------------------------------------

def test_matrices_name_every_instance():
    """the instances, written out from fixed_lds_kernel, launch_part, launch_fixed_packed, launch_multi and launch_fixed_v1"""
    lds = {("generic", False, False), ("spec52", False, False), ("a20", False, False), ("generic", True, False), ("spec52", True, False), ("a20", True, False),
           ("generic", False, True), ("spec52", False, True), ("a20", False, True), ("generic", True, True), ("spec52", True, True), ("a20", True, True)}
    scatter = {("generic", 16), ("spec52", 16), ("a20", 16), ("generic", 8), ("spec52", 8), ("a20", 8), ("generic", 4), ("spec52", 4), ("a20", 4)}
    part_count = {False, True}
    packed = {(True, "spec52"), (True, "generic"), (False, "spec52"), (False, "generic")}
    multi = {True, False}
    v1 = {True, False}
    assert len(lds) + len(scatter) + len(part_count) + len(packed) + len(multi) + len(v1) == 12 + 9 + 2 + 4 + 2 + 2
    assert {(v, near, mw) for v, near, mw, *_ in FC.MATRIX_LDS} == lds
    assert {(v, pw) for v, pw, *_ in FC.MATRIX_PART} == scatter
    assert {near for _, _, near, *_ in FC.MATRIX_PART} == part_count
    for v, pw in scatter:                                        # every scatter instance with both k_part_count instances
        assert {near for vv, p, near, *_ in FC.MATRIX_PART if (vv, p) == (v, pw)} == part_count
    assert {(l, v) for l, v, *_ in FC.MATRIX_PACKED} == packed
    for inst in packed:                                          # ... at every --m
        assert {miss for l, v, _, _, miss, _ in FC.MATRIX_PACKED if (l, v) == inst} == {0, 1, 2, 3}
    assert {l for l, *_ in FC.MATRIX_MULTI} == multi
    assert {l for l, *_ in FC.MATRIX_V1} == v1


def test_window_edges_of_the_matrix():
    """the single-window rows of the library-in-LDS matrix put the first window byte on every byte of a quality word, and
    the last one too (qm_first / qm_last); four, five and six quality rows"""
    geoms = {(st, L) for _, _, mw, st, L, *_ in FC.MATRIX_LDS if not mw}
    assert {min(FC.qmasks(st, L)[0]) for st, L in geoms} == {0, 1, 2, 3}
    assert {max(FC.qmasks(st, L)[1]) for st, L in geoms} == {0, 1, 2, 3}
    assert {FC.fixed_geom(st, L) for st, L in geoms} >= {(5, 2), (6, 2), (4, 2)}


@pytest.mark.parametrize("variant,near,mw,st,L,phred,miss,env", FC.MATRIX_LDS, ids=str)
def test_lds_rows(variant, near, mw, st, L, phred, miss, env):
    case = _lds_case(mw, st, L, phred)
    run = case.run(miss)
    assert near == (miss > 0)
    assert FC.fixed_variant(0 if mw else st, L, phred) == variant            # (several windows: the joined window, stored at 0)
    assert FC.fixed_variant(0 if mw else st, L, phred, generic=True) == "generic"
    for e in (env, dict(env, F2Q_GENERIC="1")):
        assert FC.expected_path(case, run, e) == (FC.PATH_MULTI_LDS if mw else FC.PATH_FIXED_LDS)
    assert FC.expected_path(case, run, {"F2Q_FORCE_GENERAL": "1"}) == FC.PATH_NONE
    want = FC.expect(case, **run)
    if phred >= 2:
        _all_five(want[1], case.n, miss)
    else:
        assert want[1][4] == 0                                   # the rule is off: nothing fails
    (counts, stats, fast, gen), acct = _emu(case, run)
    assert (counts, stats) == want
    assert gen == FC.general_reads(case, run) and fast + gen == case.n and gen > 0
    assert acct["lt_ok"] and acct["lt"] > case.n // 2 and acct["pt"] == 0


@pytest.mark.parametrize("variant,pw,near,st,L,phred,miss,parts", FC.MATRIX_PART, ids=str)
def test_partitioned_rows(variant, pw, near, st, L, phred, miss, parts):
    case = FC.block(FC.library(L), (st,), phred=phred)
    run = case.run(miss)
    assert near == (miss > 0) and FC.fixed_variant(st, L, phred) == variant and FC.part_waves(parts) == pw
    for env in ({"F2Q_PT_PARTS": str(parts)}, {"F2Q_PT_PARTS": str(parts), "F2Q_PT_CHUNK": FC.PART_CHUNK, "F2Q_GENERIC": "1"}):
        assert FC.expected_path(case, run, env) == FC.PATH_FIXED_PART
    assert -(-case.n // FC.TILE) > int(FC.PART_CHUNK) // FC.TILE                          # the chunk cuts the block into several rounds
    want = FC.expect(case, **run)
    _all_five(want[1], case.n, miss)
    (counts, stats, fast, gen), acct = _emu(case, run, pt_parts=parts)
    assert (counts, stats) == want and gen == FC.general_reads(case, run) and fast + gen == case.n
    assert acct["parts"] == parts and acct["pt"] > case.n // 2 and acct["lt"] == 0        # the builder kept the forced number


@pytest.mark.parametrize("lds,variant,st,L,miss,big", FC.MATRIX_PACKED, ids=str)
def test_packed_rows(lds, variant, st, L, miss, big):
    lib = FC.big_library(L) if big else FC.library(L)
    case = FC.block(lib, (st,))
    run = case.run(miss)
    assert lds == (len(lib) <= FC.HIST_MAX) and FC.fixed_variant(st, L, FC.PHRED) == variant
    assert FC.expected_path(case, run, FC.PACKED_ENV) == FC.PATH_FIXED_PACKED
    want = FC.expect(case, **run)
    _all_five(want[1], case.n, miss)
    assert not big or sum(want[0][FC.HIST_MAX:]) > 0
    (counts, stats, fast, gen), acct = _emu(case, run, lt=False)
    if not big:                                                  # (the host build takes a library this large through its partitioned tables)
        assert acct["lt"] == 0 and acct["pt"] == 0
    assert (counts, stats) == want and gen == FC.general_reads(case, run) and fast + gen == case.n


@pytest.mark.parametrize("lds,name,starts,L,miss", FC.MATRIX_MULTI, ids=str)
def test_multi_rows(lds, name, starts, L, miss):
    lib = FC.multi_library(name, L)
    case = FC.block(lib, starts)
    run = case.run(miss)
    assert lds == (len(lib) <= FC.HIST_MAX)
    assert FC.expected_path(case, run) == FC.PATH_MULTI
    want = FC.expect(case, **run)
    _all_five(want[1], case.n, miss)
    assert not name == "big" or sum(want[0][FC.HIST_MAX:]) > 0
    (counts, stats, fast, gen), acct = _emu(case, run)
    assert (counts, stats) == want and gen == FC.general_reads(case, run) and fast + gen == case.n and acct["lt"] == 0
    if name == "mixed":                                          # a read with one failed part finds the one-part features
        assert sum(want[0][len(lib) - lib.singles:]) > 0


@pytest.mark.parametrize("lds,st,L,miss,big", FC.MATRIX_V1, ids=str)
def test_v1_rows(lds, st, L, miss, big):
    lib = FC.big_library(L) if big else FC.library(L)
    case = FC.block(lib, (st,))
    run = case.run(miss)
    assert lds == (len(lib) <= FC.HIST_MAX)
    assert FC.expected_path(case, run, FC.V1_ENV) == FC.PATH_FIXED_V1
    want = FC.expect(case, **run)
    _all_five(want[1], case.n, miss)
    (counts, stats, fast, gen), acct = _emu(case, run, v2=False)
    assert (counts, stats) == want and gen == FC.general_reads(case, run) and acct["v2"] == 0 and acct["lt"] == 0 and acct["pt"] == 0


# ---- the libraries -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", LENGTHS)
def test_constellations_are_what_they_claim(L):
    """Hamming distances, and the halves the differences lie in, on the library itself"""
    lib = FC.library(L)
    h, K = L // 2, lib.keys
    assert len(set(K)) == len(K) and all(len(k) == L and set(k) <= set("ACGT") for k in K)
    assert {c["kind"]: 0 for c in lib.cons}.keys() == set(FC.CONSTELLATIONS) and all(len(v) == FC.N_CONSTELLATIONS for v in lib.by_kind.values())
    halves = lambda a, b: sorted(int(p >= h) for p in FC.hamming(a, b))
    for c in lib.cons:
        g, kind = K[c["guide"]], c["kind"]
        assert c["p"] < L and (kind == "twin" or (c["p"] < h <= c["q"] and c["p2"] < h <= c["q2"]))
        if kind == "cross":
            assert FC.hamming(g, K[c["partner"]]) == [c["p"], c["q"]]
        elif kind == "same0":
            assert halves(g, K[c["partner"]]) == [0, 0]
        elif kind == "same1":
            assert halves(g, K[c["partner"]]) == [1, 1]
        elif kind in ("star_absent", "star_present"):
            assert FC.hamming(c["centre"], g) == [h - 1] and FC.hamming(c["centre"], K[c["arm"]]) == [h] and halves(g, K[c["arm"]]) == [0, 1]
            assert (c["centre"] in K) == (kind == "star_present") and (kind == "star_absent" or K[c["centre_id"]] == c["centre"])
        elif kind == "twin":
            assert FC.hamming(g, K[c["partner"]]) == [c["p"]]
        elif kind == "d1_d2":
            assert halves(g, K[c["partner"]]) == [0, 1, 1] and c["p"] in FC.hamming(g, K[c["partner"]])
        else:
            same, apart = (slice(0, h), slice(h, L)) if kind == "share_h0" else (slice(h, L), slice(0, h))
            group = [g] + [K[o] for o in c["others"]]
            assert len(group) == 3 and len({k[same] for k in group}) == 1 and len({k[apart] for k in group}) == 3
            assert sum(k[same] == g[same] for k in K) == 3                          # three in all: the tables hold four of a half


@pytest.mark.parametrize("L", LENGTHS)
def test_tables_exist_for_three_of_a_half_not_for_five(L):
    for lib in (FC.library(L), FC.pair_library(L) if L % 2 == 0 else None, FC.library(L, share=5)):
        if lib is None:
            continue
        starts = "0" if lib.parts == 1 else f"0,{L // 2}"
        e = Emu(features=list(lib.feats), miss=1, length=L // lib.parts, start=starts)
        assert e.lt_ok() == lib.lt and e.pt_parts() == 0
        e.close()
        if lib.parts == 1:
            e = Emu(features=list(lib.feats), pt_parts=3, miss=1, length=L, start=starts)
            assert e.pt_parts() == (3 if lib.pt else 0)
            e.close()
    assert FC.library(L).lt and not FC.library(L, share=5).lt and not FC.library(L, share=5).pt


def test_share5_library_takes_the_packed_tables():
    case = FC.block(FC.library(20, share=5), (0,))
    run = case.run(1)
    assert FC.expected_path(case, run) == FC.PATH_FIXED_PACKED == FC.expected_path(case, run, {"F2Q_PT_PARTS": "3"})
    (counts, stats, _, _), acct = _emu(case, run)
    assert (counts, stats) == FC.expect(case, **run) and not acct["lt_ok"] and acct["lt"] == 0 and acct["pt"] == 0


def test_big_libraries():
    for lib in (FC.big_library(20), FC.big_library(20, pairs=True)):
        assert len(lib) > FC.HIST_MAX and not lib.lt
    e = Emu(features=list(FC.big_library(20).feats), miss=1, length=20, start="0")
    assert not e.lt_ok() and e.pt_parts() > 0                    # the partitioned tables hold it: F2Q_NO_PT=1 keeps them out
    e.close()
    case = FC.block(FC.big_library(20), (4,))
    assert FC.expected_path(case, case.run(1)) == FC.PATH_FIXED_PACKED        # (a block below F2Q_PT_MIN_READS)
    assert FC.expected_path(case, case.run(1), {"F2Q_PT_MIN_READS": "0"}) == FC.PATH_FIXED_PART


# ---- the blocks --------------------------------------------------------------------------------------------------------

def _blocks():
    out = [_lds_case(mw, st, L, phred) for _, _, mw, st, L, phred, *_ in FC.MATRIX_LDS]
    out += [FC.block(FC.multi_library(name, L), starts) for _, name, starts, L, _ in FC.MATRIX_MULTI if name != "big"]
    return list(dict.fromkeys(out))


def test_every_kind_occurs():
    """in every block of two cycles or more, every kind that applies to its starts; the one-partial-tile block holds the
    first 37 kinds of the cycle"""
    for case in _blocks() + FC.tile_blocks(FC.library(20))[1:] + FC.tile_blocks(FC.multi_library("mixed", 20), (2, 15))[1:]:
        kinds = FC.MW_KINDS if len(case.starts) > 1 else FC.KINDS
        assert case.n >= 2 * len(kinds)
        assert set(case.kinds) == {k for k in kinds if FC.applies(k, case.starts)}, case.starts
        for w in range(0, case.n - 63, 128):                     # waves with and without a flagged read
            assert any("N" in s for s, _ in case.recs[w:w + 64]) and not any("N" in s for s, _ in case.recs[w + 64:w + 128])
    small = FC.tile_blocks(FC.library(20))[0]
    assert small.n == 37 and small.kinds == [k if FC.applies(k, (0,)) else "exact" for k in FC.KINDS[:37]]
    assert FC.block(FC.library(20), (0,)) is FC.block(FC.library(20), (0,))     # one object: the cached expectations key on it


def test_block_shape():
    for case in _blocks():
        end = max(case.starts) + case.l
        assert case.n == FC.N17 + 37
        for (s, q), kind in zip(case.recs, case.kinds):
            assert set(s) <= set("ACGTNacgt") and 1 <= len(s) <= end + 12
            assert (len(q) != len(s)) == (kind in ("qlen_short", "qlen_long"))
            assert (len(s) < end) == (kind in ("end_in_win", "end_before_win")) and (kind != "end_at_win" or len(s) == end)
            assert all(ord(c) < 128 for c in q)
        assert FC.general_reads(case, case.run(1)) == sum(k in ("qlen_short", "qlen_long") or (len(case.starts) > 1 and k in ("end_in_win", "end_before_win"))
                                                          for k in case.kinds)


@pytest.mark.parametrize("st,L", [(0, 20), (3, 17), (5, 14), (2, 21)])
def test_kinds_do_what_they_say(st, L):
    """one read of each kind alone, --ph 30: the verdict the kind is named for (and the feature, where the kind names one)"""
    case = FC.block(FC.library(L), (st,))
    lib, K = case.lib, case.lib.keys
    P, I, NA, QF = [1, 1, 0, 0, 0], [1, 0, 1, 0, 0], [1, 0, 0, 1, 0], [1, 0, 0, 0, 1]
    want = {"exact": (P, P, P), "sub_first": (NA, I, I), "sub_last": (NA, I, I), "sub_half_lo": (NA, I, I), "sub_half_hi": (NA, I, I),
            "sub2_split": (NA, NA, I), "sub2_same_half": (NA, NA, I),
            "cross_a": (NA, NA, None), "cross_b": (NA, NA, None), "same0": (NA, NA, None), "same1": (NA, NA, None), "star_centre": (NA, NA, None),
            "twin_third": (NA, NA, None), "twin_n": (NA, NA, None), "star_exact": (P, P, P), "d1_d2": (NA, I, I),
            "share_exact": (P, P, P), "share_near_other_half": (NA, I, I), "share_near_same_half": (NA, I, I),
            "n_first": (NA, I, I), "n_last": (NA, I, I), "n_mid": (NA, I, I), "n2": (NA, NA, I), "sub1_n1": (NA, NA, I),
            "n_before": (P, P, P), "n_after": (P, P, P), "q_before": (P, P, P), "q_after": (P, P, P), "q_pass_first": (P, P, P),
            "q_1f": (P, P, P), "q_7f": (P, P, P), "q_first": (QF, QF, QF), "q_last": (QF, QF, QF), "q_bang": (QF, QF, QF), "q_and_n": (QF, QF, QF),
            "lower": (P, P, P), "lower_sub": (NA, I, I), "end_in_win": (NA, NA, NA), "end_before_win": (NA, NA, NA), "end_at_win": (P, P, P),
            "qlen_long": (P, P, P)}
    seen = {}
    for i, kind in enumerate(case.kinds):
        if kind not in want or seen.get(kind, 0) >= 3 or (kind == "exact" and i % 16 == 5):
            continue
        seen[kind] = seen.get(kind, 0) + 1
        for miss in (0, 1, 2):
            if want[kind][miss] is not None:
                counts, st5 = FC.verdict_of(case, i, **case.run(miss))
                assert st5 == want[kind][miss], (kind, miss, case.recs[i])
    assert set(seen) == {k for k in want if FC.applies(k, case.starts)}
    # the feature: star_exact the centre, d1_d2 the guide at --m 1 and --m 2
    for kind, who in (("star_exact", "centre_id"), ("d1_d2", "guide")):
        k = 0
        for i, kd in enumerate(case.kinds):
            if kd == kind:
                con = lib.by_kind[FC.TIE_KINDS[kind][0]][k % FC.N_CONSTELLATIONS]
                k += 1
                for miss in ((0, 1, 2) if kind == "star_exact" else (1, 2)):
                    assert FC.verdict_of(case, i, **case.run(miss))[0] == {con[who]: 1}
                if k >= 3:
                    break
    # the rule's border: --ph 29 passes the byte --ph 30 fails
    i = case.kinds.index("q_first")
    assert FC.verdict_of(case, i, **case.run(1, phred=29))[1] == P and FC.verdict_of(case, i, **case.run(1, phred=31))[1] == QF
    i = case.kinds.index("q_pass_first")
    assert FC.verdict_of(case, i, **case.run(1, phred=31))[1] == QF


def test_multi_window_part_kinds():
    """several windows: a low byte in one part shortens the key (no pair feature matches; against the mixed library the
    part that passed can be a one-part feature), one in every part fails the read"""
    case = FC.block(FC.pair_library(20), (2, 15))
    run = case.run(1)
    for kind, st5 in (("part_q_fail_one", [1, 0, 0, 1, 0]), ("part_q_fail_all", [1, 0, 0, 0, 1]),
                      ("part_q_edge_lo", [1, 0, 0, 1, 0]), ("part_q_edge_hi", [1, 0, 0, 1, 0]), ("q_first", [1, 0, 0, 1, 0]), ("exact", [1, 1, 0, 0, 0]),
                      ("q_after", [1, 1, 0, 0, 0]), ("cross_a", [1, 0, 0, 1, 0]), ("star_centre", [1, 0, 0, 1, 0])):
        assert FC.verdict_of(case, case.kinds.index(kind), **run)[1] == st5, kind


def test_q_and_n_shares_a_quality_word():
    for case in _blocks():
        W, both = len(case.starts), set()
        for (s, q), kind in zip(case.recs, case.kinds):
            if kind == "q_and_n":
                a, b = s.index("N"), q.index(FC.lowq(case.phred))
                stored = (lambda p: p) if W == 1 else (lambda p: next(w * case.l + p - st for w, st in enumerate(case.starts) if st <= p < st + case.l))
                assert abs(stored(a) - stored(b)) == 1 and stored(a) // 4 == stored(b) // 4 and s.count("N") == 1
                both.add(a < b)
        assert both == {True, False}


def test_tile_count_blocks():
    for lib, starts in ((FC.library(20), (0,)), (FC.library(20), (4,)), (FC.multi_library("mixed", 20), (2, 15))):
        blocks = FC.tile_blocks(lib, starts)
        assert [b.n for b in blocks] == [37, 256 + 37, 15 * 256 + 37, 16 * 256 + 37, 32 * 256 + 37]
        assert [-(-b.n // 256) for b in blocks] == [1, 2, 16, 17, 33]
        for case in blocks:
            for miss in (0, 1):
                run = case.run(miss)
                want = FC.expect(case, **run)
                _all_five(want[1], case.n, miss)
                for kw in ({}, {"pt_parts": 3}, {"lt": False}):
                    if len(starts) > 1 and kw:
                        continue
                    (counts, stats, fast, gen), _ = _emu(case, run, **kw)
                    assert (counts, stats) == want and gen == FC.general_reads(case, run)
        # 33 tiles on 16 waves: three tiles on one wave, two on the others
        assert sorted({len(range(w, 33, 16)) for w in range(16)}) == [2, 3]


def test_skewed_block():
    lib = FC.library(20)
    case = FC.skewed(lib)
    assert case.n == 80000 and not any("N" in s for s, _ in case.recs) and all(len(s) == len(q) for s, q in case.recs)
    assert not any(FC.SKEW_HOT in (c["guide"], c.get("partner"), c.get("arm"), c.get("centre_id")) or FC.SKEW_HOT in c.get("others", ()) for c in lib.cons)
    run = case.run(1)
    counts, stats = FC.expect(case, **run)
    assert stats[0] == 80000 and counts[FC.SKEW_HOT] > 2 * 0x8000 and stats[2] > 20000
    counts0, _ = FC.expect(case, **case.run(0))
    assert 0x8000 < counts0[FC.SKEW_HOT] < counts[FC.SKEW_HOT]   # exact hits alone pass 0x8000 once
    assert FC.expected_path(case, run) == FC.PATH_FIXED_LDS and FC.general_reads(case, run) == 0
    assert FC.expected_path(case, run, {"F2Q_PT_PARTS": "3", "F2Q_LT_WGS": "1"}) == FC.PATH_FIXED_PART
    for kw in ({}, {"pt_parts": 3}):
        (ecounts, estats, _, gen), _ = _emu(case, run, **kw)
        assert (ecounts, estats) == (counts, stats) and gen == 0


# ---- the lane logic on every block, every way ----------------------------------------------------------------------------

@pytest.mark.parametrize("miss", [0, 1, 2])
@pytest.mark.parametrize("st,L,phred", sorted({(st, L, phred) for _, _, mw, st, L, phred, *_ in FC.MATRIX_LDS if not mw}))
def test_lane_logic_equals_oracle(st, L, phred, miss):
    """with the LDS tables, dealt into 3, 12 and 20 partitions, on the packed tables and one read per lane"""
    case = FC.block(FC.library(L), (st,), phred=phred)
    run = case.run(miss)
    want = FC.expect(case, **run)
    ways = [({}, "lt"), ({"pt_parts": 3}, "pt"), ({"pt_parts": 12}, "pt"), ({"pt_parts": 20}, "pt"), ({"lt": False}, None), ({"v2": False}, None)]
    for kw, decided in ways:
        if miss > 1 and decided:
            continue                                             # (--m 2: neither kind of tables is built)
        (counts, stats, fast, gen), acct = _emu(case, run, **kw)
        assert (counts, stats) == want, kw
        assert gen == FC.general_reads(case, run) and fast + gen == case.n
        assert (acct["lt"] > case.n // 2) == (decided == "lt") and (acct["pt"] > case.n // 2) == (decided == "pt")
        assert acct["lt"] == 0 or acct["pt"] == 0
        assert "pt_parts" not in kw or acct["parts"] == kw["pt_parts"]
