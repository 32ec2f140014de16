"""The Extract+Count (mode="EC") kernels, every template instance and every stage pinned: k_extract_anchor_hot (24
instances), k_extract_fixed4_hot<LEARN>, the stepped k_count_anchor / k_count_anchor_pairs / k_extract_fixed4, the hot
set's build and re-link, the three deferred passes and the device rehashes count the designed blocks of
tests/ec_cases.py through the C ABI.  Keys, counts and first-seen order exactly equal to the oracle's, the five
statistics too; every hot-path run equal, first-read indices included, to the stepped run (F2Q_NO_HOT=1) of the same
blocks; the launches that ran (the `[f2q sync] <step> done` lines of F2Q_TRACE_SYNC=1) equal to what ec_cases derives from
the input; the kernel family (`timing["path"]`) and the reads outside the packed tiles too.  The designed blocks are
4352 + 37 reads or fewer.  The larger ones: the fixed tile walk's last block, 8741 reads for 33 packed tiles; the hot
set's capacity, 72 000 + 26 000 reads at 12 000 keys and 198 000 + 68 000 at 33 000; the single-word table's growth,
8192 + 120 000 + 2048 reads; the byte-string table's, 2 x 4024; a full table, 141 024 (the sizes are derived in ec_cases).

Measured on an MI355X in one session: this module's 72 tests in 5.7 s, the slowest test_table_full[anchored] at 0.90 s
(141 024 reads, twice); tests/test_fixed_kernels_gpu.py, 173 tests, in 10.2 s, its slowest at 0.67 s."""
import re

import pytest

import ec_cases as EC
from conftest import pkg

pytestmark = pytest.mark.gpu

ENV = ("F2Q_LT_WGS", "F2Q_NO_HOT", "F2Q_HOT_LEARN", "F2Q_FORCE_GENERAL", "F2Q_EC_STEP", "F2Q_NO_LT", "F2Q_NO_PW")
NO_HOT = {"F2Q_NO_HOT": "1"}


@pytest.fixture(scope="module")
def P():
    return pkg()


def _steps(capfd):
    return [s for s in re.findall(r"\[f2q sync\] (.*) done", capfd.readouterr().err) if s in EC.STEPS]


def _count(P, monkeypatch, capfd, blocks, run, env, bases=None, reset_before=()):
    """counts the blocks in a fresh context under `env` -> (rows with their first-read index, stats, timings, the steps of
    each block)"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("F2Q_TRACE_SYNC", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    capfd.readouterr()
    timings, steps = [], []
    with P.Counter(**run) as c:
        for i, b in enumerate(blocks):
            if i in reset_before:
                c.reset()
            if bases is not None:
                c.set_read_base(bases[i])
            _, t = c.count_block(b.fq, want_timing=True)
            timings.append(t); steps.append(_steps(capfd))
        _, stats = c.read_counts()
        rows = c.ec_results()
    assert _steps(capfd) == []
    return rows, [int(x) for x in stats], timings, steps


def _check(P, monkeypatch, capfd, case, run, env, path, steps=None, general=None):
    """one block in a fresh context: everything a check here asserts"""
    want_rows, want_stats = EC.expect(case, **run)
    rows, stats, (t,), (got_steps,) = _count(P, monkeypatch, capfd, [case], run, env)
    assert stats == want_stats
    assert [(k, n) for k, n, _ in rows] == want_rows             # keys, counts and the first-seen order
    if path is not None:
        assert t["path"] == path
    assert t["fast_reads"] + t["general_reads"] == case.n
    assert t["general_reads"] == (EC.general_reads(case, run) if general is None else general)
    if steps is not None:
        assert got_steps == steps
    return rows, stats, got_steps


def _no_hot_step(steps):
    return not set(steps) & set(EC.HOT_STEPS)


def _hot_and_stepped(P, monkeypatch, capfd, case, run, env, steps, path=EC.PATH_EXTRACT, general_too=False):
    """the hot-key path, then the stepped kernels on the same block: the same rows (first-read index included) and stats"""
    hot = _check(P, monkeypatch, capfd, case, run, env, path, steps)
    stepped = _check(P, monkeypatch, capfd, case, run, dict(env, **NO_HOT), path)
    assert stepped[:2] == hot[:2] and _no_hot_step(stepped[2])
    if general_too:                                              # every read a raw record: k_count_general alone
        general = _check(P, monkeypatch, capfd, case, run, {"F2Q_FORCE_GENERAL": "1"}, None, general=case.n)
        assert general[:2] == hot[:2] and _no_hot_step(general[2])
    return hot


@pytest.mark.parametrize("max_len,ms,extra,anchors", EC.HOT_MATRIX, ids=lambda v: str(v))
def test_hot_single_pair_instances(P, monkeypatch, capfd, max_len, ms, extra, anchors):
    """k_extract_anchor_hot<NW, KB, SAMEQ, true> on 4 learning tiles, the hot set's build, <.., false> on the other 13, the
    deferred passes the block's reads need; then k_count_anchor<NW, KB, true, false, SQ> (F2Q_NO_HOT=1) on the same block"""
    case, run = EC.block(max_len), EC.run_kw(anchors, ms, **extra)
    steps = EC.stages(case, run)
    assert steps[:3] == [EC.S_LEARN, EC.S_BUILD, EC.S_HOT] and len(EC.instances(case, run)) == 2
    _hot_and_stepped(P, monkeypatch, capfd, case, run, {"F2Q_HOT_LEARN": EC.LEARN}, steps, general_too=ms == 1 and not extra)


def test_stepped_wide_reads(P, monkeypatch, capfd):
    """reads of up to 200 bases (NW = 10): the hot-key kernels have no such instance, k_count_anchor<10, ..> counts them"""
    case, run = EC.block(200), EC.run_kw("both", 1)
    assert EC.nw_of(case) == 10
    _, _, steps = _check(P, monkeypatch, capfd, case, run, {"F2Q_HOT_LEARN": EC.LEARN}, EC.PATH_EXTRACT)
    assert _no_hot_step(steps)


@pytest.mark.parametrize("max_len,ms,extra", EC.PAIR_MATRIX, ids=lambda v: str(v))
def test_two_pairs(P, monkeypatch, capfd, max_len, ms, extra):
    """k_count_anchor_pairs in Extract+Count mode: a read's parts joined with ':' (byte-string table), a read with one part
    alone a single-word key"""
    case, run = EC.pair_block(max_len), EC.run_kw(ms=ms, pairs=True, **extra)
    keys = [k for k, _ in EC.expect(case, **run)[0]]
    assert any(":" in k for k in keys) and any(k and ":" not in k for k in keys)
    rows, stats, steps = _check(P, monkeypatch, capfd, case, run, {"F2Q_HOT_LEARN": EC.LEARN}, EC.PATH_PAIRS)
    assert _no_hot_step(steps)
    if ms == 0:
        general = _check(P, monkeypatch, capfd, case, run, {"F2Q_FORCE_GENERAL": "1"}, None, general=case.n)
        assert general[:2] == (rows, stats)


@pytest.mark.parametrize("st,L,phred", EC.FIXED_ROWS, ids=lambda v: str(v))
def test_fixed_window(P, monkeypatch, capfd, st, L, phred):
    """k_extract_fixed4_hot<true> on 4 tiles, the build, <false> on the rest; then k_extract_fixed4 (F2Q_NO_HOT=1).  The
    blocks hold reads that end inside the window and before it, and windows with 'N's (a single-word key where they fit)"""
    case = EC.fixed_block(st, L, phred)
    run = EC.fixed_run(case)
    _hot_and_stepped(P, monkeypatch, capfd, case, run, {"F2Q_HOT_LEARN": EC.LEARN}, [EC.S_LEARN, EC.S_BUILD, EC.S_HOT],
                     general_too=(st, L, phred) == (3, 17, 30))


@pytest.mark.parametrize("learn", [256, 1000000], ids=["learn_256", "all_learning"])
@pytest.mark.parametrize("wgs", [None, "1"], ids=["all_cus", "one_workgroup"])
@pytest.mark.parametrize("which", range(4), ids=["1_tile", "2_tiles", "4_tiles", "17_tiles"])
def test_anchored_tile_walk(P, monkeypatch, capfd, which, wgs, learn):
    """three groups of 256 threads per workgroup, two tiles in flight each: in one workgroup (F2Q_LT_WGS=1) idle groups,
    a partial last tile, a second round for some groups (5 tiles) and six rounds for all (18)"""
    case, run = EC.tile_blocks()[which], EC.run_kw("both", 1)
    env = dict({"F2Q_HOT_LEARN": learn}, **({"F2Q_LT_WGS": wgs} if wgs else {}))
    _hot_and_stepped(P, monkeypatch, capfd, case, run, env, EC.stages(case, run, learn))


@pytest.mark.parametrize("learn", [256, 1000000], ids=["learn_256", "all_learning"])
@pytest.mark.parametrize("wgs", [None, "1"], ids=["all_cus", "one_workgroup"])
@pytest.mark.parametrize("which", range(5), ids=[f"{t}_tiles" for t in EC.FC.TILE_COUNTS])
def test_fixed_tile_walk(P, monkeypatch, capfd, which, wgs, learn):
    """one wave per tile, 16 waves per workgroup: in one workgroup fewer tiles than waves, one more than 16, three rounds.
    The stepped run checks the first-read indices the later rounds give"""
    case = EC.fixed_tile_blocks()[which]
    run = EC.fixed_run(case)
    env = dict({"F2Q_HOT_LEARN": learn}, **({"F2Q_LT_WGS": wgs} if wgs else {}))
    _hot_and_stepped(P, monkeypatch, capfd, case, run, env, EC.stages(case, run, learn))


@pytest.mark.parametrize("wgs", [None, "1"], ids=["all_cus", "one_workgroup"])
@pytest.mark.parametrize("which", [3, 4], ids=["17_tiles", "33_tiles"])
def test_fixed_tile_walk_with_the_set(P, monkeypatch, capfd, which, wgs):
    """the set learnt on the designed block of the same library; then every tile of the 17- and the 33-tile block goes
    through k_extract_fixed4_hot<false>: in one workgroup a second round for one wave, and a third"""
    a, b = EC.fixed_block(0, 20), EC.fixed_tile_blocks()[which]
    run = EC.fixed_run(a)
    env = dict({"F2Q_HOT_LEARN": EC.LEARN}, **({"F2Q_LT_WGS": wgs} if wgs else {}))
    want_rows, want_stats = EC.expect((a, b), **run)
    rows, stats, timings, steps = _count(P, monkeypatch, capfd, [a, b], run, env)
    assert stats == want_stats
    assert [(k, n) for k, n, _ in rows] == want_rows
    assert steps == [EC.stages(a, run), [EC.S_HOT]]
    for t, blk in zip(timings, (a, b)):
        assert t["path"] == EC.PATH_EXTRACT and t["fast_reads"] + t["general_reads"] == blk.n
        assert t["general_reads"] == EC.general_reads(blk, run)
    stepped = _count(P, monkeypatch, capfd, [a, b], run, dict(env, **NO_HOT))
    assert stepped[:2] == (rows, stats) and all(_no_hot_step(s) for s in stepped[3])


def _blocks_vs_oracle(P, monkeypatch, capfd, blocks, run, env, steps):
    """several blocks of plain ACGT(N) reads in one context, hot path and stepped: rows, stats, steps per block"""
    want_rows, want_stats = EC.expect(tuple(blocks), **run)
    rows, stats, timings, got = _count(P, monkeypatch, capfd, blocks, run, env)
    assert stats == want_stats
    assert [(k, n) for k, n, _ in rows] == want_rows
    assert got == steps
    for t, b in zip(timings, blocks):
        assert t["path"] == EC.PATH_EXTRACT and t["general_reads"] == 0 and t["fast_reads"] == b.n
    stepped = _count(P, monkeypatch, capfd, blocks, run, dict(env, **NO_HOT))
    assert stepped[:2] == (rows, stats) and all(_no_hot_step(s) for s in stepped[3])
    return rows


@pytest.mark.parametrize("n_keys", [12000, 33000], ids=["past_hot_cap", "past_candidate_list"])
def test_hot_set_capacity(P, monkeypatch, capfd, n_keys):
    """every key of block A reaches F2Q_HOT_MINCOUNT while learning, so the input forces more candidates than the set has
    room for (F2Q_HOT_CAP) and, at 33 000 keys, than the candidate list has (F2Q_HOT_CAND); the CPU preconditions count
    them.  Which keys the build admits is not observable and does not matter: block B counts two reads of every key, hot
    or cold, and 2000 new ones, and the result is exact either way"""
    a, b = EC.capacity_blocks(n_keys)
    rows = _blocks_vs_oracle(P, monkeypatch, capfd, [a, b], EC.FIXED20, {"F2Q_HOT_LEARN": a.n}, [[EC.S_LEARN], [EC.S_BUILD, EC.S_HOT]])
    assert sorted(n for _, n, _ in rows) == [1] * 2000 + [8] * n_keys


def test_single_word_table_grows_with_a_hot_set(P, monkeypatch, capfd):
    """ec_reserve grows the single-word table before block B's launch: the hot keys' slots move (k_ec_hot_relink), and their
    reads in B and C are counted through the re-linked set"""
    a, b, c, hot = EC.growth_blocks()
    steps = [[EC.S_LEARN, EC.S_BUILD, EC.S_HOT], [EC.S_REHASH64, EC.S_RELINK, EC.S_HOT], [EC.S_HOT]]
    rows = _blocks_vs_oracle(P, monkeypatch, capfd, [a, b, c], EC.FIXED20, {"F2Q_HOT_LEARN": EC.LEARN}, steps)
    got = {k: n for k, n, _ in rows}
    assert sum(got[k] for k in hot) == 8 * EC.GROW_HOT + (a.n - EC.LEARN) + EC.GROW_B_HOT + c.n


def test_byte_string_table_grows(P, monkeypatch, capfd):
    """more than 4096 keys of 31 bases over two blocks: the byte-string table is re-hashed on the device"""
    a, b = EC.bytes_blocks()
    run = EC.run_kw("both", 0)
    steps = [[EC.S_LEARN, EC.S_BUILD, EC.S_HOT, EC.S_KEYS], [EC.S_REHASHB, EC.S_HOT, EC.S_KEYS]]
    rows = _blocks_vs_oracle(P, monkeypatch, capfd, [a, b], run, {"F2Q_HOT_LEARN": EC.LEARN}, steps)
    assert sum(len(k) == 31 for k, _, _ in rows) == 2 * EC.BYTES_KEYS


@pytest.mark.parametrize("fixed", [False, True], ids=["anchored", "fixed_window"])
def test_table_full(P, monkeypatch, capfd, fixed):
    """more new keys than the single-word table has slots: the inserts that find it full are set aside (in tiles behind
    slot_base = 1024, some with an 'N'), the table grows with the hot set valid, and the deferred pass inserts them"""
    case = EC.full_block(fixed)
    run = EC.FIXED20 if fixed else EC.run_kw("both", 0)
    steps = [[EC.S_LEARN, EC.S_BUILD, EC.S_HOT, EC.S_REHASH64, EC.S_RELINK, EC.S_FIXED if fixed else EC.S_SLOW]]
    rows = _blocks_vs_oracle(P, monkeypatch, capfd, [case], run, {"F2Q_HOT_LEARN": EC.LEARN}, steps)
    assert len(rows) == EC.FULL_HOT + EC.FULL_NEW and sum("N" in k for k, _, _ in rows) == EC.FULL_NEW // 16


def test_accumulate_and_reset(P, monkeypatch, capfd):
    """two blocks without a reset add up (the second through the set the first has learnt); after reset() the set is learnt
    again and a block counts as on its own"""
    a, b = EC.block(150), EC.tile_blocks()[2]
    run = EC.run_kw("both", 1)
    both, only_b = EC.expect((a, b), **run), EC.expect(b, **run)
    later = [s for s in EC.stages(b, run) if s not in (EC.S_LEARN, EC.S_BUILD)]
    env = {"F2Q_HOT_LEARN": EC.LEARN}
    rows, stats, _, steps = _count(P, monkeypatch, capfd, [a, b], run, env)
    assert ([(k, n) for k, n, _ in rows], stats) == both and steps == [EC.stages(a, run), later]
    assert _count(P, monkeypatch, capfd, [a, b], run, dict(env, **NO_HOT))[:2] == (rows, stats)
    rows, stats, _, steps = _count(P, monkeypatch, capfd, [a, b], run, env, reset_before=(1,))
    assert ([(k, n) for k, n, _ in rows], stats) == only_b and steps == [EC.stages(a, run), EC.stages(b, run)]
    assert _count(P, monkeypatch, capfd, [a, b], run, dict(env, **NO_HOT), reset_before=(1,))[:2] == (rows, stats)


def test_blocks_out_of_read_index_order(P, monkeypatch, capfd):
    """the block with the LOWER read indices counted second, through the hot set the first has learnt: a hot key's first
    read is lowered all the same (reads below the set's highest first read take the table's insert)"""
    x, y = EC.block(150), EC.block(150, seed=2)
    run = EC.run_kw("both", 1)
    want_rows, want_stats = EC.expect((x, y), **run)
    later = [s for s in EC.stages(x, run) if s not in (EC.S_LEARN, EC.S_BUILD)]
    res = []
    for env in ({"F2Q_HOT_LEARN": EC.LEARN}, {"F2Q_HOT_LEARN": EC.LEARN, **NO_HOT}):
        rows, stats, _, steps = _count(P, monkeypatch, capfd, [y, x], run, env, bases=[x.n, 0])
        assert stats == want_stats and [(k, n) for k, n, _ in rows] == want_rows
        if "F2Q_NO_HOT" in env:
            assert all(_no_hot_step(s) for s in steps)
        else:
            assert steps == [EC.stages(y, run), later]
        res.append((rows, stats))
    assert res[0] == res[1]
