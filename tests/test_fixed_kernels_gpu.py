"""The fixed-window (--st/--l) Counter kernels, every template instance pinned: k_count_fixed4_lds (paths 3 and 10),
k_part_scatter + k_part_count (path 4), k_count_fixed4 (path 2), k_count_multi4 (path 5) and k_count_fixed (path 1) count
the small designed blocks of tests/fixed_cases.py through the C ABI; counts and the five statistics exactly equal to the
oracle's, the kernel family that ran (`timing["path"]`) equal to what choose_path must pick for the run, and the number
of reads outside the packed tiles equal to what the packer's rules give.  Which template instance a row reaches is
stated by the row and checked on the CPU (tests/test_fixed_cases_cpu.py).  Every block is 4352 + 37 reads or fewer,
except the 33-tile block of the tile walk (8229 reads: three and two tiles per wave of one workgroup) and the skewed one,
which needs 80 000 reads in ONE workgroup (F2Q_LT_WGS=1) so that a u16 counter passes 0x8000 twice.

Wall time on one MI355X, same session: this module 10.6 s (173 tests, the slowest 0.67 s: the 24 961-feature library of
the LDS = false rows), tests/test_anchor_kernels_gpu.py 4.4 s (77 tests, the slowest 0.96 s)."""
import pytest

import fixed_cases as FC
from conftest import pkg

pytestmark = pytest.mark.gpu

ENV = ("F2Q_LT_WGS", "F2Q_NO_LT", "F2Q_NO_PT", "F2Q_PT_PARTS", "F2Q_PT_CHUNK", "F2Q_PT_MIN_READS", "F2Q_GENERIC", "F2Q_FORCE_V1",
       "F2Q_FORCE_GENERAL")


@pytest.fixture(scope="module")
def P():
    return pkg()


def _count(P, monkeypatch, case, run, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    with P.Counter(features=list(case.lib.feats), **run) as c:
        _, t = c.count_block(case.fq, want_timing=True)
        counts, stats = c.read_counts()
    return [int(x) for x in counts], [int(x) for x in stats], t


def _check(P, monkeypatch, case, run, path, env=None):
    """counts the block in a fresh context under `env`; everything a check here asserts"""
    want_counts, want_stats = FC.expect(case, **run)
    assert FC.expected_path(case, run, env) == path
    counts, stats, t = _count(P, monkeypatch, case, run, env)
    assert stats == want_stats
    assert counts == want_counts
    assert t["path"] == path                                     # the kernel under test counted the block, no other
    assert t["fast_reads"] + t["general_reads"] == case.n
    assert t["general_reads"] == FC.general_reads(case, run, env)
    return counts, stats


def _check_general(P, monkeypatch, case, run, first):
    """the same block with every read a raw record (F2Q_FORCE_GENERAL=1): no packed tiles, the results of `first`"""
    assert _check(P, monkeypatch, case, run, FC.PATH_NONE, env={"F2Q_FORCE_GENERAL": "1"}) == first


def _ids(v):
    if isinstance(v, dict):
        return "env" + "".join(f"_{k}={x}" for k, x in v.items())
    return "_".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("variant,near,mw,st,L,phred,miss,env", FC.MATRIX_LDS, ids=_ids)
def test_lds_kernel_instances(P, monkeypatch, variant, near, mw, st, L, phred, miss, env):
    """k_count_fixed4_lds<{0,0 | 5,2}, NEAR, A20, MW>: the 12 instances, and each run again on the run-time geometry
    (F2Q_GENERIC=1): specialised and generic instance on the same block"""
    lib = FC.pair_library(L) if mw else FC.library(L)
    case = FC.block(lib, st if mw else (st,), phred=phred)
    run, path = case.run(miss), FC.PATH_MULTI_LDS if mw else FC.PATH_FIXED_LDS
    first = _check(P, monkeypatch, case, run, path, env)
    assert _check(P, monkeypatch, case, run, path, dict(env, F2Q_GENERIC="1")) == first
    if (variant, st, near) in (("a20", 16, True), ("a20", (2, 15), True)):
        _check_general(P, monkeypatch, case, run, first)


@pytest.mark.parametrize("chunk", [None, FC.PART_CHUNK], ids=["one_round", "five_rounds"])
@pytest.mark.parametrize("variant,pw,near,st,L,phred,miss,parts", FC.MATRIX_PART, ids=_ids)
def test_partitioned_kernel_instances(P, monkeypatch, variant, pw, near, st, L, phred, miss, parts, chunk):
    """k_part_scatter<{0,0 | 5,2}, A20, PW 16 | 8 | 4> x k_part_count<NEAR>, the block in one round and cut into five by
    F2Q_PT_CHUNK; each run again with F2Q_GENERIC=1"""
    case = FC.block(FC.library(L), (st,), phred=phred)
    run = case.run(miss)
    env = {"F2Q_PT_PARTS": str(parts)}
    if chunk:
        env["F2Q_PT_CHUNK"] = chunk
    first = _check(P, monkeypatch, case, run, FC.PATH_FIXED_PART, env)
    assert _check(P, monkeypatch, case, run, FC.PATH_FIXED_PART, dict(env, F2Q_GENERIC="1")) == first
    if (variant, pw, near, chunk) == ("spec52", 8, True, None):
        _check_general(P, monkeypatch, case, run, first)


def _packed_case(variant, st, L, big):
    return FC.block(FC.big_library(L) if big else FC.library(L), (st,))


@pytest.mark.parametrize("lds,variant,st,L,miss,big", FC.MATRIX_PACKED, ids=_ids)
def test_packed_kernel_instances(P, monkeypatch, lds, variant, st, L, miss, big):
    """k_count_fixed4<LDS, {5,2 | 0,0}> (F2Q_NO_LT=1 F2Q_NO_PT=1) at --m 0..3; LDS = false: F2Q_HIST_MAX + 1 features,
    the feature index of every read in hit_buf and k_hist_ranges"""
    case = _packed_case(variant, st, L, big)
    run = case.run(miss)
    first = _check(P, monkeypatch, case, run, FC.PATH_FIXED_PACKED, FC.PACKED_ENV)
    if big:
        assert sum(first[0][FC.HIST_MAX:]) > 0
    if (variant, miss) == ("spec52", 1):
        _check_general(P, monkeypatch, case, run, first)


def _multi_case(name, starts, L):
    return FC.block(FC.multi_library(name, L), starts)


@pytest.mark.parametrize("lds,name,starts,L,miss", FC.MATRIX_MULTI, ids=_ids)
def test_multi_kernel_instances(P, monkeypatch, lds, name, starts, L, miss):
    """k_count_multi4<true | false>: features of several part counts, --m 2, and F2Q_HIST_MAX + 1 pair features"""
    case = _multi_case(name, starts, L)
    run = case.run(miss)
    first = _check(P, monkeypatch, case, run, FC.PATH_MULTI)
    if name == "big":
        assert sum(first[0][FC.HIST_MAX:]) > 0
    if (name, miss) == ("mixed", 1):
        _check_general(P, monkeypatch, case, run, first)


@pytest.mark.parametrize("lds,st,L,miss,big", FC.MATRIX_V1, ids=_ids)
def test_v1_kernel_instances(P, monkeypatch, lds, st, L, miss, big):
    """k_count_fixed<true | false> (F2Q_FORCE_V1=1): one read per lane on the same tiles"""
    case = _packed_case(None, st, L, big)
    run = case.run(miss)
    first = _check(P, monkeypatch, case, run, FC.PATH_FIXED_V1, FC.V1_ENV)
    if (st, big) == (0, False):
        _check_general(P, monkeypatch, case, run, first)


WALKS = {"lds": ((0,), FC.PATH_FIXED_LDS, {}), "part": ((0,), FC.PATH_FIXED_PART, {"F2Q_PT_PARTS": "3"}),
         "packed": ((4,), FC.PATH_FIXED_PACKED, FC.PACKED_ENV), "multi": ((2, 15), FC.PATH_MULTI, {})}


@pytest.mark.parametrize("wgs", [None, "1"], ids=["all_cus", "one_workgroup"])
@pytest.mark.parametrize("miss", [1, 0], ids=["m1", "m0"])
@pytest.mark.parametrize("which", range(len(FC.TILE_COUNTS)), ids=[f"{t}_tiles" for t in FC.TILE_COUNTS])
@pytest.mark.parametrize("kernel", list(WALKS))
def test_tile_walk(P, monkeypatch, kernel, which, miss, wgs):
    """one partial tile, fewer tiles than waves, as many, one more, and 33: in one workgroup (F2Q_LT_WGS=1) the waves of
    k_count_fixed4_lds and k_part_scatter<.., 16> take three and two tiles, those of k_count_fixed4 / k_count_multi4
    (fewer waves) more; with all CUs most workgroups have idle waves"""
    starts, path, env = WALKS[kernel]
    lib = FC.multi_library("mixed", 20) if kernel == "multi" else FC.library(20)
    case = FC.tile_blocks(lib, starts)[which]
    _check(P, monkeypatch, case, case.run(miss), path, dict(env, F2Q_LT_WGS=wgs) if wgs else env)


@pytest.mark.parametrize("miss", [1, 0], ids=["m1", "m0"])
@pytest.mark.parametrize("kernel", ["lds", "part"])
def test_counter_hand_off(P, monkeypatch, kernel, miss):
    """one feature takes 70 000 of 80 000 reads, a third of them at distance 1; one workgroup of k_count_fixed4_lds counts
    them all, and with three partitions and one scatter workgroup one workgroup of k_part_count nearly all: its u16 counter
    passes 0x8000 twice (--m 0: once, through the exact hits alone)"""
    _, path, env = WALKS[kernel]
    case = FC.skewed(FC.library(20))
    counts, stats = _check(P, monkeypatch, case, case.run(miss), path, dict(env, F2Q_LT_WGS="1"))
    assert stats[0] == 80000
    assert counts[FC.SKEW_HOT] > (2 if miss else 1) * 0x8000     # what the input is for (the count itself is the oracle's, above)


@pytest.mark.parametrize("kernel", ["lds", "part", "packed_big"])
def test_accumulate_and_reset(P, monkeypatch, kernel):
    """two blocks counted without a reset add up (slab rows and k_reduce_slabs; the slabs k_part_reduce clears; hit_buf,
    written anew for every block); after a reset a block counts as on its own"""
    starts, path, env = WALKS["packed" if kernel == "packed_big" else kernel]
    lib = FC.big_library(20) if kernel == "packed_big" else FC.library(20)
    a, b = FC.block(lib, starts), FC.tile_blocks(lib, starts)[2]
    run = a.run(1)
    both, only_b = FC.expect((a, b), **run), FC.expect(b, **run)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with P.Counter(features=list(lib.feats), **run) as c:
        _, ta = c.count_block(a.fq, want_timing=True)
        _, tb = c.count_block(b.fq, want_timing=True)
        counts, stats = c.read_counts()
        assert ([int(x) for x in counts], [int(x) for x in stats]) == both
        c.reset()
        _, tb2 = c.count_block(b.fq, want_timing=True)
        counts, stats = c.read_counts()
        assert ([int(x) for x in counts], [int(x) for x in stats]) == only_b
    for t, case in ((ta, a), (tb, b), (tb2, b)):
        assert t["path"] == path and t["general_reads"] == FC.general_reads(case, run) and t["fast_reads"] + t["general_reads"] == case.n
