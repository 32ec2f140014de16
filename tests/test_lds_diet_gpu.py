"""k_count_fixed4_lds after its instruction diet (lane-mask verdicts in the exact stage, the one-test settle of the
pending histogram adds, the dot-product flag gather, tags built from the hash products): small blocks through the C ABI,
counts and the five statistics exactly equal to the oracle's.  Every block is a few thousand reads (17 tiles of 256: not a
multiple of the 16 waves of a workgroup) except the skewed one, which needs 80 000 reads in ONE workgroup (F2Q_LT_WGS=1)
so that a u16 counter passes 0x8000 twice."""
import random

import pytest

from conftest import pkg
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N17 = 17 * 256


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def LIB(P):
    return P.binding.synth_library(0xD1E7, 2000, 20)


def _fastq(reads):
    return "".join(f"@r{i}\n{s}\n+\n{q}\n" for i, (s, q) in enumerate(reads)).encode()


def _oracle(lib, kw, *blocks):
    return O.count_fastq_parallel(b"".join(blocks), 4, features=[(str(i), s) for i, s in enumerate(lib)], **kw)


PATH_FIXED_LDS, PATH_MULTI_LDS = 3, 10                      # f2q.h: both are k_count_fixed4_lds


def _check(P, lib, kw, fq, all_fast=True, path=PATH_FIXED_LDS):
    orc = _oracle(lib, kw, fq)
    with P.Counter(features=lib, **kw) as c:
        _, t = c.count_block(fq, want_timing=True)
        counts, stats = c.read_counts()
    assert list(stats) == orc.stats()
    assert list(counts) == orc.counts()
    assert t["path"] == path                                # the kernel under test counted the block, no other
    assert not all_fast or t["general_reads"] == 0          # (reads that end before the last window go the general way)
    return list(counts), list(stats)


def _sub(rng, s, at=None):
    p = rng.randrange(len(s)) if at is None else at
    return s[:p] + rng.choice([b for b in "ACGT" if b != s[p]]) + s[p + 1:]


def _tail(rng, n=10):
    return "".join(rng.choice("ACGT") for _ in range(n))


@pytest.mark.parametrize("miss", [1, 0], ids=["m1", "m0"])
def test_short_block(P, LIB, miss):
    kw = dict(miss=miss, phred=30, length=20, start="0")
    with P.Counter(features=LIB, **kw) as c:
        fq = bytes(c.synth_fastq(seed=171, n_reads=N17, read_len=150))
    _, stats = _check(P, LIB, kw, fq)
    assert stats[0] == N17 and stats[1] > 0 and stats[4] > 0


def test_skewed_library_one_workgroup(P, LIB, monkeypatch):
    """one guide takes 70 000 of 80 000 reads, a third of them through the batch stage (one substitution); one workgroup
    counts them all, so its counter passes 0x8000 twice, with pending adds of both stages"""
    rng = random.Random(5)
    hot = LIB[7]
    reads = [(hot if i % 3 else _sub(rng, hot)) + _tail(rng) for i in range(70000)]
    reads += [rng.choice(LIB) + _tail(rng) for _ in range(10000)]
    rng.shuffle(reads)
    fq = _fastq([(s, "I" * len(s)) for s in reads])
    monkeypatch.setenv("F2Q_LT_WGS", "1")
    counts, stats = _check(P, LIB, dict(miss=1, phred=30, length=20, start="0"), fq)
    assert stats[0] == 80000
    assert counts[7] > 2 * 0x8000                           # what the input is for (the count itself is the oracle's, above)


def test_every_read_one_mismatch(P, LIB):
    rng = random.Random(6)
    fq = _fastq([(_sub(rng, rng.choice(LIB)) + _tail(rng), "I" * 30) for _ in range(N17 + 37)])
    _, stats = _check(P, LIB, dict(miss=1, phred=30, length=20, start="0"), fq)
    assert stats[1] == 0 and stats[2] > 0.9 * (N17 + 37)            # four full batches per tile


def test_no_batch_candidates(P, LIB):
    rng = random.Random(7)
    fq = _fastq([(rng.choice(LIB) + _tail(rng), "I" * 30) for _ in range(N17)])
    _, stats = _check(P, LIB, dict(miss=1, phred=30, length=20, start="0"), fq)
    assert stats[1] == N17


@pytest.mark.parametrize("phred", [30, 20], ids=["ph30", "ph20_rule_off"])
@pytest.mark.parametrize("miss", [1, 0], ids=["m1", "m0"])
def test_rare_paths_together(P, LIB, miss, phred):
    """N inside the window (one or two, on exact and on one-substitution reads), reads that end inside the window,
    reads failing the Phred rule in exactly one byte -- the first or the last of the window -- and a low byte just past
    the window (which must not fail)"""
    rng = random.Random(8)
    reads = []
    for i in range(N17 + 5):
        g = rng.choice(LIB)
        s, q = g + _tail(rng), ["I"] * 30
        k = i % 8
        if k == 1:
            p = rng.randrange(20); s = s[:p] + "N" + s[p + 1:]
        elif k == 2:
            p = rng.randrange(20); s = _sub(rng, s[:20]) + s[20:]; s = s[:p] + "N" + s[p + 1:]
        elif k == 3:
            n = rng.randrange(0, 20); s, q = s[:n], q[:n]
        elif k == 4:
            q[0 if i % 16 < 8 else 19] = ">"                     # Q29: fails --ph 30
        elif k == 5:
            q[20] = "#"                                         # past the window
        elif k == 6:
            p, r = rng.sample(range(20), 2); s = s[:p] + "N" + s[p + 1:]; s = s[:r] + "N" + s[r + 1:]
        reads.append((s, "".join(q)[:len(s)]))
    _, stats = _check(P, LIB, dict(miss=miss, phred=phred, length=20, start="0"), _fastq(reads))
    assert (stats[4] > 0) == (phred >= 33)


def test_counter_bookkeeping(P, LIB):
    """two blocks counted without a reset add up; after a reset a block counts as on its own"""
    kw = dict(miss=1, phred=30, length=20, start="0")
    with P.Counter(features=LIB, **kw) as c:
        a = bytes(c.synth_fastq(seed=21, n_reads=N17, read_len=150))
        b = bytes(c.synth_fastq(seed=22, n_reads=3001, read_len=150))
        both, only_b = _oracle(LIB, kw, a, b), _oracle(LIB, kw, b)
        c.count_block(a); c.count_block(b)
        counts, stats = c.read_counts()
        assert list(stats) == both.stats() and list(counts) == both.counts()
        c.reset()
        c.count_block(b)
        counts, stats = c.read_counts()
        assert list(stats) == only_b.stats() and list(counts) == only_b.counts()


@pytest.mark.parametrize("miss", [1, 0], ids=["m1", "m0"])
def test_other_instantiations(P, LIB, miss):
    """the two-window (MW) instance; a 20-base window that starts at 3: six quality rows (nq = 6), the generic instance
    <0, 0, ., false>; and one that starts at 4: five quality rows, two base rows, no 16-aligned start: <5, 2, ., false>"""
    from test_lane_logic_cpu import multi_window_uniform_case
    lib2, fq2 = multi_window_uniform_case("0,20", 10, 40, n_feat=1500, n_reads=N17, seed=11)
    _check(P, lib2, dict(miss=miss, length=10, start="0,20"), fq2, all_fast=False, path=PATH_MULTI_LDS)
    kw = dict(miss=miss, phred=30, length=20, start="3")
    with P.Counter(features=LIB, **kw) as c:
        fq = bytes(c.synth_fastq(seed=33, n_reads=N17, read_len=150, start=3))
    _, stats = _check(P, LIB, kw, fq)
    assert stats[1] > 0
    kw = dict(miss=miss, phred=30, length=20, start="4")
    with P.Counter(features=LIB, **kw) as c:
        fq = bytes(c.synth_fastq(seed=34, n_reads=N17, read_len=150, start=4))
    _, stats = _check(P, LIB, kw, fq)
    assert stats[1] > 0
