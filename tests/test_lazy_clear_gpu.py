"""The counting step in two dispatches: f2q_reset_counts only marks the accumulators "to be cleared", the first
k_reduce_slabs of the step stores its sums (later ones add), the rare u16 hand-off of the library-in-LDS kernels is
credited to Accum::carry and folded in by the reduce, and every other reader or writer of the accumulators materialises
the pending clear first.  Small blocks through the C ABI, counts and the five statistics exactly equal to the oracle's.
Blocks are 17 tiles of 256 reads (not a multiple of the 16 waves of a workgroup) unless a case says otherwise; the
library is the 2 000-guide synthetic one."""
import random

import numpy as np
import pytest

from conftest import pkg
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N17 = 17 * 256
PATH_FIXED_PACKED, PATH_FIXED_LDS, PATH_MULTI_LDS = 2, 3, 10    # f2q.h: the paths whose kernels meet the accumulators in k_reduce_slabs only


@pytest.fixture(scope="module")
def P():
    return pkg()


@pytest.fixture(scope="module")
def LIB(P):
    return P.binding.synth_library(0xD1E7, 2000, 20)


def _kw(miss=1):
    return dict(miss=miss, phred=30, length=20, start="0")


def _fastq(reads):
    return "".join(f"@r{i}\n{s}\n+\n{q}\n" for i, (s, q) in enumerate(reads)).encode()


def _oracle(lib, kw, *blocks):
    return O.count_fastq_parallel(b"".join(blocks), 4, features=[(str(i), s) for i, s in enumerate(lib)], **kw)


def _same(c, orc):
    counts, stats = c.read_counts()
    assert list(stats) == orc.stats()
    assert list(counts) == orc.counts()


def _zeros(c):
    counts, stats = c.read_counts()
    assert not np.any(stats) and not np.any(counts)


def _sub(rng, s):
    p = rng.randrange(len(s))
    return s[:p] + rng.choice([b for b in "ACGT" if b != s[p]]) + s[p + 1:]


def _tail(rng, n=10):
    return "".join(rng.choice("ACGT") for _ in range(n))


def test_reset_then_read(P, LIB):
    kw = _kw()
    with P.Counter(features=LIB, **kw) as c:
        fq = bytes(c.synth_fastq(seed=41, n_reads=N17, read_len=150))
        c.count_block(fq)
        counts, stats = c.read_counts()
        assert stats[0] == N17 and counts.sum() > 0
        c.reset()
        _zeros(c)                                           # no count between the reset and the read
        c.count_block(fq)
        c.reset(); c.reset()
        _zeros(c)
        c.count_block(fq)                                   # ... and the context counts on as a fresh one
        _same(c, _oracle(LIB, kw, fq))


@pytest.mark.parametrize("miss", [1, 0], ids=["m1", "m0"])
def test_store_then_add(P, LIB, miss):
    kw = _kw(miss)
    with P.Counter(features=LIB, **kw) as c:
        a = bytes(c.synth_fastq(seed=42, n_reads=N17, read_len=150))
        b = bytes(c.synth_fastq(seed=43, n_reads=3001, read_len=150))
        both, only_b = _oracle(LIB, kw, a, b), _oracle(LIB, kw, b)
        c.count_block(b)                                    # something for the reset to forget
        c.reset()
        _, t = c.count_block(a, want_timing=True)           # the step's first reduce stores
        assert t["path"] == PATH_FIXED_LDS and t["general_reads"] == 0
        c.count_block(b)                                    # the second adds
        _same(c, both)
        c.reset()
        c.count_block(a)
        c.reset()
        c.count_block(b)
        _same(c, only_b)


def test_handoff_through_carry(P, LIB, monkeypatch):
    """the skewed block of test_lds_diet_gpu.py: one workgroup counts 80 000 reads, 70 000 of them of one guide, so that
    guide's u16 counter passes 0x8000 twice and is credited through carry[]; then a reset and a small block on the same
    context: carry[] went back to zero and nothing of the first job survives"""
    rng = random.Random(5)
    hot = LIB[7]
    reads = [(hot if i % 3 else _sub(rng, hot)) + _tail(rng) for i in range(70000)]
    reads += [rng.choice(LIB) + _tail(rng) for _ in range(10000)]
    rng.shuffle(reads)
    fq = _fastq([(s, "I" * len(s)) for s in reads])
    kw = _kw()
    monkeypatch.setenv("F2Q_LT_WGS", "1")
    with P.Counter(features=LIB, **kw) as c:
        small = bytes(c.synth_fastq(seed=44, n_reads=N17, read_len=150))
        c.reset()
        _, t = c.count_block(fq, want_timing=True)
        assert t["path"] == PATH_FIXED_LDS and t["general_reads"] == 0
        counts, stats = c.read_counts()
        orc = _oracle(LIB, kw, fq)
        assert list(stats) == orc.stats() and list(counts) == orc.counts()
        assert counts[7] > 2 * 0x8000                       # what the input is for
        c.reset()
        c.count_block(small)
        _same(c, _oracle(LIB, kw, small))


EDGE_NF = (1, 63, 64, 65, 2000, 2001)


@pytest.fixture(scope="module")
def EDGE(P):
    """per library size: the library, a 17-tile block and a block of 17 workgroups' worth of tiles (30-base reads: the
    window is all the kernel looks at), each with its oracle"""
    out = {}
    kw = _kw()
    for nf in EDGE_NF:
        lib = P.binding.synth_library(0xED6E + nf, nf, 20)
        with P.Counter(features=lib, **kw) as c:
            small = bytes(c.synth_fastq(seed=50 + nf, n_reads=N17, read_len=150))
            wide = bytes(c.synth_fastq(seed=60 + nf, n_reads=(16 * 16 + 1) * 256, read_len=30))
        out[nf] = (lib, small, _oracle(lib, kw, small), wide, _oracle(lib, kw, wide))
    return out


@pytest.mark.parametrize("rows", [1, 2, 17])
@pytest.mark.parametrize("nf", EDGE_NF)
def test_reduce_edges(P, EDGE, monkeypatch, nf, rows):
    """feature counts that are no multiple of 4 (rows that are not 16-byte aligned: 4-byte loads) or of the 64 features a
    workgroup of the reduce owns, and two that are (64, 2 000: the 16-byte loads the flagship workload takes, the last
    workgroup partly filled with 2 000), over one, two and seventeen slab rows -- with seventeen, row lane 0 sums two live
    rows and every other lane's second row is the clamped last one; stored (first step after a reset), then added to"""
    lib, small, orc_small, wide, orc_wide = EDGE[nf]
    fq, orc = (wide, orc_wide) if rows == 17 else (small, orc_small)
    monkeypatch.setenv("F2Q_LT_WGS", str(rows))
    with P.Counter(features=lib, **_kw()) as c:
        c.reset()
        _, t = c.count_block(fq, want_timing=True)
        assert t["path"] in (PATH_FIXED_LDS, PATH_FIXED_PACKED)
        _same(c, orc)
        c.count_block(fq)                                   # add mode over the same rows
        counts, stats = c.read_counts()
        assert list(stats) == [2 * v for v in orc.stats()] and list(counts) == [2 * v for v in orc.counts()]


def test_reduce_second_round(P, monkeypatch):
    """k_count_fixed4 (F2Q_NO_LT=1) runs up to two workgroups per CU: 2 049 x 8 tiles make 257 workgroups and slab rows
    on a device of 128 CUs or more, one more than the 16 row lanes x 16 rows a thread of the reduce takes per round"""
    kw = _kw()
    lib = P.binding.synth_library(0x2B0D, 64, 20)
    monkeypatch.setenv("F2Q_NO_LT", "1")
    with P.Counter(features=lib, **kw) as c:
        fq = bytes(c.synth_fastq(seed=48, n_reads=(256 * 8 + 1) * 256, read_len=30))
        orc = _oracle(lib, kw, fq)
        c.reset()
        _, t = c.count_block(fq, want_timing=True)
        assert t["path"] == PATH_FIXED_PACKED and t["general_reads"] == 0
        _same(c, orc)
        c.count_block(fq)
        counts, stats = c.read_counts()
        assert list(stats) == [2 * v for v in orc.stats()] and list(counts) == [2 * v for v in orc.counts()]


def _mixed_two_windows(P, LIB):
    """two windows: a read that ends before the last window does leaves the tiles for the raw-record kernel"""
    from test_lane_logic_cpu import multi_window_uniform_case
    lib, mixed = multi_window_uniform_case("0,20", 10, 40, n_feat=1500, n_reads=N17, seed=13)
    recs = mixed.split(b"\n")
    pure = b"".join(b"\n".join(recs[i:i + 4]) + b"\n" for i in range(0, len(recs) - 1, 4) if len(recs[i + 1]) == 40)
    return lib, dict(miss=1, length=10, start="0,20"), pure, mixed, PATH_MULTI_LDS


def _mixed_one_window(P, LIB):
    """one window: a read that ends inside it stays in the tiles (every fifth read here); what leaves them is a read whose
    quality line has another length than its sequence (every seventh)"""
    rng = random.Random(9)
    reads = []
    for i in range(N17):
        s = rng.choice(LIB) + _tail(rng)
        if i % 5 == 0:
            s = s[:rng.randrange(1, 20)]
        reads.append((s, "I" * (len(s) - 1 if i % 7 == 0 and i % 5 else len(s))))
    kw = _kw()
    with P.Counter(features=LIB, **kw) as c:
        pure = bytes(c.synth_fastq(seed=45, n_reads=N17, read_len=150))
    return LIB, kw, pure, _fastq(reads), PATH_FIXED_LDS


@pytest.mark.parametrize("case", [_mixed_two_windows, _mixed_one_window], ids=["two_windows", "one_window"])
def test_mixed_step(P, LIB, case):
    """a block whose reads partly take the general path: the tiles are counted by a slab-reducing launch, the other reads
    by the raw-record kernel, which adds directly, in one step -- as the first step after a reset, and following a pure
    tile step without one"""
    lib, kw, pure, mixed, path = case(P, LIB)
    with P.Counter(features=lib, **kw) as c:
        c.count_block(pure)
        c.reset()
        _, t = c.count_block(mixed, want_timing=True)
        assert t["general_reads"] > 0 and t["fast_reads"] > 0 and t["path"] == path
        _same(c, _oracle(lib, kw, mixed))
        c.reset()
        _, t = c.count_block(pure, want_timing=True)
        assert t["general_reads"] == 0 and t["path"] == path
        c.count_block(mixed)
        _same(c, _oracle(lib, kw, pure, mixed))


def test_pointer_handed_out(P, LIB):
    """whoever holds f2q_counts_device_ptr may read device memory at any time: from then on a reset clears at once"""
    import json
    import os
    import subprocess
    import sys
    kw = _kw()
    with P.Counter(features=LIB, **kw) as c:
        a = bytes(c.synth_fastq(seed=46, n_reads=N17, read_len=150))
        orc = _oracle(LIB, kw, a)
        c.count_block(a)
        c.reset()                                           # a pending clear when the pointer is handed out
        ptr, n64 = c.counts_device_ptr()
        assert ptr and n64 == len(LIB) + 5
        _zeros(c)
        c.count_block(a)
        _same(c, orc)
        c.reset()
        _zeros(c)
        c.count_block(a); c.count_block(a)                  # the reduce adds from the first step on
        counts, stats = c.read_counts()
        assert list(stats) == [2 * v for v in orc.stats()] and list(counts) == [2 * v for v in orc.counts()]
    # the same through a torch tensor over the pointer, in a process of its own (torch's HIP runtime is not initialised in
    # this one): the scenario of tests/_lazy_clear_ptr_worker.py on the same block
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lazy_clear_ptr_worker.py")
    run = subprocess.run([sys.executable, worker], stdout=subprocess.PIPE, text=True, timeout=240, check=True)
    got = json.loads(run.stdout.strip().splitlines()[-1])
    want, zero = orc.counts() + orc.stats(), [0] * (len(LIB) + 5)
    assert got["n64"] == len(LIB) + 5
    assert got["handed_out"] == zero
    assert got["counted"] == want
    assert got["reset"] == zero                             # device memory, no call of the library after the reset
    assert got["reset_read_counts"] == zero
    assert got["counted_again"] == want


def test_queued_steps(P, LIB):
    kw = _kw()
    with P.Counter(features=LIB, **kw) as c:
        fq = bytes(c.synth_fastq(seed=47, n_reads=N17, read_len=150))
        blk = c.block_from_fastq(fq)
        c.queued_times()
        for _ in range(3):
            c.reset()
            c.count_resident_queued(blk)
        times = c.queued_times()
        assert len(times) == 3 and all(t > 0 for t in times)
        _same(c, _oracle(LIB, kw, fq))                      # the counts of one job
        blk.free()
