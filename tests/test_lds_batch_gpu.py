"""k_count_fixed4_lds's two stages on the GPU: the exact stage on table 0 for every read, the compacted batch of the
reads that need the --m 1 search, and histogram adds tested one stage late.  Through the C ABI, against the oracle for
small blocks and bit for bit against the pigeonhole kernel (F2Q_NO_LT=1, u32 histogram) for large ones, at the
extremes of the batch stage: several batches per tile, none, many flagged reads, a partial last tile, and one counter
passing 0x8000 many times with adds from both stages."""
import pytest

from conftest import pkg, sprinkle_symbols
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return pkg()


def _block(P, monkeypatch, env, lib, kw, spec, guides=None):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with P.Counter(features=lib, **kw) as c:
        blk = c.synth_create(guides=guides if guides is not None else lib, **spec)
        t = c.count_resident(blk)
        counts, stats = c.read_counts()
        blk.free()
    for k in env:
        monkeypatch.delenv(k)
    return list(counts), list(stats), t


def _fastq_vs_oracle(P, lib, kw, fq):
    orc = O.count_fastq_parallel(fq, 8, features=[(str(i), s) for i, s in enumerate(lib)], **kw)
    with P.Counter(features=lib, **kw) as c:
        _, t = c.count_block(fq, want_timing=True)
        counts, stats = c.read_counts()
    assert list(stats) == orc.stats() and list(counts) == orc.counts()
    assert t["general_reads"] == 0
    return list(stats)


SPECS = {
    "all_candidates": dict(p_sub=0.97, p_rand=0.02, p_n=0.0, p_lowq=0.0, p_q29=0.0, p_q28=0.0),   # (a) several batches per tile
    "no_candidates": dict(p_sub=0.0, p_rand=0.0, p_n=0.0, p_lowq=0.0, p_q29=0.0, p_q28=0.0),      # (b) every read an exact hit
    "flagged": dict(p_sub=0.2, p_rand=0.05, p_n=0.6, p_lowq=0.05),                               # (c) many flagged reads
}


@pytest.mark.parametrize("miss", [1, 0], ids=["m1", "m0"])                                     # (f) --m 0 on the same reads
@pytest.mark.parametrize("name", list(SPECS))
@pytest.mark.parametrize("n_reads", [60000, 100003])                                          # (d) a partial last tile
def test_batch_extremes_vs_oracle(P, miss, name, n_reads):
    lib = P.binding.synth_library(0xB47C, 3000, 20)
    kw = dict(miss=miss, phred=30, length=20, start="0")
    spec = dict(SPECS[name], seed=17 + n_reads, n_reads=n_reads, read_len=150)
    with P.Counter(features=lib, **kw) as c:
        fq = bytes(c.synth_fastq(**spec))
    stats = _fastq_vs_oracle(P, lib, kw, fq)
    if name == "no_candidates":
        assert stats[1] == n_reads
    elif name == "all_candidates" and miss:
        assert stats[2] > 0.9 * n_reads


@pytest.mark.parametrize("name", list(SPECS))
def test_batch_extremes_large_vs_pigeonhole(P, monkeypatch, name):
    lib = P.binding.synth_library(0xB47D, 10000, 20)
    kw = dict(miss=1, phred=30, length=20, start="0")
    spec = dict(SPECS[name], seed=0x5EED, n_reads=8_000_003, read_len=150)
    a = _block(P, monkeypatch, {}, lib, kw, spec)
    b = _block(P, monkeypatch, {"F2Q_NO_LT": "1"}, lib, kw, spec)
    assert a[:2] == b[:2]
    assert a[1][0] == 8_000_003 and a[1][0] == sum(a[1][1:])


def test_counter_handoff_from_both_stages(P, monkeypatch):
    """(e) two guides take all 40 M reads, about half of them one substitution away: every workgroup's counters of the
    two pass 0x8000 with adds from the exact stage and from the batch stage"""
    lib = P.binding.synth_library(0xB47E, 10000, 20)
    kw = dict(miss=1, phred=30, length=20, start="0")
    spec = dict(seed=0xC0DE, n_reads=40_000_000, read_len=150, p_sub=0.5, p_rand=0.0, p_n=0.0, p_lowq=0.0, p_q29=0.0, p_q28=0.0)
    a = _block(P, monkeypatch, {}, lib, kw, spec, guides=lib[:2])
    b = _block(P, monkeypatch, {"F2Q_NO_LT": "1"}, lib, kw, spec, guides=lib[:2])
    assert a[:2] == b[:2]
    counts, stats = a[0], a[1]
    assert stats[0] == 40_000_000 and 0.4 < stats[2] / stats[0] < 0.6
    assert counts[0] + counts[1] == stats[1] + stats[2] and min(counts[0], counts[1]) > 15_000_000


def test_two_windows_on_batched_kernel(P, monkeypatch):
    """(f) the two-window (MW) instance of the kernel with dense mutations and N symbols, against the oracle and F2Q_NO_LT=1"""
    from test_lane_logic_cpu import multi_window_uniform_case
    lib, fq = multi_window_uniform_case("0,20", 10, 40, n_feat=2000, n_reads=60000, seed=7)
    fq = sprinkle_symbols(fq, 5, rate=0.01)
    kw = dict(miss=1, length=10, start="0,20")
    orc = O.count_fastq_parallel(fq, 8, features=[(str(i), s) for i, s in enumerate(lib)], **kw)
    for env in ({}, {"F2Q_NO_LT": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with P.Counter(features=lib, **kw) as c:
            _, t = c.count_block(fq, want_timing=True)
            counts, stats = c.read_counts()
        for k in env:
            monkeypatch.delenv(k)
        assert list(stats) == orc.stats() and list(counts) == orc.counts(), env
