"""The raw-record kernels on the device -- k_count_general<false|true>, the four k_count_umi instances, k_count_umi_pair in
both layouts, k_count_demux<false|true> -- on the inputs of tests/raw_edge_cases.py: records at the edge of the per-lane
staging area in every alignment, odd records on the UMI / header-UMI / paired-UMI / demultiplexing contexts, and launches
in which every lane takes the grid-stride loop twice.  Everything is compared for exact equality with the plain-Python
expectation (proven against the CPU emulations in tests/test_raw_edge_cpu.py), and on UMI and demultiplexing contexts with
the counts and the five counters of a plain context as well.

The packers and the cells they reach (raw_edge_cases.device_cells / host_cells / pair_cells): the device packer hands the
kernels the text's own offsets, so a single-end sample reaches all 16 (so & 3, qo & 3) pairs with mq + qn = 191, 192, 193
each; under F2Q_HOST_PACK=1 and on merged pairs the records lie back to back, qo = so + r, so mq follows from ms and r --
every ms on both sides of 192, a quarter of the (ms, mq) pairs."""
import functools

import pytest

import raw_edge_cases as RE
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return pkg()


def umi_result(c):
    counts, stats = c.read_counts()
    umis, ok, bad = c.read_umis()
    return list(counts), list(stats), list(umis), ok, bad


def demux_result(c):
    counts, stats = c.read_counts()
    matrix, sstats, verdicts = c.read_demux()
    return list(counts), list(stats), matrix.tolist(), sstats.tolist(), list(verdicts)


def table(c):
    f, codes, reads = c.umi_pairs()
    return list(zip(f.tolist(), codes.tolist(), reads.tolist()))


def result_of(c):
    if c.sample_barcodes:
        return demux_result(c)
    if c.umi_length:
        return umi_result(c)
    counts, stats = c.read_counts()
    return ([(k, n) for k, n, _ in c.ec_results()] if c.mode == "EC" else list(counts)), list(stats)


_PLAIN = {}


def plain_result(P, lib, texts, **kw):
    """(counts, stats) of a plain context on its usual road, once per input and run"""
    key = (len(lib), tuple(lib[:2]), tuple(texts), RE.UC.run_key(kw))
    if key not in _PLAIN:
        with P.Counter(features=lib, **kw) as c:
            if len(texts) == 2:
                c.count_block_paired(*texts)
            else:
                c.count_block(texts[0])
            counts, stats = c.read_counts()
        _PLAIN[key] = (list(counts), list(stats))
    return _PLAIN[key]


def set_packer(monkeypatch, packer):
    if packer == "host":
        monkeypatch.setenv("F2Q_HOST_PACK", "1")
    else:
        monkeypatch.delenv("F2Q_HOST_PACK", raising=False)


# ---- 1. the edge sweep, every instance -------------------------------------------------------------------------------------
@pytest.mark.parametrize("packer", ["device", "host"])
@pytest.mark.parametrize("name", list(RE.EDGE_CONTEXTS))
@pytest.mark.parametrize("r", RE.EDGE_R)
def test_edge_sweep(P, monkeypatch, r, name, packer):
    tail, anchored, what = RE.EDGE_CONTEXTS[name]
    lib, bcs, fq, _ = RE.edge_sample(r, tail, anchored)
    run, want = RE.edge_run(name, r), RE.edge_expect(name, r)
    set_packer(monkeypatch, packer)
    kw = {}
    if what.get("umi"):
        kw = dict(umi=(r - 8, 8), umi_reads=bool(what.get("umi_reads")))
    elif what.get("umi_header"):
        kw = dict(umi_header=("_", 8), umi_reads=bool(what.get("umi_reads")))
    elif what.get("demux"):
        monkeypatch.setenv("F2Q_DEMUX_TABLE", what["demux"])
        kw = dict(sample_barcodes=(r - 8, [b.decode() for b in bcs]), barcode_mismatch=1)
    else:
        monkeypatch.setenv("F2Q_FORCE_GENERAL", "1")
    with P.Counter(features=None if what.get("mode") == "EC" else lib, **kw, **run) as c:
        used, t = c.count_block(fq, want_timing=True)
        got = result_of(c)
        assert used == len(fq) and t["general_reads"] == want[1][0] == len(RE.layout(fq))      # the intended kernel ran
        assert tuple(got) == tuple(want), (r, name, packer)
        if RE.edge_table(name, r) is not None:
            assert table(c) == RE.edge_table(name, r)
    if kw:
        monkeypatch.delenv("F2Q_DEMUX_TABLE", raising=False)
        assert tuple(got[:2]) == plain_result(P, lib, [fq], **run)


@pytest.mark.parametrize("packer", ["device", "host"])
@pytest.mark.parametrize("ctx", ["paired_m0", "paired_m1", "umi_paired_stage0", "umi_paired_stage1", "umi_paired_stage1_sets"])
@pytest.mark.parametrize("rc2", [False, True], ids=["fwd", "rc2"])
def test_edge_sweep_on_merged_pairs(P, monkeypatch, rc2, ctx, packer):
    lib, fq1, fq2, _ = RE.edge_pairs(rc2)
    set_packer(monkeypatch, packer)
    geom = dict(start=str(RE.PAIR_ST1[0]), start2=str(RE.PAIR_ST2[0]), rc2=rc2, length=RE.UP.LEN, phred=RE.PH)
    n = len(RE.PC.records(fq1))
    if ctx.startswith("paired"):
        miss = int(ctx[-1])
        monkeypatch.setenv("F2Q_FORCE_GENERAL", "1")
        with P.Counter(features=lib, miss=miss, **geom) as c:
            used, t = c.count_block_paired(fq1, fq2, want_timing=True)
            counts, stats = c.read_counts()
        assert used == (len(fq1), len(fq2)) and t["general_reads"] == n
        assert (list(counts), list(stats)) == RE.pair_expect(lib, fq1, fq2, rc2, miss)
        return
    monkeypatch.setenv("F2Q_UMI_PAIR_STAGE", ctx[16])
    keep = not ctx.endswith("sets")
    want = RE.pair_umi_expect(lib, fq1, fq2, rc2, 1)
    with P.Counter(features=lib, umi_paired=RE.UP.TWO, umi_reads=keep, miss=1, **geom) as c:
        used, t = c.count_block_paired(fq1, fq2, want_timing=True)
        assert used == (len(fq1), len(fq2)) and t["general_reads"] == n == want.stats[0]
        got = umi_result(c)
        assert tuple(got) == (want.counts, want.stats, RE.UP.umis_of(want), want.ok, want.bad)
        if keep:
            assert table(c) == RE.UP.table_of(want)
    monkeypatch.delenv("F2Q_UMI_PAIR_STAGE")
    assert tuple(got[:2]) == plain_result(P, lib, [fq1, fq2], miss=1, **geom)


# ---- 2. odd records --------------------------------------------------------------------------------------------------------
def count_odd(P, case, paths=None):
    """the case through count_block (paths: through count_file / count_file_paired) -> (result, table or None, bytes consumed)"""
    with P.Counter(features=case["lib"], **case["ctx"], **case["run"]) as c:
        paired = len(case["texts"]) == 2
        if paths:
            used = None
            (c.count_file_paired if paired else c.count_file)(*paths)
        elif paired:
            used = c.count_block_paired(*case["texts"])
        else:
            used = [c.count_block(case["texts"][0])]
        return result_of(c), table(c) if case["table"] else None, used


@pytest.mark.parametrize("lo", range(0, 300, 50))
def test_odd_records_count_block(P, lo):
    for seed in range(lo, lo + 50):
        case = RE.odd_case(seed)
        got, tab, used = count_odd(P, case)
        assert tuple(got) == tuple(case["expect"]()), (seed, case["kind"], case["run"])
        if case["table"]:
            assert tab == case["table"](), (seed, case["kind"])
        if case["used"]:
            assert used == case["used"](), (seed, case["kind"])
        assert tuple(got[:2]) == plain_result(P, case["lib"], case["texts"], **{k: v for k, v in case["ctx"].items() if k in ("start2", "rc2")},
                                              **case["run"]), (seed, case["kind"])


@pytest.mark.parametrize("lo", range(300, 360, 30))
def test_odd_records_count_file_in_small_pieces(P, tmp_path, monkeypatch, lo):
    monkeypatch.setenv("F2Q_FILE_CHUNK", "4096")                     # records and odd line ends fall on piece borders
    for seed in range(lo, lo + 30):
        case = RE.odd_case(seed)
        paths = []
        for k, text in enumerate(case["texts"]):
            path = tmp_path / ("s%d_R%d.fastq" % (seed, k + 1))
            path.write_bytes(text)
            paths.append(str(path))
        got, tab, _ = count_odd(P, case, paths)
        assert tuple(got) == tuple(case["expect"]()), (seed, case["kind"], case["run"])
        if case["table"]:
            assert tab == case["table"](), (seed, case["kind"])


# ---- 3. the second pass of the grid-stride loop --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def n_cu():
    """the device's multiProcessorCount, asked once in a child process: torch brings its own HIP runtime, and initialising it
    in this process next to the product's library leaves one of the two without a device (tests/test_abi_and_host.py)"""
    import subprocess
    import sys
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                           stdout=subprocess.PIPE, text=True, timeout=240, check=True)
    return int(probe.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("kind", RE.PASS_KINDS)
def test_second_pass(P, kind):
    cus = n_cu()
    fq, reps = RE.second_pass(kind, cus)
    pool = RE.pass_pool(kind)
    want = RE.scaled(kind, RE.pass_expect(kind, pool), reps)
    want_table = RE.scaled_table(RE.pass_table(kind, pool), reps)
    with P.Counter(features=RE.library(), **RE.pass_ctx(kind), **RE.PASS_RUN) as c:
        blk = c.block_from_fastq(fq)
        info = blk.info()
        assert info["n_general"] == info["n_reads"] == reps * RE.POOL and info["n_general"] > cus * 4096
        for again in (False, True):
            t = c.count_resident(blk)
            assert t["general_reads"] == info["n_general"]
            assert tuple(result_of(c)) == tuple(want), (kind, again)
            if want_table is not None:
                assert table(c) == want_table, (kind, again)
            c.reset()
        blk.free()
