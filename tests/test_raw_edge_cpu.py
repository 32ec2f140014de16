"""The raw-record road without a GPU: the preconditions of tests/raw_edge_cases.py (every alignment cell of the staging
edge occurs and has a record that feels its last byte), and its three families of inputs through the CPU emulations of the
per-lane logic (tests/emu: general_read with the UMI, header-UMI, paired-UMI and demultiplexing hooks, the host packers)
against the plain-Python expectations -- the inputs of tests/test_raw_edge_gpu.py, proven here first."""
import ctypes as C

import numpy as np
import pytest

import raw_edge_cases as RE
import test_demux_cpu as TD
import test_umi_cpu as TU
import test_umi_dir_cpu as TDIR
import test_umi_header_cpu as TH
import test_umi_pair_cpu as TP
from emu_helper import Emu

binding = TU.binding


def _features(L, set_features, h, lib):
    enc = [s.encode() for s in lib]
    offs = np.zeros(len(enc) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(b) for b in enc])
    set_features(h, b"".join(enc), offs.ctypes.data_as(C.POINTER(C.c_uint32)), len(enc))


def emu_plain(lib, fq, **run):
    """(counts or Extract+Count rows, stats, bytes consumed)"""
    e = Emu(features=lib, **run)
    used = e.count_block(fq)
    counts, stats, _, _ = e.read()
    out = (counts if lib is not None else [(k, n) for k, n, _ in e.ec_rows()]), stats, used
    e.close()
    return out


def emu_umi(lib, fq, umi, keep, **run):
    """((counts, stats, umis, valid, invalid), table or None, bytes consumed)"""
    e = (TDIR.DEmu if keep else TU.UEmu)(lib, umi, **run)
    used = e.L.uemu_count_block(e.h, fq, len(fq))
    got = e.state()[:5] if keep else e.read()[0]
    table = sorted(e.pairs()[0]) if keep else None
    e.L.uemu_destroy(e.h)
    return tuple(got), table, used


def emu_header(lib, fq, umi, keep, **run):
    L = TH._lib()
    p, _keep = binding.make_params(mode="C", **run)
    h = C.c_void_p(L.uemu_create(C.byref(p), 0, umi[1], 0))
    assert h
    _features(L, L.uemu_set_features, h, lib)
    used = L.hemu_count_block(h, fq, len(fq), umi[0], umi[1], int(keep))
    counts, umis = (C.c_int64 * len(lib))(), (C.c_int64 * len(lib))()
    stats, extra = (C.c_int64 * 5)(), (C.c_int64 * 2)()
    assert L.uemu_read(h, counts, stats, umis, extra) >= 0
    cap = sum(umis) + 1
    f, codes, reads = ((C.c_uint32 * cap)() for _ in range(3))
    n = L.hemu_pairs(h, f, codes, reads, cap)
    assert n == sum(umis)
    L.uemu_destroy(h)
    return (list(counts), list(stats), list(umis), extra[0], extra[1]), sorted(zip(f[:n], codes[:n], reads[:n])) if keep else None, used


def emu_demux(lib, fq, barcodes, at, miss_bc, **run):
    L = TD._lib()
    p, _keep = binding.make_params(mode="C", **run)
    h = C.c_void_p(L.demu_create(C.byref(p), b"".join(barcodes), len(barcodes), len(barcodes[0]), at, miss_bc))
    assert h
    _features(L, L.demu_set_features, h, lib)
    used = L.demu_count_block(h, fq, len(fq))
    nf, rows = len(lib), len(barcodes) + 1
    counts, stats, matrix, sstats, verdicts = (C.c_int64 * nf)(), (C.c_int64 * 5)(), (C.c_int64 * (rows * nf))(), (C.c_int64 * (rows * 5))(), (C.c_int64 * 5)()
    L.demu_read(h, counts, stats, matrix, sstats, verdicts)
    L.demu_destroy(h)
    return (list(counts), list(stats), [list(matrix[b * nf:(b + 1) * nf]) for b in range(rows)],
            [list(sstats[b * 5:(b + 1) * 5]) for b in range(rows)], list(verdicts)), used


# ---- (a) the staging edge ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", RE.EDGE_R)
def test_edge_samples_hold_every_cell(r):
    for tail, anchored in ((0, False), (8, False), (0, True)):
        cells = RE.check_edge_cells(r, tail, anchored)
        # the host packer (qo = so + r): mq follows from ms, so it reaches a quarter of the (ms, mq) pairs, at every ms
        host = RE.host_cells(RE.edge_sample(r, tail, anchored)[2])
        assert {c[0] for c in host if c[2] >= 188} == {0, 1, 2, 3} and all(c[1] == (c[2] & 3) for c in host)
        assert {RE.staged(c) for c in host} == {True, False} and len(cells) >= 48


def test_edge_samples_together_hold_all_144_cells():
    RE.check_edge_union()


@pytest.mark.parametrize("name", list(RE.EDGE_CONTEXTS))
@pytest.mark.parametrize("r", RE.EDGE_R)
def test_edge_cells_feel_their_last_bytes(r, name):
    n_seq, n_qual = RE.check_edge_sensitive(name, r)
    assert n_seq >= 4 and n_qual >= 4                                # (the per-cell claims are asserted inside; r = 193 with a tail: qn >= r in 4 cells)


def test_edge_kinds_come_out_as_designed():
    """bytes 31, 127 and 200 on the last quality byte pass --ph 30, '#' and byte 31 + ph fail it where a window reads it"""
    r = 190
    lib, bcs, fq, tags = RE.edge_sample(r)
    seen = set()
    for n, (ms, mq, b), kind in tags:
        perfect = RE.edge_expect("plain_m0", r, RE._one(fq, n))[1][1]
        if kind in ("exact", "q31_last", "q127_last", "q200_last"):
            assert perfect == 1, (n, kind)
        elif kind in ("q_hash_last", "q_top_last"):
            assert perfect == (b - mq > r), (n, kind)                # a quality line longer than r ends behind the window
        elif kind in ("sub_last", "n_last", "q_hash_first"):
            assert perfect == 0, (n, kind)
        seen.add(kind)
    assert seen == set(RE.KINDS) - {"q_hash_tail_first"}


@pytest.mark.parametrize("name", list(RE.EDGE_CONTEXTS))
@pytest.mark.parametrize("r", RE.EDGE_R)
def test_edge_emulation_equals_expectation(r, name):
    tail, anchored, what = RE.EDGE_CONTEXTS[name]
    lib, bcs, fq, _ = RE.edge_sample(r, tail, anchored)
    run, want = RE.edge_run(name, r), RE.edge_expect(name, r)
    if what.get("umi"):
        got, _, used = emu_umi(lib, fq, (r - 8, 8), bool(what.get("umi_reads")), **run)
    elif what.get("umi_header"):
        got, _, used = emu_header(lib, fq, (RE.HC.SEP, 8), bool(what.get("umi_reads")), **run)
    elif what.get("demux"):
        got, used = emu_demux(lib, fq, bcs, r - 8, 1, **run)
        RE.DC.check_invariants(*got)
    else:
        got = emu_plain(None if what.get("mode") == "EC" else lib, fq, **run)
        got, used = got[:2], got[2]
    assert used == len(fq) and tuple(got) == tuple(want)


# ---- (b) odd records -------------------------------------------------------------------------------------------------------
def emu_odd(case):
    """(result, table or None, bytes consumed or None) of an odd case through the emulation of its kind"""
    lib, run, ctx = case["lib"], case["run"], case["ctx"]
    if case["kind"].startswith("umi_paired"):
        e = TP.UPEmu(lib, case["parts"], case["rc2"], keep=ctx["umi_reads"], miss=run["miss"], phred=run["phred"])
        e.count(*case["texts"])
        got, table, _ = e.read()
        e.close()
        return got, table if ctx["umi_reads"] else None, None
    fq, = case["texts"]
    if "umi" in ctx:
        return emu_umi(lib, fq, ctx["umi"], ctx["umi_reads"], **run)
    if "umi_header" in ctx:
        return emu_header(lib, fq, (ord(ctx["umi_header"][0]), ctx["umi_header"][1]), ctx["umi_reads"], **run)
    got, used = emu_demux(lib, fq, [b.encode() for b in ctx["sample_barcodes"][1]], ctx["sample_barcodes"][0], ctx["barcode_mismatch"], **run)
    return got, None, used


@pytest.mark.parametrize("lo", range(0, 300, 50))
def test_odd_records_emulation_equals_expectation(lo):
    for seed in range(lo, lo + 50):
        case = RE.odd_case(seed)
        got, table, used = emu_odd(case)
        assert tuple(got) == tuple(case["expect"]()), (seed, case["kind"], case["run"])
        if case["table"]:
            assert table == case["table"](), (seed, case["kind"])
        if case["used"]:
            assert [used] == case["used"](), (seed, case["kind"])


def test_odd_records_cover_what_they_claim():
    """over the 360 seeds the tests use: every kind, fixed and anchored runs, both --m, the three --ph, CRLF, a leading blank
    line, a partial last record, a text without a final newline, empty lines, quality lines of another length, odd bytes"""
    seen, runs = set(), set()
    for seed in range(360):
        case = RE.odd_case(seed)
        seen.add(case["kind"])
        runs.add(("upstream" in case["run"], case["run"]["miss"], case["run"]["phred"]))
        for fq in case["texts"]:
            lines = fq.split(b"\n")
            seen.add("crlf" if b"\r\n" in fq else "lf")
            seen.add("leading_blank" if fq.startswith(b"\n") else "no_final_newline" if not fq.endswith(b"\n") else "partial" if fq.endswith(b"+\n") else "whole")
            for s, q in RE.UC.records(fq):
                seen.add("empty_seq" if not s else "empty_qual" if not q else "q_short" if len(q) < len(s) else "q_long" if len(q) > len(s) else "even")
                seen |= {"q%d" % c for c in (31, 127, 200) if c in q}
            seen |= {"blank_tail" for line in lines if line.rstrip(b"\r") != line.rstrip()}
    assert seen >= set(RE.ODD_KINDS) | {"crlf", "leading_blank", "no_final_newline", "partial", "empty_seq", "empty_qual", "q_short",
                                        "q_long", "q31", "q127", "q200", "blank_tail"}
    assert runs >= {(a, m, ph) for a in (False, True) for m in (0, 1) for ph in (1, 30, 41)}


# ---- (c) the second pass: the scaling rule on a stand-in device of 2 CUs -----------------------------------------------------
@pytest.mark.parametrize("kind", RE.PASS_KINDS)
def test_second_pass_expectation_scales(kind):
    n_cu = 2
    fq, reps = RE.second_pass(kind, n_cu)
    pool = RE.pass_pool(kind)
    assert fq == pool * reps and len(RE.UC.records(fq)) == reps * RE.POOL >= n_cu * 4096 + 3 * RE.POOL
    want = RE.scaled(kind, RE.pass_expect(kind, pool), reps)
    assert tuple(want) == tuple(RE.pass_expect(kind, fq))             # the rule itself, against the expectation on the whole text
    lib, ctx = RE.library(), RE.pass_ctx(kind)
    if kind == "demux":
        got, used = emu_demux(lib, fq, list(RE.DC.barcodes()), RE.PASS_AT, 1, **RE.PASS_RUN)
        table = None
    elif kind == "umi_header":
        got, table, used = emu_header(lib, fq, (RE.HC.SEP, 8), True, **RE.PASS_RUN)
    else:
        got, table, used = emu_umi(lib, fq, ctx["umi"], ctx["umi_reads"], **RE.PASS_RUN)
    assert used == len(fq) and tuple(got) == tuple(want)
    assert table == RE.scaled_table(RE.pass_table(kind, pool), reps)


# ---- (a) on merged pairs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc2", [False, True])
def test_paired_edge_sample_and_its_emulations(rc2):
    import test_paired_cpu as TPC
    RE.check_pair_cells(rc2)
    lib, fq1, fq2, _ = RE.edge_pairs(rc2)
    for miss in (0, 1):
        e = TPC.PEmu(lib, RE.PAIR_ST1 + RE.PAIR_ST2, 1, rc2, miss=miss, phred=RE.PH, length=RE.UP.LEN)
        assert tuple(e.count_all_byte_exact(fq1, fq2)) == RE.pair_expect(lib, fq1, fq2, rc2, miss)
        e.close()
        want = RE.pair_umi_expect(lib, fq1, fq2, rc2, miss)
        got, table, _, n = TP.emu_result(lib, fq1, fq2, RE.UP.TWO, rc2, st1=RE.PAIR_ST1, st2=RE.PAIR_ST2, miss=miss, phred=RE.PH)
        assert n == want.stats[0] and got == TP.wanted(want) and table == RE.UP.table_of(want)
        assert want.ok > 300 and want.stats[1] > 300 and (want.stats[2] > 50) == (miss == 1)
