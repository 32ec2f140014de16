"""tests/raw_edge_cases.py -- inputs and expected values for the raw-record kernels (k_count_general, k_count_umi,
k_count_umi_pair, k_count_demux) at three places the other case modules leave alone: the edge of the per-lane LDS staging
area, odd records on the UMI / header-UMI / paired-UMI / demultiplexing contexts, and a launch that takes the grid-stride
loop twice.  Shared by tests/test_raw_edge_cpu.py (CPU emulations) and tests/test_raw_edge_gpu.py.

No rule is restated here: every expectation is umi_cases.expect, demux_cases.expect, umi_header_cases.expect,
umi_pair_cases.expect, paired_cases.pair_oracle or the oracle itself (plain Counter and Extract+Count runs); all of them
frame by four rstrip()-ed lines as the reference does.

(a) edge_sample(r, tail, anchored) -- the staging edge.  The kernels stage a line when (offset & 3) + length <= 192.  With
the device packer a single-end record's offsets are its byte offsets in the text, so the text sets the alignment: the read
id is padded behind a blank to set so & 3, the third line is '+' and 0..3 id bytes to set qo & 3.  All long records of one
sample have r bases, because the run's window is placed from r (--st r-20-tail --l 20, or --us/--ds with the downstream
anchor on the last base).  So inside one sample ms + r is decided by ms alone; a sample holds every
(ms, mq, mq + qn in {191, 192, 193}) -- 48 cells, qn = r among the quality lengths, and qn shorter and longer -- and the
six samples r = 188 .. 193 together hold every one of the 16 x 3 x 3 cells (ms, mq, ms + r, mq + qn) with both sums in
{191, 192, 193}: both sides of both conditions, and the mixed cases where one line fits and the other does not.  The
assertions below recompute all of it from the text.  edge_pairs() is the same idea on merged pairs, where the packers' prefix
sum sets the alignment (see there).

(b) odd_case(seed) -- seeded samples of odd records (CRLF, trailing blanks, empty and ragged lines, quality lines of another
length, reads that end inside a window, odd symbols and quality bytes, a leading blank line, a partial last record, no final
newline) on the UMI, reads-per-pair, header-UMI, paired-UMI and demultiplexing contexts.

(c) second_pass(kind, n_cu) -- a pool of 257 distinct records repeated past n_cu * 4096, the lanes of a capped launch, with
the expectation computed on the pool and scaled.
"""
import functools
import random

import demux_cases as DC
import paired_cases as PC
import umi_cases as UC
import umi_dir_cases as DD
import umi_header_cases as HC
import umi_pair_cases as UP
from oracle import oracle as O

STAGE = 192                                    # bytes of one line the staging area holds (4 * F2Q_GEN_WORDS)
EDGE_R = tuple(range(188, 194))
SUMS = (191, 192, 193)
PH = 30
# what is done to a record of a cell; "last" is the last base of the window that ends the read (position r - 1) or the
# last byte of the quality line (position qn - 1); '=' is byte 31 + ph, the highest one --ph 30 fails; 31, 127 and 200 pass
KINDS = ("exact", "sub_last", "n_last", "lower_last", "q_hash_last", "q_top_last", "q31_last", "q127_last", "q200_last",
         "q_hash_first", "q_hash_tail_first")
HDR_POOL = (b"ACGTACGT", b"ACGTACGA", b"TTGCAAGC", b"GGGGCCCC", b"CATGCATG", b"ACGTNCGT", b"acgtacgt")


def library():
    return UC.library()


def fixed_run(r, tail, miss):
    return dict(start=str(r - 20 - tail), length=20, phred=PH, miss=miss)


def anchored_run(miss):
    return dict(upstream=UC.UP, downstream=UC.DOWN, miss_search_up=1, miss_search_down=1, phred=PH, length=20, miss=miss)


def _long_record(rng, lib, bcs, cell_no, kind, r, qn, tail, anchored):
    """(sequence, quality) of one long record: the same feature and the same tail window for every kind of a cell, so that
    "sub_last" is a second UMI of the feature of "exact" """
    g = lib[(7 * cell_no) % len(lib)].encode()
    if anchored:
        down = bytearray(UC.DOWN.encode())
        down[2] = ord("A") if down[2] != ord("A") else ord("C")      # one mismatch spent: with --msd 1 the last base decides
        body = UC.UP.encode() + g + bytes(down)
    else:
        body = g + bcs[cell_no % len(bcs)][:tail]
    s = bytearray(UC.rand_seq(rng, r - len(body)) + body)
    q = bytearray(b"I" * qn)
    first = r - len(body) + (len(UC.UP) if anchored else 0)          # the first base of the feature window
    if kind == "sub_last":
        s[r - 1] = ord("A") if s[r - 1] != ord("A") else ord("C")
    elif kind == "n_last":
        s[r - 1] = ord("N")
    elif kind == "lower_last":
        s[r - 1] = ord(chr(s[r - 1]).lower())
    elif kind == "q_hash_last":
        q[qn - 1] = ord("#")
    elif kind == "q_top_last":
        q[qn - 1] = 31 + PH
    elif kind in ("q31_last", "q127_last", "q200_last"):
        q[qn - 1] = int(kind[1:-5])
    elif kind == "q_hash_first":
        q[first] = ord("#")
    elif kind == "q_hash_tail_first":
        q[r - (tail or 20)] = ord("#")
    return bytes(s), bytes(q)


def _short_record(rng, lib, bcs, anchored):
    """a 60-base record: always staged, so a wave mixes the staged and the global branch"""
    g = lib[rng.randrange(len(lib))].encode()
    if anchored:
        s = UC.rand_seq(rng, 14) + UC.UP.encode() + g + UC.DOWN.encode() + UC.rand_seq(rng, 6)
    else:
        s = g + bcs[rng.randrange(len(bcs))] + UC.rand_seq(rng, 32)
    q = bytearray(b"I" * 60)
    if rng.random() < 0.2:
        q[rng.randrange(60)] = ord("#")
    return s, bytes(q)


def _append(text, i, s, q, ms, mq):
    """the record behind `text` with its sequence line at an offset = ms and its quality line at one = mq (mod 4)"""
    head = b"@e%d_%s " % (i, HDR_POOL[i % len(HDR_POOL)])
    head += b"p" * ((ms - len(text) - len(head) - 1) % 4)
    so = len(text) + len(head) + 1
    plus = b"+" + b"e" * ((mq - so - len(s) - 3) % 4)
    text += head + b"\n" + s + b"\n" + plus + b"\n" + q + b"\n"


@functools.lru_cache(maxsize=None)
def edge_sample(r, tail=0, anchored=False):
    """-> (library, barcodes, FASTQ bytes, [(record number, cell, kind)] of the long records).  cell = (ms, mq, mq + qn)"""
    assert r in EDGE_R and tail in (0, 8) and not (anchored and tail)
    rng = random.Random(0xED6E00 + 16 * r + tail + 100 * anchored)
    lib, bcs = library(), DC.barcodes()
    plan = []
    for cell_no, (ms, mq, b) in enumerate((ms, mq, b) for ms in range(4) for mq in range(4) for b in SUMS):
        for kind in KINDS:
            if kind == "q_hash_tail_first" and not tail:
                continue                                             # the window that ends the read is the feature window itself
            plan.append((cell_no, (ms, mq, b), kind))
    rng.shuffle(plan)
    text, tags, n = bytearray(), [], 0
    for k, (cell_no, (ms, mq, b), kind) in enumerate(plan):
        s, q = _long_record(rng, lib, bcs, cell_no, kind, r, b - mq, tail, anchored)
        _append(text, n, s, q, ms, mq)
        tags.append((n, (ms, mq, b), kind))
        n += 1
        if k % 2:
            s, q = _short_record(rng, lib, bcs, anchored)
            _append(text, n, s, q, rng.randrange(4), rng.randrange(4))
            n += 1
    return lib, bcs, bytes(text), tags


def layout(fq):
    """[(so, r, qo, qn)] of the complete records, from the text alone: the offsets the device packer hands the kernels"""
    out, pos, lines = [], 0, fq.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    starts = []
    for line in lines:
        starts.append(pos)
        pos += len(line) + 1
    for i in range(0, len(lines) - 3, 4):
        out.append((starts[i + 1], len(lines[i + 1].rstrip()), starts[i + 3], len(lines[i + 3].rstrip())))
    return out


def device_cells(fq):
    """{(so & 3, qo & 3, ms + r, mq + qn)} the device packer gives the kernels"""
    return {(so & 3, qo & 3, (so & 3) + r, (qo & 3) + qn) for so, r, qo, qn in layout(fq)}


def host_cells(fq):
    """the same under the host packer (pack_records): the raw records lie back to back, sequence then quality, so
    so = the bytes of the records before and qo = so + r -- mq is decided by ms and r"""
    out, at = set(), 0
    for _, r, _, qn in layout(fq):
        ms, mq = at & 3, (at + r) & 3
        out.add((ms, mq, ms + r, mq + qn))
        at += r + qn
    return out


def staged(cell):
    return cell[2] <= STAGE and cell[3] <= STAGE


def check_edge_cells(r, tail=0, anchored=False):
    """the coverage claim of the module docstring for one sample, recomputed from the text"""
    lib, bcs, fq, tags = edge_sample(r, tail, anchored)
    lay = layout(fq)
    for n, (ms, mq, b), kind in tags:
        so, rr, qo, qn = lay[n]
        assert (so & 3, rr, qo & 3, mq + qn) == (ms, r, mq, b), (n, kind)
    cells = device_cells(fq)
    want = {(ms, mq, ms + r, b) for ms in range(4) for mq in range(4) for b in SUMS}
    assert len(want) == 48 and want <= cells
    assert {staged(c) for c in cells} == {True, False}
    assert any(c[2] <= 64 for c in cells)                                  # the 60-base records
    assert any(c[2] <= STAGE < c[3] for c in cells) or r == 193            # the sequence line fits, the quality line does not
    assert any(c[3] <= STAGE < c[2] for c in cells) or r <= 189            # the other way round (r <= 189: ms + r <= 192 always)
    return cells


def check_edge_union():
    """over the six samples: every (ms, mq, ms + r, mq + qn) with both sums in {191, 192, 193}"""
    got = set()
    for r in EDGE_R:
        got |= {c for c in device_cells(edge_sample(r)[2]) if c[2] in SUMS and c[3] in SUMS}
    assert got == {(ms, mq, a, b) for ms in range(4) for mq in range(4) for a in SUMS for b in SUMS} and len(got) == 144


# ---- expectations ------------------------------------------------------------------------------------------------------
def oracle_of(lib, fq, **run):
    """plain runs: (counts, stats) in Counter mode, ([(key, count)], stats) in Extract+Count mode, and the bytes consumed"""
    o = O.Oracle(features=[(str(i), s) for i, s in enumerate(lib)] if lib is not None else None, **run)
    used = o.count_fastq(fq)
    out = (o.counts() if lib is not None else list(zip(o.keys(), o.counts()))), o.stats(), used
    o.close()
    return out


# the contexts of the edge sweep: name -> (tail of the sample, anchored, how a test builds and reads the context)
EDGE_CONTEXTS = {
    "plain_m0": (0, False, dict(miss=0)), "plain_m1": (0, False, dict(miss=1)),
    "plain_anchored_m0": (0, True, dict(miss=0)), "plain_anchored_m1": (0, True, dict(miss=1)),
    "ec": (0, False, dict(mode="EC")), "ec_anchored": (0, True, dict(mode="EC")),
    "umi": (8, False, dict(umi=True)), "umi_reads": (8, False, dict(umi=True, umi_reads=True)),
    "umi_header": (0, False, dict(umi_header=True)), "umi_header_reads": (0, False, dict(umi_header=True, umi_reads=True)),
    "demux_global": (8, False, dict(demux="global")), "demux_lds": (8, False, dict(demux="lds")),
}


def edge_run(name, r):
    tail, anchored, what = EDGE_CONTEXTS[name]
    run = anchored_run(what.get("miss", 1)) if anchored else fixed_run(r, tail, what.get("miss", 1))
    if what.get("mode") == "EC":
        run = dict(run, mode="EC")
        del run["miss"]
    return run


def edge_expect(name, r, fq=None):
    """the expectation of an edge context on its sample (or on `fq`, a text of the same shape):
    plain -> (counts, stats); ec -> (rows, stats); umi -> umi_cases.expect; umi_header -> wanted(umi_header_cases.expect);
    demux -> demux_cases.expect"""
    tail, anchored, what = EDGE_CONTEXTS[name]
    lib, bcs, text, _ = edge_sample(r, tail, anchored)
    fq = text if fq is None else fq
    run = edge_run(name, r)
    if what.get("umi"):
        return UC.expect(lib, fq, (r - 8, 8), **run)
    if what.get("umi_header"):
        return HC.wanted(HC.expect(lib, fq, (HC.SEP, 8), **run))
    if what.get("demux"):
        return DC.expect(lib, fq, bcs, r - 8, 1, **run)
    return oracle_of(None if what.get("mode") == "EC" else lib, fq, **run)[:2]


def _flipped(fq, n, which):
    """the text with the last sequence byte ('s') or the last quality byte ('q') of record n changed: a base becomes 'N'
    (an 'N' becomes 'A'), a passing quality byte '#', a failing one 'I'"""
    so, r, qo, qn = layout(fq)[n]
    b = bytearray(fq)
    if which == "s":
        b[so + r - 1] = ord("A") if b[so + r - 1] in b"Nn" else ord("N")
    else:
        c = b[qo + qn - 1]
        b[qo + qn - 1] = ord("I") if 33 <= c <= PH + 31 else ord("#")
    return bytes(b)


def _one(fq, n):
    """record n alone, its text as it stands (the expectations are sums over records)"""
    lines = fq.split(b"\n")
    return b"".join(line + b"\n" for line in lines[4 * n:4 * n + 4])


def check_edge_sensitive(name, r):
    """per cell, a record whose outcome in the expectation of context `name` changes with its last sequence byte or its last
    quality byte.  Returns the number of cells that have one for the sequence and for the quality byte.
    Holds for every cell where the rules let it: on a tail-8 sample (UMI / barcode window [r - 8, r)) a quality line
    shorter than r makes that window unreadable whatever its bytes are, and the feature window [r - 28, r - 8) ends before
    both last bytes, so there the claim is made for the cells with qn >= r only -- the cells with qn < r are sensitive
    on the tail-0 sample of the same r, which puts the same offsets and lengths in front of the same prologue."""
    tail, anchored, _ = EDGE_CONTEXTS[name]
    lib, bcs, fq, tags = edge_sample(r, tail, anchored)
    by_cell = {}
    for n, cell, kind in tags:
        by_cell.setdefault(cell, []).append(n)
    n_seq = n_qual = 0
    for cell, recs in sorted(by_cell.items()):
        ms, mq, b = cell
        qn = b - mq
        hit_s = hit_q = False
        for n in recs:
            one = _one(fq, n)
            base = edge_expect(name, r, one)
            hit_s = hit_s or edge_expect(name, r, _flipped(one, 0, "s")) != base
            hit_q = hit_q or edge_expect(name, r, _flipped(one, 0, "q")) != base
            if hit_s and hit_q:
                break
        if tail == 0:
            assert hit_s, (name, r, cell)                            # the feature window ends on the last base
            assert hit_q == (qn <= r), (name, r, cell)               # a longer quality line ends behind every window
        else:
            assert hit_s == (qn >= r) and hit_q == (qn == r), (name, r, cell)
        assert hit_s or hit_q or (tail and qn < r), (name, r, cell)
        n_seq += hit_s
        n_qual += hit_q
    return n_seq, n_qual


# ---- (b) odd records for the second-generation contexts ----------------------------------------------------------------
ODD_KINDS = ("umi", "umi_reads", "umi_header", "umi_paired_1", "umi_paired_2", "demux_m0", "demux_m1")
SEQ_ODD = b"NnRYKacgt."
QUAL_ODD = bytes([31, 127, 128, 200, 255]) + b"!#+5=>?~"             # never '\n' or '\r': they would change the framing
BLANKS = (b" ", b"\t", b" \t ", b"  ")


def _spoil(rng, s, q, windows):
    """oddities on one record, in place: symbols and quality bytes inside a window and outside, then the lengths"""
    if s and rng.random() < 0.3:
        a, b = rng.choice(windows)
        if a < len(s):
            s[rng.randrange(a, min(b, len(s)))] = rng.choice(SEQ_ODD)
    if q and rng.random() < 0.3:
        a, b = rng.choice(windows)
        if a < len(q):
            q[rng.randrange(a, min(b, len(q)))] = rng.choice(QUAL_ODD)
    if q and rng.random() < 0.2:
        q[rng.randrange(len(q))] = rng.choice(QUAL_ODD)
    t = rng.random()
    if t < 0.10:                                                     # the read ends inside a window
        a, b = rng.choice(windows)
        n = rng.randrange(a, b)
        del s[n:], q[n:]
    elif t < 0.16:
        del q[rng.randrange(len(q) + 1):]
    elif t < 0.22:
        q += b"I" * rng.randrange(1, 4)
    elif t < 0.25:
        del s[:]
    elif t < 0.28:
        del q[:]
    elif t < 0.30:
        del s[:], q[:]


def _text(rng, recs, paired=False):
    """records (header, sequence, quality) as text: CRLF per record, trailing blanks and tabs on any line, and the text's
    own oddities (a leading blank line -- single texts only --, a partial last record, no final newline)"""
    out = bytearray()
    for h, s, q in recs:
        eol = b"\r\n" if rng.random() < 0.1 else b"\n"
        for line in (h, s, b"+", q):
            out += line + (rng.choice(BLANKS) if rng.random() < 0.06 else b"") + eol
    return bytes(out)


def _finish(rng, texts):
    t = rng.random()
    if t < 0.05 and len(texts) == 1:
        return [b"\n" + x for x in texts]
    if t < 0.15:
        return [x + b"@x\nACGT\n+\n" for x in texts]
    if t < 0.25:
        return [x[:-1] for x in texts]
    return texts


def odd_case(seed):
    """-> dict(kind, ctx, run, lib, texts, expect): `ctx` are binding.Counter's keywords for the context, `texts` one FASTQ
    (two for a paired kind), expect() the tuple (counts, stats, umis, valid, invalid) -- demux: demux_cases.expect's five --
    and, where reads per pair are kept, the (feature, codes, reads) table behind it"""
    rng = random.Random(0x0DD0000 + seed)
    kind = ODD_KINDS[seed % len(ODD_KINDS)]
    miss, ph = rng.choice((0, 1)), rng.choice((1, 30, 41))
    n = rng.randint(40, 200)
    if kind.startswith("umi_paired"):
        return _odd_paired(rng, seed, kind, miss, ph, n)
    anchored = rng.random() < 0.4
    if anchored:
        lib = library()[:80]
        run = dict(anchored_run(miss), phred=ph)
        at = 2
    else:
        lib = library()
        st = rng.choice((0, 3))
        run = dict(start=str(st), length=20, phred=ph, miss=miss)
        at = st + 22
    bcs = DC.barcodes()
    umis = [UC.rand_seq(rng, 8) for _ in range(12)]
    heads = HC.random_headers(0x0DD + seed, n) if kind == "umi_header" else [b"@r%d" % i for i in range(n)]
    recs = []
    for i in range(n):
        g = lib[rng.randrange(len(lib))].encode()
        if rng.random() < 0.2:
            g = UC.mutate1(rng, g)
        w = bcs[rng.randrange(len(bcs))] if kind.startswith("demux") else umis[rng.randrange(len(umis))]
        if rng.random() < 0.15:
            w = UC.mutate1(rng, w)
        if anchored:
            spacer = UC.rand_seq(rng, rng.randrange(10))
            s = UC.rand_seq(rng, 2) + w + spacer + UC.UP.encode() + g + UC.DOWN.encode() + UC.rand_seq(rng, rng.randrange(8))
            fw = 10 + len(spacer) + len(UC.UP)
            windows = ((2, 10), (fw, fw + 20), (fw - len(UC.UP), fw), (fw + 20, fw + 30))
        else:
            s = UC.rand_seq(rng, st) + g + UC.rand_seq(rng, 2) + w + UC.rand_seq(rng, rng.choice((0, 5, 30, 170)))
            windows = ((st, st + 20), (at, at + 8))
        s, q = bytearray(s), bytearray(b"I" * len(s))
        if rng.random() < 0.6:
            _spoil(rng, s, q, windows)
        recs.append((heads[i], bytes(s), bytes(q)))
    fq, = _finish(rng, [_text(rng, recs)])
    if kind in ("umi", "umi_reads"):
        ctx = dict(umi=(at, 8), umi_reads=kind == "umi_reads")
        table = (lambda: DD.pair_table(lib, fq, (at, 8), **run)) if kind == "umi_reads" else None
        expect = lambda: UC.expect(lib, fq, (at, 8), **run)
    elif kind == "umi_header":
        keep = rng.random() < 0.5
        ctx = dict(umi_header=("_", 8), umi_reads=keep)
        table = (lambda: HC.table_of(HC.expect(lib, fq, (HC.SEP, 8), **run))) if keep else None
        expect = lambda: HC.wanted(HC.expect(lib, fq, (HC.SEP, 8), **run))
    else:
        M = int(kind[-1])
        ctx = dict(sample_barcodes=(at, [b.decode() for b in bcs]), barcode_mismatch=M)
        table = None
        expect = lambda: DC.expect(lib, fq, bcs, at, M, **run)
    return dict(kind=kind, ctx=ctx, run=run, lib=lib, texts=[fq], expect=expect, table=table, seed=seed,
                used=lambda: [oracle_of(lib, fq, **run)[2]])


def _odd_paired(rng, seed, kind, miss, ph, n):
    """pairs of umi_pair_cases' geometry (--st 5 --st2 0 --l 10): only ONE mate of a pair gets oddities that change a length,
    the other stays whole with a quality line as long, so one of paired_cases' two constructions always covers the pair"""
    rc2 = rng.random() < 0.5
    parts = (None, UP.UMI2) if kind == "umi_paired_1" else UP.TWO
    lib = PC.pair_library(200, UP.LEN, 1, 1, 21)
    pool = [UC.rand_seq(rng, 16) for _ in range(12)]
    r1, r2 = [], []
    for i in range(n):
        len1, len2 = rng.choice((40, 60, 150)), rng.choice((40, 60, 150))
        m1, m2 = UP.hand_pair(lib, rng.randrange(len(lib)), rc2, rng, len1, len2)
        UP.set_umi(m1, m2, parts, pool[rng.randrange(len(pool))][:sum(p[1] for p in parts if p)])
        if rng.random() < 0.6:
            which = rng.random() < 0.5
            s, q = m2 if which else m1
            win2 = (len2 - UP.LEN, len2) if rc2 else (0, UP.LEN)      # mate 2's window in its text as sequenced
            windows = ((win2, parts[1][:1] + (parts[1][0] + parts[1][1],)) if which else
                       ((UP.ST1[0], UP.ST1[0] + UP.LEN),) + (((parts[0][0], parts[0][0] + parts[0][1]),) if parts[0] else ()))
            _spoil(rng, s, q, windows)
        r1.append((b"@a%d" % i, bytes(m1[0]), bytes(m1[1])))
        r2.append((b"@b%d" % i, bytes(m2[0]), bytes(m2[1])))
    fq1, fq2 = _finish(rng, [_text(rng, r1), _text(rng, r2)])
    keep = rng.random() < 0.5

    @functools.lru_cache(maxsize=None)
    def e():
        x = UP.expect(lib, fq1, fq2, UP.ST1, UP.ST2, UP.LEN, rc2, parts, miss=miss, phred=ph)
        assert x.uncovered == 0, seed
        return x
    return dict(kind=kind, ctx=dict(start2="0", rc2=rc2, umi_paired=parts, umi_reads=keep), lib=lib, texts=[fq1, fq2],
                run=dict(start=str(UP.ST1[0]), length=UP.LEN, phred=ph, miss=miss), parts=parts, rc2=rc2,
                expect=lambda: (e().counts, e().stats, UP.umis_of(e()), e().ok, e().bad),
                table=(lambda: UP.table_of(e())) if keep else None, seed=seed, used=None)


# ---- (c) a launch that takes the grid-stride loop twice -------------------------------------------------------------------
PASS_KINDS = ("umi", "umi_reads", "umi_header", "demux")
POOL = 257                                     # odd: in its second pass a lane meets other neighbours than in its first
PASS_RUN = dict(start="0", length=20, phred=PH, miss=1)
PASS_AT = 20                                   # the UMI / barcode window [20, 28)


@functools.lru_cache(maxsize=None)
def pass_pool(kind):
    """257 distinct records: 30 bases, one in eight 190 (so a short record is staged over a long one's bytes in the lane's
    second pass); exact and one-mismatch windows, random ones, low quality in the feature window, and every verdict of the
    UMI or barcode window -- asserted on the expectation"""
    rng = random.Random(0x2FA55 + PASS_KINDS.index(kind))
    lib, bcs = library(), DC.barcodes()
    umis = [UC.rand_seq(rng, 8) for _ in range(10)]
    recs = []
    for i in range(POOL):
        g = lib[rng.randrange(40)].encode()
        roll = rng.random()
        if roll < 0.2:
            g = UC.mutate1(rng, g)
        elif roll < 0.3:
            g = UC.rand_seq(rng, 20)
        w = bytearray(bcs[rng.randrange(len(bcs))] if kind == "demux" else umis[rng.randrange(len(umis))])
        roll = rng.random()
        if roll < 0.15:
            w = bytearray(UC.mutate1(rng, bytes(w)))
        elif roll < 0.25:
            w[rng.randrange(8)] = ord("N")
        elif roll < 0.3:                                             # one base from barcodes 0 and 1 both
            w = bytearray(bcs[0]); p = [j for j in range(8) if bcs[0][j] != bcs[1][j]][0]; w[p] = bcs[1][p]
        elif roll < 0.4:
            w = bytearray(UC.rand_seq(rng, 8))
        n = 190 if i % 8 == 3 else 30
        s = bytearray(g + bytes(w) + UC.rand_seq(rng, n - 28))
        q = bytearray(b"I" * n)
        roll = rng.random()
        if roll < 0.1:
            q[rng.randrange(20)] = ord("#")
        elif roll < 0.2:
            q[PASS_AT + rng.randrange(8)] = ord("#")
        elif roll < 0.25:
            del s[25:], q[25:]
        head = b"@s%d_%s" % (i, umis[rng.randrange(len(umis))] if rng.random() < 0.85 else b"ACGTNACG")
        recs.append((head, bytes(s), bytes(q)))
    assert len(set(recs)) == POOL
    fq = HC.fastq_of(recs)
    e = pass_expect(kind, fq)
    stats = e[1]
    assert all(stats[1:]) and sum(stats[1:5]) >= stats[0] - stats[4]
    if kind == "demux":
        assert all(e[4]), e[4]
    else:
        assert e[3] > 20 and e[4] > 5 and max(e[2]) > 1 and sum(e[2]) < e[3]
    return fq


def pass_ctx(kind):
    if kind == "demux":
        return dict(sample_barcodes=(PASS_AT, [b.decode() for b in DC.barcodes()]), barcode_mismatch=1)
    if kind == "umi_header":
        return dict(umi_header=("_", 8), umi_reads=True)
    return dict(umi=(PASS_AT, 8), umi_reads=kind == "umi_reads")


def pass_expect(kind, fq):
    lib = library()
    if kind == "demux":
        return DC.expect(lib, fq, DC.barcodes(), PASS_AT, 1, **PASS_RUN)
    if kind == "umi_header":
        return HC.wanted(HC.expect(lib, fq, (HC.SEP, 8), **PASS_RUN))
    return UC.expect(lib, fq, (PASS_AT, 8), **PASS_RUN)


def pass_table(kind, fq):
    """the (feature, codes, reads) table of the kinds that keep reads per pair, else None"""
    if kind == "umi_reads":
        return DD.pair_table(library(), fq, (PASS_AT, 8), **PASS_RUN)
    if kind == "umi_header":
        return HC.table_of(HC.expect(library(), fq, (HC.SEP, 8), **PASS_RUN))
    return None


def scaled(kind, e, k):
    """the expectation of the pool repeated k times: counts, stats, the matrix, the sample stats, the verdicts and the reads
    with a valid / an invalid UMI multiply; the distinct UMIs per feature do not change"""
    mul = lambda x: [mul(y) for y in x] if isinstance(x, (list, tuple)) else x * k
    if kind == "demux":
        return tuple(mul(x) for x in e)
    counts, stats, umis, ok, bad = e
    return mul(counts), mul(stats), list(umis), ok * k, bad * k


def scaled_table(table, k):
    return None if table is None else [(f, c, n * k) for f, c, n in table]


def second_pass(kind, n_cu):
    """-> (FASTQ bytes, repetitions): the pool repeated until the launch has n_cu * 4096 + 3 * 257 records or more -- more
    than the n_cu * 64 workgroups of 64 lanes the launch is capped at, so every lane takes a second record"""
    reps = -(-(n_cu * 4096 + 3 * POOL) // POOL)
    assert reps * POOL >= n_cu * 4096 + 3 * POOL
    return pass_pool(kind) * reps, reps


# ---- (a) continued: the staging edge on merged pairs -----------------------------------------------------------------------
# --st 5 --st2 30 --l 10 on mates of (total - 40) + 40 bases: mate 2's window as the run takes it ends on the last byte of
# the merged record.  The packers write the merged records back to back (sequence, then quality): so = the bytes of the
# records before, qo = so + r, so a record's alignment depends on the lengths of the records before it.  A spacer pair of
# 60 + 80 bases with a mate-2 quality line 0 .. 3 bytes short goes in front of every long pair and sets its so & 3; mq is
# then (ms + r) & 3 and cannot be chosen -- the layout gives every ms on both sides of 192, and a quarter of the (ms, mq)
# pairs per total.
PAIR_ST1, PAIR_ST2, PAIR_LEN2 = (5,), (30,), 40
PAIR_KINDS = ("exact", "sub_last", "n_last", "q_hash_last", "q200_last", "q_hash_first")


@functools.lru_cache(maxsize=None)
def edge_pairs(rc2=True):
    """-> (library, fq1, fq2, [(pair number, ms, total, quality bytes short, kind)] of the long pairs); UMI parts
    umi_pair_cases.TWO"""
    rng = random.Random(0xED6E2 + rc2)
    lib = PC.pair_library(200, UP.LEN, 1, 1, 21)
    plan = [(ms, total, qd, kind) for ms in range(4) for total in EDGE_R for qd in (0, 1) for kind in PAIR_KINDS]
    rng.shuffle(plan)
    r1, r2, tags, at = [], [], [], 0

    def pair(f, len1, len2):
        p1, p2 = [p.encode() for p in lib[f].split(":")]
        s1 = bytearray(UC.rand_seq(rng, len1)); s1[PAIR_ST1[0]:PAIR_ST1[0] + UP.LEN] = p1
        m2 = bytearray(UC.rand_seq(rng, len2)); m2[len2 - UP.LEN:] = p2          # as the run takes it: the window ends the mate
        return s1, bytearray(b"I" * len1), m2, bytearray(b"I" * len2)

    def add(s1, q1, m2, mq2, u):
        s2, q2 = PC.mate2_as_taken(bytes(m2), bytes(mq2), rc2)                   # back to the text as sequenced
        a, b = [bytearray(s1), bytearray(q1)], [bytearray(s2), bytearray(q2)]
        if len(s2) >= 22:
            UP.set_umi(a, b, UP.TWO, u)
        r1.append((bytes(a[0]), bytes(a[1]))); r2.append((bytes(b[0]), bytes(b[1])))
        return len(s1) + len(s2) + len(q1) + len(q2)
    for ms, total, qd, kind in plan:
        s1, q1, m2, mq2 = pair(rng.randrange(len(lib)), 60, 80)
        m2[30:40] = m2[70:80]                                                    # the spacer carries its part at [30, 40) too
        del mq2[80 - ((at + 280 - ms) % 4):]                                     # ... and brings the next record to so & 3 = ms
        at += add(s1, q1, m2, mq2, UC.rand_seq(rng, 16))
        assert at & 3 == ms
        s1, q1, m2, mq2 = pair(rng.randrange(len(lib)), total - PAIR_LEN2, PAIR_LEN2)
        if qd:
            del mq2[:1]                                                          # the merged quality line one byte short, its last byte kept
        if kind == "sub_last":
            m2[-1] = ord("A") if m2[-1] != ord("A") else ord("C")
        elif kind == "n_last":
            m2[-1] = ord("N")
        elif kind == "q_hash_last":
            mq2[-1] = ord("#")
        elif kind == "q200_last":
            mq2[-1] = 200
        elif kind == "q_hash_first":
            mq2[len(mq2) - UP.LEN] = ord("#")
        tags.append((len(r1), ms, total, qd, kind))
        at += add(s1, q1, m2, mq2, UC.rand_seq(rng, 16))
    return lib, PC.fastq_of(r1, b"a"), PC.fastq_of(r2, b"b"), tags


def pair_cells(fq1, fq2):
    """[(ms, mq, ms + r, mq + qn)] per pair, by the prefix sum both packers use (every pair of these contexts is a raw record)"""
    out, at = [], 0
    for (s1, q1), (s2, q2) in zip(PC.records(fq1), PC.records(fq2)):
        r, qn = len(s1) + len(s2), len(q1) + len(q2)
        ms, mq = at & 3, (at + r) & 3
        out.append((ms, mq, ms + r, mq + qn))
        at += r + qn
    return out


def check_pair_cells(rc2=True):
    lib, fq1, fq2, tags = edge_pairs(rc2)
    cells = pair_cells(fq1, fq2)
    for n, ms, total, qd, kind in tags:
        assert cells[n][0] == ms and cells[n][2] == ms + total and cells[n][3] == cells[n][1] + total - qd
    long = [c for c in cells if c[2] >= 188]
    assert {c[0] for c in long if c[2] <= STAGE} == {c[0] for c in long if c[2] > STAGE} == {0, 1, 2, 3}
    assert len({c[1] for c in long if c[3] <= STAGE}) >= 3 and len({c[1] for c in long if c[3] > STAGE}) >= 3
    assert {(c[0], c[2]) for c in long} >= {(ms, a) for ms in range(4) for a in SUMS}
    assert {c[3] for c in long} >= set(SUMS) and {staged(c) for c in long} == {True, False}
    assert any(c[2] <= STAGE < c[3] for c in long) and any(c[3] <= STAGE < c[2] for c in long)
    # a pair per (ms, side of 192) whose outcome changes with the last byte of the merged sequence / quality line
    l1, l2 = fq1.split(b"\n"), fq2.split(b"\n")
    hit = set()
    for n, ms, total, qd, kind in tags:
        side = ms + total <= STAGE
        if kind != "exact" or (ms, side) in hit:
            continue
        one1, one2 = [b"".join(x + b"\n" for x in l[4 * n:4 * n + 4]) for l in (l1, l2)]
        base = pair_expect(lib, one1, one2, rc2, 0)
        so, r, qo, qn = layout(one2)[0]
        b = bytearray(one2); b[so if rc2 else so + r - 1] = ord("N")
        c = bytearray(one2); c[qo if rc2 else qo + qn - 1] = ord("#")
        assert pair_expect(lib, one1, bytes(b), rc2, 0) != base and pair_expect(lib, one1, bytes(c), rc2, 0) != base, (n, ms, total)
        hit.add((ms, side))
    assert len(hit) == 8
    return cells


def pair_expect(lib, fq1, fq2, rc2, miss):
    """(counts, stats) of the plain paired context"""
    counts, stats, uncovered = PC.pair_oracle(lib, fq1, fq2, list(PAIR_ST1), list(PAIR_ST2), UP.LEN, rc2, miss, PH)
    assert uncovered == 0
    return counts, stats


def pair_umi_expect(lib, fq1, fq2, rc2, miss):
    e = UP.expect(lib, fq1, fq2, PAIR_ST1, PAIR_ST2, UP.LEN, rc2, UP.TWO, miss=miss, phred=PH)
    assert e.uncovered == 0
    return e


def edge_table(name, r):
    """the (feature, codes, reads) table of the edge contexts that keep reads per pair, else None"""
    tail, anchored, what = EDGE_CONTEXTS[name]
    if not what.get("umi_reads"):
        return None
    lib, _, fq, _ = edge_sample(r, tail, anchored)
    run = edge_run(name, r)
    if what.get("umi"):
        return DD.pair_table(lib, fq, (r - 8, 8), **run)
    return HC.table_of(HC.expect(lib, fq, (HC.SEP, 8), **run))
