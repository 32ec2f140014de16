"""tests/demux_cases.py -- inputs and expected values shared by the --sb tests (CPU emulation and GPU).

The expectation is plain Python: 4-line framing with rstrip() as the reference frames; the feature verdict of each read
from the oracle in Counter mode (umi_cases._verdicts, as the UMI tests take it); the barcode rule of include/f2q.h
(f2q_set_sample_barcodes) written out below as barcode_of; plain additive counters."""
import functools
import random

import synth
import umi_cases as UC

S, L = 20, 8                                   # the base shape's barcode window
EXACT, ONE_MISMATCH, AMBIGUOUS, NO_MATCH, UNREADABLE = range(5)


def barcode_of(seq, qual, S, L, phred, barcodes, M):
    """(sample, verdict) of one record's rstrip()-ed lines: the rule of include/f2q.h; sample len(barcodes) = unassigned"""
    nb = len(barcodes)
    if S + L > len(seq) or S + L > len(qual):
        return nb, UNREADABLE
    ph = max(int(phred), 1)                                      # fast2q.py:1118-1125
    if any(33 <= c <= min(ph + 31, 126) for c in qual[S:S + L]):  # the fail set of --ph (:1112-1129)
        return nb, UNREADABLE
    w = seq[S:S + L].upper()
    d = [sum(x != y for x, y in zip(w, b)) for b in barcodes]
    if 0 in d:
        return d.index(0), EXACT
    if M == 1 and d.count(1) == 1:
        return d.index(1), ONE_MISMATCH
    if M == 1 and d.count(1) > 1:
        return nb, AMBIGUOUS
    return nb, NO_MATCH


def expect(lib, fq, barcodes, at, M, **run):
    """(counts, stats, matrix, sample_stats, verdicts) of the FASTQ bytes, as lists; the barcode window starts at `at`"""
    v = UC._verdicts(tuple(lib), UC.run_key(run))
    nb, length = len(barcodes), len(barcodes[0])
    counts, stats = [0] * len(lib), [0] * 5
    matrix = [[0] * len(lib) for _ in range(nb + 1)]
    sstats = [[0] * 5 for _ in range(nb + 1)]
    verdicts = [0] * 5
    for seq, qual in UC.records(fq):
        f, verdict, qfail = v.of(seq, qual)
        b, bv = barcode_of(seq, qual, at, length, run.get("phred", 30), barcodes, M)
        verdicts[bv] += 1
        for row in (stats, sstats[b]):
            row[0] += 1
            row[4] += qfail
            if verdict:
                row[verdict] += 1
        if f >= 0:
            counts[f] += 1
            matrix[b][f] += 1
    return counts, stats, matrix, sstats, verdicts


def check_invariants(counts, stats, matrix, sstats, verdicts):
    nb = len(matrix) - 1
    assert [sum(col) for col in zip(*matrix)] == list(counts)
    assert [sum(col) for col in zip(*sstats)] == list(stats)
    assert sum(verdicts) == stats[0]
    assert verdicts[EXACT] + verdicts[ONE_MISMATCH] == sum(row[0] for row in sstats[:nb])


def library():
    return UC.library()


@functools.lru_cache(maxsize=None)
def barcodes():
    """12 barcodes of 8 bases: 0 and 1 two bases apart (a window one base from both: ambiguous), 2 and 3 one base apart
    (barcode 2 is a neighbour of barcode 3: exact wins), every other pair at least three bases apart"""
    rng = random.Random(0xBC0DE)
    out = [b"ACGTACGT", b"ACGAACCT", b"GGATCCTA", b"GGATCGTA"]
    while len(out) < 12:
        cand = UC.rand_seq(rng, L)
        if all(sum(x != y for x, y in zip(cand, b)) >= 3 for b in out):
            out.append(cand)
    return tuple(out)


KINDS = (("exact", 30), ("sub1", 12), ("lower", 5), ("one_n", 5), ("two_n", 4), ("ambiguous", 5), ("exact_wins", 5), ("cut_inside", 5),
         ("short_qual", 4), ("lowq_inside", 5), ("lowq_outside", 5), ("random", 15))


def _rewrite(rng, kind, s, q, bcs):
    """the record (s, q) of 60 bases with positions [20, 28) rewritten by `kind`"""
    s, q = bytearray(s), bytearray(q)
    far = rng.randrange(4, len(bcs))                             # a barcode at least three bases from every other one
    w = bytearray(bcs[rng.randrange(len(bcs))])
    if kind == "sub1":
        w = bytearray(UC.mutate1(rng, bcs[far]))
    elif kind == "lower":
        w = bytearray(bytes(w).lower())
    elif kind == "one_n":
        w = bytearray(bcs[far]); w[rng.randrange(L)] = ord("N")
    elif kind == "two_n":
        a, b = rng.sample(range(L), 2); w[a] = ord("N"); w[b] = ord("n")
    elif kind == "ambiguous":                                    # barcode 0 with one of its two differences taken from barcode 1
        w = bytearray(bcs[0]); p = rng.choice([i for i in range(L) if bcs[0][i] != bcs[1][i]]); w[p] = bcs[1][p]
    elif kind == "exact_wins":
        w = bytearray(bcs[rng.choice((2, 3))])
    elif kind == "random":
        w = bytearray(UC.rand_seq(rng, L))
    s[S:S + L] = w
    if kind == "cut_inside":
        n = S + rng.randrange(1, L); s, q = s[:n], q[:n]
    elif kind == "short_qual":
        q = q[:S + rng.randrange(L)]
    elif kind == "lowq_inside":
        q[S + rng.randrange(L)] = ord("#")
    elif kind == "lowq_outside":
        q[S + L + rng.randrange(60 - S - L)] = ord("#")
    return bytes(s), bytes(q)


def sample(seed, n_reads=3000, bcs=None):
    """the umi_cases.sample shape (reads of 60 bases, the feature window at 0) with positions [20, 28) rewritten by kind;
    returns (FASTQ bytes, the kind of every record)"""
    rng = random.Random(seed)
    lib, bcs = library(), bcs or barcodes()
    spec = synth.Spec(seed=seed, n_reads=n_reads, read_len=60, start=0)
    names, weights = [k for k, _ in KINDS], [w for _, w in KINDS]
    recs, kinds = [], rng.choices(names, weights, k=n_reads)
    for i, kind in enumerate(kinds):
        recs.append(_rewrite(rng, kind, *synth.make_read(spec, lib, i), bcs))
    return UC.fastq_of(recs), kinds


RUN = dict(UC.RUN)
# what each kind must come out as with M = 1 (M = 0: ONE_MISMATCH and AMBIGUOUS become NO_MATCH)
KIND_VERDICT = dict(lower=EXACT, one_n=ONE_MISMATCH, two_n=NO_MATCH, ambiguous=AMBIGUOUS, exact_wins=EXACT, cut_inside=UNREADABLE,
                    short_qual=UNREADABLE, lowq_inside=UNREADABLE, lowq_outside=None, sub1=ONE_MISMATCH, exact=EXACT)


@functools.lru_cache(maxsize=None)
def base(seed=0xDE30):
    """600 guides x 20 bp, 3 000 reads of 60 bp, --st 0 --l 20, 12 barcodes of 8 bases at [20, 28) -> (lib, fq, run, barcodes, start);
    asserts here, on the CPU, that the expectation alone covers every verdict and every class of window"""
    lib, bcs = library(), barcodes()
    fq, kinds = sample(seed)
    recs = UC.records(fq)
    assert len(recs) == len(kinds)
    for M in (0, 1):
        got = [barcode_of(s, q, S, L, 30, bcs, M) for s, q in recs]
        per_verdict = [sum(v == k for _, v in got) for k in range(5)]
        assert all(n >= 50 for k, n in enumerate(per_verdict) if M == 1 or k in (EXACT, NO_MATCH, UNREADABLE)), per_verdict
        assert M == 1 or per_verdict[ONE_MISMATCH] == per_verdict[AMBIGUOUS] == 0
        for kind, want in KIND_VERDICT.items():
            if want is None:                                     # low quality outside the window only: the verdict of the window as it is
                hit = [g for g, k in zip(got, kinds) if k == kind and g[1] != UNREADABLE]
            else:
                if M == 0 and want in (ONE_MISMATCH, AMBIGUOUS):
                    want = NO_MATCH
                hit = [g for g, k in zip(got, kinds) if k == kind and g[1] == want]
                assert len(hit) == kinds.count(kind), kind
            assert len(hit) >= 20, (kind, len(hit))
        # exact wins: the window is barcode 2 (3) itself, never the neighbour's sample
        assert all(g[0] in (2, 3) for g, k in zip(got, kinds) if k == "exact_wins")
        assert all((g[0] < len(bcs)) == (M == 1) for g, k in zip(got, kinds) if k == "one_n")
    return lib, fq, dict(RUN), bcs, S


def pieces(fq, per):
    """the FASTQ text cut into pieces of `per` records"""
    lines = fq.split(b"\n")
    n_rec = (len(lines) - 1) // 4
    return [b"".join(line + b"\n" for line in lines[4 * i:4 * min(i + per, n_rec)]) for i in range(0, n_rec, per)]


@functools.lru_cache(maxsize=None)
def shapes():
    """small samples (a few hundred reads) for the table's edges: {name: (barcodes, start, fq)} --
    L = 16 with A x 16 and T x 16 among the barcodes, L = 1 with all four, one barcode, 1024 barcodes of 8 bases"""
    rng = random.Random(0x5BA9E)
    lib = library()
    out = {}

    def reads(bcs, length, n=300):
        recs = []
        for i in range(n):
            g = lib[rng.randrange(len(lib))].encode()
            w = bytearray(bcs[rng.randrange(len(bcs))])
            r = rng.random()
            if r < 0.25:
                w = bytearray(UC.mutate1(rng, bytes(w)))
            elif r < 0.35:
                w[rng.randrange(length)] = ord("N")
            elif r < 0.45:
                w = bytearray(UC.rand_seq(rng, length))
            recs.append((g + bytes(w) + UC.rand_seq(rng, 8), b"I" * (28 + length)))
        return UC.fastq_of(recs)
    wide = [b"A" * 16, b"T" * 16, b"A" * 15 + b"C", b"T" * 15 + b"G"] + [UC.rand_seq(rng, 16) for _ in range(8)]
    out["l16"] = (tuple(wide), 20, reads(wide, 16))
    out["l1"] = ((b"A", b"C", b"G", b"T"), 20, reads([b"A", b"C", b"G", b"T"], 1))
    out["l1_three"] = ((b"A", b"C", b"G"), 20, reads([b"A", b"C", b"G", b"T"], 1))
    out["nb1"] = ((b"GATTACAG",), 20, reads([b"GATTACAG"], 8))
    many = set()
    while len(many) < 1024:
        many.add(UC.rand_seq(rng, 8))
    many = tuple(sorted(many))
    out["nb1024"] = (many, 20, reads(many, 8, n=400))
    return out


@functools.lru_cache(maxsize=None)
def long_reads():
    """reads of 250 bases with the barcode at [230, 238) -- past the kernel's 192-byte staging area -- mixed with 60-base
    reads for which that window is UNREADABLE -> (lib, fq, run, barcodes, start)"""
    rng = random.Random(0x10E6)
    lib, bcs = library(), barcodes()
    recs = []
    for i in range(400):
        g = lib[rng.randrange(len(lib))].encode()
        if rng.random() < 0.2:
            g = UC.mutate1(rng, g)
        if i % 4 == 3:
            recs.append((g + UC.rand_seq(rng, 40), b"I" * 60))
            continue
        w = bcs[rng.randrange(len(bcs))]
        r = rng.random()
        if r < 0.2:
            w = UC.mutate1(rng, w)
        elif r < 0.3:
            w = w[:2] + b"N" + w[3:]
        q = bytearray(b"I" * 250)
        if rng.random() < 0.1:
            q[230 + rng.randrange(8)] = ord("#")
        recs.append((g + UC.rand_seq(rng, 210) + w + UC.rand_seq(rng, 12), bytes(q)))
    return lib, UC.fastq_of(recs), dict(RUN), bcs, 230


@functools.lru_cache(maxsize=None)
def anchored():
    """--us/--ds with --msu 1 --msd 1: the barcode in read positions [2, 10), then a spacer of 0 .. 9 bases, the cassette"""
    rng = random.Random(0xA9C4)
    lib, bcs = library()[:80], barcodes()
    recs = []
    for i in range(1200):
        g = lib[rng.randrange(len(lib))].encode()
        w = UC.mutate1(rng, g) if rng.random() < 0.2 else g
        up = UC.mutate1(rng, UC.UP.encode()) if rng.random() < 0.1 else UC.UP.encode()
        b = bcs[rng.randrange(len(bcs))]
        r = rng.random()
        if r < 0.15:
            b = UC.mutate1(rng, b)
        elif r < 0.2:
            b = b[:3] + b"N" + b[4:]
        elif r < 0.3:
            b = UC.rand_seq(rng, 8)
        s = UC.rand_seq(rng, 2) + b + UC.rand_seq(rng, rng.randrange(10)) + up + w + UC.DOWN.encode() + UC.rand_seq(rng, rng.randrange(8))
        q = bytearray(b"I" * len(s))
        if rng.random() < 0.1:
            q[rng.randrange(len(q))] = ord("#")
        recs.append((s, bytes(q)))
    run = dict(upstream=UC.UP, downstream=UC.DOWN, miss_search_up=1, miss_search_down=1, phred=30, length=20)
    return lib, UC.fastq_of(recs), run, bcs, 2
