"""tests/strand_cases.py -- inputs and expected values shared by the --strand tests (CPU emulation and GPU).

The expectation is plain Python: umi_cases._verdicts (the oracle in Counter mode, once per distinct record text) applied to
a record's (seq, qual) and to mirrored(seq, qual), combined by strand_verdict -- the two functions of include/f2q.h
(f2q_set_strand), and the only rule stated here.  Framing is umi_cases.records: four rstrip()-ed lines per record."""
import functools
import random

import raw_edge_cases as RE
import synth
import umi_cases as UC

FWD, REV, BOTH = "fwd", "rev", "both"
FORWARD, REVERSE = 0, 1
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")     # comp8: every other byte stays what it is, case is kept
RUN = dict(start="0", length=20, phred=30)


def mirrored(seq, qual):
    # each line is mirrored by ITS OWN length; quality bytes are never translated.  The second rstrip() is deliberate: the
    # reverse strand of a record is exactly what the reference would read from the four lines "@", revcomp(seq), "+",
    # reversed(qual) -- leading blanks of a line become trailing ones and fall away
    return seq.translate(COMP)[::-1].rstrip(), qual[::-1].rstrip()


def strand_verdict(verdict, seq, qual, mode):
    """-> ((feature or -1, counter 0..3, quality_failed), strand); `verdict` is umi_cases._Verdicts.of"""
    if mode == REV:
        return verdict(*mirrored(seq, qual)), REVERSE
    F = verdict(seq, qual)
    if mode == FWD or F[0] >= 0:                     # forward first: an assigned forward strand is never re-examined,
        return F, FORWARD                            # not even when it is imperfect and the reverse strand is perfect
    R = verdict(*mirrored(seq, qual))
    return (R, REVERSE) if R[0] >= 0 else (F, FORWARD)   # nobody assigns it: counted as the forward strand counts it


def expect(lib, fq, mode, **run):
    """(counts, stats, rev_counts, extra) of the FASTQ bytes, as lists"""
    v = UC._verdicts(tuple(lib), UC.run_key(run)).of
    counts, stats, rev, extra = [0] * len(lib), [0] * 5, [0] * len(lib), [0] * 4
    for seq, qual in UC.records(fq):
        (f, which, qfail), strand = strand_verdict(v, seq, qual, mode)
        stats[0] += 1
        stats[4] += qfail
        if which:
            stats[which] += 1
        if f >= 0:
            counts[f] += 1
            if strand == REVERSE:
                rev[f] += 1
                extra[which] += 1                    # 1: perfect, 2: imperfect
            else:
                extra[0] += 1
        # the reverse strand was examined: always under rev; under both whenever the forward strand assigned nothing
        extra[3] += mode == REV or (mode == BOTH and (strand == REVERSE or f < 0))
    return counts, stats, rev, extra


def check_invariants(mode, counts, stats, rev, extra):
    """the invariants of include/f2q.h (f2q_read_strands)"""
    assert all(r <= c for r, c in zip(rev, counts))
    assert sum(rev) == extra[1] + extra[2]
    assert extra[0] + extra[1] + extra[2] == stats[1] + stats[2] == sum(counts)
    if mode == BOTH:
        assert extra[3] == stats[0] - extra[0]
    if mode == REV:
        assert extra[0] == 0 and extra[3] == stats[0] and list(rev) == list(counts)


def revcomp(s):
    return s.translate(COMP)[::-1]


def flip(rec):
    """the record whose reverse strand is `rec`'s forward strand (lines without blanks at either end)"""
    return revcomp(rec[0]), rec[1][::-1]


def mirror_text(fq, which=lambda i: True):
    """the text with the sequence and quality lines of the records `which` picks mirrored in place, each by its own
    rstrip()-ed length: every offset and every length of the text stays what it was (whole 4-line records only)"""
    lines = fq.split(b"\n")
    for i in range(0, len(lines) - 3, 4):
        if which(i // 4):
            for k, comp in ((1, True), (3, False)):
                body = lines[i + k].rstrip()
                tail = lines[i + k][len(body):]
                lines[i + k] = (revcomp(body) if comp else body[::-1]) + tail
    return b"\n".join(lines)


def pieces(fq, per):
    """the text cut into blocks of `per` whole records"""
    lines = fq.split(b"\n")
    assert lines.pop() == b"" and len(lines) % 4 == 0
    return [b"\n".join(lines[i:i + 4 * per]) + b"\n" for i in range(0, len(lines), 4 * per)]


library = UC.library


# ---- 1: the base shape ---------------------------------------------------------------------------------------------------
CLASSES = ("forward_only", "reverse_perfect", "reverse_imperfect", "both_assigned", "fwd_imperfect_rev_perfect", "neither_non_aligned",
           "neither_quality_failed", "rescued_from_quality_failed")


@functools.lru_cache(maxsize=None)
def base(seed=0x57A0):
    """600 guides x 20 bases, 3 000 reads of 60 bases, --st 0 --l 20: 1 000 as tests/synth.py makes them (exact, substituted,
    random and 'N' windows at 0, a low-quality share), 1 500 made the same way and mirrored, 500 with a feature at 0 and the
    reverse complement of another at the far end (either may be one base off; a quarter with a low quality byte in the
    forward window)"""
    rng = random.Random(seed)
    lib = library()
    spec = synth.Spec(seed=seed, n_reads=2500, read_len=60, start=0, p_lowq=0.10)
    recs = []
    for i in range(2500):
        s, q = synth.make_read(spec, lib, i)
        rec = (bytes(s), bytes(q))
        recs.append(rec if i < 1000 else flip(rec))
    for i in range(500):
        a, b = lib[rng.randrange(len(lib))].encode(), lib[rng.randrange(len(lib))].encode()
        if rng.random() < 0.3:
            a = UC.mutate1(rng, a)
        if rng.random() < 0.4:
            b = UC.mutate1(rng, b)
        q = bytearray(b"I" * 60)
        if rng.random() < 0.25:
            q[rng.randrange(20)] = ord("#")
        recs.append((a + UC.rand_seq(rng, 20) + revcomp(b), bytes(q)))
    rng.shuffle(recs)
    return lib, UC.fastq_of(recs), dict(RUN)


def classes(lib, fq, **run):
    """records per class of CLASSES, from the two verdicts of every record"""
    v = UC._verdicts(tuple(lib), UC.run_key(run)).of
    n = dict.fromkeys(CLASSES, 0)
    for seq, qual in UC.records(fq):
        F, R = v(seq, qual), v(*mirrored(seq, qual))
        if F[0] >= 0:
            n["both_assigned" if R[0] >= 0 else "forward_only"] += 1
            n["fwd_imperfect_rev_perfect"] += F[1] == 2 and R[0] >= 0 and R[1] == 1
        elif R[0] >= 0:
            n["reverse_perfect" if R[1] == 1 else "reverse_imperfect"] += 1
            n["rescued_from_quality_failed"] += F[2]
        else:
            n["neither_quality_failed" if F[2] else "neither_non_aligned"] += 1
    return n


# ---- 2: odd records --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def odd(seed):
    """1 000 records, half of them mirrored, through raw_edge_cases' oddities (CRLF, trailing blanks, quality lines of
    another length, reads that end inside a window, lower case, 'N' and other bytes, odd quality bytes, empty lines, a
    partial last record, no final newline) plus a leading blank in either line.  -> (library, text, run)"""
    rng = random.Random(0x0DD57 + seed)
    lib = library()
    recs = []
    for i in range(1000):
        g = lib[rng.randrange(len(lib))].encode()
        if rng.random() < 0.2:
            g = UC.mutate1(rng, g)
        n = rng.choice((24, 30, 60, 61, 62, 63, 150))
        s, q = bytearray(g + UC.rand_seq(rng, n - 20)), bytearray(b"I" * n)
        if rng.random() < 0.5:
            s, q = bytearray(revcomp(bytes(s))), q
            windows = ((n - 20, n), (n - 20, n), (0, 20))
        else:
            windows = ((0, 20), (0, 20), (n - 20, n))
        if rng.random() < 0.6:
            RE._spoil(rng, s, q, windows)
        if rng.random() < 0.08:
            s[:0] = rng.choice(RE.BLANKS)
        if rng.random() < 0.08:
            q[:0] = rng.choice(RE.BLANKS)
        recs.append((b"@o%d" % i, bytes(s), bytes(q)))
    fq, = RE._finish(rng, [RE._text(rng, recs)])
    return lib, fq, dict(RUN, miss=1)


# ---- 3: the staging edge ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge(r, anchored):
    """raw_edge_cases.edge_sample(r) with every second record mirrored in place: the offsets and lengths, and so the cells
    (so & 3, qo & 3, ms + r, mq + qn), are the sample's own.  The run's window is at the far end of an unmirrored record
    (--st r-20) or between the anchors.  -> (library, text, run)"""
    lib, _, fq, _ = RE.edge_sample(r, 0, anchored)
    text = mirror_text(fq, lambda i: i % 2 == 1)
    assert RE.layout(text) == RE.layout(fq)
    return lib, text, (RE.anchored_run(1) if anchored else RE.fixed_run(r, 0, 1))


# ---- 4: long reads ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_reads():
    """400 reads of 250 bases (walked in global memory) among 400 of 60 bases, half of each mirrored; --st 0 --l 20"""
    rng = random.Random(0x10A6)
    lib = library()
    recs = []
    for i in range(800):
        n = 250 if i % 2 else 60
        g = lib[rng.randrange(len(lib))].encode()
        roll = rng.random()
        g = UC.mutate1(rng, g) if roll < 0.2 else UC.rand_seq(rng, 20) if roll < 0.3 else g
        q = bytearray(b"I" * n)
        if rng.random() < 0.1:
            q[rng.randrange(20)] = ord("#")
        rec = (g + UC.rand_seq(rng, n - 20), bytes(q))
        recs.append(flip(rec) if rng.random() < 0.5 else rec)
    return lib, UC.fastq_of(recs), dict(RUN, miss=1)


# ---- 5: anchored -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def anchored():
    """--us/--ds --msu 1 --msd 1: 1 200 reads, spacers of 0 .. 9 bases, anchors one base off, half mirrored"""
    rng = random.Random(0xA2C4)
    lib = library()[:80]
    recs = []
    for i in range(1200):
        g = lib[rng.randrange(len(lib))].encode()
        roll = rng.random()
        w = UC.mutate1(rng, g) if roll < 0.2 else UC.rand_seq(rng, 20) if roll < 0.3 else g
        up = UC.mutate1(rng, UC.UP.encode()) if rng.random() < 0.15 else UC.UP.encode()
        down = UC.mutate1(rng, UC.DOWN.encode()) if rng.random() < 0.15 else UC.DOWN.encode()
        s = UC.rand_seq(rng, 2 + rng.randrange(10)) + up + w + down + UC.rand_seq(rng, rng.randrange(8))
        q = bytearray(b"I" * len(s))
        if rng.random() < 0.1:
            q[rng.randrange(len(q))] = ord("#")
        rec = (s, bytes(q))
        recs.append(flip(rec) if rng.random() < 0.5 else rec)
    run = dict(upstream=UC.UP, downstream=UC.DOWN, miss_search_up=1, miss_search_down=1, phred=30, length=20, miss=1)
    return lib, UC.fastq_of(recs), run


# ---- 6: two windows --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_windows():
    """--st 0,30 --l 10 on an A:B library of 200 features: 1 000 reads of 60 bases, half mirrored"""
    rng = random.Random(0x2B1D)
    parts = set()
    while len(parts) < 400:
        parts.add(UC.rand_seq(rng, 10))
    parts = sorted(parts)
    rng.shuffle(parts)
    lib = [(a + b":" + b).decode() for a, b in zip(parts[:200], parts[200:])]
    recs = []
    for i in range(1000):
        a, b = lib[rng.randrange(200)].encode().split(b":")
        roll = rng.random()
        if roll < 0.2:
            a = UC.mutate1(rng, a)
        elif roll < 0.3:
            b = UC.mutate1(rng, b)
        elif roll < 0.4:
            b = UC.rand_seq(rng, 10)
        q = bytearray(b"I" * 60)
        if rng.random() < 0.1:
            q[rng.choice((0, 30)) + rng.randrange(10)] = ord("#")
        rec = (a + UC.rand_seq(rng, 20) + b + UC.rand_seq(rng, 20), bytes(q))
        recs.append(flip(rec) if rng.random() < 0.5 else rec)
    return lib, UC.fastq_of(recs), dict(start="0,30", length=10, phred=30, miss=1)


# ---- 7: a second trip through the grid-stride loop -------------------------------------------------------------------------
POOL = RE.POOL
PASS_RUN = dict(RUN, miss=1)


@functools.lru_cache(maxsize=None)
def pass_pool():
    """257 distinct records of 30 bases, one in eight 190 (a short record is staged -- and mirrored -- over a long one's
    bytes in the lane's second pass), half mirrored"""
    rng = random.Random(0x2FA57)
    lib = library()
    recs = []
    for i in range(POOL):
        g = lib[rng.randrange(40)].encode()
        roll = rng.random()
        g = UC.mutate1(rng, g) if roll < 0.2 else UC.rand_seq(rng, 20) if roll < 0.3 else g
        n = 190 if i % 8 == 3 else 30
        q = bytearray(b"I" * n)
        if rng.random() < 0.1:
            q[rng.randrange(20)] = ord("#")
        rec = (g + UC.rand_seq(rng, n - 20), bytes(q))
        recs.append(flip(rec) if rng.random() < 0.5 else rec)
    assert len(set(recs)) == POOL
    return UC.fastq_of(recs)


def second_pass(n_cu):
    """-> (FASTQ bytes, repetitions), as raw_edge_cases.second_pass: more records than the lanes of a capped launch"""
    reps = -(-(n_cu * 4096 + 3 * POOL) // POOL)
    return pass_pool() * reps, reps


def scaled(e, k):
    return tuple([x * k for x in part] for part in e)


# the cases of the list by name: -> (library, text, run)
CASES = {"base": base, "odd0": lambda: odd(0), "odd1": lambda: odd(1), "odd2": lambda: odd(2), "long_reads": long_reads,
         "anchored": anchored, "two_windows": two_windows, "pass_pool": lambda: (library(), pass_pool(), dict(PASS_RUN))}
CASES.update({f"edge{r}{'a' if a else ''}": (lambda r=r, a=a: edge(r, a)) for r in RE.EDGE_R for a in (False, True)})


def check_coverage():
    """what the cases claim, from the expectation alone"""
    lib, fq, run = base()
    n = classes(lib, fq, miss=1, **run)
    assert all(n[k] >= 30 for k in CLASSES), n
    plain = expect(lib, fq, FWD, miss=1, **run)
    both = expect(lib, fq, BOTH, miss=1, **run)
    assert all(b >= f for b, f in zip(both[0], plain[0])) and sum(both[0]) > sum(plain[0]) + 1000
    for name in ("odd0", "odd1", "odd2"):
        lib, fq, run = CASES[name]()
        recs = UC.records(fq)
        assert len(recs) >= 999
        assert any(s[:1] in b" \t" and s for s, q in recs) and any(q[:1] in b" \t" and q for s, q in recs)      # the second rstrip
        assert any(len(q) < len(s) for s, q in recs) and any(len(q) > len(s) for s, q in recs)
        assert any(0 < len(s) < 20 for s, q in recs) and any(not s for s, q in recs) and any(not q for s, q in recs)
        assert b"\r\n" in fq and any(c in s for s, q in recs for c in b"acgt") and any(b"N" in s for s, q in recs)
        e = expect(lib, fq, BOTH, **run)
        assert e[3][1] > 50 and e[3][2] > 10 and e[3][0] > 50, e[3]
    cells = set()
    for r in RE.EDGE_R:
        for a in (False, True):
            lib, fq, run = edge(r, a)
            here = RE.device_cells(fq)
            assert {RE.staged(c) for c in here} == {True, False}
            cells |= here
            e = expect(lib, fq, BOTH, **run)
            assert e[3][0] > 50 and e[3][1] + e[3][2] > 50, (r, a, e[3])
    assert any(c[2] <= RE.STAGE < c[3] for c in cells) and any(c[3] <= RE.STAGE < c[2] for c in cells)
    assert {(c[0], c[1], c[2], c[3]) for c in cells if c[2] in RE.SUMS and c[3] in RE.SUMS} == \
        {(ms, mq, a, b) for ms in range(4) for mq in range(4) for a in RE.SUMS for b in RE.SUMS}
    for name in ("long_reads", "anchored", "two_windows", "pass_pool"):
        lib, fq, run = CASES[name]()
        e = expect(lib, fq, BOTH, **run)
        assert e[3][0] > 40 and e[3][1] > 40 and e[3][2] > 10 and e[1][3] > 10, (name, e[1], e[3])
