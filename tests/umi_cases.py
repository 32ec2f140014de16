"""tests/umi_cases.py -- inputs and expected values shared by the --umi tests (CPU emulation and GPU).

The expectation is plain Python: 4-line framing with rstrip() as the reference frames; the feature of each read from the
oracle in Counter mode, run once per distinct record text on a one-record FASTQ (cached); the UMI rule of include/f2q.h
(f2q_set_umi); a set() of UMIs per feature."""
import functools
import random

import synth
from oracle import oracle as O

S, L = 20, 8                                   # the base shape's UMI window


def fastq_of(recs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(recs))


def records(fq):
    """[(sequence line, quality line)] of the complete records, each line rstrip()ped (fast2q.py:324-328)"""
    lines = fq.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [(lines[i + 1].rstrip(), lines[i + 3].rstrip()) for i in range(0, len(lines) - 3, 4)]


def run_key(run):
    return tuple(sorted((k, str(v)) for k, v in run.items()))


class _Verdicts:
    """one Counter-mode oracle per (library, run): (feature or -1, index of the counter the read adds to, quality_failed)"""

    def __init__(self, lib, run):
        self.o = O.Oracle(features=[(str(i), s) for i, s in enumerate(lib)], **dict(run))
        self.memo = {}

    def of(self, seq, qual):
        got = self.memo.get((seq, qual))
        if got is None:
            self.o.reset()
            self.o.count_fastq(b"@k\n" + seq + b"\n+\n" + qual + b"\n")
            counts, st = self.o.counts(), self.o.stats()
            assert st[0] == 1 and sum(st[1:4]) <= 1 and sum(counts) == st[1] + st[2]
            verdict = 1 if st[1] else 2 if st[2] else 3 if st[3] else 0
            got = self.memo[(seq, qual)] = (counts.index(1) if st[1] + st[2] else -1, verdict, st[4])
        return got


@functools.lru_cache(maxsize=None)
def _verdicts(lib, rk):
    return _Verdicts(lib, rk)


def umi_of(seq, qual, start, length, phred):
    """the valid UMI of a read, else None"""
    u, q = seq[start:start + length].upper(), qual[start:start + length]
    if len(u) < length or len(q) < length or set(u) - set(b"ACGT"):
        return None
    ph = max(int(phred), 1)                                      # fast2q.py:1118-1125
    if any(33 <= c <= min(ph + 31, 126) for c in q):             # the fail set of --ph (:1112-1129); --ph <= 1: empty
        return None
    return bytes(u)


def expect(lib, fq, umi, **run):
    """(counts, stats, umis, umi_reads, umi_failed) of the FASTQ bytes"""
    v = _verdicts(tuple(lib), run_key(run))
    counts, stats = [0] * len(lib), [0] * 5
    seen = [set() for _ in lib]
    ok = bad = 0
    for seq, qual in records(fq):
        f, verdict, qfail = v.of(seq, qual)
        stats[0] += 1
        stats[4] += qfail
        if verdict:
            stats[verdict] += 1
        if f >= 0:
            counts[f] += 1
            u = umi_of(seq, qual, umi[0], umi[1], run.get("phred", 30))
            if u is None:
                bad += 1
            else:
                ok += 1
                seen[f].add(u)
    return counts, stats, [len(s) for s in seen], ok, bad


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def mutate1(rng, s, lo=0, hi=None):
    b = bytearray(s)
    pos = rng.randrange(lo, len(b) if hi is None else hi)
    b[pos] = rng.choice([c for c in b"ACGT" if c != b[pos]])
    return bytes(b)


def library():
    return synth.make_library(600, 20, 0x0A11)


def sample(seed, n_reads=4000, pool=48):
    """the base shape: reads of 60 bases from tests/synth.py's generator (window at 0: exact, substituted, random and 'N'
    windows, a low-quality share), positions [20, 28) rewritten with one of `pool` UMIs"""
    rng = random.Random(seed)
    lib = library()
    umis = [rand_seq(rng, L) for _ in range(pool)]
    spec = synth.Spec(seed=seed, n_reads=n_reads, read_len=60, start=0)
    recs = []
    for i in range(n_reads):
        s, q = synth.make_read(spec, lib, i)
        recs.append((s[:S] + umis[rng.randrange(pool)] + s[S + L:], q))
    return fastq_of(recs)


RUN = dict(start="0", length=20, phred=30)


@functools.lru_cache(maxsize=None)
def base(seed=0x0B5E):
    """600 guides x 20 bp, 4 000 reads of 60 bp, --st 0 --l 20, UMI at 20,8 from a pool of 48"""
    return library(), sample(seed), dict(RUN), (S, L)


@functools.lru_cache(maxsize=None)
def invalid():
    """reads of one feature each, every UMI distinct: whole; cut to 24, 27 and 28 bases; an 'N' / an 'n' / a lower-case
    base in the UMI; one UMI quality byte that fails --ph (first and last position) and one that just passes; a quality
    line cut to 27 bytes under a whole sequence line; a low byte just outside the window"""
    rng = random.Random(77)
    lib = library()
    recs, kinds = [], []
    for kind in ("whole", "cut24", "cut27", "cut28", "N", "n", "lower", "lowq_first", "lowq_last", "q29_last", "qual27", "lowq_outside") * 12:
        g = lib[rng.randrange(len(lib))].encode()
        s = bytearray(g + rand_seq(rng, 40))
        q = bytearray(b"I" * 60)
        if kind.startswith("cut"):
            n = int(kind[3:]); s, q = s[:n], q[:n]
        elif kind == "N":
            s[S + rng.randrange(L)] = ord("N")
        elif kind == "n":
            s[S + rng.randrange(L)] = ord("n")
        elif kind == "lower":
            s[S + 3] = ord(chr(s[S + 3]).lower())
        elif kind == "lowq_first":
            q[S] = ord("#")
        elif kind == "lowq_last":
            q[S + L - 1] = ord("=")                              # Phred 28: the highest score --ph 30 fails (fast2q.py:1112-1129)
        elif kind == "q29_last":
            q[S + L - 1] = ord(">")                              # Phred 29 passes
        elif kind == "qual27":
            q = q[:27]
        elif kind == "lowq_outside":
            q[S + L] = ord("#")
        recs.append((bytes(s), bytes(q)))
        kinds.append(kind)
    return lib, fastq_of(recs), kinds


@functools.lru_cache(maxsize=None)
def imperfect():
    """--m 1: feature 3 read exactly and at distance 1 with the SAME UMI (one pair), feature 3 and feature 9 with the same
    UMI (two pairs), feature 9 at distance 1 with two UMIs of its own"""
    rng = random.Random(78)
    lib = library()
    u1, u2, u3 = b"ACGTACGT", b"TTGCAAGC", b"GGGGCCCC"
    q = b"I" * 60

    def read(window, umi):
        return (window + umi + rand_seq(rng, 32), q)
    a, b = lib[3].encode(), lib[9].encode()
    recs = [read(a, u1), read(mutate1(rng, a), u1), read(mutate1(rng, a), u1), read(b, u1),
            read(mutate1(rng, b), u2), read(mutate1(rng, b), u3), read(mutate1(rng, b), u3)]
    return lib, fastq_of(recs), {3: 1, 9: 3}


@functools.lru_cache(maxsize=None)
def wide():
    """UMI 0,16 on top of the feature window (--st 0 --l 20), features 512 .. 601 only: the whole 32-bit UMI field next
    to feature indices that need more than 9 bits; features 600 / 601 start with sixteen 'T's / 'A's (all-ones and zero
    codes).  Reads at distance 1 inside the first 16 bases give one feature several UMIs"""
    rng = random.Random(79)
    lib = library() + ["T" * 16 + "ACGA", "A" * 16 + "CCAT"]
    recs = []
    for i in range(900):
        f = 512 + rng.randrange(90)
        w = lib[f].encode()
        if rng.random() < 0.5:
            w = mutate1(rng, w, 0, 16)
        recs.append((w + rand_seq(rng, 20), b"I" * 40))
    return lib, fastq_of(recs), dict(start="0", length=20, phred=30), (0, 16)


UP, DOWN = "GTTTAAGAGC", "CGAAACACCG"


@functools.lru_cache(maxsize=None)
def anchored():
    """--us/--ds with --msu 1 --msd 1: the UMI in read positions [2, 10), then a spacer of 0 .. 9 bases, the cassette"""
    rng = random.Random(80)
    lib = library()[:80]
    umis = [rand_seq(rng, 8) for _ in range(24)]
    recs = []
    for i in range(1500):
        g = lib[rng.randrange(len(lib))].encode()
        w = mutate1(rng, g) if rng.random() < 0.2 else g
        up = mutate1(rng, UP.encode()) if rng.random() < 0.1 else UP.encode()
        u = umis[rng.randrange(24)]
        if rng.random() < 0.05:
            u = u[:3] + b"N" + u[4:]
        s = rand_seq(rng, 2) + u + rand_seq(rng, rng.randrange(10)) + up + w + DOWN.encode() + rand_seq(rng, rng.randrange(8))
        q = bytearray(b"I" * len(s))
        if rng.random() < 0.1:
            q[rng.randrange(len(q))] = ord("#")
        recs.append((s, bytes(q)))
    run = dict(upstream=UP, downstream=DOWN, miss_search_up=1, miss_search_down=1, phred=30, length=20)
    return lib, fastq_of(recs), run, (2, 8)
