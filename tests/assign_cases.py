"""tests/assign_cases.py -- inputs and expected values shared by the Extract+Count-with-a-library tests (CPU emulation and
GPU).  The yardstick is the oracle in Counter mode: over the same FASTQ bytes for the count vector and the five counters,
and per key by feeding a fresh Counter-mode oracle one record that carries the key as its whole window."""
import functools
import random

import synth
from conftest import sprinkle_symbols
from oracle import oracle as O


def fastq_of(recs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(recs))


def feats(lib):
    return [(str(i), s) for i, s in enumerate(lib)]


def hamming(a, b):
    assert len(a) == len(b)
    return sum(x != y for x, y in zip(a, b))


def mutate(rng, s, k):
    """s with k distinct positions changed to another base"""
    b = bytearray(s.encode() if isinstance(s, str) else s)
    for pos in rng.sample(range(len(b)), k):
        b[pos] = rng.choice([c for c in b"ACGT" if c != b[pos]])
    return bytes(b)


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def aggregate(lib, fq, miss, **run):
    """(counts, stats) of a Counter-mode oracle over the FASTQ bytes"""
    o = O.Oracle(features=feats(lib), miss=miss, **run)
    o.count_fastq(fq)
    out = (o.counts(), o.stats())
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def _key_verdict(lib, key, miss):
    o = O.Oracle(features=feats(lib), miss=miss, phred=1, length=len(key), start="0")
    k = key.encode("latin-1")
    o.count_fastq(b"@k\n" + k + b"\n+\n" + b"I" * len(k) + b"\n")
    counts, st = o.counts(), o.stats()
    o.close()
    assert st[0] == 1 and st[1] + st[2] + st[3] == 1 and sum(counts) == st[1] + st[2]
    if st[3]:
        return -1, -1
    f = counts.index(1)
    return f, (0 if st[1] else hamming(key, lib[f]))


def key_verdict(lib, key, miss):
    """(feature, distance) the reference gives a read whose joined key is `key` (no ':' in it); (-1, -1): non-aligned"""
    return _key_verdict(tuple(lib), key, miss)


def check_rows(lib, rows, counts, stats, miss):
    """rows = [(key, reads, first, feature, dist)] of one assign against its own aggregate and, per key, the oracle"""
    by_feature = [0] * len(lib)
    verdicts = [0, 0, 0]
    for key, n, _first, f, d in rows:
        if ":" in key:
            assert (f == -1) == (d == -1), key
            if f >= 0:
                assert len(lib[f]) == len(key) and d == hamming(key, lib[f]) and d <= miss, (key, f, d)
        else:
            assert (f, d) == key_verdict(lib, key, miss), (key, f, d)
        if f >= 0:
            by_feature[f] += n
        verdicts[0 if d == 0 else 1 if d > 0 else 2] += n
    assert by_feature == list(counts)
    assert verdicts == list(stats[1:4])


# ---- the cases (each: lib, fastq, run keywords, the --m values) --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixed_window():
    """--st 5 --l 20: 60 guides, 3 000 reads of 40 bases with 0..3 substitutions, N / IUPAC / junk / lower-case symbols,
    300 reads that end inside the window, 50 that end before it, reads with >= 4 'N's, a Phred-failing share"""
    rng = random.Random(101)
    start, length = 5, 20
    lib = synth.make_library(60, length, 0xA551)
    recs = []
    for i in range(3000):
        g = lib[rng.randrange(len(lib))]
        win = mutate(rng, g, rng.choice((1, 2, 3))) if rng.random() < 0.3 else g.encode()
        if rng.random() < 0.05:
            win = rand_seq(rng, length)
        s = rand_seq(rng, start) + win + rand_seq(rng, 40 - start - length)
        q = bytearray(b"I" * 40)
        if rng.random() < 0.06:
            q[start + rng.randrange(length)] = ord("#")
        recs.append((s, bytes(q)))
    for i in range(300):                                        # clipped keys of 18 bases
        s = rand_seq(rng, start) + lib[rng.randrange(len(lib))].encode()[:18]
        recs.append((s, b"I" * len(s)))
    for i in range(50):                                         # the empty key
        n = rng.randrange(0, start + 1)
        recs.append((rand_seq(rng, n), b"I" * n))
    rng.shuffle(recs)
    fq = sprinkle_symbols(fastq_of(recs), 7, rate=0.08)
    many_n = []
    for i in range(30):                                         # >= 4 'N's: the byte-string table
        w = bytearray(lib[rng.randrange(len(lib))].encode())
        for pos in rng.sample(range(length), rng.choice((4, 5, 6))):
            w[pos] = ord("N")
        many_n.append((rand_seq(rng, start) + bytes(w) + rand_seq(rng, 15), b"I" * 40))
    return lib, fq + fastq_of(many_n), dict(start=str(start), length=length, phred=30), (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def ties():
    """feature pairs at Hamming distance 2; reads carrying the midpoint (distance 1 from both: unassigned at every m >= 1)
    and reads at distance 1 from one and 3 from the other (the nearer one's at m = 3)"""
    rng = random.Random(202)
    length = 20
    lib, mids, near = [], [], []
    for _ in range(8):
        a = rand_seq(rng, length)
        p, q, r = rng.sample(range(length), 3)
        b = bytearray(a)
        for pos in (p, q):
            b[pos] = rng.choice([c for c in b"ACGT" if c != a[pos]])
        m = bytearray(a); m[p] = b[p]
        n = bytearray(a); n[r] = rng.choice([c for c in b"ACGT" if c != a[r]])
        lib += [a.decode(), bytes(b).decode()]
        mids.append(bytes(m)); near.append((bytes(n), len(lib) - 2))
    lib += synth.make_library(10, length, 0x7135)
    assert len(set(lib)) == len(lib)
    recs = []
    for i in range(2000):
        c = rng.random()
        w = mids[rng.randrange(8)] if c < 0.3 else near[rng.randrange(8)][0] if c < 0.6 else lib[rng.randrange(len(lib))].encode()
        recs.append((w + rand_seq(rng, 10), b"I" * 30))
    return lib, fastq_of(recs), dict(start="0", length=length, phred=30), (1, 2, 3), mids, near


@functools.lru_cache(maxsize=None)
def irregular():
    """features of 18, 20 and 24 bases, one holding an 'N', one of 36 bases: the byte-string index decides every key.
    --st 3 --l 40 on reads that end 18 / 20 / 24 / 36 bases behind the start: the clipped windows are the keys"""
    rng = random.Random(303)
    lib = [rand_seq(rng, n).decode() for n in (18,) * 12 + (20,) * 12 + (24,) * 12]
    withn = bytearray(rand_seq(rng, 20)); withn[7] = ord("N")
    lib += [bytes(withn).decode(), rand_seq(rng, 36).decode()]
    assert len(set(lib)) == len(lib)
    recs = []
    for i in range(2500):
        g = lib[rng.randrange(len(lib))]
        w = mutate(rng, g, rng.choice((1, 2))) if rng.random() < 0.3 else g.encode()
        if rng.random() < 0.05:
            w = rand_seq(rng, rng.choice((18, 20, 24, 36)))
        s = rand_seq(rng, 3) + w
        recs.append((s, b"I" * len(s)))
    fq = sprinkle_symbols(fastq_of(recs), 9, rate=0.01, symbols=b"NnacgtR")
    return lib, fq, dict(start="3", length=40, phred=30), (0, 1, 2)


@functools.lru_cache(maxsize=None)
def two_windows():
    """--st 0,10 --l 10 against an A:B library (plus a few one-part features): low-quality parts leave single-part keys"""
    rng = random.Random(404)
    lib = []
    while len(lib) < 50:
        f = rand_seq(rng, 10).decode() + ":" + rand_seq(rng, 10).decode()
        if f not in lib:
            lib.append(f)
    parts = [f.split(":")[i] for f in lib[:6] for i in (0, 1)]
    lib += [p for p in dict.fromkeys(parts)]
    recs = []
    for i in range(3000):
        a, b = lib[rng.randrange(50)].split(":")
        a = mutate(rng, a, 1) if rng.random() < 0.15 else a.encode()
        b = mutate(rng, b, 1) if rng.random() < 0.15 else b.encode()
        if rng.random() < 0.05:
            a = rand_seq(rng, 10)
        q = bytearray(b"I" * 26)
        c = rng.random()
        if c < 0.12:
            q[rng.randrange(10)] = ord("#")
        elif c < 0.24:
            q[10 + rng.randrange(10)] = ord("#")
        elif c < 0.28:
            q[2] = q[13] = ord("#")
        recs.append((a + b + rand_seq(rng, 6), bytes(q)))
    fq = sprinkle_symbols(fastq_of(recs), 11, rate=0.01, symbols=b"N")
    return lib, fq, dict(start="0,10", length=10, phred=30), (0, 1, 2)


UP, DOWN = "GTTTAAGAGC", "CGAAACACCG"


@functools.lru_cache(maxsize=None)
def anchored(n_reads=10000):
    """--us/--ds with --msu 1 --msd 1, features of 18 / 20 / 22 bases, the cassette at a varying offset"""
    rng = random.Random(505)
    lib = [rand_seq(rng, n).decode() for n in (18,) * 20 + (20,) * 20 + (22,) * 20]
    assert len(set(lib)) == len(lib)
    recs = []
    for i in range(n_reads):
        g = lib[rng.randrange(len(lib))]
        w = mutate(rng, g, rng.choice((1, 2))) if rng.random() < 0.2 else g.encode()
        if rng.random() < 0.03:
            w = rand_seq(rng, rng.choice((18, 20, 22)))
        up = mutate(rng, UP, 1) if rng.random() < 0.1 else UP.encode()
        down = mutate(rng, DOWN, 1) if rng.random() < 0.1 else DOWN.encode()
        s = rand_seq(rng, rng.randrange(0, 20)) + up + w + down + rand_seq(rng, rng.randrange(0, 12))
        q = bytearray(b"I" * len(s))
        if rng.random() < 0.05:
            q[rng.randrange(len(q))] = ord("#")
        recs.append((s, bytes(q)))
    fq = sprinkle_symbols(fastq_of(recs), 13, rate=0.003, symbols=b"NnR")
    run = dict(upstream=UP, downstream=DOWN, miss_search_up=1, miss_search_down=1, phred=30, length=20)
    return lib, fq, run, (0, 1, 2)


@functools.lru_cache(maxsize=None)
def growth():
    """three blocks of a fixed-window sample in which most windows are random: >= 20 000 distinct keys in 40 000 reads"""
    rng = random.Random(606)
    lib = synth.make_library(60, 20, 0xB10C)
    blocks = []
    for n in (15000, 15000, 10000):
        recs = []
        for i in range(n):
            w = rand_seq(rng, 20) if rng.random() < 0.8 else lib[rng.randrange(60)].encode()
            if rng.random() < 0.1:
                w = mutate(rng, lib[rng.randrange(60)], 1)
            recs.append((w + rand_seq(rng, 5), b"I" * 25))
        blocks.append(fastq_of(recs))
    return lib, blocks, dict(start="0", length=20, phred=30)
