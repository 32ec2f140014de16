"""tests/parts_cases.py -- inputs and expected values shared by the --parts tests (CPU emulation and GPU).

The expectation is plain Python.  The verdict of part i of a read is, by definition (include/f2q.h, f2q_set_parts), what a
Counter run with the single window --st s_i gives the read against part library i: it comes from the oracle, one
single-window run per part (umi_cases._verdicts, one record at a time, cached), for mate 2 on the mate as the run takes it
(paired_cases.mate2_as_taken).  The class rule is written out below."""
import functools
import random

from paired_cases import fastq_of, mate2_as_taken, pair_library, records
from umi_cases import _verdicts, run_key

CLASSES = ("pair_perfect", "pair_imperfect", "recombinant", "part1_only", "part2_only", "neither")
L = 10


def part_libraries(lib):
    """(lib1, lib2, ids): the distinct first / second parts in first-occurrence order, and (i1, i2) per feature"""
    lib1, lib2, at1, at2, ids = [], [], {}, {}, []
    for f in lib:
        a, b = f.split(":")
        if a not in at1:
            at1[a] = len(lib1); lib1.append(a)
        if b not in at2:
            at2[b] = len(lib2); lib2.append(b)
        ids.append((at1[a], at2[b]))
    return lib1, lib2, ids


def expect(lib, fq1, fq2, st1, st2, length, rc2=False, miss=1, phred=30):
    """dict(parts_counts, part1, part2, classes, recombinants={(i1, i2): reads}) of the reads of fq1 (fq2 None: single
    reads with both windows in the one read) or of the pairs (fq1, fq2)"""
    lib1, lib2, ids = part_libraries(lib)
    v1 = _verdicts(tuple(lib1), run_key(dict(start=str(st1), length=length, phred=phred, miss=miss)))
    v2 = _verdicts(tuple(lib2), run_key(dict(start=str(st2), length=length, phred=phred, miss=miss)))
    feature_of = {}
    for f, pair in enumerate(ids):
        feature_of.setdefault(pair, f)                       # a repeated feature: the first
    out = dict(parts_counts=[0] * len(lib), part1=[0] * len(lib1), part2=[0] * len(lib2), classes=[0] * 6, recombinants={})
    recs1 = records(fq1)
    recs2 = recs1 if fq2 is None else [mate2_as_taken(s, q, rc2) for s, q in records(fq2)]
    for (s1, q1), (s2, q2) in zip(recs1, recs2):
        i1, k1, _ = v1.of(s1, q1)                            # k: 1 perfect, 2 imperfect, 3 non-aligned, 0 quality-failed
        i2, k2, _ = v2.of(s2, q2)
        if i1 >= 0:
            out["part1"][i1] += 1
        if i2 >= 0:
            out["part2"][i2] += 1
        if i1 < 0 and i2 < 0:
            cls = 5
        elif i2 < 0:
            cls = 3
        elif i1 < 0:
            cls = 4
        elif (i1, i2) not in feature_of:
            cls = 2
            out["recombinants"][(i1, i2)] = out["recombinants"].get((i1, i2), 0) + 1
        else:
            cls = 0 if k1 == 1 and k2 == 1 else 1
            out["parts_counts"][feature_of[(i1, i2)]] += 1
        out["classes"][cls] += 1
    return out


def _part(rng, n=L):
    return "".join(rng.choice("ACGT") for _ in range(n))


@functools.lru_cache(maxsize=None)
def library(seed=0x9A27):
    """96 combinatorial features of 10 + 10 bases (parts shared by many features), then: a sequence that is part 1 of
    feature 0 and also a part 2 (of a feature of its own); two part-1 sequences one substitution apart at position 4 (a
    read with a third base there is one substitution from both: ambiguous, so non-aligned at --m 1)"""
    rng = random.Random(seed)
    lib = pair_library(96, L, 1, 1, seed, combinatorial=True)
    both = lib[0].split(":")[0]
    lib.append(_part(rng) + ":" + both)
    p = _part(rng)
    p = p[:4] + "A" + p[5:]
    lib.append(p + ":" + _part(rng))
    lib.append(p[:4] + "C" + p[5:] + ":" + _part(rng))
    assert len(set(lib)) == len(lib)
    return tuple(lib)


def ambiguous_part1(lib):
    """the window text one substitution from both of the last two part-1 sequences of library()"""
    p = lib[-1].split(":")[0]
    return p[:4] + "G" + p[5:]


def _sub1(rng, s):
    j = rng.randrange(len(s))
    return s[:j] + rng.choice([c for c in "ACGT" if c != s[j]]) + s[j + 1:]


def make_reads(lib, st1, st2, n, seed, paired=False, rc2=False, read_len=44, ragged=True):
    """(fastq1, fastq2 or None).  Window 1 at st1 (of the read / of mate 1), window 2 at st2 (of the read / of mate 2 as the
    run takes it).  Kinds: a library pair (45 %), a planted recombinant (20 %), one error in EACH part of a library pair
    (6 %: pair_imperfect here, non-aligned by the joined rule at --m 1), the ambiguous part 1 (4 %), the both-positions
    sequence next to parts it is not paired with (3 %), one good part beside junk (6 % + 6 %), junk (the rest).  On top:
    one substitution (8 %), an 'N' (4 %), lower case (6 %), a low quality byte in a window (6 %), and with `ragged` reads
    that end inside window 2 (single) or one mate cut anywhere from empty to whole (paired; never both)."""
    rng = random.Random(seed)
    lib1, lib2, ids = part_libraries(lib)
    held = set(ids)
    both = lib[0].split(":")[0]
    r1, r2 = [], []
    for _ in range(n):
        k = rng.random()
        f = rng.randrange(len(lib))
        a, b = lib[f].split(":")
        if k < 0.45:
            pass
        elif k < 0.65:
            while len(held) < len(lib1) * len(lib2):            # (a library that pairs everything has no recombinant to plant)
                i1, i2 = rng.randrange(len(lib1)), rng.randrange(len(lib2))
                if (i1, i2) not in held:
                    a, b = lib1[i1], lib2[i2]
                    break
        elif k < 0.71:
            a, b = _sub1(rng, a), _sub1(rng, b)
        elif k < 0.75:
            a = ambiguous_part1(lib)
        elif k < 0.78:
            a, b = (both, both) if rng.random() < 0.5 else (rng.choice(lib1), both)
        elif k < 0.84:
            b = _part(rng)
        elif k < 0.90:
            a = _part(rng)
        else:
            a, b = _part(rng), _part(rng)
        if rng.random() < 0.08:
            a = _sub1(rng, a)
        if rng.random() < 0.08:
            b = _sub1(rng, b)
        s1 = bytearray(_part(rng, read_len).encode())
        s2 = bytearray(_part(rng, read_len).encode()) if paired else s1
        s1[st1:st1 + L] = a.encode()
        s2[st2:st2 + L] = b.encode()
        q1 = bytearray(b"I" * read_len)
        q2 = bytearray(b"I" * read_len) if paired else q1
        for s, q, st in ((s1, q1, st1), (s2, q2, st2)):
            if rng.random() < 0.04:
                s[st + rng.randrange(L)] = ord("N")
            if rng.random() < 0.06:
                for j in range(st, st + L):
                    if rng.random() < 0.5:
                        s[j] = ord(chr(s[j]).lower())
            if rng.random() < 0.06:
                q[st + rng.randrange(L)] = rng.choice(b"!#+5:=")
            if rng.random() < 0.02:
                q[st + rng.randrange(L)] = ord(">")             # Phred 29 passes --ph 30
        if ragged and rng.random() < 0.08:
            if not paired:
                cut = rng.randrange(st2, st2 + L)                # the read ends inside window 2 (or just before it)
                del s1[cut:], q1[cut:]
            elif rng.random() < 0.5:
                cut = rng.randrange(0, read_len + 1)
                del s1[cut:], q1[cut:]
            else:
                cut = rng.randrange(0, read_len + 1)
                del s2[cut:], q2[cut:]
        r1.append((bytes(s1), bytes(q1)))
        if paired:
            r2.append(mate2_as_taken(bytes(s2), bytes(q2), rc2))  # back to mate 2 as the sequencer wrote it
    return fastq_of(r1, b"a"), (fastq_of(r2, b"b") if paired else None)


SINGLE = dict(st1=0, st2=20)
PAIRED = dict(st1=5, st2=3)


@functools.lru_cache(maxsize=None)
def sample(paired=False, rc2=False, n=1500, seed=0x51AB):
    """(library, fastq1, fastq2 or None, st1, st2)"""
    lib = library()
    shape = PAIRED if paired else SINGLE
    fq1, fq2 = make_reads(lib, shape["st1"], shape["st2"], n, seed + (2 if rc2 else 1 if paired else 0), paired=paired, rc2=rc2)
    return lib, fq1, fq2, shape["st1"], shape["st2"]


def long_reads(n=400, seed=0x10E6):
    """single reads of 150 .. 400 bases, so that most records are longer than the 192-byte LDS staging area of a line and
    take the global-memory walk; windows at 0 and 20"""
    rng = random.Random(seed)
    lib = library()
    base, _ = make_reads(lib, 0, 20, n, seed, ragged=False)
    recs = []
    for s, q in records(base):
        extra = rng.randrange(106, 357)
        recs.append((s + _part(rng, extra).encode(), q + b"I" * extra))
    return lib, fastq_of(recs, b"l")


def one_feature():
    return ("ACGTACGTAC:TTGCATGCAA",)


def star_library(n2=12, seed=0x57A2):
    """one part 1 paired with every part 2: no pair of assigned parts can be a recombinant"""
    rng = random.Random(seed)
    a = _part(rng)
    seen = []
    while len(seen) < n2:
        b = _part(rng)
        if b not in seen:
            seen.append(b)
    return tuple(a + ":" + b for b in seen)
