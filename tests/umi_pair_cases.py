"""tests/umi_pair_cases.py -- the yardstick and the inputs shared by the paired UMI tests (--umi1 / --umi2 with --pe;
f2q_set_umi_paired), CPU emulation and GPU.

Plain Python over the existing oracle.  Per pair, the feature and the verdict come from the oracle on that pair's ONE
merged record, built exactly as paired_cases.merged_groups builds it (memoised per distinct pair); a pair no
construction covers is reported as `uncovered`, and every test asserts there is none.  The UMI comes from the two
ORIGINAL mates by the rule of include/f2q.h: part 1 from mate 1, part 2 from mate 2 as sequenced, each by
umi_cases.umi_of on its own mate, the UMI their concatenation and valid when every present part is.  What the collapse
rules make of the (feature, UMI, reads) table is left to tests/umi_collapse_cases.py and tests/umi_dir_cases.py."""
import collections
import functools
import random

import paired_cases as PC
import umi_cases as UC
import umi_collapse_cases as CC
import umi_dir_cases as DC
from oracle import oracle as O


class _PairVerdicts:
    """(feature or -1, counter index, quality_failed) per distinct pair, or None for a pair no construction covers"""

    def __init__(self, lib, st1, st2, length, rc2, miss, phred):
        self.feats = [(str(i), s) for i, s in enumerate(lib)]
        self.geom = (list(st1), list(st2), length, rc2)
        self.run = dict(miss=miss, phred=phred, length=length)
        self.oracles, self.memo = {}, {}

    def of(self, m1, m2):
        key = (m1, m2)
        if key not in self.memo:
            groups, uncovered = PC.merged_groups(PC.fastq_of([m1]), PC.fastq_of([m2]), *self.geom)
            if uncovered:
                self.memo[key] = None
            else:
                (start, fq), = groups.items()
                o = self.oracles.get(start)
                if o is None:
                    o = self.oracles[start] = O.Oracle(features=self.feats, start=start, **self.run)
                o.reset()
                o.count_fastq(fq)
                counts, st = o.counts(), o.stats()
                assert st[0] == 1 and sum(st[1:4]) <= 1 and sum(counts) == st[1] + st[2]
                verdict = 1 if st[1] else 2 if st[2] else 3 if st[3] else 0
                self.memo[key] = (counts.index(1) if st[1] + st[2] else -1, verdict, st[4])
        return self.memo[key]


@functools.lru_cache(maxsize=None)
def _verdicts(lib, st1, st2, length, rc2, miss, phred):
    return _PairVerdicts(lib, st1, st2, length, rc2, miss, phred)


def umi_of_pair(m1, m2, parts, phred):
    """the valid UMI of a pair of (sequence, quality) mates as sequenced, else None"""
    out = b""
    for (seq, qual), part in zip((m1, m2), parts):
        if part:
            u = UC.umi_of(seq, qual, part[0], part[1], phred)
            if u is None:
                return None
            out += u
    return out


Expected = collections.namedtuple("Expected", "counts stats per ok bad uncovered")


def expect(lib, fq1, fq2, st1, st2, length, rc2, parts, miss=1, phred=30):
    """counts, the five counters, per feature {UMI: reads} in first-seen order, pairs with a valid / an invalid UMI, and
    the pairs no construction covers"""
    v = _verdicts(tuple(lib), tuple(st1), tuple(st2), length, bool(rc2), miss, phred)
    counts, stats = [0] * len(lib), [0] * 5
    per = [collections.OrderedDict() for _ in lib]
    ok = bad = uncovered = 0
    for m1, m2 in zip(PC.records(fq1), PC.records(fq2)):
        got = v.of(m1, m2)
        if got is None:
            uncovered += 1
            continue
        f, verdict, qfail = got
        stats[0] += 1
        stats[4] += qfail
        if verdict:
            stats[verdict] += 1
        if f >= 0:
            counts[f] += 1
            u = umi_of_pair(m1, m2, parts, phred)
            if u is None:
                bad += 1
            else:
                ok += 1
                per[f][u] = per[f].get(u, 0) + 1
    return Expected(counts, stats, per, ok, bad, uncovered)


def umis_of(e):
    return [len(c) for c in e.per]


def cluster_of(e):
    """(molecules per feature, pairs, edges): umi_collapse_cases.components per feature"""
    per = [CC.components(set(c)) for c in e.per]
    return [m for m, _ in per], sum(len(c) for c in e.per), sum(x for _, x in per)


def directional_of(e):
    """(molecules, pairs, edges, dominated, reads): umi_dir_cases' restatement of UMI-tools, under its three tie orders"""
    mol = None
    for tie in DC.TIE_ORDERS:
        got = [DC.umitools_directional(c, DC.ordered(c, tie, f)) for f, c in enumerate(e.per)]
        assert mol is None or got == mol, tie
        mol = got
    return mol, sum(len(c) for c in e.per), cluster_of(e)[2], sum(DC.dominated(c) for c in e.per), e.ok


def code_of(u):
    return sum(b"ACGT".index(ch) << (2 * j) for j, ch in enumerate(u))


def table_of(e):
    """[(feature, codes, reads)] sorted by (feature, codes): what f2q_umi_pairs returns"""
    return sorted((f, code_of(u), n) for f, c in enumerate(e.per) for u, n in c.items())


# ---- inputs ------------------------------------------------------------------------------------------------------------
ST1, ST2, LEN = (5,), (0,), 10                 # --st 5 --st2 0 --l 10
UMI2 = (12, 8)                                 # behind mate 2's window: a mate 2 cut inside the UMI keeps its window whole
TWO = ((20, 6), (12, 10))                      # all 32 code bits


def _records(fq):
    return PC.records(fq)


def plant(fq1, fq2, parts, pool, seed):
    """every pair's UMI positions rewritten with a UMI of the pool (as sequenced), where the mate holds them all"""
    rng = random.Random(seed)
    r1, r2 = [list(map(bytearray, r)) for r in _records(fq1)], [list(map(bytearray, r)) for r in _records(fq2)]
    for a, b in zip(r1, r2):
        u = pool[rng.randrange(len(pool))]
        at = 0
        for rec, part in ((a, parts[0]), (b, parts[1])):
            if part:
                if len(rec[0]) >= part[0] + part[1]:
                    rec[0][part[0]:part[0] + part[1]] = u[at:at + part[1]]
                at += part[1]
    return PC.fastq_of([tuple(map(bytes, r)) for r in r1], b"a"), PC.fastq_of([tuple(map(bytes, r)) for r in r2], b"b")


@functools.lru_cache(maxsize=None)
def base(rc2, n_pairs=3000, seed=0x0B5E):
    """pair_library(200, 10, 1, 1), --st 5 --st2 0 --l 10, mates of 60 bases, UMI2 12,8 from a pool of 48.  Under rc2
    make_pairs puts mate 2's window at the END of the text as sequenced, so positions [12, 20) are free of it either way"""
    lib = PC.pair_library(200, LEN, 1, 1, 21)
    fq1, fq2 = PC.make_pairs(lib, LEN, list(ST1), list(ST2), rc2, n_pairs, seed=seed, len1=60, len2=60)
    rng = random.Random(seed + 1)
    pool = [UC.rand_seq(rng, 8) for _ in range(48)]
    fq1, fq2 = plant(fq1, fq2, (None, UMI2), pool, seed + 2)
    return lib, fq1, fq2


def hand_pair(lib, f, rc2, rng, len1=60, len2=60):
    """one exact pair of feature f with random filler: (s1, q1), (s2, q2) as sequenced, all qualities 'I'"""
    p1, p2 = [p.encode() for p in lib[f].split(":")]
    s1 = bytearray(UC.rand_seq(rng, len1)); s1[ST1[0]:ST1[0] + LEN] = p1
    t2 = bytearray(UC.rand_seq(rng, len2)); t2[ST2[0]:ST2[0] + LEN] = p2      # as the run takes it
    s2 = PC.revcomp(bytes(t2)) if rc2 else bytes(t2)
    return [bytearray(s1), bytearray(b"I" * len1)], [bytearray(s2), bytearray(b"I" * len2)]


def set_umi(m1, m2, parts, u):
    at = 0
    for rec, part in ((m1, parts[0]), (m2, parts[1])):
        if part:
            rec[0][part[0]:part[0] + part[1]] = u[at:at + part[1]]
            at += part[1]


def fastqs(pairs):
    return (PC.fastq_of([(bytes(a[0]), bytes(a[1])) for a, _ in pairs], b"a"), PC.fastq_of([(bytes(b[0]), bytes(b[1])) for _, b in pairs], b"b"))


ORIENT_UMIS = [b"AAAAAAAC", b"GTTTTTTT", b"ACGTTGCA", b"CCCCAAAA", b"TTTTGGGG", b"GATTACAG", b"CTGTAATC", b"AAGGCCTA", b"TAGGCCTT",
               b"CAGTCAGG", b"CCTGACTG", b"AAAACCCC"]


@functools.lru_cache(maxsize=None)
def orientation():
    """a dozen pairs, rc2 on, mate-2 UMIs that are not their own reverse complement: AAAAAAAC and its reverse complement
    GTTTTTTT on feature 0 (two pairs of the set), the others on features 1 .. 10.  Mates of 40 bases: under rc2 the window
    of mate 2 as sequenced is [30, 40), the UMI at [12, 20)"""
    rng = random.Random(0x0121)
    lib = PC.pair_library(200, LEN, 1, 1, 21)
    pairs, want = [], []
    for i, u in enumerate(ORIENT_UMIS):
        assert PC.revcomp(u) != u
        f = 0 if i < 2 else i - 1
        m1, m2 = hand_pair(lib, f, True, rng, 40, 40)
        set_umi(m1, m2, (None, UMI2), u)
        pairs.append((m1, m2)); want.append((f, code_of(u), 1))
    return lib, fastqs(pairs), sorted(want)


INVALID_KINDS = ("whole", "cut_in", "cut_exact", "N", "n", "lower", "lowq_first", "lowq_last", "q29_first", "q29_last", "lowq_before",
                 "lowq_after", "qual_minus1", "qual_into")
# kinds whose UMI is valid at --ph 30
VALID_KINDS = {"whole", "cut_exact", "lower", "q29_first", "q29_last", "lowq_before", "lowq_after", "qual_minus1"}


@functools.lru_cache(maxsize=None)
def invalid(rc2):
    """umi_cases.invalid()'s kinds applied to mate 2 (the UMI part 12,8 of its text as sequenced), twelve pairs per kind,
    every UMI distinct, mate 1 whole with a quality line as long (it carries the construction).  Without rc2 mate 2 has 40
    bases, its window [0, 10) in front of the UMI: cutting it to 19 / 20 bases leaves the window whole.  Under rc2 the
    window the run takes is the END of the text as sequenced, so a cut mate 2 gets the feature's part written there again
    (over the UMI's tail: the UMI of "cut_exact" is then what those positions hold).  A byte just outside the part lies on
    the other side of it in the merged record under rc2"""
    rng = random.Random(0x1A7 + rc2)
    lib = PC.pair_library(200, LEN, 1, 1, 21)
    S, L = UMI2
    pairs, kinds, seen = [], [], set()
    for kind in INVALID_KINDS * 12:
        while True:
            f = rng.randrange(len(lib))
            m1, m2 = hand_pair(lib, f, rc2, rng, 40, 40)
            u = UC.rand_seq(rng, L)
            set_umi(m1, m2, (None, UMI2), u)
            s, q = m2
            if kind in ("cut_in", "cut_exact"):
                n = S + L - 1 if kind == "cut_in" else S + L
                del s[n:], q[n:]
                if rc2:                                              # the window the run takes is the end of the text that is left
                    s[n - LEN:] = PC.revcomp(lib[f].split(":")[1].encode())
                    u = bytes(s[S:S + L]).ljust(L, b"-")
            if u not in seen:
                break
        seen.add(u)
        if kind == "N":
            s[S + rng.randrange(L)] = ord("N")
        elif kind == "n":
            s[S + rng.randrange(L)] = ord("n")
        elif kind == "lower":
            s[S + 3] = ord(chr(s[S + 3]).lower())
        elif kind == "lowq_first":
            q[S] = ord("#")
        elif kind == "lowq_last":
            q[S + L - 1] = ord("=")                                  # Phred 28: the highest score --ph 30 fails
        elif kind == "q29_first":
            q[S] = ord(">")                                          # Phred 29 passes
        elif kind == "q29_last":
            q[S + L - 1] = ord(">")
        elif kind == "lowq_before":
            q[S - 1] = ord("#")
        elif kind == "lowq_after":
            q[S + L] = ord("#")
        elif kind == "qual_minus1":
            del q[len(q) - 1:]                                       # the sequence line whole, the quality line one byte short
        elif kind == "qual_into":
            del q[S + L - 2:]
        pairs.append((m1, m2)); kinds.append(kind)
    return lib, fastqs(pairs), kinds


@functools.lru_cache(maxsize=None)
def two_parts():
    """600 features (indices above 511 in use), UMI1 20,6 + UMI2 12,10, rc2 on, mates of 40 bases: pairs that share part 1
    and differ in part 2 and the other way round (one base apart: edges of the collapse), the all-T and all-A UMIs, one
    part invalid next to a valid one (both ways); the same pairs serve the mate-1-only layout"""
    rng = random.Random(0x2B)
    lib = PC.pair_library(600, LEN, 1, 1, 22)
    pairs = []

    def add(f, u, n=1, spoil=None):
        for _ in range(n):
            m1, m2 = hand_pair(lib, f, True, rng, 40, 40)
            set_umi(m1, m2, TWO, u)
            if spoil == 1:
                m1[0][TWO[0][0] + 2] = ord("N")
            elif spoil == 2:
                m2[1][TWO[1][0] + 9] = ord("#")
            pairs.append((m1, m2))
    a, b = UC.rand_seq(rng, 6), UC.rand_seq(rng, 10)
    add(599, a + b, 5)
    add(599, a + UC.mutate1(rng, b), 1)                              # part 1 shared, part 2 one base apart
    add(599, UC.mutate1(rng, a) + b, 2)                              # the other way round
    add(599, UC.rand_seq(rng, 6) + b, 1)
    add(598, a + b, 1)                                               # the same UMI on another feature
    add(550, b"T" * 16, 2); add(550, b"A" * 16, 1); add(550, b"T" * 15 + b"G", 1)
    add(513, a + b, 2, spoil=1); add(513, a + b, 2, spoil=2); add(513, a + b, 1)
    for _ in range(300):
        add(512 + rng.randrange(88), rng.choice((a, UC.rand_seq(rng, 6))) + rng.choice((b, UC.rand_seq(rng, 10))))
    rng.shuffle(pairs)
    return lib, fastqs(pairs)


def staging_edge(width_words):
    """pairs whose merged sequence lines have 4 W - 4 .. 4 W + 4 bytes (mate 1 of 4 W - 60 + d bases, mate 2 of 60), and
    mates of 300 bases each; rc2 on, UMI1 20,6 + UMI2 12,10.  The records lie back to back in the block; every third pair has
    a mate-2 quality line one byte short, so the record sizes are odd and even and all four byte alignments occur"""
    rng = random.Random(0x57A6E + width_words)
    lib = PC.pair_library(200, LEN, 1, 1, 21)
    pairs = []
    for rep in range(6):
        for d in list(range(-4, 5)) + [None]:
            len1, len2 = (300, 300) if d is None else (4 * width_words - 60 + d, 60)
            m1, m2 = hand_pair(lib, rng.randrange(len(lib)), True, rng, len1, len2)
            set_umi(m1, m2, TWO, UC.rand_seq(rng, 16))
            if rng.random() < 0.2:
                m2[1][TWO[1][0] + rng.randrange(10)] = ord("#")
            if len(pairs) % 3 == 1:
                del m2[1][len(m2[1]) - 1:]
            pairs.append((m1, m2))
    return lib, fastqs(pairs)


@functools.lru_cache(maxsize=None)
def many(n_pairs=6000, seed=0x6A0):
    """several thousand distinct (feature, UMI) pairs: the base shape with random UMIs in mate 2, a share of them repeated"""
    lib = PC.pair_library(200, LEN, 1, 1, 21)
    fq1, fq2 = PC.make_pairs(lib, LEN, list(ST1), list(ST2), True, n_pairs, seed=seed, len1=60, len2=60)
    rng = random.Random(seed + 1)
    pool = [UC.rand_seq(rng, 8) for _ in range(n_pairs)]
    fq1, fq2 = plant(fq1, fq2, (None, UMI2), pool, seed + 2)
    return lib, fq1, fq2
