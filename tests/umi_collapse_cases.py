"""tests/umi_collapse_cases.py -- inputs and expected values shared by the --mu 1 tests (CPU emulation and GPU).

The expectation is plain Python on top of tests/umi_cases.py: the set of valid UMIs per feature exactly as
umi_cases.expect builds it (the oracle's verdict per read, the UMI rule), then per feature a dictionary union-find over
the 3L neighbours at Hamming distance 1 of every UMI: molecules = connected components, edges = joined unordered pairs."""
import functools
import random

import umi_cases as UC

RUN = dict(UC.RUN)
Q60 = b"I" * 60


def umi_sets(lib, fq, umi, **run):
    """the valid UMIs per feature (umi_cases.expect's `seen`)"""
    v = UC._verdicts(tuple(lib), UC.run_key(run))
    seen = [set() for _ in lib]
    for seq, qual in UC.records(fq):
        f = v.of(seq, qual)[0]
        if f >= 0:
            u = UC.umi_of(seq, qual, umi[0], umi[1], run.get("phred", 30))
            if u is not None:
                seen[f].add(u)
    return seen


def components(umis):
    """(connected components, edges) of one feature's UMIs joined at Hamming distance 1"""
    parent = {u: u for u in umis}

    def find(u):
        while parent[u] != u:
            parent[u] = parent[parent[u]]
            u = parent[u]
        return u
    edges = 0
    for u in umis:
        for j in range(len(u)):
            for c in b"ACGT":
                if c > u[j]:                                         # each unordered pair once
                    w = u[:j] + bytes([c]) + u[j + 1:]
                    if w in parent:
                        edges += 1
                        a, b = find(u), find(w)
                        if a != b:
                            parent[a] = b
    return sum(1 for u in umis if find(u) == u), edges


def expect(lib, fq, umi, **run):
    """(molecules per feature, pairs, edges)"""
    sets = umi_sets(lib, fq, umi, **run)
    per = [components(s) for s in sets]
    return [m for m, _ in per], sum(len(s) for s in sets), sum(e for _, e in per)


def text_of(code, length):
    return bytes(b"ACGT"[(code >> (2 * j)) & 3] for j in range(length))


def reads_of(lib, pairs, start, rng):
    """60-base reads: the feature's 20 bases, filler, the UMI at `start`, filler"""
    recs = []
    for f, u in pairs:
        s = lib[f].encode() + UC.rand_seq(rng, 40)
        recs.append((s[:start] + u + s[start + len(u):], Q60))
    return recs


@functools.lru_cache(maxsize=None)
def known():
    """shape 1, UMI 20,4: feature 0 all 256 UMIs; feature 1 AAAA, AAAC, GGGG; features 2 and 3 ACGT, feature 2 also ACGA"""
    rng = random.Random(0xC011)
    lib = UC.library()
    pairs = [(0, text_of(c, 4)) for c in range(256)] + [(1, b"AAAA"), (1, b"AAAC"), (1, b"GGGG"), (1, b"AAAA")]
    pairs += [(2, b"ACGT"), (2, b"ACGA"), (3, b"ACGT"), (3, b"ACGT")]
    rng.shuffle(pairs)
    want = [1, 2, 1, 1] + [0] * (len(lib) - 4)
    return lib, UC.fastq_of(reads_of(lib, pairs, 20, rng)), dict(RUN), (20, 4), (want, 262, 1538)


@functools.lru_cache(maxsize=None)
def short(length):
    """shape 2, UMI 20,1 / 20,2: 80 features with 1 .. `4 ** length` random UMIs each"""
    rng = random.Random(0xC012 + length)
    lib = UC.library()
    pairs = []
    for f in range(0, 160, 2):
        pairs += [(f, text_of(rng.randrange(4 ** length), length)) for _ in range(1 + rng.randrange(6))]
    rng.shuffle(pairs)
    return lib, UC.fastq_of(reads_of(lib, pairs, 20, rng)), dict(RUN), (20, length)


TINY_RECORDS = 11
TINY_WANT = ([1, 1], 5, 3)                                           # molecules, pairs, edges


@functools.lru_cache(maxsize=None)
def tiny():
    """UMI 20,4, two features, eleven records: feature 0 AAAA x 5 - AAAC x 1 - AACC x 1 (a chain), feature 1 AAAA x 2 - AAAC
    x 2.  From a first set of 2 slots one block of them gives a set of 32 slots (the host's rule: the smallest power of two
    >= 2 x 11 records): less than one wave of the linking kernels, a quarter of a 256-thread workgroup of the others.
    The reads per pair are chosen for tests/umi_dir_cases.py: the directional rule keeps the two UMIs of feature 1 apart"""
    rng = random.Random(0xC015)
    lib = UC.library()[:2]
    pairs = [(0, b"AAAA")] * 5 + [(0, b"AAAC"), (0, b"AACC")] + [(1, b"AAAA"), (1, b"AAAC")] * 2
    assert len(pairs) == TINY_RECORDS
    rng.shuffle(pairs)
    return lib, UC.fastq_of(reads_of(lib, pairs, 20, rng)), dict(RUN), (20, 4), TINY_WANT


def gray(n, digits=8):
    """code n of the base-4 reflected Gray code, digit i in bits 2i .. 2i+1"""
    code = 0
    for i in range(digits):
        d = (n // 4 ** i) % 4
        if (n // 4 ** (i + 1)) % 2:
            d = 3 - d
        code |= d << (2 * i)
    return code


GRAY_N, GRAY_FEATURE = 20000, 7
CONTENTION_WANT = (1, 20000, 206896)                                 # feature 7 alone: molecules, pairs, edges


@functools.lru_cache(maxsize=None)
def contention():
    """shape 4, UMI 20,8: feature 7 holds the first 20 000 codes of the reflected Gray code (consecutive codes differ in
    one digit: one tree, every union lands in it); 600 features x 6 random seed UMIs, each with a chain of 0 .. 3
    successive one-base mutations, about 10 000 reads"""
    rng = random.Random(0xC014)
    lib = UC.library()
    codes = [gray(n) for n in range(GRAY_N)]
    pairs = [(GRAY_FEATURE, text_of(c, 8)) for c in codes]
    for f in range(len(lib)):
        if f == GRAY_FEATURE:
            continue
        for _ in range(6):
            u = UC.rand_seq(rng, 8)
            pairs.append((f, u))
            for _ in range(rng.choice((0, 0, 0, 1, 2, 3))):       # (half the seeds stay alone: some features keep every UMI)
                u = UC.mutate1(rng, u)
                pairs.append((f, u))
    pairs += [pairs[rng.randrange(len(pairs))] for _ in range(2500)]            # repeated pairs
    rng.shuffle(pairs)
    return lib, UC.fastq_of(reads_of(lib, pairs, 20, rng)), dict(RUN), (20, 8), codes


def shape(name):
    """(lib, fq, run, umi) of 'known', 'short1', 'short2', 'wide' (with --m 1, as tests/test_umi_*.py run it), 'contention',
    'tiny'"""
    if name == "wide":
        lib, fq, run, umi = UC.wide()
        return lib, fq, dict(run, miss=1), umi
    return {"known": known, "short1": lambda: short(1), "short2": lambda: short(2), "contention": contention, "tiny": tiny}[name]()[:4]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the Python expectation of a shape, computed once"""
    lib, fq, run, umi = shape(name)
    return expect(lib, fq, umi, **run)


def pieces(fq, per):
    """the FASTQ cut into pieces of `per` records"""
    recs = fq.split(b"\n@r")
    recs = [recs[0] + b"\n"] + [b"@r" + r + b"\n" for r in recs[1:-1]] + [b"@r" + recs[-1]]
    return [b"".join(recs[i:i + per]) for i in range(0, len(recs), per)]
