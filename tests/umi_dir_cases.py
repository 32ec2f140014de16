"""tests/umi_dir_cases.py -- inputs and expected values shared by the --mur directional tests (CPU emulation and GPU).

The expectation is a literal restatement of what UMI-tools does per feature (network.py: _get_adj_list_directional,
_get_connected_components_adjacency), in plain Python on top of tests/umi_cases.py: the reads of every valid (feature,
UMI) pair exactly as umi_cases.expect finds them; the directed graph with an edge a -> b iff Hamming(a, b) == 1 and
reads(a) >= 2 * reads(b) - 1; the UMIs sorted by reads, descending, with a STABLE sort; a breadth-first search along the
edges from every UMI not yet reached; molecules = the searches started.  The order among equal counts is UMI-tools' own
business (the order of a dict), so every expectation is computed under three of them -- first seen, reversed, shuffled --
and must be the same number under each.  The closed form the device computes appears nowhere in this file."""
import collections
import functools
import random

import umi_cases as UC
import umi_collapse_cases as CC

RUN = dict(UC.RUN)
Q60 = b"I" * 60
FILLER = b"ACGTTGCA" * 5
TIE_ORDERS = ("first", "reversed", "shuffled")


def pair_reads(lib, fq, umi, **run):
    """per feature {UMI: reads} of the valid pairs, in first-seen order; also (valid reads, invalid reads)"""
    v = UC._verdicts(tuple(lib), UC.run_key(run))
    seen = [collections.OrderedDict() for _ in lib]
    ok = bad = 0
    for seq, qual in UC.records(fq):
        f = v.of(seq, qual)[0]
        if f >= 0:
            u = UC.umi_of(seq, qual, umi[0], umi[1], run.get("phred", 30))
            if u is None:
                bad += 1
            else:
                ok += 1
                seen[f][u] = seen[f].get(u, 0) + 1
    return seen, ok, bad


def neighbours(u):
    for j in range(len(u)):
        for c in b"ACGT":
            if c != u[j]:
                yield u[:j] + bytes([c]) + u[j + 1:]


def umitools_directional(counts, order):
    """the molecules of one feature: `counts` {UMI: reads}, `order` the UMIs as UMI-tools happens to hold them"""
    adj = {a: [b for b in neighbours(a) if b in counts and counts[a] >= 2 * counts[b] - 1] for a in order}
    found, starts = set(), 0
    for node in sorted(order, key=lambda u: counts[u], reverse=True):       # (stable: ties keep `order`)
        if node in found:
            continue
        starts += 1
        queue = collections.deque([node])
        found.add(node)
        while queue:
            for b in adj[queue.popleft()]:
                if b not in found:                                       # (everything an earlier search reached is closed
                    found.add(b)                                         # under the edges: walking it again finds nothing new)
                    queue.append(b)
    return starts


def ordered(umis, tie, seed=0):
    umis = list(umis)
    if tie == "reversed":
        umis.reverse()
    elif tie == "shuffled":
        random.Random(0xD1 + seed).shuffle(umis)
    return umis


def dominated(counts):
    """UMIs some neighbour with two reads or more absorbs directly"""
    return sum(1 for b, cb in counts.items() if any(counts.get(a, 0) >= 2 and counts[a] >= 2 * cb - 1 for a in neighbours(b)))


def expect(lib, fq, umi, **run):
    """(molecules per feature, pairs, edges, dominated, reads), the molecules the same under every tie order"""
    per, ok, _ = pair_reads(lib, fq, umi, **run)
    mol = None
    for tie in TIE_ORDERS:
        got = [umitools_directional(c, ordered(c, tie, f)) for f, c in enumerate(per)]
        assert mol is None or got == mol, tie
        mol = got
    edges = sum(CC.components(set(c))[1] for c in per)
    assert ok == sum(sum(c.values()) for c in per)
    return mol, sum(len(c) for c in per), edges, sum(dominated(c) for c in per), ok


def pair_table(lib, fq, umi, **run):
    """[(feature, codes, reads)] sorted by (feature, codes): what f2q_umi_pairs returns"""
    per = pair_reads(lib, fq, umi, **run)[0]
    rows = [(f, sum(b"ACGT".index(ch) << (2 * j) for j, ch in enumerate(u)), n) for f, c in enumerate(per) for u, n in c.items()]
    return sorted(rows)


def reads_of(lib, pairs, start):
    """60-base reads: the feature's 20 bases and a fixed filler, the UMI at `start` (equal pairs give equal records)"""
    recs = []
    for f, u in pairs:
        s = lib[f].encode() + FILLER
        recs.append((s[:start] + u + s[start + len(u):], Q60))
    return recs


def _fastq(lib, counted, seed, start=20):
    pairs = [(f, u) for f, u, n in counted for _ in range(n)]
    random.Random(seed).shuffle(pairs)
    return UC.fastq_of(reads_of(lib, pairs, start))


N_SPREAD = 16                                                        # features 6 .. 21 of `known`


@functools.lru_cache(maxsize=None)
def known():
    """UMI 20,4, one feature per case: 0: 10/1/1 on the chain AAAA-AAAC-AACC; 1: 3/3 neighbours; 2: 2/2; 3: 2/1; 4: 3/2
    (3 >= 2*2 - 1: the boundary, 2/2 its other side); 5: a chain of three single reads; 6 .. 21: two single-read neighbours
    X - Y and a 5-read neighbour Z of Y alone, random UMIs (the dominated Y above or below X in the set)"""
    rng = random.Random(0xD101)
    lib = UC.library()
    counted = [(0, b"AAAA", 10), (0, b"AAAC", 1), (0, b"AACC", 1), (1, b"AAAA", 3), (1, b"AAAC", 3), (2, b"AAAA", 2), (2, b"AAAC", 2),
               (3, b"AAAA", 2), (3, b"AAAC", 1), (4, b"AAAA", 3), (4, b"AAAC", 2), (5, b"AAAA", 1), (5, b"AAAC", 1), (5, b"AACC", 1)]
    spread = []
    for f in range(6, 6 + N_SPREAD):
        x = UC.rand_seq(rng, 4)
        y = UC.mutate1(rng, x, 0, 2)
        z = UC.mutate1(rng, y, 2, 4)                                  # another base: two from X
        counted += [(f, x, 1), (f, y, 1), (f, z, 5)]
        spread.append((x, y, z))
    directional = [1, 2, 2, 1, 1, 1] + [1] * N_SPREAD
    cluster = [1] * (6 + N_SPREAD)
    umis = [3, 2, 2, 2, 2, 3] + [3] * N_SPREAD
    pad = [0] * (len(lib) - len(umis))
    return lib, _fastq(lib, counted, 0xD102), dict(RUN), (20, 4), (directional + pad, cluster + pad, umis + pad), tuple(spread)


@functools.lru_cache(maxsize=None)
def known1():
    """UMI 20,1: all four UMIs with reads 5/1/1/1 (feature 0: one molecule) and 2/2/2/2 (feature 1: four)"""
    lib = UC.library()
    counted = [(0, b"G", 5), (0, b"A", 1), (0, b"C", 1), (0, b"T", 1)] + [(1, bytes([c]), 2) for c in b"ACGT"]
    pad = [0] * (len(lib) - 2)
    return lib, _fastq(lib, counted, 0xD103), dict(RUN), (20, 1), ([1, 4] + pad, [1, 1] + pad, [4, 4] + pad)


TINY_WANT = ([1, 2], 5, 3, 1, 11)                                    # umi_collapse_cases.tiny: molecules, pairs, edges, dominated, reads
TINY_UMIS = [3, 2]

GRAY_N, GRAY_FEATURE = CC.GRAY_N, CC.GRAY_FEATURE
SKEW = (1, 1, 1, 1, 2, 2, 3, 5, 12)


@functools.lru_cache(maxsize=None)
def contention(twice):
    """UMI 20,8: feature 7 holds the first 20 000 codes of the reflected Gray code (umi_collapse_cases.gray; consecutive
    codes differ in one digit), each read once -- or, `twice`, every second code read twice: then each two-read code
    stands alone (a neighbour would need three reads) and absorbs its single-read neighbours, exactly 10 000 molecules.
    Around it umi_collapse_cases.contention's random part -- 600 features x 6 seed UMIs with chains of 0 .. 3 one-base
    mutations -- with 1 .. 12 reads per pair, skewed to few"""
    rng = random.Random(0xD104)
    lib = UC.library()
    counted = [(GRAY_FEATURE, CC.text_of(CC.gray(n), 8), 2 if twice and n % 2 == 0 else 1) for n in range(GRAY_N)]
    rest = {}
    for f in range(len(lib)):
        if f == GRAY_FEATURE:
            continue
        for _ in range(6):
            u = UC.rand_seq(rng, 8)
            rest[(f, u)] = rng.choice(SKEW)
            for _ in range(rng.choice((0, 0, 0, 1, 2, 3))):
                u = UC.mutate1(rng, u)
                rest[(f, u)] = rng.choice(SKEW)
    counted += [(f, u, n) for (f, u), n in rest.items()]
    return lib, _fastq(lib, counted, 0xD105), dict(RUN), (20, 8)


def shape(name):
    """(lib, fq, run, umi) of 'known', 'known1', 'ones', 'twice' (the two contention inputs), 'wide' (umi_cases.wide with
    --m 1 and every third record read three more times: sixteen-base UMIs with skewed reads), 'tiny' (umi_collapse_cases.tiny:
    5/1/1 on a chain -- one molecule by either rule -- and 2/2 neighbours -- one by the cluster rule, two by this one)"""
    if name == "wide":
        lib, fq, run, umi = UC.wide()
        recs = UC.records(fq)
        return lib, UC.fastq_of(recs + [r for i, r in enumerate(recs) if i % 3 == 0] * 3), dict(run, miss=1), umi
    return {"known": known, "known1": known1, "ones": lambda: contention(False), "twice": lambda: contention(True), "tiny": CC.tiny}[name]()[:4]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(molecules, pairs, edges, dominated, reads) of a shape, computed once"""
    lib, fq, run, umi = shape(name)
    return expect(lib, fq, umi, **run)


@functools.lru_cache(maxsize=None)
def expected_cluster(name):
    """(molecules, pairs, edges) by the cluster rule (umi_collapse_cases.expect) and the distinct UMIs per feature"""
    lib, fq, run, umi = shape(name)
    return CC.expect(lib, fq, umi, **run), [len(s) for s in CC.umi_sets(lib, fq, umi, **run)]


@functools.lru_cache(maxsize=None)
def expected_pairs(name):
    lib, fq, run, umi = shape(name)
    return pair_table(lib, fq, umi, **run)


def separates(name):
    """the shape tells the three answers apart: some feature with directional != cluster, some with directional != umis,
    and cluster <= directional <= umis everywhere"""
    mol = expected(name)[0]
    (cl, _, _), umis = expected_cluster(name)
    assert all(a <= b <= c for a, b, c in zip(cl, mol, umis))
    return any(a != b for a, b in zip(cl, mol)) and any(b != c for b, c in zip(mol, umis))
