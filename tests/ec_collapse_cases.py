"""Extract+Count keys one base apart collapsed (f2q_ec_collapse): the rule in plain Python -- the specification of
include/f2q.h restated, the only reference there is -- and the shapes the CPU and GPU tests share.  A shape is
(run, table, ratio): Counter keyword arguments, the key -> reads table its FASTQ gives, the ratio to collapse at."""
import functools
import random

UP, DOWN = "GTTGAAGAGC", "TAGCAAGTCA"


# ---- the rule ---------------------------------------------------------------------------------------------------
def eligible(key):
    return 1 <= len(key) <= 29 and set(key) <= set("ACGT")


def parents(table, ratio):
    parent = {}
    for b, nb in table.items():
        if not eligible(b):
            continue
        best = None
        for j in range(len(b)):
            for x in "ACGT":
                if x == b[j]:
                    continue
                a = b[:j] + x + b[j + 1:]
                if a in table and table[a] >= ratio * nb and (best is None or table[a] > table[best]):
                    best = a
        if best is not None:
            parent[b] = best
    return parent


def ec_collapse(table, ratio, dist=1):
    """{key: (centroid, cluster_reads)} and the four counters (eligible, absorbed, absorbed reads, longest chain)"""
    parent = parents(table, ratio) if dist else {}
    cent, longest = {}, 0
    for k in table:
        c, depth = k, 0
        while c in parent:
            c, depth = parent[c], depth + 1
        cent[k], longest = c, max(longest, depth)
    cluster = dict.fromkeys(table, 0)
    for k, n in table.items():
        cluster[cent[k]] += n
    extra = dict(eligible_keys=sum(eligible(k) for k in table) if dist else 0, absorbed_keys=len(parent),
                 absorbed_reads=sum(table[k] for k in parent), longest_chain=longest)
    return {k: (cent[k], cluster[k]) for k in table}, extra


def check(rows, extra, table, ratio, dist=1, want=None):
    """rows of Counter.ec_collapsed() and the dict of Counter.ec_collapse() against the rule, key for key (want: the rule's
    answer when the caller has it already)"""
    want, want_extra = want or ec_collapse(table, ratio, dist)
    assert {r[0]: r[1] for r in rows} == table and len(rows) == len(table)
    assert {r[0]: (r[3], r[4]) for r in rows} == want
    assert extra == want_extra
    return want, want_extra


# ---- tables and their FASTQ --------------------------------------------------------------------------------------
def rand_key(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def sub(key, j, x):
    assert key[j] != x
    return key[:j] + x + key[j + 1:]


def rand_sub(rng, key):
    j = rng.randrange(len(key))
    return sub(key, j, rng.choice([x for x in "ACGT" if x != key[j]]))


def planted(seed, length, n_true=5, n_err=14, top=(120, 400), junk=20):
    """a few abundant keys, their one-base errors at 1 .. 3 reads, errors of errors, a few neighbours near top / 5 and
    top / 2 (either side of common ratios), unrelated single reads"""
    rng = random.Random(seed)
    table = {}
    for _ in range(n_true):
        t = rand_key(rng, length)
        table[t] = rng.randint(*top)
        errs = []
        for _ in range(n_err):
            e = rand_sub(rng, t)
            table.setdefault(e, rng.randint(1, 3))
            errs.append(e)
        for e in errs[:4]:
            table.setdefault(rand_sub(rng, e), 1)
        for d in (5, 2):
            table.setdefault(rand_sub(rng, t), max(1, table[t] // d + rng.choice((-1, 0, 1))))
    for _ in range(junk):
        table.setdefault(rand_key(rng, length), 1)
    return table


def fastq_of_table(table, seed=1, up="", down="", tail=""):
    """every key as often as its reads say, shuffled; a read is up + key + down + tail, all at Phred 40"""
    rng = random.Random(seed)
    reads = [k for k, n in table.items() for _ in range(n)]
    rng.shuffle(reads)
    out = []
    for i, k in enumerate(reads):
        s = up + k + down + tail
        out.append("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    return "".join(out).encode()


def fixed(length):
    return dict(start="0", length=length, phred=30)


ANCHORED = dict(upstream=UP, downstream=DOWN, phred=30, length=20)


def chain(rng, length, depth, prefix):
    """k0 (2 ** depth reads), k1, ... k_depth (1 read): k_i is k_(i-1) with position i changed, so only neighbours in the chain
    are one base apart.  `prefix` keeps the families of one table apart"""
    k = prefix + rand_key(rng, length - len(prefix))
    out = {k: 2 ** depth}
    for i in range(1, depth + 1):
        j = len(prefix) + i
        k = sub(k, j, "ACGT"[("ACGT".index(k[j]) + 1) % 4])
        out[k] = 2 ** (depth - i)
    return out


@functools.lru_cache(maxsize=None)
def shapes():
    """name -> (run, table, ratio, fastq)"""
    rng = random.Random(77)
    S = {}

    def add(name, run, table, ratio, **fq):
        assert all(n >= 1 for n in table.values())
        S[name] = (run, table, ratio, fastq_of_table(table, seed=len(S) + 1, **fq))

    # lengths: 3 neighbours (21 groups), 3L = 63 (one full group), 66 (the first two-trip length), 87 (the maximum)
    add("len1", fixed(1), {"A": 50, "C": 5, "G": 10, "T": 1}, 5)
    for length in (21, 22, 29):
        add("len%d" % length, fixed(length), planted(1000 + length, length), 5)
        add("len%d_r2" % length, fixed(length), planted(2000 + length, length, n_true=3), 2)
    # ACG and ACGA share their codes (A = 0): only the length field tells them apart
    add("lengths_share_codes", ANCHORED, {"ACG": 100, "ACGA": 3, "ACT": 5, "ACGC": 30, "ACGT": 1, "AAG": 100, "AAGA": 1}, 5,
        up=UP, down=DOWN, tail="TT")
    # boundaries at R = 2 and R = 255: equal absorbs, one short does not
    for ratio in (2, 255):
        x, y = "AC" + rand_key(rng, 10), "GT" + rand_key(rng, 10)
        add("boundary_r%d" % ratio, fixed(12), {x: 3 * ratio, rand_sub(rng, x): 3, y: 2 * ratio - 1, rand_sub(rng, y): 2}, ratio)
    # ties: the earlier position wins; at one position the smaller base wins
    add("ties", fixed(8), {"AAAAAAAA": 1, "AAAAAAAC": 10, "CAAAAAAA": 10, "AAAATAAA": 10,
                           "GGGGGGGG": 1, "GGGTGGGG": 10, "GGGCGGGG": 10, "GGGAGGGG": 9}, 5)
    # chains of depth 1, 2 and 6 at R = 2
    t = {}
    for depth, prefix in ((1, "AA"), (2, "CC"), (6, "GG")):
        t.update(chain(rng, 16, depth, prefix))
    add("chains", fixed(16), t, 2)
    # a key with an 'N' and many reads next to its plain neighbour with few: neither joins; a plain family beside them
    t = {"ACGTNCGT": 50, "ACGTACGT": 2, "ACGTCCGT": 1, "TTGTACGA": 40, "TTGTACGC": 2, "NTGTACGA": 1}
    add("n_keys", fixed(8), t, 2)
    # a 30-base window: everything is in the byte-string table
    add("len30", fixed(30), planted(3030, 30, n_true=2), 5)
    # the counting roads of a fixed window (hot keys in LDS / the ordinary insert / the byte-exact routine)
    add("roads", fixed(20), planted(4040, 20, n_true=8, n_err=30, top=(300, 900), junk=60), 5)
    return S


@functools.lru_cache(maxsize=None)
def growth():
    """two blocks of 52 000 reads of 12 bases, nearly every window distinct: the first table is the smallest there is
    (131 072 slots, room for 98 304 keys: what F2Q_TRACE=1 shows) and the second call passes its room.  A few abundant keys with their errors are spread over both blocks.  -> (run, blocks, tables
    after each block, the rule's answers for them at ratio 5)"""
    rng = random.Random(909)
    plant = planted(5050, 12, n_true=6, n_err=20, top=(200, 500), junk=0)
    reads = [k for k, n in plant.items() for _ in range(n)]
    reads += [rand_key(rng, 12) for _ in range(104000 - len(reads))]
    rng.shuffle(reads)
    blocks, tables, table = [], [], {}
    for part in (reads[:52000], reads[52000:]):
        for k in part:
            table[k] = table.get(k, 0) + 1
        blocks.append("".join("@r\n%s\n+\nIIIIIIIIIIII\n" % k for k in part).encode())
        tables.append(dict(table))
    return fixed(12), blocks, tables, [ec_collapse(t, 5) for t in tables]


def random_table(seed):
    """the CPU invariants' tables: a few hundred keys, plain ones of mixed lengths, some with 'N', some too long"""
    rng = random.Random(seed)
    table = {}
    for length in rng.sample(range(6, 30), 3) + [rng.randint(1, 5)]:
        table.update(planted(rng.randrange(1 << 30), length, n_true=rng.randint(2, 4), n_err=rng.randint(10, 30),
                             top=(rng.randint(5, 50), rng.randint(50, 3000)), junk=10))
    for _ in range(8):
        k = rng.choice(list(table))
        if len(k) >= 2:
            j = rng.randrange(len(k))
            table.setdefault(k[:j] + "N" + k[j + 1:], rng.randint(1, 2000))
    for _ in range(5):
        k = rand_key(rng, rng.randint(30, 40))
        table[k] = rng.randint(1, 500)
        table.setdefault(rand_sub(rng, k), 1)
    table.setdefault("", 7)
    table.setdefault("ACGT:ACGT", 3)
    return table
