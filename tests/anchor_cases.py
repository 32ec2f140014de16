"""tests/anchor_cases.py -- inputs and expected values shared by the tests of the anchored (--us/--ds) Counter kernels
(CPU preconditions and GPU).  Pure Python, seeded `random`, no GPU.

A read is prefix + UP + window + DOWN + tail (two cassettes for the two-pair runs), upper-case ACGT plus 'N' where the
kind says so, quality 'I' except for the one byte the Phred kinds lower.  The yardstick is the oracle over the same
FASTQ bytes; which kernel must count a block (`expected_path`) and how many of its reads must leave the packed tiles
(`general_reads`) are derived from the run and the input alone, never from a run of the code under test."""
import functools
import random

from oracle import oracle as O

UP, DOWN = "GTTTAAGAGCTA", "CGTTACCAGGTT"
UP2, DOWN2 = "ACCTGGATCCAA", "TTCAGGCATGCA"
PHRED = 30
LOWQ = chr(PHRED + 31)                 # '=': the highest byte --ph 30 fails, one below the first that passes (fast2q.py:1112-1129)
TILE = 256
N17 = 17 * TILE
HIST_MAX = 24576                       # F2Q_HIST_MAX: the largest library with a per-workgroup histogram in LDS
PATH_ANCHOR, PATH_ANCHOR_LDS, PATH_PAIRS, PATH_EXTRACT = 6, 7, 8, 9      # include/f2q.h

# the kinds of one cycle of reads; the frequent ones several times so that every statistic stays well away from zero
KINDS = ("exact",) * 6 + ("sub1",) * 3 + (
    "sub2",                            # two substitutions: no match at --m 1
    "n1", "n2", "sub1_n1", "sub1_n2",  # 'N' in the window, one and two, on exact and on one-substitution windows
    "n_up", "n_down",                  # 'N' inside an anchor
    "win19", "win21",                  # a window of another length than the features between both anchors
    "end_in_win", "end_in_down",       # the read ends inside the window / inside the downstream anchor
    "q_win_first", "q_win_last", "q_up", "q_down",       # one quality byte one below the threshold
    "q_past_down",                     # ... one base past the downstream anchor: must not fail
    "no_up",                           # no upstream anchor and a window cut at the read start (down-only: a negative start)
    "up_mm1", "down_mm1", "up_mm2", "down_mm2")          # an anchor with 1 and with 2 mismatches
N_KINDS = ("n1", "n2", "sub1_n1", "sub1_n2", "n_up", "n_down")

LIB_SEED, PAIR_SEEDS = 0xA7C4, (0xA7C5, 0xA7C6)                # synth.make_library(n, 20, seed) == binding.synth_library(seed, n, 20)

# (miss, --msu = --msd, anchors, longest read) of the runs that must take the library-in-LDS kernel: its 12 instances
# <NW 5|3, KB 0|1|3, NEAR> with each anchor form
MATRIX7 = [(miss, ms, anchors, max_len) for max_len in (150, 96) for miss in (0, 1) for ms in (0, 1, 2) for anchors in ("both", "up", "down")]
# (variant, miss, --msu = --msd, anchors, longest read, extra parameters) of the runs that must take k_count_anchor: every
# (NW, KB) once per variant, the anchor forms in turn; SAMEQ = false is the qual_up variant
MATRIX6 = [(variant, 2 if variant == "miss2" else (ms + 1) % 2 if variant == "no_lt" else 1, ms, ("both", "up", "down")[(ms + (max_len == 96)) % 3], max_len,
            {"qual_up": 20} if variant == "qual_up" else {})
           for variant in ("no_lt", "qual_up", "miss2") for max_len in (150, 96) for ms in (0, 1, 2)]


def fastq_of(recs):
    return "".join(f"@r{i}\n{s}\n+\n{q}\n" for i, (s, q) in enumerate(recs)).encode()


def feats(lib):
    return [(str(i), s) for i, s in enumerate(lib)]


def rand_seq(rng, n):
    v = rng.getrandbits(2 * n) if n else 0
    return "".join("ACGT"[(v >> (2 * j)) & 3] for j in range(n))


def sub(rng, s, k=1):
    """s with k distinct positions changed to another base"""
    b = list(s)
    for p in rng.sample(range(len(b)), k):
        b[p] = rng.choice([c for c in "ACGT" if c != b[p]])
    return "".join(b)


def put_n(rng, s, k=1):
    b = list(s)
    for p in rng.sample(range(len(b)), k):
        b[p] = "N"
    return "".join(b)


def make_read(rng, kind, cassettes, which, max_len, prefix_max, tail_max, prefix=None, tail=None):
    """(sequence, quality) of one read: cassettes = [(up, window, down), ...], the kind is applied to cassette `which`;
    never longer than max_len (the caller keeps prefix_max + the cassettes below it)"""
    seq = rand_seq(rng, rng.randrange(prefix_max + 1) if prefix is None else prefix)
    low = cut = None
    for k, (u, w, d) in enumerate(cassettes):
        if k == which:
            if kind == "sub1": w = sub(rng, w)
            elif kind == "sub2": w = sub(rng, w, 2)
            elif kind == "n1": w = put_n(rng, w)
            elif kind == "n2": w = put_n(rng, w, 2)
            elif kind == "sub1_n1": w = put_n(rng, sub(rng, w))
            elif kind == "sub1_n2": w = put_n(rng, sub(rng, w), 2)
            elif kind == "n_up": u = put_n(rng, u)
            elif kind == "n_down": d = put_n(rng, d)
            elif kind == "win19": w = w[:-1]
            elif kind == "win21": w = w + rng.choice("ACGT")
            elif kind == "up_mm1": u = sub(rng, u)
            elif kind == "down_mm1": d = sub(rng, d)
            elif kind == "up_mm2": u = sub(rng, u, 2)
            elif kind == "down_mm2": d = sub(rng, d, 2)
            elif kind == "no_up" and k == 0: seq, u, w = "", "", w[rng.randrange(1, len(w)):]
            # Extract+Count kinds (tests/ec_cases.py): the window's own length, 'N's at stated places, case, an odd symbol
            elif kind.startswith("len:"): w = (w * 4)[:int(kind[4:])]                       # len:L -- a window of L bases
            elif kind.startswith("nn:"):                                                     # nn:L:K:first|last -- L bases, K 'N's, one of
                _, L, K, where = kind.split(":")                                             # them at the first / last position
                L, K = int(L), int(K)
                b = list((w * 2)[:L])
                for p in ([0] if where == "first" else [L - 1]) + [3 + 4 * j for j in range(K - 1)]:
                    b[p] = "N"
                w = "".join(b)
                assert w.count("N") == K
            elif kind == "lower": w = w.lower()
            elif kind == "odd": w = w[:7] + "R" + w[8:]
            a = len(seq)
            if kind == "q_win_first": low = a + len(u)
            elif kind == "q_win_last": low = a + len(u) + len(w) - 1
            elif kind == "q_up": low = a + rng.randrange(len(u))
            elif kind == "q_down": low = a + len(u) + len(w) + rng.randrange(len(d))
            elif kind == "q_past_down": low = a + len(u) + len(w) + len(d)
            elif kind == "end_in_win": cut = a + len(u) + rng.randrange(1, len(w))
            elif kind == "end_in_down": cut = a + len(u) + len(w) + rng.randrange(1, len(d))
        seq += u + w + d
        if k + 1 < len(cassettes):
            seq += rand_seq(rng, rng.randrange(6))
    room = max_len - len(seq)
    assert room >= 1
    t = rng.randrange(min(tail_max, room) + 1) if tail is None else tail
    if low is not None and low >= len(seq):
        t = max(t, 1)                                            # (q_past_down needs a base there)
    seq += rand_seq(rng, t)
    if cut is not None:
        seq = seq[:cut]
    q = ["I"] * len(seq)
    if low is not None:
        q[low] = LOWQ
    assert len(seq) <= max_len
    return seq, "".join(q)


class Case:
    """a library and a block of reads; identity-hashed, so the cached builders' objects key the cached expectations"""

    def __init__(self, lib, recs, kinds, max_len):
        self.lib, self.recs, self.kinds, self.max_len = list(lib), recs, kinds, max_len
        self.n = len(recs)
        self.fq = fastq_of(recs)
        self.pairs = ":" in self.lib[0]


@functools.lru_cache(maxsize=None)
def block(lib, n=N17, max_len=150, seed=1):
    """the mixed block: n reads of at most max_len bases (150: five plane words, 96: three), the kinds of KINDS in turn.
    `lib` is a tuple of features, plain ones (one cassette per read) or A:B (two cassettes, the kind applied to one of
    them).  Every second wave of 64 reads holds no 'N' (the kernels take another branch for a wave without flag bits).
    Read 0 is an exact read of exactly max_len bases; every 16th read is on the last feature of the library."""
    rng = random.Random(seed)
    pairs = ":" in lib[0]
    body = (len(UP) + len(DOWN)) * (2 if pairs else 1) + len(lib[0]) + (4 if pairs else 0) + 1      # cassettes, spacer, a 21st base
    prefix_max = min(60, max_len - body - 1) if max_len > 96 else max_len - body - 22
    assert prefix_max >= 0
    recs, kinds = [], []
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        if kind in N_KINDS and (i // 64) % 2:
            kind = "exact"
        f = len(lib) - 1 if i % 16 == 5 else rng.randrange(len(lib))
        if pairs:
            a, b = lib[f].split(":")
            cas, which = [(UP, a, DOWN), (UP2, b, DOWN2)], (0 if kind == "no_up" else 1 if kind == "q_past_down" else rng.randrange(2))
        else:
            cas, which = [(UP, lib[f], DOWN)], 0
        if i == 0:
            kind = "exact"
            s, _ = make_read(rng, kind, cas, which, max_len, 0, 0, prefix=prefix_max, tail=0)
            s += rand_seq(rng, max_len - len(s))
            q = "I" * len(s)
        else:
            s, q = make_read(rng, kind, cas, which, max_len, prefix_max, 46)
        recs.append((s, q)); kinds.append(kind)
    return Case(lib, recs, kinds, max_len)


def tile_blocks(lib):
    """1, 2, 4 and 17 tiles' worth of reads, each plus 37 so that the last tile is partial"""
    return [block(lib, n=t * TILE + 37, max_len=150, seed=20 + t) for t in (1, 2, 4, 17)]


@functools.lru_cache(maxsize=None)
def skewed(lib, hot=7, seed=5):
    """80 000 reads for ONE workgroup of the library-in-LDS kernel: 70 000 on one feature, every third of them with one
    substitution, 10 000 spread over the library; shuffled.  Flanks from a small pool (no 'N', five plane words)."""
    rng = random.Random(seed)
    pre, post = [rand_seq(rng, rng.randrange(40, 71)) for _ in range(64)], [rand_seq(rng, rng.randrange(11)) for _ in range(64)]
    g = lib[hot]
    wins = [(g if i % 3 else sub(rng, g)) for i in range(70000)] + [rng.choice(lib) for _ in range(10000)]
    rng.shuffle(wins)
    recs = []
    for w in wins:
        s = rng.choice(pre) + UP + w + DOWN + rng.choice(post)
        recs.append((s, "I" * len(s)))
    return Case(lib, recs, None, 150)


PAIR_HOT = ((6, 70000), (7, 40000), (-1, 40000))     # (feature, reads): 6 and 7 share a histogram word, the last has no partner half
PAIR_SPREAD = 10000


@functools.lru_cache(maxsize=None)
def skewed_pairs(lib, seed=9):
    """160 000 two-cassette reads for ONE workgroup of the pairs kernel against an A:B library with an odd number of
    features: 70 000 on feature 6 (every third with one substitution in one part), 40 000 on feature 7, 40 000 on the
    last feature, 10 000 spread; shuffled, no 'N'.  (120 000 reads cannot hold a counter above 2 x 0x8000 next to two
    above 0x8000: 65 537 + 2 x 32 769 > 120 000.)"""
    assert len(lib) % 2 == 1 and ":" in lib[0]
    rng = random.Random(seed)
    pre, mid, post = ([rand_seq(rng, rng.randrange(n)) for _ in range(64)] for n in (25, 6, 20))
    keys = []
    for f, n in PAIR_HOT:
        a, b = lib[f].split(":")
        for i in range(n):
            if f == 6 and i % 3 == 0:
                keys.append((sub(rng, a), b) if i % 2 else (a, sub(rng, b)))
            else:
                keys.append((a, b))
    keys += [tuple(rng.choice(lib).split(":")) for _ in range(PAIR_SPREAD)]
    rng.shuffle(keys)
    recs = []
    for a, b in keys:
        s = rng.choice(pre) + UP + a + DOWN + rng.choice(mid) + UP2 + b + DOWN2 + rng.choice(post)
        recs.append((s, "I" * len(s)))
    return Case(lib, recs, None, 150)


def pair_library(parts_a, parts_b):
    return tuple(f"{a}:{b}" for a, b in zip(parts_a, parts_b))


def run_kw(anchors="both", miss=1, ms=0, pairs=False, **extra):
    """the run's parameters as binding.Counter and oracle.Oracle take them"""
    kw = dict(miss=miss, phred=PHRED, length=20, miss_search_up=ms, miss_search_down=ms)
    if pairs:
        kw["upstream"], kw["downstream"] = f"{UP},{UP2}", f"{DOWN},{DOWN2}"
    else:
        if anchors in ("both", "up"):
            kw["upstream"] = UP
        if anchors in ("both", "down"):
            kw["downstream"] = DOWN
    kw.update(extra)
    return kw


def expected_path(case, run, no_lt=False):
    """the kernel family choose_path must pick for the packed tiles of a Counter-mode block of this case"""
    if case.pairs:
        return PATH_PAIRS
    longest = max(len(s) for s, _ in case.recs)
    lds = (run["miss"] <= 1 and not no_lt and len(case.lib) <= HIST_MAX and len({len(f) for f in case.lib}) == 1 and
           14 <= len(case.lib[0]) <= 21 and run.get("qual_up", 30) == run.get("qual_down", 30) == run["phred"] and longest <= 160)
    return PATH_ANCHOR_LDS if lds else PATH_ANCHOR


def general_reads(case, run, pair_tables=True):
    """reads of the block that must leave the packed tiles, by the packer's rules for anchored runs (read_is_clean):
    a quality line of another length than the sequence, more than 320 bases, a quality byte >= 128, lower-case bases
    next to another non-ACGT symbol; non-ACGT symbols travel in band against a plain ACGT library, and 'N' alone against
    a pure A:B library on the pair tables (two pairs, --m <= 1) -- against ':' features on the string index not at all"""
    in_band = "any" if not case.pairs else ("N" if pair_tables and run["miss"] <= 1 else "")
    n = 0
    for s, q in case.recs:
        odd = set(s) - set("ACGTacgt")
        lower = bool(set(s) & set("acgt"))
        bad = len(s) != len(q) or len(s) > 320 or any(ord(c) >= 128 for c in q) or (lower and odd)
        bad = bad or (odd and (in_band == "" or (in_band == "N" and odd != {"N"})))
        n += bool(bad)
    return n


def run_key(run):
    return tuple(sorted((k, str(v)) for k, v in run.items()))


@functools.lru_cache(maxsize=None)
def _oracle(cases, rk, threads):
    run = {k: (v if k in ("upstream", "downstream") else int(v)) for k, v in rk}
    o = O.count_fastq_parallel(b"".join(c.fq for c in cases), threads, features=feats(cases[0].lib), **run)
    return o.counts(), o.stats()


def expect(cases, **run):
    """(counts, stats) of the oracle over the blocks of one case or of several (of one library), concatenated"""
    cases = cases if isinstance(cases, tuple) else (cases,)
    return _oracle(cases, run_key(run), 4 if sum(c.n for c in cases) > 20000 else 1)


def verdict_of(case, i, **run):
    """the oracle's five statistics for read i of the block alone"""
    o = O.Oracle(features=feats(case.lib), **run)
    o.count_fastq(fastq_of([case.recs[i]]))
    st = o.stats()
    o.close()
    return st
