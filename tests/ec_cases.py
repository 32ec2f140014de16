"""tests/ec_cases.py -- inputs and expected values shared by the tests of the Extract+Count (mode="EC") kernels (CPU
preconditions and GPU).  Pure Python, seeded `random`, no GPU.

The anchored reads come from anchor_cases.make_read (its kinds plus the Extract+Count kinds added there), the fixed-window
reads from fixed_cases.block.  The yardstick is the oracle over the same FASTQ bytes.  What must happen to a block is
derived from the run and the input alone, never from a run of the code under test: which reads leave the packed tiles
(`classify` restates the packer's rule), which reads the hot-key kernels insert in place, set aside for
k_ec_deferred_keys or for k_ec_deferred_slow (`classify` restates ec64_word's rule and takes the window from the
oracle's sequence_tinder), which launches follow (`stages`, the step names as f2q_lib.hip prints them under
F2Q_TRACE_SYNC=1), which template instances they are (`instances`), and how many keys make ec_reserve grow a table or
leave it full (`reserve_room`, `expect_of`: the arithmetic of ec_reserve and launch_block restated)."""
import ctypes as C
import functools
import random

import anchor_cases as AC
import fixed_cases as FC
import synth
from oracle import oracle as O

TILE = 256
N17 = 17 * TILE
LEARN = 1024                           # F2Q_HOT_LEARN of the designed blocks: 4 learning tiles, then 13 with the set
PATH_PAIRS, PATH_EXTRACT = AC.PATH_PAIRS, AC.PATH_EXTRACT
EC64_MAXLEN, EC64_MAXN = 29, 3                                   # f2q_device.h
HOT_CAP, HOT_CAND, HOT_MINCOUNT, HOT_MAXPROBE = 11264, 32768, 6, 96
WIN_SEED = 0xEC01

S_LEARN, S_BUILD, S_HOT = "k_extract_anchor_hot (learning)", "hot set: build", "k_extract_anchor_hot"
S_KEYS, S_SLOW, S_FIXED = "k_ec_deferred_keys", "k_ec_deferred_slow", "k_ec_deferred_fixed"
S_REHASH64, S_RELINK, S_REHASHB = "reserve: k_ec64_rehash", "reserve: k_ec_hot_relink", "reserve: k_ec_rehash"
STEPS = (S_LEARN, S_BUILD, S_HOT, S_KEYS, S_SLOW, S_FIXED, S_REHASH64, S_RELINK, S_REHASHB)
HOT_STEPS = (S_LEARN, S_BUILD, S_HOT, S_KEYS, S_SLOW, S_FIXED, S_RELINK)

# ---- the Extract+Count kinds of anchor_cases.make_read ------------------------------------------------------------------
LENS = (0, 1, 28, 29, 30, 31, 32, 33, 64, 65)                    # bases between both anchors: around the single-word limit and the plane words
N_EDGES = ((25, 1), (26, 1), (23, 2), (24, 2), (20, 3), (21, 3), (20, 4), (29, 1))      # (length, 'N's): each side of ec64_word's edges; 4 'N's; 29 + 'N'
STARTS = (31, 32, 33, 63, 64, 65)                                # read position of the window's first base: around the plane words' borders
EC_KINDS = (tuple(f"len:{L}" for L in LENS) + tuple(f"nn:{L}:{K}:{w}" for L, K in N_EDGES for w in ("first", "last")) +
            tuple(f"at:{p}" for p in STARTS) + ("lower", "odd"))
KINDS = AC.KINDS + EC_KINDS
N_KINDS = AC.N_KINDS + tuple(k for k in EC_KINDS if k.startswith("nn:"))


def ec64_fits(length, n_n):
    """ec64_word's rule: the key has a single-word form"""
    if length < 0 or length > EC64_MAXLEN:
        return False
    return n_n == 0 or (n_n <= EC64_MAXN and 2 * length + 2 + 5 * n_n <= 58)


@functools.lru_cache(maxsize=None)
def windows(n=24, length=20, seed=WIN_SEED):
    return tuple(synth.make_library(n, length, seed))


def _applies(kind, max_len):
    """at:P needs the window at P, the downstream anchor and one more base inside max_len"""
    return not kind.startswith("at:") or int(kind[3:]) + 20 + len(AC.DOWN) + 1 <= max_len


@functools.lru_cache(maxsize=None)
def block(max_len=150, n=N17, seed=1, kinds=KINDS):
    """the designed anchored block: n reads of at most max_len bases on 24 windows (half of the reads on the first four, so
    that keys reach F2Q_HOT_MINCOUNT inside the learning reads), the kinds of `kinds` in turn.  Every second wave of 64 reads
    holds no 'N'.  Read 0 is an exact read of exactly max_len bases."""
    rng = random.Random(seed * 7919 + max_len)
    lib = windows()
    body = len(AC.UP) + len(AC.DOWN) + 20 + 1
    prefix_max = min(60, max_len - body - 1) if max_len > 96 else max_len - body - 22
    recs, out_kinds = [], []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        if (kind in N_KINDS and (i // 64) % 2) or not _applies(kind, max_len):
            kind = "exact"
        w = lib[rng.randrange(4) if rng.random() < 0.5 else rng.randrange(len(lib))]
        cas = [(AC.UP, w, AC.DOWN)]
        if i == 0:
            kind = "exact"
            s, _ = AC.make_read(rng, kind, cas, 0, max_len, 0, 0, prefix=prefix_max, tail=0)
            s += AC.rand_seq(rng, max_len - len(s))
            q = "I" * len(s)
        elif kind.startswith("at:"):
            s, q = AC.make_read(rng, "exact", cas, 0, max_len, 0, 46, prefix=int(kind[3:]) - len(AC.UP))
        elif kind.startswith(("len:", "nn:")):
            L = int(kind.split(":")[1])
            s, q = AC.make_read(rng, kind, cas, 0, max_len, 0, 46, prefix=rng.randrange(min(prefix_max, max_len - 1 - (24 + L)) + 1))
        else:
            s, q = AC.make_read(rng, kind, cas, 0, max_len, prefix_max, 46)
        recs.append((s, q)); out_kinds.append(kind)
    return AC.Case(lib, recs, out_kinds, max_len)


def tile_blocks():
    """1, 2, 4 and 17 tiles' worth of reads, each plus 37 so that the last tile is partial; without the kind that leaves
    the tiles, so that every read takes a slot"""
    return [block(150, n=t * TILE + 37, seed=20 + t, kinds=tuple(k for k in KINDS if k != "odd")) for t in (1, 2, 4, 17)]


@functools.lru_cache(maxsize=None)
def pair_block(max_len=150):
    """anchor_cases.block on 24 A:B features: two cassettes per read, the kinds of anchor_cases.KINDS on one of them"""
    lib = AC.pair_library(synth.make_library(24, 20, AC.PAIR_SEEDS[0]), synth.make_library(24, 20, AC.PAIR_SEEDS[1]))
    return AC.block(lib, max_len=max_len)


def run_kw(anchors="both", ms=0, pairs=False, **extra):
    """the run's parameters as binding.Counter and oracle.Oracle take them"""
    kw = AC.run_kw(anchors, 1, ms, pairs, **extra)
    kw["mode"] = "EC"
    return kw


# ---- fixed windows ------------------------------------------------------------------------------------------------------
FIXED_ROWS = [(0, 20, 30), (16, 20, 30), (3, 17, 30), (5, 29, 30), (2, 12, 30), (0, 20, 1)]      # (st, L, --ph)


@functools.lru_cache(maxsize=None)
def fixed_library(L):
    """fixed_cases' constellations on the smallest library that holds them: few plain guides, so their windows repeat"""
    return FC.library(L, n=330 if L >= 16 else 600)


def fixed_block(st, L, phred=30, n=N17 + 37, seed=1):
    return FC.block(fixed_library(L), (st,), n=n, seed=seed, phred=phred)


FIXED_TILE_READS = (37, 256 + 37, 16 * 256 + 37, 17 * 256 + 37, 34 * 256 + 37)


def fixed_tile_blocks():
    """blocks whose packed reads fill fixed_cases.TILE_COUNTS tiles (1, 2, 16, 17, 33), the last one partly: about one read
    in 25 of fixed_cases.block has a quality line of another length and leaves the tiles"""
    return [FC.block(fixed_library(20), (0,), n=n, seed=20 + i) for i, n in enumerate(FIXED_TILE_READS)]


def fixed_run(case, phred=None):
    return dict(case.run(1, phred), mode="EC")


# ---- what must happen to a read -------------------------------------------------------------------------------------------
def _py_slice(n, a, b):
    a = max(a + n, 0) if a < 0 else min(a, n)
    b = max(b + n, 0) if b < 0 else min(b, n)
    return a, max(a, b)


def _spans(recs, run):
    """(start, end) of every read's window as the oracle's sequence_tinder finds it, None where it finds none"""
    kw = {k: v for k, v in run.items() if k in ("upstream", "downstream", "miss_search_up", "miss_search_down", "qual_up", "qual_down", "length")}
    o = O.Oracle(mode="EC", **kw)
    L, a, b = O.lib(), C.c_long(), C.c_long()
    out = []
    for s, q in recs:
        sb, qb = s.encode("latin-1"), q.encode("latin-1")
        ok = L.orc_sequence_tinder(o._h, sb, len(sb), qb, len(qb), 0, C.byref(a), C.byref(b))
        out.append((int(a.value), int(b.value)) if ok and b.value >= a.value else None)
    o.close()
    return out


def _fails(q, a, b, phred):
    qa, qb = _py_slice(len(q), a, b)
    return any(33 <= ord(c) <= min(phred + 31, 126) for c in q[qa:qb])


@functools.lru_cache(maxsize=None)
def _classify(case, rk):
    run = dict(rk)
    fixed = "upstream" not in run and "downstream" not in run
    phred = int(run["phred"])
    out = []
    if fixed:
        st, L = int(run["start"]), int(run["length"])
        for s, q in case.recs:
            a, b = _py_slice(len(s), st, st + L)
            w = s[a:b].upper()
            odd = [c for c in w if c not in "ACGT"]
            stays = (len(s) == len(q) and not any(ord(c) >= 128 for c in q[a:b]) and all(c == "N" for c in odd) and
                     (not odd or ec64_fits(b - a, len(odd))))
            out.append("raw" if not stays else "fail" if _fails(q, st, st + L, phred) else "inplace")
        return tuple(out)
    run = {k: (v if k in ("upstream", "downstream", "mode") else int(v)) for k, v in run.items()}
    for (s, q), span in zip(case.recs, _spans(case.recs, run)):
        odd, lower = set(s) - set("ACGTacgt"), bool(set(s) & set("acgt"))
        if len(s) != len(q) or len(s) > 320 or any(ord(c) >= 128 for c in q) or (odd and (lower or odd != {"N"})):
            out.append("raw")
        elif span is None:
            out.append("fail")
        elif span[0] < 0:
            out.append("slow")                                   # a negative start: the byte-exact slice routine
        elif _fails(q, span[0], span[1], phred):
            out.append("fail")
        else:
            a, b = _py_slice(len(s), *span)
            w = s[a:b].upper()
            out.append("inplace" if ec64_fits(len(w), w.count("N")) else "keys")
    return tuple(out)


def classify(case, run):
    """per read of a single-pair or fixed-window block: "raw" (leaves the packed tiles: the packer's Extract+Count rule),
    "fail" (no window, or a Phred test failed), "slow" (k_ec_deferred_slow), "keys" (k_ec_deferred_keys: no single-word
    form) or "inplace" (the table's insert, or a hot hit)"""
    return _classify(case, AC.run_key(run))


def general_reads(case, run):
    if case_pairs(case):
        return AC.general_reads(case, dict(run, miss=1), pair_tables=True)      # 'N' in band, any other symbol leaves the tiles
    return classify(case, run).count("raw")


def case_pairs(case):
    return bool(getattr(case, "pairs", False))


def stages(case, run, learn=LEARN):
    """the launches of one block in a fresh context on the hot-key path, while no table grows and none fills up"""
    cl = [c for c in classify(case, run) if c != "raw"]
    tiles, lt = -(-len(cl) // TILE), -(-learn // TILE)
    out = [S_LEARN] + ([S_BUILD, S_HOT] if lt < tiles else [])
    return out + ([S_KEYS] if "keys" in cl else []) + ([S_SLOW] if "slow" in cl else [])


def nw_of(case):
    longest = max(len(s) for s, _ in case.recs)
    return 3 if longest <= 96 else 5 if longest <= 160 else 10


def instances(case, run, learn=LEARN):
    """the instances <NW, KB, SAMEQ, LEARN> of k_extract_anchor_hot the block's launches are"""
    ms = max(run.get("miss_search_up", 0), run.get("miss_search_down", 0))
    kb = 0 if ms == 0 else 1 if ms <= 1 else 3
    sq = run.get("qual_up", 30) == run.get("qual_down", 30) == run["phred"]
    return {(nw_of(case), kb, sq, s == S_LEARN) for s in stages(case, run, learn) if s in (S_LEARN, S_HOT)}


# (longest read, --msu = --msd, extra parameters, anchors): the anchor forms rotate over the rows
FORMS = ("both", "up", "down")
HOT_MATRIX = [(ml, ms, extra, FORMS[i % 3]) for i, (ml, ms, extra) in
              enumerate((ml, ms, extra) for ml in (150, 96) for ms in (0, 1, 2) for extra in ({}, {"qual_up": 20}))]
PAIR_MATRIX = [(150, 0, {}), (150, 1, {}), (150, 2, {}), (150, 1, {"qual_up": 20}), (200, 1, {})]


# ---- table sizes: ec_alloc64 / ec_reserve / launch_block restated -----------------------------------------------------------
def slots_for(keys):
    s = 1024
    while 3 * s < 4 * keys:
        s *= 2
    return s


def aside_of(n_slots):
    return 4096 + n_slots // 2048


def first_reserve(n_slots, learn):
    """(slots, room) of the single-word table after the first block's first ec_reserve (no raw records)"""
    to_learn = min(n_slots, learn)
    keys64 = to_learn + (n_slots - to_learn) // 6 + aside_of(n_slots)
    need_r = keys64 + 16
    slots = slots_for(max(need_r + keys64 // 4, 1 << 16))
    return slots, 3 * slots // 4


def expect_of(reads, keys, learned):
    return min(reads, int(min(1.0, keys / max(learned, 1)) * reads) + 4096)


def grows_before_launch(n_slots, keys, learned, room):
    """ec_reserve before a later block's launch finds too little room in the single-word table"""
    return keys + expect_of(n_slots, keys, learned) + aside_of(n_slots) + 16 > room


class Plain:
    """a block without kinds: reads and their FASTQ"""

    def __init__(self, recs):
        self.recs, self.n = recs, len(recs)
        self.fq = AC.fastq_of(recs)


def _distinct(rng, n, length, avoid=()):
    seen, out = set(avoid), []
    while len(out) < n:
        w = AC.rand_seq(rng, length)
        if w not in seen:
            seen.add(w); out.append(w)
    return out


def _plain(wins):
    return Plain([(w, "I" * len(w)) for w in wins])


FIXED20 = dict(mode="EC", miss=1, phred=30, length=20, start="0")


@functools.lru_cache(maxsize=None)
def capacity_blocks(n_keys=12000):
    """20-base reads, window (0, 20).  A: n_keys distinct windows x 6 reads, shuffled (all learning: every key becomes a
    candidate); B: two reads of every window and 2000 new windows, shuffled"""
    rng = random.Random(n_keys)
    wins = _distinct(rng, n_keys + 2000, 20)
    a = wins[:n_keys] * 6
    rng.shuffle(a)
    b = wins[:n_keys] * 2 + wins[n_keys:]
    rng.shuffle(b)
    return _plain(a), _plain(b)


GROW_HOT, GROW_SINGLES, GROW_NEW, GROW_B_HOT = 24, 832, 105000, 15000


@functools.lru_cache(maxsize=None)
def growth_blocks():
    """20-base reads, window (0, 20), F2Q_HOT_LEARN = 1024.  A: 8192 reads; the 1024 learning reads are 8 of each of 24 keys
    and 832 keys seen once (the rate of new keys the sample shows: 856 / 1024), the rest is on the 24 keys.  B: 105 000 new
    keys and 15 000 reads of the 24 keys: expect_of gives 0.836 x 120 064 + 4096 keys, more than the 98 304 the table of
    2^17 slots takes, so ec_reserve grows it before the launch.  C: 2048 reads of the 24 keys, counted through the re-linked set."""
    rng = random.Random(0x6E0)
    wins = _distinct(rng, GROW_HOT + GROW_SINGLES + GROW_NEW, 20)
    hot, singles, new = wins[:GROW_HOT], wins[GROW_HOT:GROW_HOT + GROW_SINGLES], wins[GROW_HOT + GROW_SINGLES:]
    learn = hot * 8 + singles
    rng.shuffle(learn)
    a = learn + [rng.choice(hot) for _ in range(8192 - LEARN)]
    b = new + [rng.choice(hot) for _ in range(GROW_B_HOT)]
    rng.shuffle(b)
    c = [rng.choice(hot) for _ in range(2048)]
    return _plain(a), _plain(b), _plain(c), tuple(hot)


BYTES_KEYS = 3000                      # per block: 6000 byte-string keys in all, more than the floor of 4096 entries


@functools.lru_cache(maxsize=None)
def bytes_blocks():
    """anchored, both anchors: two blocks of 3000 reads with distinct 31-base windows (byte-string keys) next to 1024 reads
    on four 20-base windows.  The entry arrays hold max(aside + 16 + aside / 4, 4096) = 5137 entries after the first reserve
    (aside = 4096 + slots / 2048: the reads a launch may set aside); the second block's reserve needs 3000 + aside + 16."""
    rng = random.Random(0xB17E)
    wins = _distinct(rng, 2 * BYTES_KEYS, 31)
    hot = windows()[:4]
    out = []
    for k in range(2):
        ws = [rng.choice(hot) for _ in range(LEARN)] + wins[k * BYTES_KEYS:(k + 1) * BYTES_KEYS]
        recs = [AC.rand_seq(rng, rng.randrange(9)) + AC.UP + w + AC.DOWN + AC.rand_seq(rng, rng.randrange(5)) for w in ws]
        out.append(Plain([(s, "I" * len(s)) for s in recs]))
    return tuple(out)


FULL_HOT, FULL_NEW = 24, 140000


def _with_n(rng, w):
    p = rng.randrange(len(w))
    return w[:p] + "N" + w[p + 1:]


@functools.lru_cache(maxsize=None)
def full_block(fixed):
    """one block: 1024 learning reads on 24 keys (a rate of 24 new keys in 1024 reads, so launch_block reserves the floor:
    2^16 keys of room at a load of 3/4 are 2^17 slots), then 140 000 reads with 140 000 new keys -- more keys than the table
    has slots, so at least 140 024 - 131 072 inserts find it full, in tiles behind slot_base = 1024.  Every 16th of the new
    windows holds an 'N' (a single-word key all the same).  fixed: 20-base reads, window (0, 20); else short reads with both
    anchors."""
    rng = random.Random(0xF011 + fixed)
    wins = _distinct(rng, FULL_HOT + FULL_NEW, 20)
    hot, new = wins[:FULL_HOT], wins[FULL_HOT:]
    new = [(_with_n(rng, w) if i % 16 == 3 else w) for i, w in enumerate(new)]
    assert len(set(new)) == len(new)
    ws = [hot[i % FULL_HOT] for i in range(LEARN)] + new
    if fixed:
        return _plain(ws)
    recs = [AC.rand_seq(rng, rng.randrange(9)) + AC.UP + w + AC.DOWN + AC.rand_seq(rng, rng.randrange(5)) for w in ws]
    return Plain([(s, "I" * len(s)) for s in recs])


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(cases, rk):
    run = {k: (v if k in ("upstream", "downstream", "start", "mode") else int(v)) for k, v in rk}
    o = O.Oracle(**run)
    for c in cases:
        o.count_fastq(c.fq)
    out = list(zip(o.keys(), o.counts())), o.stats()
    o.close()
    return out


def expect(cases, **run):
    """(rows [(key, count)] in first-seen order, stats) of the oracle over the blocks, in read-index order"""
    cases = cases if isinstance(cases, tuple) else (cases,)
    return _oracle(cases, AC.run_key(run))


def rows_of(case, i, **run):
    """the oracle's rows and statistics for read i of the block alone"""
    o = O.Oracle(**run)
    o.count_fastq(AC.fastq_of([case.recs[i]]))
    out = list(zip(o.keys(), o.counts())), o.stats()
    o.close()
    return out
