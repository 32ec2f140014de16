"""tests/gk_cases.py -- inputs for the byte-string feature index (GkDesc: build_gk in f2q_host.h, gk_exact / gk_near /
lib_scan under match_key_dist in f2q_device.h) at its edges.  Shared by tests/test_gk_edges_cpu.py (CPU emulation) and
tests/test_gk_edges_gpu.py.  Every case is (library, FASTQ bytes, run keywords); the expectation is the oracle's.

(1) fixed_case(L, miss): one window of L bases at 6, L in LENS, miss in MISSES.  A few dozen random features; siblings one
byte away from some of them, the byte taken from chosen_bytes(L, miss): byte 0, the last byte, bytes 62 / 63 / 64, the last
byte of every 8-byte word and both sides of every piece cut p * L / (miss + 1); pairs of features equidistant from a planted
key (ties); a feature with an 'N'; a feature written with a lower-case base in the csv; two features a byte shorter and two
a byte longer.  For L >= 65, collider pairs (F, K): K differs from feature F at one byte >= 64 only and hashes to F's home
slot in the exact table, so K's exact probe compares F first (one K is a feature itself and sits behind F).  Reads are a
feature with 0, 1, 2, miss or miss + 1 substitutions AT THE CHOSEN BYTES, planted keys, collider keys, random windows and
reads that end inside the window, behind a 6-base prefix and in front of a tail of 0, 3 or 100 bases.

(2) many_groups_case(miss): a dozen length groups between 5 and 110 (one of 1 feature, one of 8 -- 16 slots, two features
with home slot 15 --, one of 9), --st 4 --l 120 on reads that end inside the window: keys of every group's length, of
lengths in the gaps, below the smallest and above the largest group.

(3) joined_case(kind, miss): --st a,b,c --l 34 (104-byte keys), --l 35 (107 bytes) and two windows of 40.

(4) pair_case(plen): two --us/--ds pairs with parts of 31 + 31 (63-byte keys) and 34 + 34 bases (69 bytes).

(5) Model: build_gk and the probe restated in Python (FNV-1a with the salt, gk_mix, the cuts, linear probing).  It proves
what the inputs reach (reach()); it is never the reference for a verdict.
"""
import functools
import random

import numpy as np

from conftest import loader_view
from oracle import oracle as O

LENS = (2, 7, 8, 9, 56, 57, 63, 64, 65, 72, 96, 103, 104, 105, 120)
MISSES = (0, 1, 2, 3, 7, 8, 9)
# the fixed-window cases the GPU test runs: every L at misses 0, 1 and 8, four lengths at every miss
GPU_FIXED = sorted({(L, m) for L in LENS for m in (0, 1, 8)} | {(L, m) for L in (64, 65, 104, 105) for m in MISSES})
PREFIX = 6
PH = 30
GK_MAXP = 8                                     # F2Q_GK_MAXP
GK_WORD_BYTES = 104                             # 8 * F2Q_GK_MAXW
STAGE = 192                                     # bytes of a line k_count_general stages in LDS
N_READS = 2000

_ACGT = bytes(b"ACGT"[i & 3] for i in range(256))
_M64 = (1 << 64) - 1


def rand_seq(rng, n):
    return rng.randbytes(n).translate(_ACGT)


def sub(rng, b, pos):
    """another base at b[pos] (a bytearray), whatever stands there"""
    cur = b[pos] & 0xDF
    b[pos] = rng.choice([c for c in b"ACGT" if c != cur])


def chosen_bytes(L, miss):
    """the bytes of a key of L bytes at which a wrong bit position or a cut off by one changes a verdict"""
    s = {0, L - 1} | {b for b in (62, 63, 64) if b < L} | {b for b in range(7, L, 8)}
    for p in range(1, miss + 1):
        c = p * L // (miss + 1)
        s |= {x for x in (c - 1, c) if 0 <= x < L}
    return sorted(s)


def mutate(rng, w, k, ch):
    """k substitutions in w (a bytearray) at chosen bytes, at other bytes once those run out"""
    ch = [c for c in ch if c < len(w)]
    k = min(k, len(w))
    pos = rng.sample(ch, k) if k <= len(ch) else ch + rng.sample([i for i in range(len(w)) if i not in set(ch)], k - len(ch))
    for p in pos:
        sub(rng, w, p)
    return pos


def fastq_of(recs):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(recs))


def records(fq):
    lines = fq.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [(lines[i + 1].rstrip(), lines[i + 3].rstrip()) for i in range(0, len(lines) - 3, 4)]


def _spoil(rng, s, q, at, n, ch):
    """oddities that change no length: a lower-case base or an 'N' at a chosen byte of the window [at, at + n), a low
    quality byte on the window's first, last or a chosen byte, and one just outside it (which must not fail the read)"""
    ch = [c for c in ch if c < n and at + c < len(s)]
    roll = rng.random()
    if ch and roll < 0.05:
        p = at + rng.choice(ch)
        s[p] = s[p] | 0x20
    elif ch and roll < 0.08:
        s[at + rng.choice(ch)] = ord("N")
    roll = rng.random()
    if ch and roll < 0.06:
        q[at + rng.choice((0, ch[-1], rng.choice(ch)))] = ord("#")
    elif roll < 0.09:
        p = rng.choice((at - 1, at + n))
        if 0 <= p < len(q):
            q[p] = ord("#")


# ---- (5) the index restated ------------------------------------------------------------------------------------------------
def gk_mix(h):
    h ^= h >> 29
    h = h * 0xBF58476D1CE4E5B9 & _M64
    return h ^ (h >> 32)


def gk_hash(bs, a, b, salt):
    h = 1469598103934665603 ^ salt
    for k in range(a, b):
        h = (h ^ bs[k]) * 1099511628211 & _M64
    return gk_mix(h)


def table_bits(n):
    bits = 4
    while (1 << bits) < 2 * n:
        bits += 1
    return bits


class Group:
    def __init__(self, length, ids, miss, tab):
        self.len, self.ids, self.n, self.bits = length, ids, len(ids), table_bits(len(ids))
        P = miss + 1 if miss > 0 else 0
        self.n_pieces = P if 1 <= P <= GK_MAXP and P <= length else 0
        self.cut = [p * length // self.n_pieces for p in range(self.n_pieces)] + [length]
        self.exact_off = len(tab)
        tab.extend([0] * (1 << self.bits))
        self.piece_off = []
        for _ in range(self.n_pieces):
            self.piece_off.append(len(tab))
            tab.extend([0] * (1 << self.bits))


class Model:
    """build_gk: groups by length (stable), per group an exact table and n_pieces piece tables of feature ids + 1"""

    def __init__(self, lib, miss):
        self.feat = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in lib]
        self.tab, self.groups = [0], []
        order = sorted(range(len(self.feat)), key=lambda f: len(self.feat[f]))
        i = 0
        while i < len(order):
            j = i
            while j < len(order) and len(self.feat[order[j]]) == len(self.feat[order[i]]):
                j += 1
            g = Group(len(self.feat[order[i]]), order[i:j], miss, self.tab)
            for f in g.ids:
                self._put(g, g.exact_off, gk_hash(self.feat[f], 0, g.len, 0xE0), f)
                for p in range(g.n_pieces):
                    self._put(g, g.piece_off[p], gk_hash(self.feat[f], g.cut[p], g.cut[p + 1], p), f)
            self.groups.append(g)
            i = j
        self.by_len = {g.len: g for g in self.groups}

    def _put(self, g, off, h, f):
        s, m = h >> (64 - g.bits), (1 << g.bits) - 1
        while self.tab[off + s]:
            s = (s + 1) & m
        self.tab[off + s] = f + 1

    def chain(self, g, off, h, stop=None):
        """the features a probe from hash h meets in order, until an empty slot (or feature `stop`); wrapped: it went
        from the last slot of the table to slot 0"""
        s, m = h >> (64 - g.bits), (1 << g.bits) - 1
        out, wrapped = [], False
        while self.tab[off + s]:
            out.append(self.tab[off + s] - 1)
            if out[-1] == stop:
                break
            wrapped |= s == m
            s = (s + 1) & m
        return out, wrapped

    def exact(self, g, key):
        """gk_exact: (features compared before the verdict, the hit or -1, wrapped)"""
        seen, wrapped, s, m = [], False, gk_hash(key, 0, g.len, 0xE0) >> (64 - g.bits), (1 << g.bits) - 1
        while self.tab[g.exact_off + s]:
            f = self.tab[g.exact_off + s] - 1
            if self.feat[f] == key:
                return seen, f, wrapped
            seen.append(f)
            wrapped |= s == m
            s = (s + 1) & m
        return seen, -1, wrapped


def reach(lib, keys, miss):
    """what the distinct keys reach in the index of (lib, miss), as counts:
    hi_only   a feature compared by an exact probe, before its end, that differs from the key at bytes >= 64 only   (a)
    dup_hi    a candidate met through a piece wholly at bytes >= 64 that an earlier piece had met already            (b)
    straddle  a candidate met through a piece with bytes on both sides of 63 / 64                                    (c)
    wrap16    probe chains (exact or piece) that go round the end of a 16-slot table                                 (d)
    scans     keys whose group is scanned (n_pieces == 0) after an exact miss; scan_lens: the lengths of those groups
    word / byte  keys on the word road (<= 104 bytes) and on the byte road, among those that find a group
    no_group  keys of a length no feature has"""
    m = Model(lib, miss)
    out = dict(hi_only=0, dup_hi=0, straddle=0, wrap16=0, scans=0, scan_lens=set(), word=0, byte=0, no_group=0)
    for key in sorted(set(keys)):
        g = m.by_len.get(len(key))
        if g is None:
            out["no_group"] += 1
            continue
        out["word" if len(key) <= GK_WORD_BYTES else "byte"] += 1
        seen, hit, wrapped = m.exact(g, key)
        for f in seen:
            d = [i for i in range(g.len) if m.feat[f][i] != key[i]]
            out["hi_only"] += bool(d) and d[0] >= 64
        out["wrap16"] += wrapped and g.bits == 4
        if hit >= 0 or miss == 0:
            continue
        if not g.n_pieces:
            out["scans"] += 1
            out["scan_lens"].add(g.len)
            continue
        for p in range(g.n_pieces):
            a, b = g.cut[p], g.cut[p + 1]
            cands, wrapped = m.chain(g, g.piece_off[p], gk_hash(key, a, b, p))
            out["wrap16"] += wrapped and g.bits == 4
            for f in cands:
                fb = m.feat[f]
                if fb[a:b] != key[a:b]:
                    continue
                out["straddle"] += a <= 63 and b >= 65
                if a >= 64 and any(fb[g.cut[q]:g.cut[q + 1]] == key[g.cut[q]:g.cut[q + 1]] for q in range(p)):
                    out["dup_hi"] += 1
    return out


def verdict_classes(lib, keys, miss):
    """keys per class -- perfect, imperfect, far (no feature of the key's length within miss), tie (the nearest distance is
    shared) --, by brute force over the features of the key's length.  Coverage only: the oracle gives the expectation."""
    feat = [s.encode("latin-1") for s in lib]
    by_len = {}
    for f in feat:
        by_len.setdefault(len(f), []).append(np.frombuffer(f, dtype=np.uint8))
    mats = {n: np.stack(v) for n, v in by_len.items()}
    out = dict(perfect=0, imperfect=0, far=0, tie=0)
    for key in keys:
        M = mats.get(len(key))
        if M is None or not len(key):
            out["far"] += 1
            continue
        d = (M != np.frombuffer(key, dtype=np.uint8)).sum(axis=1)
        best = int(d.min())
        if best == 0:
            out["perfect"] += 1
        elif best > miss:
            out["far"] += 1
        elif int((d == best).sum()) > 1:
            out["tie"] += 1
        else:
            out["imperfect"] += 1
    return out


def fixed_keys(fq, run):
    """the keys of a fixed-window run, from the text: the windows whose quality slice passes, upper-cased, joined by ':'
    (fast2q.py:349-363; the slices clip as Python's do)"""
    starts, n, ph = [int(x) for x in str(run["start"]).split(",")], run["length"], max(int(run.get("phred", 30)), 1)
    keys = []
    for seq, qual in records(fq):
        parts = [seq[s:s + n].upper() for s in starts if not any(33 <= c <= min(ph + 31, 126) for c in qual[s:s + n])]
        if parts:
            keys.append(b":".join(parts))
    return keys


# ---- (1) one window of L bases ---------------------------------------------------------------------------------------------
def _as_library(feats, lower=None):
    """the library as the loader leaves the csv [(name, sequence as written)]; `lower`: the feature written with its last
    base in lower case"""
    csv = [("g%d" % i, (f[:-1] + f[-1:].lower() if f == lower else f).decode()) for i, f in enumerate(feats)]
    lib = [s for _, s in loader_view(csv)]
    assert lib == [f.decode() for f in feats]
    return lib


@functools.lru_cache(maxsize=None)
def fixed_plan(L, miss, n_reads=N_READS):
    rng = random.Random(0x6B000000 + 4096 * L + miss)
    ch = chosen_bytes(L, miss)
    seen, feats = set(), []

    def add(s):
        s = bytes(s)
        if s in seen:
            return False
        seen.add(s)
        feats.append(s)
        return True
    nb = min(36, max(2, 4 ** L // 5))
    bases = []
    while len(bases) < nb:
        s = rand_seq(rng, L)
        if add(s):
            bases.append(s)
    for k, c in enumerate(ch):                                       # siblings one chosen byte away
        b = bytearray(bases[k % max(1, nb // 2)])
        sub(rng, b, c)
        add(b)
    planted = []                                                     # keys with two features equally far away
    for t in range(4):
        K = rand_seq(rng, L)
        if t < 3:
            pa, pb = [ch[(2 * t) % len(ch)]], [ch[(2 * t + 1) % len(ch)]]
        else:
            pa, pb = ch[:2], ch[-2:]
        if K in seen or set(pa) & set(pb) or len(ch) < len(pa) + len(pb):
            continue
        for pos in (pa, pb):
            f = bytearray(K)
            for p in pos:
                sub(rng, f, p)
            add(f)
        planted.append(K)
    odd = bytearray(rand_seq(rng, L))
    odd[L // 2] = ord("N")
    add(odd)
    lower = rand_seq(rng, L)
    while not add(lower):
        lower = rand_seq(rng, L)
    add(bases[0][:-1]), add(rand_seq(rng, L - 1)), add(bases[0] + b"A"), add(rand_seq(rng, L + 1))
    colliders = []
    if L >= 65:
        bits = table_bits(sum(len(f) == L for f in feats) + 4)
        hi = [c for c in ch if c >= 64]
        while len(colliders) < 3:
            F = rand_seq(rng, L)
            home = gk_hash(F, 0, L, 0xE0) >> (64 - bits)
            for c, x in ((c, x) for c in hi for x in b"ACGT"):
                K = F[:c] + bytes([x]) + F[c + 1:]
                if x != F[c] and gk_hash(K, 0, L, 0xE0) >> (64 - bits) == home:
                    colliders.append((F, K, c))
                    break
        for i, (F, K, c) in enumerate(colliders):
            assert add(F) and (i or add(K))
        assert table_bits(sum(len(f) == L for f in feats)) == bits
    own = [f for f in feats if len(f) == L]
    recs = []
    for i in range(n_reads):
        roll, tail = rng.random(), rng.choice((0, 3, 100))
        if 0.55 <= roll < 0.65 and planted:
            w = bytearray(rng.choice(planted))
            if rng.random() < 0.3:
                mutate(rng, w, 1, ch)
        elif 0.65 <= roll < 0.73 and colliders:
            w = bytearray(rng.choice(colliders)[1])
            if rng.random() < 0.3:
                sub(rng, w, rng.choice([c for c in ch if c < 64]))
        elif roll < 0.73:
            w = bytearray(rng.choice(own))
            mutate(rng, w, rng.choice((0, 1, 1, 2, miss, miss + 1)), ch)
        elif roll < 0.80:
            w = bytearray(rand_seq(rng, L))
        elif roll < 0.88:                                            # the read ends inside the window
            src = rng.choice(feats)
            w, tail = bytearray(src[:rng.choice((L - 1, len(src) - 1, rng.randrange(L)))]), 0
            mutate(rng, w, rng.choice((0, 0, 1)), ch)
        else:
            w = bytearray(rng.choice(bases))
            mutate(rng, w, rng.choice((0, 1)), ch)
        s = bytearray(rand_seq(rng, PREFIX) + bytes(w) + rand_seq(rng, tail))
        q = bytearray(b"I" * len(s))
        _spoil(rng, s, q, PREFIX, L, ch)
        recs.append((bytes(s), bytes(q)))
    return dict(lib=_as_library(feats, lower), fq=fastq_of(recs), run=dict(start=str(PREFIX), length=L, phred=PH, miss=miss),
                planted=planted, colliders=colliders, chosen=ch)


def fixed_case(L, miss):
    p = fixed_plan(L, miss)
    return p["lib"], p["fq"], p["run"]


# ---- (2) a dozen length groups ------------------------------------------------------------------------------------------------
GROUPS = ((5, 12), (6, 9), (9, 14), (16, 8), (31, 12), (32, 1), (40, 16), (57, 12), (64, 10), (65, 12), (88, 14), (110, 12))
GAP_LENS = (7, 8, 20, 33, 50, 63, 66, 100, 104, 105, 109)
BELOW, ABOVE = (0, 1, 3, 4), (111, 119, 120)
MG_START, MG_LEN = 4, 120


@functools.lru_cache(maxsize=None)
def many_groups_library():
    rng = random.Random(0x6B0A11)
    feats = []
    for n, count in GROUPS:
        grp = set()
        if count == 8:                                               # 16 slots: two features whose home is the last slot
            while len(grp) < 2:
                s = rand_seq(rng, n)
                if gk_hash(s, 0, n, 0xE0) >> 60 == 15:
                    grp.add(s)
        while len(grp) < count:
            grp.add(rand_seq(rng, n))
        grp = sorted(grp)
        if n == 40:
            grp[0] = grp[0][:20] + b"N" + grp[0][21:]
        feats += grp
    rng.shuffle(feats)
    return _as_library(feats)


@functools.lru_cache(maxsize=None)
def many_groups_case(miss, n_reads=2400):
    rng = random.Random(0x6B0A12 + miss)
    lib = many_groups_library()
    feats = [s.encode() for s in lib]
    recs = []
    for i in range(n_reads):
        roll, tail, pre = rng.random(), 0, MG_START
        if roll < 0.6:
            w = bytearray(rng.choice(feats))
            mutate(rng, w, rng.choice((0, 0, 1, 2, miss, miss + 1)), chosen_bytes(len(w), miss))
        elif roll < 0.9:
            n = rng.choice(GAP_LENS if roll < 0.75 else BELOW if roll < 0.82 else ABOVE)
            src = rng.choice(feats)
            w = bytearray((src + rand_seq(rng, 120))[:n] if rng.random() < 0.5 else rand_seq(rng, n))
            tail = rng.choice((0, 20)) if n == MG_LEN else 0         # a read that goes on behind the window
        elif roll < 0.93:
            w, pre = bytearray(), rng.randrange(MG_START)            # ends before the window starts
        else:
            w = bytearray(rand_seq(rng, rng.choice(GROUPS)[0]))
        s = bytearray(rand_seq(rng, pre) + bytes(w) + rand_seq(rng, tail))
        q = bytearray(b"I" * len(s))
        _spoil(rng, s, q, MG_START, len(w), chosen_bytes(max(len(w), 1), miss))
        recs.append((bytes(s), bytes(q)))
    return lib, fastq_of(recs), dict(start=str(MG_START), length=MG_LEN, phred=PH, miss=miss)


# ---- (3) joined keys -------------------------------------------------------------------------------------------------------
JOINED = {"3x34": ((3, 40, 80), 34, 120), "3x35": ((3, 40, 80), 35, 120), "2x40": ((2, 50), 40, 96)}


def _shifted(parts, x):
    """the joined parts with their last ':' one byte later: as long as the joined key, a base (x) where the key holds ':'
    and ':' where the key holds the last part's first base -- two bytes away from it"""
    return b":".join(parts[:-2] + [parts[-2] + x]) + b":" + parts[-1][1:]


@functools.lru_cache(maxsize=None)
def joined_library(kind):
    starts, n, _ = JOINED[kind]
    rng = random.Random(0x6B0C00 + 8 * len(starts) + n)
    W = len(starts)
    pools = [[rand_seq(rng, n) for _ in range(24)] for _ in range(W)]
    combos = []
    while len(combos) < 92:
        c = tuple(rng.choice(pools[w]) for w in range(W))
        if c not in combos:
            combos.append(c)
    combos, fresh = combos[:90], combos[90:]                         # fresh: planted in reads, not in the library
    feats = [b":".join(c) for c in combos]
    feats += pools[0][:6] + pools[1][:4]                             # one part: the other windows failed their Phred test
    if W == 3:
        feats += [b":".join(c[:2]) for c in combos[:8]] + [b":".join(c[1:]) for c in combos[8:12]] + [c[0] + b":" + c[2] for c in combos[12:16]]
    feats += [_shifted(list(combos[0]), b"A"), _shifted(list(fresh[0]), b"C")]
    feats.append(b"G".join(fresh[1]))                               # no ':' at all: both separators of the key mismatch
    lone = rand_seq(rng, n)
    feats.append(lone[:16] + b":" + lone[17:])                      # a one-part key holds a base where this holds ':'
    feats = list(dict.fromkeys(feats))
    return _as_library(feats), combos, fresh, pools, lone


@functools.lru_cache(maxsize=None)
def joined_case(kind, miss, n_reads=N_READS):
    starts, n, rlen = JOINED[kind]
    lib, combos, fresh, pools, lone = joined_library(kind)
    rng = random.Random(0x6B0C80 + 64 * len(starts) + 8 * n + miss)
    W = len(starts)
    at = (0, n - 1, 15, 16, 17, n // 2)
    recs = []
    for i in range(n_reads):
        roll = rng.random()
        lowq = []
        if roll < 0.68:
            parts = list(rng.choice(combos))
        elif roll < 0.76:
            parts = list(rng.choice(fresh))
        elif roll < 0.80:                                            # the lone part in window 0, the other windows fail
            parts, lowq = [lone] + [rand_seq(rng, n) for _ in range(W - 1)], list(range(1, W))
        elif roll < 0.92:
            parts = [rng.choice(pools[w]) for w in range(W)]
        else:
            parts = [rand_seq(rng, n) for _ in range(W)]
        parts = [bytearray(p) for p in parts]
        for _ in range(rng.choice((0, 0, 1, 1, 2, miss + 1))):     # substitutions inside each part, at its edges
            sub(rng, parts[rng.randrange(W)], rng.choice(at))
        s = bytearray(rand_seq(rng, rlen))
        for w in range(W):
            s[starts[w]:starts[w] + n] = parts[w]
        q = bytearray(b"I" * rlen)
        roll = rng.random()
        if not lowq and roll < 0.25:
            lowq = [rng.randrange(W)]
        elif not lowq and roll < 0.30:
            lowq = rng.sample(range(W), 2)
        elif not lowq and roll < 0.32:
            lowq = list(range(W))
        for w in lowq:
            q[starts[w] + rng.choice(at)] = ord("#")
        roll = rng.random()
        if roll < 0.03:
            s[starts[rng.randrange(W)] + rng.choice(at)] = ord("N")
        elif roll < 0.06:
            p = starts[rng.randrange(W)] + rng.choice(at)
            s[p] = s[p] | 0x20
        elif roll < 0.10:                                            # the read ends inside the last window
            cut = rng.randrange(starts[-1], starts[-1] + n)
            del s[cut:], q[cut:]
        recs.append((bytes(s), bytes(q)))
    return lib, fastq_of(recs), dict(start=",".join(map(str, starts)), length=n, phred=PH, miss=miss)


# ---- (4) two --us/--ds pairs -------------------------------------------------------------------------------------------------
UPS, DOWNS = ("GTTTAAGAGCTA", "ACCTGGATCCAA"), ("CGTTACCAGGTT", "TTCAGGCATGCA")
PAIRS_KEYMAX = 68                                                    # F2Q_PAIRS_KEYMAX: a joined key must stay below it


@functools.lru_cache(maxsize=None)
def pair_case(plen, n_reads=N_READS):
    """parts of plen + plen bases between the anchors; the library is A:B plus some one-part features (parts longer than
    20 bases: no pair tables, the byte-string index decides).  --m 1, --msu 1 --msd 1"""
    rng = random.Random(0x6B0D00 + plen)
    pools = [[rand_seq(rng, plen) for _ in range(20)] for _ in range(2)]
    combos = []
    while len(combos) < 100:
        c = (rng.choice(pools[0]), rng.choice(pools[1]))
        if c not in combos:
            combos.append(c)
    feats = [a + b":" + b for a, b in combos] + pools[0][:6] + pools[1][:6]
    at = (0, plen - 1, plen // 2, 30)
    recs = []
    for i in range(n_reads):
        roll = rng.random()
        parts = list(rng.choice(combos)) if roll < 0.8 else [rng.choice(pools[0]), rng.choice(pools[1])] if roll < 0.93 else \
            [rand_seq(rng, plen), rand_seq(rng, plen)]
        parts = [bytearray(p) for p in parts]
        for _ in range(rng.choice((0, 0, 1, 1, 2))):
            sub(rng, parts[rng.randrange(2)], rng.choice(at))
        anchors = [bytearray(x.encode()) for x in (UPS[0], DOWNS[0], UPS[1], DOWNS[1])]
        roll = rng.random()
        if roll < 0.10:
            sub(rng, anchors[rng.randrange(4)], rng.randrange(12))
        elif roll < 0.18:                                            # an anchor beyond --msu / --msd: the part drops out
            a = anchors[rng.randrange(4)]
            for p in (1, 5, 9):
                sub(rng, a, p)
        s = bytearray(rand_seq(rng, rng.randrange(9)) + anchors[0] + parts[0] + anchors[1] + rand_seq(rng, rng.randrange(6)) +
                      anchors[2] + parts[1] + anchors[3] + rand_seq(rng, rng.randrange(6)))
        q = bytearray(b"I" * len(s))
        roll = rng.random()
        if roll < 0.04:
            s[rng.randrange(len(s))] = ord("N")
        elif roll < 0.07:
            p = rng.randrange(len(s))
            s[p] = s[p] | 0x20
        if rng.random() < 0.15:
            q[rng.randrange(len(q))] = rng.choice(b"#+5:")
        recs.append((bytes(s), bytes(q)))
    run = dict(miss=1, phred=PH, upstream=",".join(UPS), downstream=",".join(DOWNS), miss_search_up=1, miss_search_down=1)
    return _as_library(feats), fastq_of(recs), run


# ---- the expectation ---------------------------------------------------------------------------------------------------------
CASES = {"fixed": fixed_case, "groups": many_groups_case, "joined": joined_case, "pairs": pair_case}


def case(name, *args):
    return CASES[name](*args)


@functools.lru_cache(maxsize=None)
def expect(name, *args):
    """(counts, stats) of the oracle in Counter mode on the case's bytes, computed once"""
    lib, fq, run = case(name, *args)
    o = O.Oracle(features=[(str(i), s) for i, s in enumerate(lib)], **run)
    assert o.count_fastq(fq) == len(fq)
    out = o.counts(), o.stats()
    o.close()
    return out
