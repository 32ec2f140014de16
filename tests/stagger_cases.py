"""tests/stagger_cases.py -- inputs and expected values shared by the --stagger tests (CPU emulation and GPU).

The expectation is plain Python: V(d) is umi_cases._verdicts (the oracle in Counter mode, once per distinct record text) of
a run with --st s+d, one oracle per start, memoised and asked lazily in the order the rule needs; stagger_verdict is the
function of include/f2q.h (f2q_set_stagger), and the only rule stated here.  Framing is umi_cases.records: four
rstrip()-ed lines per record."""
import functools
import random

import raw_edge_cases as RE
import synth
import umi_cases as UC

S, L, N = 2, 20, 8                              # the base shape: --st 2 --l 20 --stagger 8
RUN = dict(start=str(S), length=L, phred=30)


class V:
    """V(d) of one record: the verdict (feature or -1, counter 1..3 or 0, quality_failed) of the run with --st s+d"""

    def __init__(self, lib, run, seq, qual):
        self.lib, self.run, self.seq, self.qual, self.s = tuple(lib), run, seq, qual, int(run["start"])

    def __call__(self, d):
        return UC._verdicts(self.lib, UC.run_key(dict(self.run, start=str(self.s + d)))).of(self.seq, self.qual)


def stagger_verdict(v, n):
    """-> (verdict, offset or None)"""
    for d in range(n + 1):
        if v(d)[1] == 1:                             # the earliest exact start; it outranks a window with
            return v(d), d                           # mismatches at an earlier start
    for d in range(n + 1):
        if v(d)[1] == 2:                             # else the earliest start within --m; a start whose window is
            return v(d), d                           # ambiguous is non-aligned there and is passed over
    return v(0), None                                # nobody assigns it: counted as start s counts it


def per_read(lib, fq, n, **run):
    """[(feature or -1, counter, quality_failed, offset or None)] of the records of the text"""
    out = []
    for seq, qual in UC.records(fq):
        (f, which, qfail), off = stagger_verdict(V(lib, run, seq, qual), n)
        out.append((f, which, qfail, off))
    return out


def expect(lib, fq, n, **run):
    """(counts, stats, perfect[n + 1], imperfect[n + 1]) of the FASTQ bytes, as lists"""
    counts, stats, hist = [0] * len(lib), [0] * 5, ([0] * (n + 1), [0] * (n + 1))
    for f, which, qfail, off in per_read(lib, fq, n, **run):
        stats[0] += 1
        stats[4] += qfail
        if which:
            stats[which] += 1
        if f >= 0:
            counts[f] += 1
            hist[which - 1][off] += 1
    return counts, stats, hist[0], hist[1]


def check_invariants(counts, stats, perfect, imperfect):
    """the invariants of include/f2q.h (f2q_read_stagger)"""
    assert sum(perfect) == stats[1] and sum(imperfect) == stats[2] and sum(counts) == stats[1] + stats[2]
    assert stats[1] + stats[2] + stats[3] + stats[4] == stats[0]          # one window: every read adds to exactly one of the four


def pieces(fq, per):
    """the text cut into blocks of `per` whole records"""
    lines = fq.split(b"\n")
    assert lines.pop() == b"" and len(lines) % 4 == 0
    return [b"\n".join(lines[i:i + 4 * per]) + b"\n" for i in range(0, len(lines), 4 * per)]


# ---- 1: the base shape ---------------------------------------------------------------------------------------------------
CLASSES = ("perfect_at_0", "perfect_later", "imperfect_at_0", "imperfect_later", "imperfect_earlier_perfect_later", "perfect_at_two_starts",
           "ambiguous_earlier_assigned_later", "lowq_at_assigned_start_not_at_0", "lowq_at_0_assigned_later",
           "none_non_aligned", "none_quality_failed")
N_H = 12                                        # constructed features H = x3 + G[:17] of the guides 0 .. N_H - 1
N_AMB = 12                                      # constructed triples W1, W2 (one base from W each) and G' = W[k:] + y


@functools.lru_cache(maxsize=None)
def base_library():
    """600 guides of 20 bases, then N_H features H_i = x3 + G_i[:17] (a window three bases in front of G_i's reads H_i), then
    N_AMB triples: W1, W2 one substitution from a 20-mer W that is no feature, and G' = W[k:] + y, the window k bases on"""
    rng = random.Random(0x57A66)
    lib = UC.library()
    extra, amb = [], []
    for i in range(N_H):
        extra.append((UC.rand_seq(rng, 3) + lib[i].encode()[:17]).decode())
    for i in range(N_AMB):
        w = UC.rand_seq(rng, 20)
        k = 1 + i % 5
        w1, w2 = UC.mutate1(rng, w, 0, 8), UC.mutate1(rng, w, 12, 20)
        later = w[k:] + UC.rand_seq(rng, k)
        extra += [w1.decode(), w2.decode(), later.decode()]
        amb.append((w, k, later))
    assert len(set(lib + extra)) == len(lib) + len(extra)
    return lib + extra, amb


@functools.lru_cache(maxsize=None)
def base(seed=0x57A6):
    """~1 500 reads of 60 bases, --st 2 --l 20 --stagger 8.  900 as tests/synth.py makes them (exact, substituted, random
    and 'N' windows, a low-quality share) with the window at offset 0 .. 8 uniformly, 60 each at offset 9 and at -1 (which
    must not be rescued), and constructed reads for every class of CLASSES"""
    rng = random.Random(seed)
    lib, amb = base_library()
    guides = lib[:600]
    specs = {d: synth.Spec(seed=seed + d, n_reads=1, read_len=60, start=S + d, p_lowq=0.10) for d in range(-1, 10)}
    recs = []
    for i in range(900):
        recs.append(synth.make_read(specs[i % 9], guides, i))
    for i in range(120):
        recs.append(synth.make_read(specs[9 if i % 2 else -1], guides, 1000 + i))
    q60 = b"I" * 60

    def place(window, d, q=q60):
        return UC.rand_seq(rng, S + d) + window + UC.rand_seq(rng, 60 - S - d - len(window)), q
    for i in range(100):                                             # H_i at d, G_i at d + 3: exact / one base off in the x3 (the later, exact G_i wins)
        g, h = lib[i % N_H].encode(), lib[600 + i % N_H].encode()
        head = h[:3] if i % 2 else UC.mutate1(rng, h[:3])
        recs.append(place(head + g, rng.randrange(N - 2)))
    for i in range(100):                                             # W at d (one base from W1 and from W2), G' at d + k: exact / one base off
        w, k, later = amb[i % N_AMB]
        tail = later[20 - k:] if i % 2 else UC.mutate1(rng, later[20 - k:])
        recs.append(place(w + tail, rng.randrange(N - k + 1)))
    for i in range(160):                                             # a low quality byte: in the window at d alone / at 0 alone
        d = 1 + rng.randrange(N)
        g = guides[rng.randrange(600)].encode()
        if i % 4 == 3:
            g = UC.mutate1(rng, g)
        q = bytearray(q60)
        q[(S + 20 + rng.randrange(d)) if i % 2 else (S + rng.randrange(d))] = ord("#")
        recs.append(place(g, d, bytes(q)))
    for i in range(60):                                              # nothing anywhere, the window at 0 of low quality
        q = bytearray(q60)
        q[S + rng.randrange(20)] = ord("#")
        recs.append((UC.rand_seq(rng, 60), bytes(q)))
    for i in range(100):                                             # one substitution, at 0 and at a later start
        d = rng.randrange(1, N + 1) if i % 2 else 0
        recs.append(place(UC.mutate1(rng, guides[rng.randrange(600)].encode()), d))
    rng.shuffle(recs)
    return lib, UC.fastq_of(recs), dict(RUN)


def classes(lib, fq, n, **run):
    """records per class of CLASSES, from every V(d) of every record"""
    out = dict.fromkeys(CLASSES, 0)
    for seq, qual in UC.records(fq):
        v = V(lib, run, seq, qual)
        all_v = [v(d) for d in range(n + 1)]
        (f, which, qfail), off = stagger_verdict(v, n)
        perfect = [d for d in range(n + 1) if all_v[d][1] == 1]
        imperfect = [d for d in range(n + 1) if all_v[d][1] == 2]
        if f < 0:
            out["none_quality_failed" if qfail else "none_non_aligned"] += 1
            continue
        out[("perfect" if which == 1 else "imperfect") + ("_at_0" if off == 0 else "_later")] += 1
        out["imperfect_earlier_perfect_later"] += which == 1 and bool(imperfect) and imperfect[0] < off
        out["perfect_at_two_starts"] += len(perfect) > 1
        # ambiguous (--m 1): non-aligned at an earlier start although two features are one substitution from its window
        out["ambiguous_earlier_assigned_later"] += any(all_v[d][1] == 3 and _two_at_distance_1(lib, seq, int(run["start"]) + d, int(run["length"]))
                                                       for d in range(off))
        out["lowq_at_0_assigned_later"] += off > 0 and all_v[0][2] == 1
    return out


@functools.lru_cache(maxsize=None)
def _feature_set(lib):
    return frozenset(f.encode() for f in lib)


def _two_at_distance_1(lib, seq, start, length):
    """the window is whole and two or more features are one substitution away from it"""
    w = seq[start:start + length].upper()
    have = _feature_set(tuple(lib))
    return len(w) == length and sum(w[:j] + bytes([c]) + w[j + 1:] in have for j in range(length) for c in b"ACGT" if c != w[j]) >= 2


# ---- 2: the extremes of the span -------------------------------------------------------------------------------------------
def _placed(rng, lib, n_reads, s, n, length, read_len, p_beyond=0.08):
    """reads with a feature (exact, one base off, or a random window) at offset 0 .. n uniformly, some beyond n; a low
    quality byte in a tenth; an 'N' in a few"""
    recs = []
    for i in range(n_reads):
        d = n + 1 + rng.randrange(2) if rng.random() < p_beyond else i % (n + 1)
        g = lib[rng.randrange(len(lib))].encode()
        roll = rng.random()
        w = bytearray(UC.mutate1(rng, g) if roll < 0.25 and len(g) > 1 else UC.rand_seq(rng, len(g)) if roll < 0.35 else g)
        if rng.random() < 0.05:
            w[rng.randrange(len(w))] = ord("N")
        if rng.random() < 0.05:
            w = bytearray(bytes(w).lower())
        seq = UC.rand_seq(rng, s + d) + bytes(w) + UC.rand_seq(rng, max(read_len - s - d - len(w), 0))
        q = bytearray(b"I" * len(seq))
        if rng.random() < 0.12:
            q[min(s + rng.randrange(n + length), len(q) - 1)] = ord("#")
        recs.append((seq, bytes(q)))
    return UC.fastq_of(recs)


@functools.lru_cache(maxsize=None)
def extreme(name):
    """-> (library, text, run, n)"""
    rng = random.Random(0xE87 + sum(name.encode()))
    if name == "n32_l31":                                            # 63 positions: both code words and the top mask bit
        lib = synth.make_library(150, 31, 0x31)
        return lib, _placed(rng, lib, 330, 3, 32, 31, 100), dict(start="3", length=31, phred=30, miss=1), 32
    if name == "n1":
        lib = UC.library()
        return lib, _placed(rng, lib, 300, 2, 1, 20, 60, 0.2), dict(start="2", length=20, phred=30, miss=1), 1
    if name in ("l1", "l1_m1"):                                      # reads of C and T with one base of the library at offset 0 .. 10, or none
        lib = ["A", "G"] if name == "l1" else ["A"]                  # (--m 1 against one feature: every other base is one substitution away)
        recs = []
        for i in range(300):
            seq = bytearray(rng.choice(b"CT") for _ in range(12))
            if i % 4:
                seq[2 + rng.randrange(10)] = ord(rng.choice(lib))
            if rng.random() < 0.1:
                seq[2 + rng.randrange(10)] = rng.choice(b"Na")
            q = bytearray(b"I" * 12)
            if rng.random() < 0.3:
                q[2 + rng.randrange(10)] = ord("#")
            recs.append((bytes(seq), bytes(q)))
        return lib, UC.fastq_of(recs), dict(start="2", length=1, phred=30, miss=int(name == "l1_m1")), 8
    if name == "l32":                                                # longer than the 2-bit keys: the walk layout only
        lib = synth.make_library(150, 32, 0x32)
        return lib, _placed(rng, lib, 300, 2, 8, 32, 80), dict(start="2", length=32, phred=30, miss=1), 8
    if name == "st0":
        lib = UC.library()
        return lib, _placed(rng, lib, 300, 0, 8, 20, 60), dict(start="0", length=20, phred=30, miss=1), 8
    raise KeyError(name)


EXTREMES = ("n32_l31", "n1", "l1", "l1_m1", "l32", "st0")


# ---- 3: irregular libraries ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def with_n_feature():
    """one feature holds an 'N': the library is irregular and every record takes the walk layout"""
    rng = random.Random(0x1AA6)
    lib = UC.library()[:200] + ["ACGTNACGTACGTTGCATGC"]
    return lib, _placed(rng, lib, 300, S, N, L, 60), dict(RUN, miss=1), N


@functools.lru_cache(maxsize=None)
def mixed_lengths():
    """features of 18, 20 and 22 bases, --l 22: 400 reads, half of them ending 18 or 20 bases behind the start their feature
    sits at, so that the clipped window reads a shorter feature exactly (or one base off)"""
    rng = random.Random(0x18202)
    lib = synth.make_library(80, 18, 0x18) + synth.make_library(80, 20, 0x20) + synth.make_library(80, 22, 0x22)
    recs = []
    for i in range(400):
        d = i % (N + 1)
        g = lib[rng.randrange(len(lib))].encode()
        w = UC.mutate1(rng, g) if rng.random() < 0.25 else g
        if i % 2:
            seq = UC.rand_seq(rng, S + d) + w                        # the read ends with the feature: clipped unless it has 22 bases
        else:
            seq = UC.rand_seq(rng, S + d) + w + UC.rand_seq(rng, 30)
        q = bytearray(b"I" * len(seq))
        if rng.random() < 0.1:
            q[rng.randrange(S, len(q))] = ord("#")
        if rng.random() < 0.1:
            del q[len(q) - rng.randrange(1, 4):]                     # a quality line that ends first: whole sequence windows, clipped quality slices
        recs.append((seq, bytes(q)))
    return lib, UC.fastq_of(recs), dict(start=str(S), length=22, phred=30, miss=1), N


# ---- 4: odd records --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def odd(seed):
    """1 000 records with the feature at offset 0 .. 8, through raw_edge_cases' oddities (CRLF, trailing blanks, quality lines
    of another length, reads that end inside a window, lower case, 'N' and other bytes, odd quality bytes, empty lines, a
    partial last record, no final newline) plus a leading blank in either line.  -> (library, text, run, n)"""
    rng = random.Random(0x0DD57A + seed)
    lib = UC.library()
    recs = []
    for i in range(1000):
        g = lib[rng.randrange(len(lib))].encode()
        if rng.random() < 0.2:
            g = UC.mutate1(rng, g)
        d = rng.randrange(N + 1)
        n = rng.choice((32, 40, 60, 61, 62, 63, 150))
        s, q = bytearray(UC.rand_seq(rng, S + d) + g + UC.rand_seq(rng, n - S - d - 20)), bytearray(b"I" * n)
        if rng.random() < 0.6:
            RE._spoil(rng, s, q, ((S + d, S + d + 20), (S + d, S + d + 20), (S, S + N + 20)))
        if rng.random() < 0.08:
            s[:0] = rng.choice(RE.BLANKS)
        if rng.random() < 0.08:
            q[:0] = rng.choice(RE.BLANKS)
        recs.append((b"@o%d" % i, bytes(s), bytes(q)))
    fq, = RE._finish(rng, [RE._text(rng, recs)])
    return lib, fq, dict(RUN, miss=1), N


# ---- 5: the staging edge ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge(r):
    """raw_edge_cases.edge_sample(r): the feature window ends the read, so with --st r-20-N it sits at offset N, the far end
    of the span, on both sides of the 192-byte limit.  -> (library, text, run, n)"""
    lib, _, fq, _ = RE.edge_sample(r, 0, False)
    return lib, fq, dict(start=str(r - 20 - N), length=20, phred=RE.PH, miss=1), N


# ---- 6: long reads ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_reads():
    """400 reads of 250 bases (walked in global memory) among 400 of 60 bases"""
    rng = random.Random(0x10A65)
    lib = UC.library()
    a, b = _placed(rng, lib, 400, S, N, L, 250), _placed(rng, lib, 400, S, N, L, 60)
    ra, rb = pieces(a, 1), pieces(b, 1)
    return lib, b"".join(x + y for x, y in zip(ra, rb)), dict(RUN, miss=1), N


# ---- 7: a second trip through the grid-stride loop -------------------------------------------------------------------------
POOL = RE.POOL


@functools.lru_cache(maxsize=None)
def pass_pool():
    """257 distinct records of 40 bases, one in eight 190 (a short record is staged over a long one's bytes in the lane's
    second pass), the feature at offset 0 .. 8"""
    rng = random.Random(0x2FA58)
    lib = UC.library()
    recs = []
    for i in range(POOL):
        g = lib[rng.randrange(40)].encode()
        roll = rng.random()
        g = UC.mutate1(rng, g) if roll < 0.2 else UC.rand_seq(rng, 20) if roll < 0.3 else g
        n, d = (190 if i % 8 == 3 else 40), i % (N + 1)
        q = bytearray(b"I" * n)
        if rng.random() < 0.1:
            q[S + rng.randrange(N + 20)] = ord("#")
        recs.append((UC.rand_seq(rng, S + d) + g + UC.rand_seq(rng, n - S - d - 20), bytes(q)))
    assert len(set(recs)) == POOL
    return UC.fastq_of(recs)


def second_pass(n_cu):
    """-> (FASTQ bytes, repetitions), as raw_edge_cases.second_pass: more records than the lanes of a capped launch"""
    reps = -(-(n_cu * 4096 + 3 * POOL) // POOL)
    return pass_pool() * reps, reps


def scaled(e, k):
    return tuple([x * k for x in part] for part in e)


# ---- every guide at offset 0 -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_at_zero():
    """600 reads with an exact feature at --st 2 and nothing else: any --stagger gives the plain run's counts"""
    rng = random.Random(0xA770)
    lib = UC.library()
    recs = [(UC.rand_seq(rng, S) + lib[rng.randrange(len(lib))].encode() + UC.rand_seq(rng, 38), b"I" * 60) for _ in range(600)]
    return lib, UC.fastq_of(recs), dict(RUN, miss=1)


# the cases of the list by name: -> (library, text, run, n)
CASES = {"base": lambda: base() + (N,), "odd0": lambda: odd(0), "odd1": lambda: odd(1), "odd2": lambda: odd(2), "long_reads": long_reads,
         "with_n_feature": with_n_feature, "mixed_lengths": mixed_lengths,
         "pass_pool": lambda: (UC.library(), pass_pool(), dict(RUN, miss=1), N)}
CASES.update({name: (lambda name=name: extreme(name)) for name in EXTREMES})
CASES.update({f"edge{r}": (lambda r=r: edge(r)) for r in RE.EDGE_R})


def check_coverage():
    """what the cases claim, from the expectation alone"""
    lib, fq, run = base()
    recs = UC.records(fq)
    assert 1400 <= len(recs) <= 1600
    got = classes(lib, fq, N, miss=1, **run)
    # a low quality byte in the window at d but not at 0 leaves a read that start d would have assigned without its verdict
    # there; it shows as a read whose later windows fail the Phred test while the one at 0 does not
    got["lowq_at_assigned_start_not_at_0"] = _lowq_blocks(lib, fq, N, miss=1, **run)
    assert all(got[k] >= 30 for k in CLASSES), got
    # reads whose feature sits at offset 9 or at -1 are not rescued: the plain runs at those starts assign them, the stagger does not
    for beyond in (N + 1, -1):
        there = UC._verdicts(tuple(lib), UC.run_key(dict(run, miss=1, start=str(S + beyond)))).of
        assert sum(1 for (s, q), x in zip(recs, per_read(lib, fq, N, miss=1, **run)) if there(s, q)[0] >= 0 and x[0] < 0) >= 30, beyond
    # no read that the plain run assigns perfectly is assigned otherwise
    plain = UC._verdicts(tuple(lib), UC.run_key(dict(run, miss=1))).of
    for (s, q), x in zip(recs, per_read(lib, fq, N, miss=1, **run)):
        p = plain(s, q)
        assert p[1] != 1 or (x[0], x[1], x[3]) == (p[0], 1, 0)
    e = expect(*extreme("n32_l31")[:2], 32, **extreme("n32_l31")[2])
    assert e[2][32] >= 3 and e[2][0] >= 3 and sum(e[3]) >= 20 and sum(1 for x in e[2] if x) >= 30, e[2:]
    for name in EXTREMES:
        lib, fq, run, n = extreme(name)
        assert 290 <= len(UC.records(fq)) <= 340
        e = expect(lib, fq, n, **run)
        assert e[1][1] > 40 and (e[1][3] > 10 or name == "l1_m1") and sum(e[2][1:]) > 20, (name, e[1], e[2])
    lib, fq, run, n = mixed_lengths()
    clipped = [(s, x) for (s, q), x in zip(UC.records(fq), per_read(lib, fq, n, **run)) if x[0] >= 0 and len(s) < S + x[3] + 22]
    assert sum(1 for s, x in clipped if x[1] == 1) >= 30 and sum(1 for s, x in clipped if x[1] == 2) >= 10      # a clipped window reads a shorter feature
    assert {len(lib[x[0]]) for s, x in clipped} == {18, 20}
    assert any("N" in f for f in with_n_feature()[0])
    for name in ("odd0", "odd1", "odd2"):
        lib, fq, run, n = CASES[name]()
        recs = UC.records(fq)
        assert len(recs) >= 999
        assert any(s[:1] in b" \t" and s for s, q in recs) and any(q[:1] in b" \t" and q for s, q in recs)
        assert any(len(q) < len(s) for s, q in recs) and any(len(q) > len(s) for s, q in recs)
        assert any(0 < len(s) < 20 for s, q in recs) and any(not s for s, q in recs) and any(not q for s, q in recs)
        assert b"\r\n" in fq and any(c in s for s, q in recs for c in b"acgt") and any(b"N" in s for s, q in recs)
        e = expect(lib, fq, n, **run)
        assert sum(e[2][1:]) > 100 and sum(e[3][1:]) > 30 and e[1][3] > 30 and e[1][4] > 10, (e[1], e[2], e[3])
    cells = set()
    for r in RE.EDGE_R:
        lib, fq, run, n = edge(r)
        here = RE.device_cells(fq)
        assert {RE.staged(c) for c in here} == {True, False}
        cells |= here
        e = expect(lib, fq, n, **run)
        assert e[2][N] > 50 and e[3][N] > 50 and e[1][4] > 30, (r, e[1], e[2], e[3])
    assert any(c[2] <= RE.STAGE < c[3] for c in cells) and any(c[3] <= RE.STAGE < c[2] for c in cells)
    assert {(c[0], c[1], c[2], c[3]) for c in cells if c[2] in RE.SUMS and c[3] in RE.SUMS} == \
        {(ms, mq, a, b) for ms in range(4) for mq in range(4) for a in RE.SUMS for b in RE.SUMS}
    for name in ("long_reads", "pass_pool"):
        lib, fq, run, n = CASES[name]()
        e = expect(lib, fq, n, **run)
        assert sum(e[2][1:]) > 40 and sum(e[3][1:]) > 10 and e[1][3] > 10 and e[1][4] > 5, (name, e[1], e[2], e[3])


def _lowq_blocks(lib, fq, n, **run):
    """reads with a start d > 0 that fails the Phred test, passes it at 0, and whose window at d a run without the Phred test
    (--ph 1) assigns"""
    free = dict(run, phred=1)
    count = 0
    for seq, qual in UC.records(fq):
        v, w = V(lib, run, seq, qual), V(lib, free, seq, qual)
        count += v(0)[2] == 0 and any(v(d)[2] == 1 and w(d)[0] >= 0 for d in range(1, n + 1))
    return count
