"""tests/indel_cases.py -- inputs and expected values shared by the --indel tests (CPU emulation and GPU).

The expectation is plain Python: V0 is umi_cases._verdicts (the oracle in Counter mode, once per distinct record text);
indel_verdict restates the function of include/f2q.h (f2q_set_indel) over a dict of the candidates' deletion variants, and
is the only rule stated here.  Framing is umi_cases.records: four rstrip()-ed lines per record."""
import functools
import random

import raw_edge_cases as RE
import synth
import umi_cases as UC

S, L = 2, 20                                    # the base shape: --st 2 --l 20
RUN = dict(start=str(S), length=L, phred=30)


# ---- the rule ------------------------------------------------------------------------------------------------------------
def passes(q, phred):
    """the Phred test of a feature window: umi_cases.umi_of's fail set; --ph <= 1 never fails"""
    ph = max(int(phred), 1)
    return not any(33 <= c <= min(ph + 31, 126) for c in q)


@functools.lru_cache(maxsize=None)
def candidates(lib, length):
    """({sequence: first index} of the features of exactly `length` bases, all A/C/G/T,
    {variant: {feature: smallest removed position}} without the variants equal to the feature's own first length - 1 bases)"""
    cand, variants = {}, {}
    for i, f in enumerate(lib):
        f = f.encode()
        if len(f) == length and not set(f) - set(b"ACGT"):
            cand.setdefault(f, i)
    for f, i in cand.items():
        for p in range(length):
            v = f[:p] + f[p + 1:]
            if v == f[:length - 1]:
                continue
            variants.setdefault(v, {}).setdefault(i, p)
    return cand, variants


def indel_verdict(v0, seq, qual, s, length, cand, variants, phred):
    """-> None (no indel read), "ambiguous", or (kind, feature, position)"""
    if v0[1] in (1, 2):                              # a substitution match is never re-examined
        return None
    d, i = {}, {}
    wd, qd = seq[s:s + length - 1].upper(), qual[s:s + length - 1]
    if len(wd) == length - 1 and len(qd) == length - 1 and passes(qd, phred):
        d = dict(variants.get(wd, {}))
    wi, qi = seq[s:s + length + 1].upper(), qual[s:s + length + 1]
    if len(wi) == length + 1 and len(qi) == length + 1 and passes(qi, phred):
        assert wi[:length] not in cand                   # p == L cannot occur: the plain window would have been exact
        for p in range(length):
            f = cand.get(wi[:p] + wi[p + 1:])
            if f is not None:
                i.setdefault(f, p)
    both = set(d) | set(i)
    if len(both) >= 2:
        return "ambiguous"
    for f in both:
        return ("ins", f, i[f]) if f in i else ("del", f, d[f])
    return None


def per_read(lib, fq, **run):
    """[(v0, verdict)] of the records of the text; v0 = (feature or -1, counter, quality_failed)"""
    s, length, phred = int(run["start"]), int(run["length"]), int(run.get("phred", 30))
    cand, variants = candidates(tuple(lib), length)
    of = UC._verdicts(tuple(lib), UC.run_key(run)).of
    out = []
    for seq, qual in UC.records(fq):
        v0 = of(seq, qual)
        out.append((v0, indel_verdict(v0, seq, qual, s, length, cand, variants, phred)))
    return out


def expect(lib, fq, **run):
    """(counts, stats, del_counts, ins_counts, del_pos[L], ins_pos[L], totals[4]) of the FASTQ bytes, as lists"""
    length = int(run["length"])
    counts, stats = [0] * len(lib), [0] * 5
    per = ([0] * len(lib), [0] * len(lib))
    pos = ([0] * length, [0] * length)
    totals = [0] * 4
    for (f, which, qfail), verdict in per_read(lib, fq, **run):
        stats[0] += 1
        stats[4] += qfail
        if which:
            stats[which] += 1
        if f >= 0:
            counts[f] += 1
            continue
        totals[0] += 1
        if verdict == "ambiguous":
            totals[3] += 1
        elif verdict is not None:
            k = ("del", "ins").index(verdict[0])
            per[k][verdict[1]] += 1
            pos[k][verdict[2]] += 1
            totals[1 + k] += 1
    return counts, stats, per[0], per[1], pos[0], pos[1], totals


def check_invariants(counts, stats, dels, inss, del_pos, ins_pos, totals):
    """the invariants of include/f2q.h (f2q_read_indels)"""
    assert sum(dels) == sum(del_pos) == totals[1] and sum(inss) == sum(ins_pos) == totals[2]
    assert totals[0] == stats[3] + stats[4] and totals[1] + totals[2] + totals[3] <= totals[0]
    assert sum(counts) == stats[1] + stats[2] and stats[1] + stats[2] + stats[3] + stats[4] == stats[0]


def pieces(fq, per):
    """the text cut into blocks of `per` whole records"""
    lines = fq.split(b"\n")
    assert lines.pop() == b"" and len(lines) % 4 == 0
    return [b"\n".join(lines[i:i + 4 * per]) + b"\n" for i in range(0, len(lines), 4 * per)]


def delete(g, p):
    return g[:p] + g[p + 1:]


def insert(g, p, b):
    """the L + 1 bases that give g back when base p leaves them"""
    return g[:p] + bytes([b]) + g[p:]


# ---- 1: the base shape ---------------------------------------------------------------------------------------------------
N_PAIR = 8                                      # pairs of features one substitution apart
N_CROSS = 8                                     # features g that a deletion read of another feature is an insertion read of
N_TAIL = 8                                      # features whose last bases alternate: one read is a deletion AND an insertion of them
HOMO = "A" * 20
N_FEATURE = "ACGTNACGTACGTTGCATGC"


@functools.lru_cache(maxsize=None)
def base_library():
    """600 guides of 20 bases, then the constructed features; -> (library, pairs, cross, tails)"""
    rng = random.Random(0x1DE1)
    lib = UC.library()
    extra, pairs, cross, tails = [], [], [], []
    for i in range(N_PAIR):                                          # a, b differ at position k: deleting it leaves the same 19 bases
        a = UC.rand_seq(rng, 20)
        k = 1 + 2 * i
        b = UC.mutate1(rng, a, k, k + 1)
        extra += [a.decode(), b.decode()]
        pairs.append((a, b, k))
    for i in range(N_CROSS):                                         # the read f - p, x, y is an insertion read of g = (f - p + x + y) - q
        f = lib[100 + i].encode()
        p, q = 2 + i, 11 - i
        wi = delete(f, p) + UC.rand_seq(rng, 2)
        g = delete(wi, q)
        extra.append(g.decode())
        cross.append((f, p, wi, g, q))
    for i in range(N_TAIL):                                          # f[q - 1:] alternates two bases: inserting f[q - 1] at q - 1 is deleting base q
        q = 6 + i
        x, y = (b"AC", b"GT", b"CA", b"TG")[i % 4]
        head = UC.rand_seq(rng, q - 2) + bytes([rng.choice([c for c in b"ACGT" if c not in (x, y)])])
        f = head + bytes((x, y)[j % 2] for j in range(21 - q))
        assert len(f) == 20
        extra.append(f.decode())
        tails.append((f, q))
    extra += [HOMO, N_FEATURE] + synth.make_library(6, 18, 0x18) + synth.make_library(6, 22, 0x22)
    assert len(set(lib + extra)) == len(lib) + len(extra)
    return lib + extra, pairs, cross, tails


@functools.lru_cache(maxsize=None)
def base(seed=0x1DE15):
    """~1 500 reads of 60 bases, --st 2 --l 20.  -> (library, text, run, tags): tags[i] names how record i was made"""
    rng = random.Random(seed)
    lib, pairs, cross, tails = base_library()
    guides = [g.encode() for g in lib[:600]]
    q60 = b"I" * 60
    recs = []

    def place(window, tag, q=q60, n=60):
        seq = UC.rand_seq(rng, S) + window + UC.rand_seq(rng, max(n - S - len(window), 0))
        recs.append((seq[:n], q[:n], tag))

    def other(c):
        return rng.choice([x for x in b"ACGT" if x != c])
    spec = synth.Spec(seed=seed, n_reads=1, read_len=60, start=S, p_lowq=0.10)
    for i in range(420):                                             # exact, substituted, random and 'N' windows, a low-quality share
        recs.append(synth.make_read(spec, lib[:600], i) + ("synth",))
    for i in range(40):                                              # nothing anywhere
        place(UC.rand_seq(rng, 22), "random")
    for i in range(170):                                             # a deletion at every position; 30 more of the last base, which is excluded
        g = guides[rng.randrange(600)]
        place(delete(g, min(i, 139) % 20), "del%d" % (min(i, 139) % 20))
    for i in range(120):                                             # an insertion at every position, 19 included
        g = guides[rng.randrange(600)]
        p = i % 20
        place(insert(g, p, other(g[p])), "ins%d" % p)
    runs = [(g, p) for g in guides for p in range(1, 18) if g[p] == g[p - 1]]
    for i in range(40):                                              # the second base of a run of equal bases leaves: the smallest p is reported
        g, p = runs[rng.randrange(len(runs))]
        place(delete(g, p), "del_run")
    for i in range(40):                                              # a base is doubled
        g, p = runs[rng.randrange(len(runs))]
        place(insert(g, p, g[p]), "ins_run")
    for i in range(40):                                              # a and b share the variant
        a, b, k = pairs[i % N_PAIR]
        place(delete(b if i % 2 else a, k), "shared_variant")
    for i in range(40):                                              # a deletion of f and an insertion of g
        f, p, wi, g, q = cross[i % N_CROSS]
        place(wi, "across_kinds")
    for i in range(40):                                              # both a deletion and an insertion of the same feature: ins
        f, q = tails[i % N_TAIL]
        place(insert(f, q - 1, f[q - 1]), "del_and_ins")
    for i in range(40):                                              # the homopolymer: every variant is its own first 19 bases
        place(HOMO.encode()[:19] + bytes([rng.choice(b"CGT"), rng.choice(b"CGT")]), "homopolymer")
    for i in range(100):                                             # an indel so near the 3' end that the plain rule reads substitutions:
        g = guides[rng.randrange(600)]
        if i % 2:
            place(insert(g, 19, other(g[19])), "late_ins")           # one of them: --m 1 and --m 2 take the read
        else:
            place(delete(g, 18) + bytes([other(g[19])]), "late_del") # two of them: --m 2 takes it, --m 1 reports the deletion
    for i in range(240):                                             # a low quality byte: at s + L - 1, at s + L, inside both windows
        g = guides[rng.randrange(600)]
        p = rng.randrange(16)
        window = delete(g, p) if i % 2 else insert(g, p, other(g[p]))
        q = bytearray(q60)
        where = ("last", "past", "inside")[(i // 2) % 3]
        q[{"last": S + L - 1, "past": S + L, "inside": S + rng.randrange(L - 1)}[where]] = ord("#")
        place(window, ("lowq_%s_" % where) + ("del" if i % 2 else "ins"), bytes(q))
    for i in range(120):                                             # the quality line, or the whole read, ends before s + L + 1
        g = guides[rng.randrange(600)]
        p = rng.randrange(16)
        window = delete(g, p) if i % 3 else insert(g, p, other(g[p]))
        n = S + L - (i % 2)
        if i % 4 < 2:
            place(window, "short_qual_" + ("del" if i % 3 else "ins"), q60[:n])
        else:
            place(window, "short_read_" + ("del" if i % 3 else "ins"), n=n)
    for i in range(80):                                              # lower case
        g = guides[rng.randrange(600)]
        p = rng.randrange(16)
        window = delete(g, p) if i % 2 else insert(g, p, other(g[p]))
        place(window.lower() if i % 4 < 2 else window[:5] + window[5:9].lower() + window[9:], "lower_" + ("del" if i % 2 else "ins"))
    for i in range(120):                                             # the inserted base is an 'N'; an 'N' elsewhere
        g = guides[rng.randrange(600)]
        p = rng.randrange(16)
        if i % 3 == 0:
            place(insert(g, p, ord("N")), "n_inserted")
        else:
            w = bytearray(delete(g, p) if i % 3 == 1 else insert(g, p, other(g[p])))
            w[(p + 1 + rng.randrange(3)) % 19] = ord("N")
            place(bytes(w), "n_elsewhere")
    for i in range(40):                                              # the feature with an 'N' without it: 19 plain bases, but it is no candidate
        place(N_FEATURE.replace("N", "").encode() + UC.rand_seq(rng, 2), "n_feature")
    order = list(range(len(recs)))
    rng.shuffle(order)
    recs = [recs[i] for i in order]
    return lib, UC.fastq_of([(s, q) for s, q, _ in recs]), dict(RUN), tuple(t for _, _, t in recs)


def by_tag(lib, fq, tags, **run):
    """{tag: [(v0, verdict)]}"""
    out = {}
    for tag, got in zip(tags, per_read(lib, fq, **run)):
        out.setdefault(tag, []).append(got)
    return out


# ---- 2: the extremes -------------------------------------------------------------------------------------------------------
def _edited(rng, lib, n_reads, s, length, read_len):
    """reads with a feature of the library at s: one base deleted or inserted at a position that walks over the feature, exact,
    one base off, or random; a low quality byte in a tenth; an 'N' and lower case in a few"""
    recs = []
    for i in range(n_reads):
        g = lib[rng.randrange(len(lib))].encode()
        p = len(g) - 1 if i % 7 == 3 else i % len(g)                 # (the last position more often than the others)
        roll = rng.random()
        if roll < 0.3:
            w = delete(g, p)
        elif roll < 0.6:
            w = insert(g, p, rng.choice(b"ACGT"))
        elif roll < 0.75:
            w = g
        elif roll < 0.85 and len(g) > 1:
            w = UC.mutate1(rng, g)
        else:
            w = UC.rand_seq(rng, len(g))
        w = bytearray(w)
        if rng.random() < 0.05:
            w[rng.randrange(len(w))] = ord("N")
        if rng.random() < 0.05:
            w = bytearray(bytes(w).lower())
        seq = UC.rand_seq(rng, s) + bytes(w) + UC.rand_seq(rng, max(read_len - s - len(w), 0))
        q = bytearray(b"I" * len(seq))
        if rng.random() < 0.12:
            q[min(s + rng.randrange(length + 2), len(q) - 1)] = ord("#")
        recs.append((seq, bytes(q)))
    return UC.fastq_of(recs)


@functools.lru_cache(maxsize=None)
def extreme(name):
    """-> (library, text, run)"""
    rng = random.Random(0x1DE + sum(name.encode()))
    if name == "l2":                                                 # one base of evidence for a deletion, three for an insertion
        lib = ["AC", "GT", "TA", "CC"]
        recs = []
        for i in range(300):
            seq = bytearray(rng.choice(b"ACGT") for _ in range(rng.choice((3, 4, 5, 8))))
            if rng.random() < 0.1:
                seq[rng.randrange(len(seq))] = rng.choice(b"Na")
            q = bytearray(b"I" * len(seq))
            if rng.random() < 0.2:
                q[rng.randrange(len(q))] = ord("#")
            recs.append((bytes(seq), bytes(q)))
        return lib, UC.fastq_of(recs), dict(start="1", length=2, phred=30, miss=0)
    if name in ("l31", "l30"):                                       # L = 31: the word of 32 bases is full, the insertion lands at p = 30
        length = int(name[1:])
        lib = synth.make_library(150, length, 0x31 + length)
        return lib, _edited(rng, lib, 330, 3, length, 100), dict(start="3", length=length, phred=30, miss=int(name == "l30"))
    if name == "st0":
        lib = UC.library()
        return lib, _edited(rng, lib, 300, 0, 20, 60), dict(start="0", length=20, phred=30, miss=1)
    raise KeyError(name)


EXTREMES = ("l2", "l31", "l30", "st0")


# ---- 3: odd records --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def odd(seed):
    """1 000 records with an edited feature at --st 2, through raw_edge_cases' oddities (CRLF, trailing blanks, quality lines
    of another length, reads that end inside a window, lower case, 'N' and other bytes, odd quality bytes, empty lines, a
    partial last record, no final newline) plus a leading blank in either line.  -> (library, text, run)"""
    rng = random.Random(0x0DD1DE + seed)
    lib = UC.library()
    recs = []
    for i in range(1000):
        g = lib[rng.randrange(len(lib))].encode()
        roll = rng.random()
        p = rng.randrange(20)
        w = delete(g, p) if roll < 0.35 else insert(g, p, rng.choice(b"ACGT")) if roll < 0.7 else UC.mutate1(rng, g) if roll < 0.8 else g
        n = rng.choice((23, 24, 40, 60, 61, 62, 63, 150))
        s, q = bytearray((UC.rand_seq(rng, S) + w + UC.rand_seq(rng, max(n - S - len(w), 0)))[:n]), bytearray(b"I" * n)
        if rng.random() < 0.6:
            RE._spoil(rng, s, q, ((S, S + L - 1), (S, S + L + 1), (S + L - 2, S + L + 2)))
        if rng.random() < 0.08:
            s[:0] = rng.choice(RE.BLANKS)
        if rng.random() < 0.08:
            q[:0] = rng.choice(RE.BLANKS)
        recs.append((b"@o%d" % i, bytes(s), bytes(q)))
    fq, = RE._finish(rng, [RE._text(rng, recs)])
    return lib, fq, dict(RUN, miss=1)


# ---- 4: the staging edge ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge(r):
    """raw_edge_cases.edge_sample(r): a feature ends the read, so with --st r-21 the insertion window ends there too and the
    long records are insertion reads at position 0, on both sides of the 192-byte limit.  -> (library, text, run)"""
    lib, _, fq, _ = RE.edge_sample(r, 0, False)
    return lib, fq, dict(start=str(r - 21), length=20, phred=RE.PH, miss=1)


# ---- 5: long reads ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_reads():
    """400 reads of 250 bases (read where they lie in global memory) among 400 of 60 bases"""
    rng = random.Random(0x10A1DE)
    lib = UC.library()
    a, b = _edited(rng, lib, 400, S, L, 250), _edited(rng, lib, 400, S, L, 60)
    return lib, b"".join(x + y for x, y in zip(pieces(a, 1), pieces(b, 1))), dict(RUN, miss=1)


# ---- 6: a second trip through the grid-stride loop -------------------------------------------------------------------------
POOL = RE.POOL


@functools.lru_cache(maxsize=None)
def pass_pool():
    """257 distinct records of 40 bases, one in eight 190 (a short record is staged over a long one's bytes in the lane's
    second pass), an edited feature at --st 2"""
    rng = random.Random(0x2FA1DE)
    lib = UC.library()
    recs = []
    for i in range(POOL):
        g = lib[rng.randrange(40)].encode()
        roll = rng.random()
        p = rng.randrange(19)
        w = delete(g, p) if roll < 0.35 else insert(g, p, rng.choice(b"ACGT")) if roll < 0.7 else UC.rand_seq(rng, 20) if roll < 0.8 else g
        n = 190 if i % 8 == 3 else 40
        q = bytearray(b"I" * n)
        if rng.random() < 0.1:
            q[S + rng.randrange(L + 2)] = ord("#")
        recs.append((UC.rand_seq(rng, S) + w + UC.rand_seq(rng, n - S - len(w)), bytes(q)))
    assert len(set(recs)) == POOL
    return UC.fastq_of(recs)


def second_pass(n_cu):
    """-> (FASTQ bytes, repetitions), as raw_edge_cases.second_pass: more records than the lanes of a capped launch"""
    reps = -(-(n_cu * 4096 + 3 * POOL) // POOL)
    return pass_pool() * reps, reps


def scaled(e, k):
    return tuple([x * k for x in part] for part in e)


# the cases of the list by name: -> (library, text, run)
CASES = {"base": lambda: base()[:3], "odd0": lambda: odd(0), "odd1": lambda: odd(1), "odd2": lambda: odd(2), "long_reads": long_reads,
         "pass_pool": lambda: (UC.library(), pass_pool(), dict(RUN, miss=1))}
CASES.update({name: (lambda name=name: extreme(name)) for name in EXTREMES})
CASES.update({f"edge{r}": (lambda r=r: edge(r)) for r in RE.EDGE_R})


def check_coverage():
    """what the cases claim, from the expectation alone: every class has at least 30 reads"""
    lib, fq, run, tags = base()
    assert 1400 <= len(tags) <= 1700 and len(UC.records(fq)) == len(tags)
    assert any("N" in f for f in lib) and {len(f) for f in lib} == {18, 20, 22}
    cand, variants = candidates(tuple(lib), L)
    assert len(cand) == sum(len(f) == 20 and "N" not in f for f in lib) and lib.index(N_FEATURE) not in cand.values()
    assert not any(lib.index(HOMO) in v for v in variants.values())                      # all of the homopolymer's variants are excluded
    assert sum(len(v) > 1 for v in variants.values()) >= N_PAIR
    m0, m1, m2 = (by_tag(lib, fq, tags, miss=m, **run) for m in (0, 1, 2))

    def count(rows, test):
        return sum(1 for v0, verdict in rows if test(v0, verdict))

    def kind(verdict):
        return verdict[0] if isinstance(verdict, tuple) else verdict
    # the synth reads: every plain verdict, and unassigned reads the trial gives nothing
    for which in (1, 2):
        assert count(m1["synth"], lambda v0, v: v0[1] == which) >= 30
    assert count(m1["synth"], lambda v0, v: v0[2] == 1) >= 30 and count(m1["synth"] + m1["random"], lambda v0, v: v0[1] == 3 and v is None) >= 30
    # a deletion and an insertion at every position; the deletion of the last base is excluded, the insertion at 19 is reported at --m 0
    dels = [v for t in m0 if t.startswith("del") and t[3:].isdigit() for _, v in m0[t]]
    inss = [v for t in m0 if t.startswith("ins") and t[3:].isdigit() for _, v in m0[t]]
    assert {v[2] for v in dels if kind(v) == "del"} == set(range(19)) and sum(kind(v) == "del" for v in dels) >= 100
    assert {v[2] for v in inss if kind(v) == "ins"} == set(range(20)) and sum(kind(v) == "ins" for v in inss) >= 100
    assert not any(kind(v) == "del" for _, v in m0["del19"]) and len(m0["del19"]) >= 30
    assert count(m0["late_ins"] + m0["ins19"], lambda v0, v: kind(v) == "ins" and v[2] == 19) >= 30
    # ... and --m 1 / --m 2 take those reads as substitutions: they are not reported
    for rows in (m1, m2):
        assert count(rows["late_ins"] + rows["ins19"], lambda v0, v: v0[1] == 2 and v is None) >= 30
    assert count(m2["late_del"], lambda v0, v: v0[1] == 2 and v is None) >= 30
    assert count(m1["late_del"], lambda v0, v: v0[0] < 0 and kind(v) == "del" and v[2] >= 15) >= 30
    # runs of equal bases: the smallest position, which is not the one the read was made with
    for tag, k in (("del_run", "del"), ("ins_run", "ins")):
        assert count(m1[tag], lambda v0, v: kind(v) == k) >= 30
    # ambiguous reads: a shared variant, and a deletion of one feature that is an insertion of another
    for tag in ("shared_variant", "across_kinds"):
        assert count(m1[tag], lambda v0, v: v == "ambiguous") >= 30, tag
    # both a deletion and an insertion of the same feature: ins
    both = 0
    for (seq, qual), tag, (v0, v) in zip(UC.records(fq), tags, per_read(lib, fq, miss=1, **run)):
        if tag == "del_and_ins":
            both += kind(v) == "ins" and v[1] in variants.get(seq[S:S + L - 1].upper(), {})
    assert both >= 30
    assert count(m0["homopolymer"], lambda v0, v: v0[0] < 0 and v is None) >= 30
    # a low quality byte at s + L - 1 (V0 quality failed, the deletion window passes), at s + L (the insertion window alone
    # fails) and inside both windows
    assert count(m1["lowq_last_del"], lambda v0, v: v0[2] == 1 and kind(v) == "del") >= 30
    assert count(m1["lowq_past_del"], lambda v0, v: v0[2] == 0 and kind(v) == "del") >= 30
    assert count(m1["lowq_past_ins"], lambda v0, v: v0[2] == 0 and v0[0] < 0 and v is None) >= 30
    assert count(m1["lowq_inside_del"] + m1["lowq_inside_ins"], lambda v0, v: v0[2] == 1 and v is None) >= 60
    assert count(m1["lowq_last_ins"], lambda v0, v: v0[2] == 1 and v is None) >= 30
    # a quality line, or a read, that ends before s + L + 1: only the deletion trial is made
    for tag in ("short_qual", "short_read"):
        assert count(m1[tag + "_del"], lambda v0, v: kind(v) == "del") >= 30 and count(m1[tag + "_ins"], lambda v0, v: v is None) >= 15, tag
    assert count(m1["lower_del"], lambda v0, v: kind(v) == "del") + count(m1["lower_ins"], lambda v0, v: kind(v) == "ins") >= 60
    assert count(m1["n_inserted"], lambda v0, v: kind(v) == "ins") >= 30 and count(m1["n_elsewhere"], lambda v0, v: v is None and v0[0] < 0) >= 60
    assert count(m1["n_feature"], lambda v0, v: v is None and v0[0] < 0) >= 30
    # the extremes
    e = expect(*extreme("l31")[:2], **extreme("l31")[2])
    assert e[5][30] >= 5 and sum(e[4][25:]) >= 5 and sum(e[4]) >= 40 and sum(e[5]) >= 40, (e[4], e[5])
    for name in EXTREMES:
        lib_, fq_, run_ = extreme(name)
        assert 290 <= len(UC.records(fq_)) <= 340
        e = expect(lib_, fq_, **run_)
        assert e[6][1] >= 10 and e[6][2] >= 10 and e[6][0] > e[6][1] + e[6][2], (name, e[6])
        assert e[6][3] >= 10 or name != "l2", (name, e[6])
    for name in ("odd0", "odd1", "odd2"):
        lib_, fq_, run_ = CASES[name]()
        recs = UC.records(fq_)
        assert len(recs) >= 999
        assert any(s[:1] in b" \t" and s for s, q in recs) and any(q[:1] in b" \t" and q for s, q in recs)
        assert any(len(q) < len(s) for s, q in recs) and any(len(q) > len(s) for s, q in recs)
        assert any(0 < len(s) < 20 for s, q in recs) and any(not s for s, q in recs) and any(not q for s, q in recs)
        assert b"\r\n" in fq_ and any(c in s for s, q in recs for c in b"acgt") and any(b"N" in s for s, q in recs)
        e = expect(lib_, fq_, **run_)
        assert e[6][1] > 100 and e[6][2] > 100 and e[1][4] > 10, (e[1], e[6])
    cells = set()
    for r in RE.EDGE_R:
        lib_, fq_, run_ = edge(r)
        here = RE.device_cells(fq_)
        assert {RE.staged(c) for c in here} == {True, False}
        cells |= here
        e = expect(lib_, fq_, **run_)
        assert e[5][0] >= 15 and e[6][2] == e[5][0] and e[6][0] > 300 and e[1][4] > 30, (r, e[1], e[6])
    assert any(c[2] <= RE.STAGE < c[3] for c in cells) and any(c[3] <= RE.STAGE < c[2] for c in cells)
    assert {(c[0], c[1], c[2], c[3]) for c in cells if c[2] in RE.SUMS and c[3] in RE.SUMS} == \
        {(ms, mq, a, b) for ms in range(4) for mq in range(4) for a in RE.SUMS for b in RE.SUMS}
    for name in ("long_reads", "pass_pool"):
        lib_, fq_, run_ = CASES[name]()
        e = expect(lib_, fq_, **run_)
        assert e[6][1] > 40 and e[6][2] > 40 and e[1][4] > 5, (name, e[1], e[6])
