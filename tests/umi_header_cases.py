"""tests/umi_header_cases.py -- inputs and expected values shared by the --umih tests (UMIs in read headers;
f2q_set_umi_header), CPU emulation and GPU.

The expectation is plain Python: 4-line framing with rstrip() as the reference frames; the feature of each read from
umi_cases._verdicts (the oracle in Counter mode, once per distinct record text); the UMI from the record's header line by
header_umi() below, the restatement of the rule in include/f2q.h; per feature the reads of every UMI."""
import collections
import functools
import random

import umi_cases as UC
import umi_collapse_cases as CC

SEP, L = ord("_"), 8                           # the base shape: @r<i>_<UMI>


def header_umi(header_line, sep, L):           # bytes, int (one byte), int -> bytes or None
    h = header_line.rstrip()                   # the record's line 0, rstrip()-ed as the other three are
    for i, c in enumerate(h):
        if c in b" \t":
            h = h[:i]                          # the read id: up to the first space or tab
            break
    k = h.rfind(bytes([sep]))
    if k < 0:
        return None                            # no separator in the id
    tail = h[k + 1:]
    if tail.count(b"+") > 1:
        return None                            # at most one '+' (dual UMI) is skipped, wherever it stands
    tail = tail.replace(b"+", b"")
    if len(tail) != L or set(tail.upper()) - set(b"ACGT"):
        return None
    return tail.upper()                        # lower case counts, as for --umi; N makes it invalid


def code_of(u):
    """the 2-bit codes of a UMI, base j in bits 2j .. 2j+1"""
    return sum(b"ACGT".index(ch) << (2 * j) for j, ch in enumerate(u))


def entry_of(header_line, sep, L):
    """what the ingest array holds for a record: the codes with the validity mark above their 32 bits, 0 for an invalid one"""
    u = header_umi(header_line, sep, L)
    return 0 if u is None else (1 << 32) | code_of(u)


def records(fq):
    """[(header line as it stands, sequence line, quality line)] of the complete records; the last two rstrip()ped"""
    lines = fq.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [(lines[i], lines[i + 1].rstrip(), lines[i + 3].rstrip()) for i in range(0, len(lines) - 3, 4)]


def fastq_of(recs, eol=b"\n"):
    """recs: (header line without its end, sequence, quality)"""
    return b"".join(h + eol + s + eol + b"+" + eol + q + eol for h, s, q in recs)


Expected = collections.namedtuple("Expected", "counts stats per ok bad")


def expect(lib, fq, umi, **run):
    """umi = (separator, bases): counts, the five counters, per feature {UMI: reads} in first-seen order, assigned reads
    with a valid / an invalid UMI"""
    v = UC._verdicts(tuple(lib), UC.run_key(run))
    counts, stats = [0] * len(lib), [0] * 5
    per = [collections.OrderedDict() for _ in lib]
    ok = bad = 0
    for head, seq, qual in records(fq):
        f, verdict, qfail = v.of(seq, qual)
        stats[0] += 1
        stats[4] += qfail
        if verdict:
            stats[verdict] += 1
        if f >= 0:
            counts[f] += 1
            u = header_umi(head, umi[0], umi[1])
            if u is None:
                bad += 1
            else:
                ok += 1
                per[f][u] = per[f].get(u, 0) + 1
    return Expected(counts, stats, per, ok, bad)


def wanted(e):
    """what (read_counts, read_umis) give: counts, stats, umis, valid, invalid"""
    return e.counts, e.stats, [len(c) for c in e.per], e.ok, e.bad


def table_of(e):
    """[(feature, codes, reads)] sorted by (feature, codes): what f2q_umi_pairs returns"""
    return sorted((f, code_of(u), n) for f, c in enumerate(e.per) for u, n in c.items())


def cluster_of(e):
    """(molecules per feature, pairs, edges) by umi_collapse_cases.components"""
    per = [CC.components(set(c)) for c in e.per]
    return [m for m, _ in per], sum(len(c) for c in e.per), sum(x for _, x in per)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def reheaded(fq, header_of):
    """the records of a FASTQ of umi_cases with header i replaced by header_of(i, sequence, quality)"""
    return fastq_of([(header_of(i, s, q), s, q) for i, (s, q) in enumerate(UC.records(fq))])


@functools.lru_cache(maxsize=None)
def base(seed=0x0B5E):
    """umi_cases.base()'s library and reads (600 guides x 20 bp, 4 000 reads of 60 bp, --st 0 --l 20), the headers
    @r<i>_<UMI> with UMIs from a pool of 48"""
    lib, fq, run, _ = UC.base(seed)
    rng = random.Random(seed ^ 0x4844)
    pool = [UC.rand_seq(rng, L) for _ in range(48)]
    return lib, reheaded(fq, lambda i, s, q: b"@r%d_%s" % (i, pool[rng.randrange(48)])), dict(run), (SEP, L)


# kind -> is the UMI valid.  `u` is a distinct 8-base UMI per read, i the read's number
INVALID_KINDS = collections.OrderedDict([
    ("whole", True), ("no_sep", False), ("sep_in_comment", False), ("short", False), ("long", False), ("empty_tail", False),
    ("N", False), ("lower", True), ("dual", True), ("two_plus", False), ("lead_plus", True), ("tab_comment", True),
    ("crlf", True), ("one_byte", False), ("illumina", True), ("illumina_dual_comment", True), ("last_sep_wins", True),
    ("trailing_blanks", True)])


def invalid_header(kind, i, u):
    """the header line (with a '\\r' where the kind asks for it), and the separator it is read with"""
    return {
        "whole": (b"@r%d_%s" % (i, u), SEP),
        "no_sep": (b"@r%d%s" % (i, u), SEP),
        "sep_in_comment": (b"@r%d 1:N:0:1_%s" % (i, u), SEP),
        "short": (b"@r%d_%s" % (i, u[:L - 1]), SEP),
        "long": (b"@r%d_%sA" % (i, u), SEP),
        "empty_tail": (b"@r%d_" % i, SEP),
        "N": (b"@r%d_%sN%s" % (i, u[:3], u[4:]), SEP),
        "lower": (b"@r%d_%s" % (i, u[:2] + u[2:5].lower() + u[5:]), SEP),
        "dual": (b"@r%d_%s+%s" % (i, u[:4], u[4:]), SEP),
        "two_plus": (b"@r%d_%s+%s+%s" % (i, u[:2], u[2:5], u[5:]), SEP),
        "lead_plus": (b"@r%d_+%s" % (i, u), SEP),
        "tab_comment": (b"@r%d_%s\t1:N:0:ACGT_TTTTTTTT" % (i, u), SEP),
        "crlf": (b"@r%d_%s\r" % (i, u), SEP),
        "one_byte": (b"@", SEP),
        "illumina": (b"@M0:7:FC:1:1101:%d:200:%s 1:N:0:ATCACG" % (i, u), ord(":")),
        "illumina_dual_comment": (b"@M0:7:FC:1:1101:%d:200:%s+%s 2:N:0:ATCACG+TTGACA" % (i, u[:4], u[4:]), ord(":")),
        "last_sep_wins": (b"@r_%d_ACGTACGT_%s" % (i, u), SEP),
        "trailing_blanks": (b"@r%d_%s \t " % (i, u), SEP),
    }[kind]


@functools.lru_cache(maxsize=None)
def invalid():
    """per kind 12 reads of one feature each (the window whole and clean, quality 'I'), every UMI distinct:
    {kind: (FASTQ, separator)}; the crlf kind ends all four lines in \\r\\n"""
    rng = random.Random(177)
    lib = UC.library()
    out, seen, n = collections.OrderedDict(), set(), 0
    for kind in INVALID_KINDS:
        recs, sep = [], SEP
        for _ in range(12):
            u = UC.rand_seq(rng, L)
            while u in seen:
                u = UC.rand_seq(rng, L)
            seen.add(u)
            head, sep = invalid_header(kind, n, u)
            n += 1
            recs.append((head.rstrip(b"\r") if kind == "crlf" else head, lib[rng.randrange(len(lib))].encode() + UC.rand_seq(rng, 40), b"I" * 60))
        out[kind] = (fastq_of(recs, b"\r\n" if kind == "crlf" else b"\n"), sep)
    return lib, out


def random_headers(seed, n, sep=SEP, length=L):
    """seeded header lines built from the pieces of invalid_header plus random printable bytes, cut and glued at random"""
    rng = random.Random(seed)
    printable = bytes(range(32, 127)) + b"\t\r"
    kinds = list(INVALID_KINDS)
    out = []
    for i in range(n):
        u = UC.rand_seq(rng, rng.choice([length, length, length, length - 1, length + 1, 0, 16]))
        roll = rng.random()
        if roll < 0.5:
            h = invalid_header(rng.choice(kinds), i, (u + b"ACGTACGTACGTACGT")[:max(length, 8)])[0]
            if sep != SEP:
                h = h.replace(b"_", bytes([sep]))
        elif roll < 0.8:
            pieces = [b"@r%d" % i, bytes([sep]), u, b"+", b" ", b"\t", b"N", b"acgt", b"\r", bytes([sep]) + u, b"1:N:0:1", b":"]
            h = b"".join(rng.choice(pieces) for _ in range(rng.randrange(1, 7)))
        else:
            h = bytes(rng.choice(printable) for _ in range(rng.randrange(0, 40)))
        if rng.random() < 0.2 and h:
            k = rng.randrange(len(h))
            h = h[:k] + bytes([rng.choice(printable)]) + h[k + 1:]
        out.append(h.replace(b"\n", b""))
    return out


@functools.lru_cache(maxsize=None)
def edge(n):
    """the first n reads of the base shape"""
    lib, fq, run, umi = base()
    return lib, b"".join(line + b"\n" for line in fq.split(b"\n")[:4 * n]), run, umi


@functools.lru_cache(maxsize=None)
def long_headers(all_long):
    """200 reads of 150 bp; headers of 420 bytes (a long id in front of the UMI field) on every read, or on read 70 alone:
    64 such records span more than the 40 KiB a wave stages, and the header is walked in global memory"""
    rng = random.Random(0x420 + all_long)
    lib = UC.library()
    pool = [UC.rand_seq(rng, L) for _ in range(24)]
    recs = []
    for i in range(200):
        g = lib[rng.randrange(len(lib))].encode()
        s = (UC.mutate1(rng, g) if rng.random() < 0.2 else g) + UC.rand_seq(rng, 130)
        u = pool[rng.randrange(24)] if rng.random() < 0.9 else b"ACGTNACG"
        head = b"@r%d" % i
        if all_long or i == 70:
            head += b":" + b"x" * (420 - len(head) - 2 - L)
        head += b"_" + u
        assert not (all_long or i == 70) or len(head) == 420
        recs.append((head, s, b"I" * 150))
    return lib, fastq_of(recs), dict(UC.RUN), (SEP, L)


@functools.lru_cache(maxsize=None)
def wide16():
    """umi_cases.wide()'s reads (features 512 .. 601 only) with 16-base header UMIs: sixteen 'T's (all-ones codes) and
    sixteen 'A's (zero) among ordinary ones"""
    lib, fq, run, _ = UC.wide()
    rng = random.Random(0x1616)
    pool = [b"T" * 16, b"A" * 16] + [UC.rand_seq(rng, 16) for _ in range(30)]
    return lib, reheaded(fq, lambda i, s, q: b"@w%d_%s" % (i, pool[i % 32] if i < 64 else pool[rng.randrange(32)])), dict(run), (SEP, 16)


def neighbour_pool(rng, n, length):
    """n UMIs, every second one a neighbour at distance 1 of the one before it"""
    pool = []
    while len(pool) < n:
        u = UC.rand_seq(rng, length)
        pool += [u, UC.mutate1(rng, u)]
    return pool[:n]


@functools.lru_cache(maxsize=None)
def twin():
    """the base shape's reads with one UMI both inline at [20, 28) (quality all 'I', so only its bases decide) and in the
    header, from a pool of 40 that has neighbours at distance 1; one read in 25 carries an 'N' in both places"""
    lib, fq, run, umi = UC.base()
    rng = random.Random(0x7717)
    pool = neighbour_pool(rng, 40, L)
    recs = []
    for i, (s, q) in enumerate(UC.records(fq)):
        u = pool[min(rng.randrange(60), rng.randrange(60)) % 40]
        if rng.random() < 0.04:
            u = u[:5] + b"N" + u[6:]
        s = s[:UC.S] + u + s[UC.S + L:]
        recs.append((b"@t%d_%s" % (i, s[UC.S:UC.S + L]), s, b"I" * len(s)))
    return lib, fastq_of(recs), dict(run), umi, (SEP, L)


@functools.lru_cache(maxsize=None)
def twin_anchored():
    """umi_cases.anchored()'s reads (--us/--ds, the UMI at [2, 10), some with an 'N'), quality all 'I', the same eight bytes
    in the header"""
    lib, fq, run, umi = UC.anchored()
    recs = [(b"@a%d_%s" % (i, s[umi[0]:umi[0] + umi[1]]), s, b"I" * len(s)) for i, (s, q) in enumerate(UC.records(fq))]
    return lib, fastq_of(recs), dict(run), umi, (SEP, umi[1])


@functools.lru_cache(maxsize=None)
def twin_paired(n_pairs=2000):
    """umi_pair_cases' pairs (--st 5 --st2 0 --rc2 --l 10): positions [0, 5) of mate 1 from a pool with neighbours, quality
    all 'I', and mate 1's first eight bases -- the UMI of --umi1 0,8 -- in R1's header; R2's header carries another string"""
    import paired_cases as PC
    import umi_pair_cases as UP
    lib, fq1, fq2 = UP.base(True, n_pairs, 0x0B5E)
    rng = random.Random(0x2217)
    pool = neighbour_pool(rng, 24, 5)
    r1, r2 = [], []
    for i, ((s1, q1), (s2, q2)) in enumerate(zip(PC.records(fq1), PC.records(fq2))):
        if len(s1) >= 5:
            s1 = pool[rng.randrange(24)] + s1[5:]
        r1.append((b"@p%d_%s 1:N:0:1" % (i, s1[:8]), s1, b"I" * len(s1)))
        r2.append((b"@p%d_%s 2:N:0:1" % (i, UC.rand_seq(rng, 8)), s2, b"I" * len(s2)))
    return lib, fastq_of(r1), fastq_of(r2)
