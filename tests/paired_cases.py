"""tests/paired_cases.py -- generators and the oracle construction shared by the paired-end tests (CPU and GPU).

The yardstick is the existing oracle on MERGED reads.  With m2 = mate 2 as the run takes it (reverse-complemented under
rc2), a pair whose mate-1 windows all lie inside mate 1 equals the single read r1 + m2 counted with
--st a_1..a_n1, L1+b_1..L1+b_n2 (L1 = len(r1.seq)): mate-2 windows clip at the end of the merged read as they would at
the end of m2.  A pair whose mate-2 windows all lie inside m2 equals m2 + r1 with --st L2+a_.., b_.. -- the oracle takes
the windows in the order given, so the parts keep the order a.., b...  Counter-mode counts are a sum over reads of a
pure function: the pairs are grouped by L1 (or L2), the oracle runs once per group, and the results are added up."""
import random

from oracle import oracle as O

COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(seq):
    return seq.translate(COMP)[::-1]


def mate2_as_taken(seq, qual, rc2):
    return (revcomp(seq), qual[::-1]) if rc2 else (seq, qual)


def records(fastq):
    """[(seq, qual)] as fastq_parser frames them: 4 rstrip()-ed lines per record, a trailing partial record ignored"""
    lines = fastq.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [(lines[i + 1].rstrip(), lines[i + 3].rstrip()) for i in range(0, len(lines) - 3, 4)]


def fastq_of(recs, prefix=b"r", eol=b"\n"):
    return b"".join(b"@" + prefix + str(i).encode() + eol + s + eol + b"+" + eol + q + eol for i, (s, q) in enumerate(recs))


def pair_library(n, length, n1, n2, seed, combinatorial=False):
    """n features of n1 + n2 parts of `length` ACGT bases joined with ':'; combinatorial: a part shared by many features"""
    rng = random.Random(seed)
    part = lambda: "".join(rng.choice("ACGT") for _ in range(length))
    feats = []
    pool = [part() for _ in range(max(6, n // 8))]
    while len(feats) < n:
        parts = [part() for _ in range(n1 + n2)]
        if combinatorial and rng.random() < 0.6:
            parts[rng.randrange(n1 + n2)] = rng.choice(pool)
        f = ":".join(parts)
        if f not in feats:
            feats.append(f)
    return feats


def _mutate(rng, s, p_sub):
    b = bytearray(s)
    for j in range(len(b)):
        if rng.random() < p_sub:
            b[j] = rng.choice(b"ACGT")
    return bytes(b)


def make_pairs(lib, length, st1, st2, rc2, n_pairs, seed, len1=150, len2=150, p_sub=0.02, p_rand=0.1, p_lowq=0.05, ragged=False,
               dirty=False):
    """(fastq1, fastq2): pair i carries the parts of a library feature at st1 in mate 1 and at st2 in mate 2 AS THE RUN TAKES
    IT (so with rc2 the text of mate 2 is the reverse complement of that).  ragged: mate lengths 0 .. 160, but never BOTH
    mates ending inside a window (see pair_oracle); dirty: N / IUPAC / lower-case bases, quality lines of another length,
    quality bytes >= 128, CRLF and trailing blanks."""
    rng = random.Random(seed)
    need1 = max(st1) + length
    need2 = max(st2) + length
    r1, r2 = [], []
    for i in range(n_pairs):
        l1, l2 = len1, len2
        if ragged:
            l1, l2 = rng.randrange(0, 161), rng.randrange(0, 161)
            if l1 < need1 and l2 < need2:                  # never both cut short: one construction always covers the pair
                if rng.random() < 0.5:
                    l1 = rng.randrange(need1, 161)
                else:
                    l2 = rng.randrange(need2, 161)
        s1 = bytearray(rng.choice(b"ACGT") for _ in range(max(l1, need1)))
        s2 = bytearray(rng.choice(b"ACGT") for _ in range(max(l2, need2)))
        if rng.random() >= p_rand:
            parts = [p.encode() for p in rng.choice(lib).split(":")]
            for w, st in enumerate(st1):
                s1[st:st + length] = _mutate(rng, parts[w], p_sub)
            for w, st in enumerate(st2):
                s2[st:st + length] = _mutate(rng, parts[len(st1) + w], p_sub)
        s1, s2 = bytes(s1[:l1]), bytes(s2[:l2])
        q1 = bytearray(b"I" * l1)
        q2 = bytearray(b"I" * l2)
        for q in (q1, q2):
            for j in range(len(q)):
                if rng.random() < p_lowq / 10:
                    q[j] = rng.choice(b"!#+5:>?@")
        if dirty:
            for s in (1, 2):
                b = bytearray(s1 if s == 1 else s2)
                for j in range(len(b)):
                    if rng.random() < 0.02:
                        b[j] = rng.choice(b"NnRYacgt.")
                if s == 1:
                    s1 = bytes(b)
                else:
                    s2 = bytes(b)
            alter = rng.random()                           # a quality line of another length, in at most one mate and only where
            if alter < 0.05 and l2 >= need2 and len(q1):   # the other mate is whole: one construction still covers the pair
                q1 = q1[:rng.randrange(len(q1))]
            elif 0.05 <= alter < 0.10 and l1 >= need1:
                q2 = q2 + b"II"
            if rng.random() < 0.03 and len(q1):
                q1[rng.randrange(len(q1))] = rng.choice((0x80, 0xC9, 0xFF))
            if rng.random() < 0.03 and len(q2):
                q2[rng.randrange(len(q2))] = rng.choice((0x80, 0xC9, 0xFF))
        q1, q2 = bytes(q1), bytes(q2)
        s2, q2 = mate2_as_taken(s2, q2, rc2)             # back to the text of mate 2 as the sequencer wrote it
        r1.append((s1, q1)); r2.append((s2, q2))
    if not dirty:
        return fastq_of(r1, b"a"), fastq_of(r2, b"b")
    out = []
    for recs, prefix in ((r1, b"a"), (r2, b"b")):
        txt = b""
        for i, (s, q) in enumerate(recs):
            eol = b"\r\n" if rng.random() < 0.1 else b"\n"
            pad = b" \t" if rng.random() < 0.1 else b""
            txt += b"@" + prefix + str(i).encode() + b" 1:N:0" + eol + s + pad + eol + b"+" + eol + q + pad + eol
        out.append(txt)
    return out[0], out[1]


def merged_groups(fq1, fq2, st1, st2, length, rc2):
    """{(start string): merged FASTQ} covering every pair exactly once, pairs in their order inside each group; and the
    number of pairs in which BOTH mates end inside one of their windows (no construction covers those)."""
    groups, order, uncovered = {}, [], 0
    need1, need2 = max(st1) + length, max(st2) + length
    for (s1, q1), (s2, q2) in zip(records(fq1), records(fq2)):
        m2, mq2 = mate2_as_taken(s2, q2, rc2)
        # the quality line is sliced by ITS OWN length: the merged quality line clips like the mates' only when it splits
        # where the sequence does
        if len(s1) >= need1 and len(q1) == len(s1):
            key = ",".join([str(a) for a in st1] + [str(len(s1) + b) for b in st2])
            rec = (s1 + m2, q1 + mq2)
        elif len(m2) >= need2 and len(mq2) == len(m2):
            key = ",".join([str(len(m2) + a) for a in st1] + [str(b) for b in st2])
            rec = (m2 + s1, mq2 + q1)
        else:
            uncovered += 1
            continue
        if key not in groups:
            groups[key] = []
            order.append(key)
        groups[key].append(rec)
    return {k: fastq_of(groups[k]) for k in order}, uncovered


def pair_oracle(lib, fq1, fq2, st1, st2, length, rc2, miss, phred=30):
    """Counter mode: (counts, stats, uncovered) of the pairs by the group-by-length construction"""
    groups, uncovered = merged_groups(fq1, fq2, st1, st2, length, rc2)
    counts, stats = [0] * len(lib), [0] * 5
    for start, fq in groups.items():
        o = O.Oracle(features=[(str(i), s) for i, s in enumerate(lib)], miss=miss, phred=phred, length=length, start=start)
        o.count_fastq(fq)
        counts = [a + b for a, b in zip(counts, o.counts())]
        stats = [a + b for a, b in zip(stats, o.stats())]
        o.close()
    return counts, stats, uncovered


def make_pairs_uniform(lib, length, st1, st2, rc2, n_pairs, seed, len1=150, len2=150, p_sub=0.02, p_rand=0.1, p_lowq=0.004, p_n=0.002):
    """make_pairs for uniform mates, vectorised (100 k pairs in a fraction of a second): planted features with
    substitutions, random pairs, low quality bytes and 'N's anywhere in the mates"""
    import numpy as np
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parts = np.array([[list(p.encode()) for p in f.split(":")] for f in lib], np.uint8)
    pick, planted = rng.integers(0, len(lib), n_pairs), rng.random(n_pairs) >= p_rand
    out = []
    for mate, (ln, sts, w0) in enumerate(((len1, st1, 0), (len2, st2, len(st1)))):
        s = acgt[rng.integers(0, 4, (n_pairs, ln))]
        for w, st in enumerate(sts):
            seg = parts[pick, w0 + w].copy()
            sub = rng.random(seg.shape) < p_sub
            seg[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
            s[planted, st:st + length] = seg[planted]
        s[rng.random(s.shape) < p_n] = ord("N")
        q = np.full((n_pairs, ln), ord("I"), np.uint8)
        low = rng.random(q.shape) < p_lowq
        q[low] = np.frombuffer(b"!#+5:>?@", np.uint8)[rng.integers(0, 8, int(low.sum()))]
        if mate == 1 and rc2:
            s, q = np.frombuffer(s.tobytes().translate(COMP), np.uint8).reshape(s.shape)[:, ::-1], q[:, ::-1]
        head = np.frombuffer(b"".join(b"@%c%08d\n" % (b"ab"[mate], i) for i in range(n_pairs)), np.uint8).reshape(n_pairs, 11)
        nl = np.full((n_pairs, 1), 10, np.uint8)
        plus = np.tile(np.frombuffer(b"\n+\n", np.uint8), (n_pairs, 1))
        out.append(np.concatenate([head, s, plus, q, nl], axis=1).tobytes())
    return out[0], out[1]
