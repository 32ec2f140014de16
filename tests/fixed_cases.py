"""tests/fixed_cases.py -- inputs and expected values shared by the tests of the fixed-window (--st/--l) Counter kernels
(CPU preconditions and GPU).  Pure Python, seeded `random`, no GPU.

A read is `st` random bases + window + random tail (multi-window runs: the parts of the joined window planted at the
starts), quality 'I' except for the bytes a Phred kind sets.  The libraries hold, next to random guides, designed
constellations of features: pairs at distance 2 with one difference in each half of the key (a read between them has one
neighbour in each of the two tables), pairs with both differences in one half, stars, twins, features that share a whole
half.  The yardstick is the oracle over the same FASTQ bytes; which template instance must run (`fixed_variant`, the
rows of the matrices), which kernel family must count a block (`expected_path`) and how many of its reads must leave the
packed tiles (`general_reads`) are derived from the run and the input alone, never from a run of the code under test."""
import collections
import functools
import random

import synth
from oracle import oracle as O

PHRED = 30
TILE = 256
N17 = 17 * TILE
HIST_MAX = 24576                       # F2Q_HIST_MAX: the largest library with a per-workgroup histogram in LDS
PT_MIN_READS = 1 << 21                 # f2q_ctx::pt_min_reads: smaller blocks keep the packed tables unless F2Q_PT_PARTS is set
PATH_NONE, PATH_FIXED_V1, PATH_FIXED_PACKED, PATH_FIXED_LDS, PATH_FIXED_PART, PATH_MULTI, PATH_MULTI_LDS = 0, 1, 2, 3, 4, 5, 10      # include/f2q.h
LIB_SEED = 0xF1C5


def lowq(phred=PHRED):
    """the highest byte --ph fails, one below the first that passes (phred_threshold: fail set chr(33) .. chr(ph + 31)).
    --ph 1 fails no byte: '!' then, the lowest byte of the scale (a blank would not survive the line's rstrip)"""
    return chr(max(phred + 31, 33))


# ---- geometry and instance selection, restated from f2q_device.h (fixed_geom_at) and f2q_lib.hip (fixed_variant) ----

def fixed_geom(st, L):
    """(nq, nb): quality rows (4 bytes) and base rows (16 bases) under the window [st, st + L)"""
    return ((st + L - 1) >> 2) - (st >> 2) + 1, ((st + L - 1) >> 4) - (st >> 4) + 1


def fixed_variant(st, L, phred, generic=False):
    """the specialisation of the fixed-window kernels for a window: "a20", "spec52" or "generic" (F2Q_GENERIC=1, --ph
    below the Phred rule: always generic)"""
    nq, nb = fixed_geom(st, L)
    if generic or nq != 5 or nb != 2 or max(phred, 1) + 31 < 33:
        return "generic"
    return "a20" if L == 20 and st % 16 == 0 else "spec52"


def qmasks(st, L):
    """bytes of the first and of the last quality word that lie in the window (qm_first / qm_last, as sets of byte indices)"""
    return set(range(st & 3, 4)), set(range(0, ((st + L - 1) & 3) + 1))


def part_waves(parts):
    """scatter waves per workgroup of launch_part: n_parts KiB of rings per wave"""
    return 16 if parts <= 8 else 8 if parts <= 16 else 4


# ---- reads and libraries ----------------------------------------------------------------------------------------------

def fastq_of(recs):
    return "".join(f"@r{i}\n{s}\n+\n{q}\n" for i, (s, q) in enumerate(recs)).encode("latin-1")


def feats(lib):
    return [(str(i), s) for i, s in enumerate(lib)]


def rand_seq(rng, n):
    v = rng.getrandbits(2 * n) if n else 0
    return "".join("ACGT"[(v >> (2 * j)) & 3] for j in range(n))


def other(rng, c, *avoid):
    return rng.choice([b for b in "ACGT" if b != c and b not in avoid])


def change(rng, s, *pos):
    """s with each of the positions changed to another base"""
    b = list(s)
    for p in pos:
        b[p] = other(rng, b[p])
    return "".join(b)


def put(s, p, c):
    return s[:p] + c + s[p + 1:]


def hamming(a, b):
    assert len(a) == len(b)
    return [i for i in range(len(a)) if a[i] != b[i]]


CONSTELLATIONS = ("cross", "same0", "same1", "star_absent", "star_present", "twin", "d1_d2", "share_h0", "share_h1")
N_CONSTELLATIONS = 32                  # of each kind: 9 x 32 guides carry one


class Library:
    """features (joined keys, no ':') and what was planted among them.  Identity-hashed: the cached builders' objects key
    the cached blocks and expectations.  `lt` / `pt`: whether the cuckoo builds of the LDS tables / of the partitioned
    tables must succeed for it (at most 4 features may share a half; a size check for the LDS tables) -- declared by
    design, asserted on the CPU (test_fixed_cases_cpu.py) with the host build of build_lt / build_pt."""

    def __init__(self, keys, L, cons, lt, pt, parts=1, singles=0):
        self.keys, self.L, self.cons, self.lt, self.pt, self.parts, self.singles = tuple(keys), L, cons, lt, pt, parts, singles
        l = L // parts
        self.feats = tuple(":".join(k[i:i + l] for i in range(0, L, l)) for k in self.keys[:len(keys) - singles]) + self.keys[len(keys) - singles:]
        self.by_kind = {}
        for c in cons:
            self.by_kind.setdefault(c["kind"], []).append(c)

    def __len__(self):
        return len(self.feats)


def _library(L, n, seed, share, parts=1, singles=0, lt=True, pt=True):
    rng = random.Random(seed * 131 + L)
    h = L // 2
    guides = synth.make_library(n, L, seed)
    seen, keys, cons = set(guides), list(guides), []

    shared = (set(), set())                                      # half values that three features share by design: no fourth

    def add(make, fresh=None):
        """a new feature; `fresh`: its half 0 / half 1 must be a value no feature has yet"""
        for _ in range(1000):
            s = make()
            if s in seen or s[:h] in shared[0] or s[h:] in shared[1]:
                continue                                         # (a second draw where a random feature exists already)
            if fresh is None or not any((k[h:] if fresh else k[:h]) == (s[h:] if fresh else s[:h]) for k in keys):
                break
        else:
            raise AssertionError("no room for a designed feature")
        assert len(s) == L
        seen.add(s); keys.append(s)
        return len(keys) - 1

    # a constellation goes to a guide neither of whose halves another guide has (short halves coincide by chance: three
    # features that share a half by design would be five)
    n0, n1 = collections.Counter(g[:h] for g in guides), collections.Counter(g[h:] for g in guides)
    centres = [i for i, g in enumerate(guides) if n0[g[:h]] == 1 and n1[g[h:]] == 1][:len(CONSTELLATIONS) * N_CONSTELLATIONS]
    assert len(centres) == len(CONSTELLATIONS) * N_CONSTELLATIONS
    for j, i in enumerate(centres):
        kind, g = CONSTELLATIONS[j % len(CONSTELLATIONS)], guides[i]
        p, p2 = rng.sample(range(h), 2)
        q, q2 = rng.sample(range(h, L), 2)
        c = dict(kind=kind, guide=i, p=p, p2=p2, q=q, q2=q2)
        if kind == "cross":
            c["partner"] = add(lambda: change(rng, g, p, q))
        elif kind == "same0":
            c["partner"] = add(lambda: change(rng, g, p, p2))
        elif kind == "same1":
            c["partner"] = add(lambda: change(rng, g, q, q2))
        elif kind in ("star_absent", "star_present"):           # the arms differ from the centre next to the border of the halves
            c["p"], c["q"] = p, q = h - 1, h
            centre = change(rng, g, p)
            while centre in seen or centre[:h] in shared[0] or centre[h:] in shared[1]:
                centre = change(rng, g, p)
            c["centre"] = centre
            c["arm"] = add(lambda: change(rng, centre, q))
            if kind == "star_present":
                c["centre_id"] = add(lambda: centre)
        elif kind == "twin":
            c["p"] = p = (j * 7) % L
            c["partner"] = add(lambda: change(rng, g, p))
        elif kind == "d1_d2":
            c["partner"] = add(lambda: change(rng, g, p, q, q2))
        elif kind == "share_h0":                                 # `share` features in all with the guide's half 0
            c["others"] = [add(lambda: g[:h] + rand_seq(rng, L - h), fresh=1) for _ in range(share - 1)]
            shared[0].add(g[:h])
        elif kind == "share_h1":
            c["others"] = [add(lambda: rand_seq(rng, h) + g[h:], fresh=0) for _ in range(share - 1)]
            shared[1].add(g[h:])
        cons.append(c)
    if singles:                                                  # features of one part next to the pairs: no uniform k-part library
        keys += [k[:L // parts] for k in guides[-singles:]]
        assert len(set(keys)) == len(keys)
    lib = Library(keys, L, cons, lt, pt, parts, singles)
    lib.plain = [i for i in range(n) if i not in set(centres)]                # guides without a designed neighbour
    return lib


@functools.lru_cache(maxsize=None)
def library(L, n=None, seed=LIB_SEED, share=3):
    """synth.make_library(n, L, seed) (== binding.synth_library(seed, n, L)) plus, for the first 288 guides with halves of their own in rotation,
    the constellations.  h = L // 2 (the tables' half 0 is bases [0, h)), p, p2 < h <= q, q2:
      cross         partner = guide changed at p and q
      same0 / same1 partner = guide changed at two positions of one half
      star_*        centre = guide changed at h - 1, second arm = centre changed at h; the centre absent / a feature
      twin          partner = guide changed at one position
      d1_d2         partner = guide changed at p, q, q2
      share_h0/_h1  `share` - 1 more features with the guide's half 0 / half 1 (the other half random)
    share = 3: the LDS tables hold it; share = 5: neither they nor the partitioned tables can (4 slots per half value)"""
    n = n or (2000 if L >= 16 else 800)      # (of 2000 random 14-base guides too many share a 7-base half by chance for the tables)
    return _library(L, n, seed, share, lt=share <= 4 and n <= 14000, pt=share <= 4)


@functools.lru_cache(maxsize=None)
def pair_library(L, n=None, seed=LIB_SEED + 1, singles=0):
    """the same keys as A:B features of two parts of L // 2 bases (half 0 = part A); singles > 0: that many one-part
    features besides, so that the run keeps k_count_multi4 (features of several part counts)"""
    assert L % 2 == 0
    n = n or (2000 if L >= 16 else 800)
    return _library(L, n, seed, 3, parts=2, singles=singles, lt=singles == 0 and n <= 14000)


# the kinds of one cycle of reads; the frequent ones several times so that no statistic is near zero.  The first 37 are
# the whole of the one-partial-tile block: they hold a read of every verdict.
KINDS = (
    "exact", "sub_first", "cross_a", "q_first", "exact", "n_first", "star_centre", "sub_last", "q_last", "exact",
    "sub_half_lo", "sub_half_hi", "sub2_split", "sub2_same_half", "cross_b", "same0", "same1", "exact", "star_exact",
    "near_centre", "twin_third", "d1_d2", "share_exact", "share_near_other_half", "share_near_same_half", "exact",
    "n_last", "n_mid", "n2", "sub1_n1", "twin_n", "n_before", "n_after", "q_before", "q_after", "q_pass_first", "q_bang",
    "q_1f", "q_7f", "q_and_n", "lower", "lower_sub", "exact", "end_in_win", "end_at_win", "end_before_win", "qlen_short",
    "qlen_long", "sub_first", "sub_last")
MW_KINDS = ("part_q_fail_all", "part_q_fail_one", "part_q_edge_lo", "part_q_edge_hi") + KINDS      # (in front: the 37-read block needs a read that fails)
N_KINDS = ("n_first", "n_last", "n_mid", "n2", "sub1_n1", "twin_n", "n_before", "n_after", "q_and_n")
TIE_KINDS = {"cross_a": ("cross",), "cross_b": ("cross",), "same0": ("same0",), "same1": ("same1",), "star_centre": ("star_absent",),
             "star_exact": ("star_present",), "near_centre": ("star_present",), "twin_third": ("twin",), "twin_n": ("twin",), "d1_d2": ("d1_d2",),
             "share_exact": ("share_h0", "share_h1"), "share_near_other_half": ("share_h0", "share_h1"),
             "share_near_same_half": ("share_h0", "share_h1")}


def applies(kind, starts):
    """kinds that need a base before the first window do not apply to windows at the read start"""
    return min(starts) > 0 or kind not in ("n_before", "q_before", "end_before_win")


class Case:
    """a library and a block of reads; identity-hashed"""

    def __init__(self, lib, recs, kinds, starts, l, phred):
        self.lib, self.recs, self.kinds, self.starts, self.l, self.phred = lib, recs, kinds, starts, l, phred
        self.n = len(recs)
        self.fq = fastq_of(recs)

    def run(self, miss=1, phred=None):
        """the run's parameters as binding.Counter and oracle.Oracle take them"""
        return dict(miss=miss, phred=self.phred if phred is None else phred, length=self.l, start=",".join(str(s) for s in self.starts))


def _window(rng, lib, kind, f, k_of_kind):
    """(joined window, constellation) of one read: what the kind does to the bases inside the window"""
    L, h = lib.L, lib.L // 2
    key = lib.keys[f]
    con = None
    if kind in TIE_KINDS:
        groups = TIE_KINDS[kind]
        group = lib.by_kind[groups[k_of_kind % len(groups)]]
        con = group[k_of_kind // len(groups) % len(group)]
        g = lib.keys[con["guide"]]
        if kind == "cross_a": w = put(g, con["p"], lib.keys[con["partner"]][con["p"]])                  # guide through table 1, partner through table 0
        elif kind == "cross_b": w = put(g, con["q"], lib.keys[con["partner"]][con["q"]])                # guide through table 0, partner through table 1
        elif kind == "same0": w = put(g, con["p"], lib.keys[con["partner"]][con["p"]])                  # both through table 1
        elif kind == "same1": w = put(g, con["q"], lib.keys[con["partner"]][con["q"]])                  # both through table 0
        elif kind in ("star_centre", "star_exact"): w = con["centre"]
        elif kind == "near_centre": w = change(rng, con["centre"], con["q2"] if con["q2"] != con["q"] else L - 1)
        elif kind == "twin_third": w = put(g, con["p"], other(rng, g[con["p"]], lib.keys[con["partner"]][con["p"]]))
        elif kind == "twin_n": w = put(g, con["p"], "N")
        elif kind == "d1_d2": w = put(g, con["p"], lib.keys[con["partner"]][con["p"]])
        else:                                                    # three features share half 0 (share_h0) or half 1 (share_h1)
            shared = range(h) if con["kind"] == "share_h0" else range(h, L)
            apart = range(h, L) if con["kind"] == "share_h0" else range(h)
            w = lib.keys[con["others"][k_of_kind % len(con["others"])]]
            if kind == "share_near_other_half": w = change(rng, w, rng.choice(apart))      # the shared half kept: its buckets hold three tags of that half
            elif kind == "share_near_same_half": w = change(rng, w, rng.choice(shared))    # found through the other table
        return w, con
    if kind in ("sub_first", "lower_sub"): w = change(rng, key, 0 if kind == "sub_first" else rng.randrange(L))
    elif kind == "sub_last": w = change(rng, key, L - 1)
    elif kind == "sub_half_lo": w = change(rng, key, h - 1)
    elif kind == "sub_half_hi": w = change(rng, key, h)
    elif kind == "sub2_split": w = change(rng, key, rng.randrange(h), rng.randrange(h, L))
    elif kind == "sub2_same_half": w = change(rng, key, *(rng.sample(range(h), 2) if rng.random() < 0.5 else rng.sample(range(h, L), 2)))
    elif kind == "n_first": w = put(key, 0, "N")
    elif kind == "n_last": w = put(key, L - 1, "N")
    elif kind == "n_mid": w = put(key, rng.randrange(1, L - 1), "N")
    elif kind == "n2":
        a, b = rng.sample(range(L), 2); w = put(put(key, a, "N"), b, "N")
    elif kind == "sub1_n1":
        a, b = rng.sample(range(L), 2); w = put(change(rng, key, a), b, "N")
    else: w = key
    if kind in ("lower", "lower_sub"): w = w.lower()
    return w, con


@functools.lru_cache(maxsize=None)
def block(lib, starts=(0,), n=N17 + 37, seed=1, phred=PHRED):
    """n reads on the windows at `starts` (one: a window of lib.L bases; several: lib.parts parts of lib.L // lib.parts
    bases), the kinds of KINDS (MW_KINDS) in turn; a kind that does not apply to the starts is an exact read.  Every second
    wave of 64 reads holds no 'N' (the kernels take another branch for a wave without flag bits).  Every 16th read is on
    the last feature of the library, the others (but for the tie kinds) on guides without a designed neighbour.  Quality kinds, with LOWQ = chr(phred + 31) the highest failing byte:
      q_first / q_last   LOWQ on the first / last byte of the (joined) window
      q_before / q_after LOWQ one byte before the first window / one past the last: must not fail
      q_pass_first       LOWQ + 1 on the first byte: passes
      q_bang             '!' in the window;  q_1f / q_7f: bytes 0x1f and 0x7f in the window, both pass
      q_and_n            'N' and, in the same 4-byte quality word, LOWQ on the byte next to it
      part_q_fail_one    (several windows) LOWQ in one part: a shorter key;  part_q_fail_all: LOWQ in every part
      part_q_edge_lo/_hi (several windows) LOWQ on the last byte of the first part / the first byte of the second: in the
                         tile they are neighbours, in the read they are not; one part fails, not both
    A tile holds nothing past the end of a single window (the packer stores a read up to there), so of q_before and
    q_after only the first can reach a single-window kernel; between the parts of several windows both neighbours are
    stored.
    Length kinds: the read ends inside the last window, exactly at its end, before the first window; a quality line
    three bytes shorter / two longer than the sequence (raw path)."""
    rng = random.Random(seed)
    W, L = len(starts), lib.L
    assert (W == lib.parts or lib.parts == 1 == W) and L % W == 0
    l = L // W
    first, end = min(starts), max(starts) + l
    pos = lambda k: starts[k // l] + k % l                       # read position of base k of the joined window
    low = lowq(phred)
    kinds_of = MW_KINDS if W > 1 else KINDS
    recs, kinds, seen = [], [], {}
    n_pairs = len(lib) - lib.singles
    for i in range(n):
        kind = kinds_of[i % len(kinds_of)]
        if (kind in N_KINDS and (i // 64) % 2) or not applies(kind, starts):
            kind = "exact"
        k_of_kind = seen[kind] = seen.get(kind, -1) + 1
        f = n_pairs - 1 if i % 16 == 5 else rng.choice(lib.plain)
        w, con = _window(rng, lib, kind, f, k_of_kind)
        tail = rng.randrange(2, 13)
        seq = list(rand_seq(rng, end + tail))
        for k in range(L):
            seq[pos(k)] = w[k]
        q = ["I"] * len(seq)
        cut = qlen = None
        if kind == "n_before": seq[first - 1] = "N"
        elif kind == "n_after": seq[end] = "N"
        elif kind == "q_first": q[pos(0)] = low
        elif kind == "q_last": q[pos(L - 1)] = low
        elif kind == "q_before": q[first - 1] = low
        elif kind == "q_after": q[end] = low
        elif kind == "q_pass_first": q[pos(0)] = chr(ord(low) + 1)
        elif kind == "q_bang": q[pos(rng.randrange(L))] = "!"
        elif kind == "q_1f": q[pos(rng.randrange(L - 1))] = "\x1f"
        elif kind == "q_7f": q[pos(rng.randrange(L - 1))] = "\x7f"
        elif kind == "q_and_n":                                  # two neighbouring bytes of one quality word of the tile (stored position:
            k = rng.choice([k for k in range(L - 1) if (k if W > 1 else first + k) % 4 != 3])      # several windows are stored back to back)
            side = i // len(kinds_of) % 2                        # the 'N' before the low byte, and after it
            seq[pos(k + side)], q[pos(k + 1 - side)] = "N", low
        elif kind == "part_q_fail_one": q[pos(rng.randrange(W) * l + rng.randrange(l))] = low
        elif kind == "part_q_edge_lo": q[pos(l - 1)] = low
        elif kind == "part_q_edge_hi": q[pos(l)] = low
        elif kind == "part_q_fail_all":
            for part in range(W): q[pos(part * l + rng.randrange(l))] = low
        elif kind == "end_in_win": cut = rng.randrange(max(starts) + 1, end)
        elif kind == "end_at_win": cut = end
        elif kind == "end_before_win": cut = rng.randrange(1, first + 1)
        elif kind == "qlen_short": qlen = len(seq) - 3
        elif kind == "qlen_long": qlen = len(seq) + 2
        s, q = "".join(seq), "".join(q)
        if cut is not None: s, q = s[:cut], q[:cut]
        if qlen is not None: q = (q + "II")[:qlen]
        recs.append((s, q)); kinds.append(kind)
    return Case(lib, recs, kinds, tuple(starts), l, phred)


TILE_COUNTS = (1, 2, 16, 17, 33)


def tile_blocks(lib, starts=(0,)):
    """1, 2, 16, 17 and 33 tiles, the last one of 37 reads.  The kernels with 16 waves per workgroup walk 33 tiles, in one
    workgroup, with three tiles on wave 0 and two on the others: both parities of the alternating register sets.  (The
    33-tile block has 8229 reads: the one designed block above 4389.)"""
    return [block(lib, starts, n=(t - 1) * TILE + 37, seed=20 + t) for t in TILE_COUNTS]


SKEW_HOT = 1500                        # a plain guide: no constellation around it


@functools.lru_cache(maxsize=None)
def skewed(lib, seed=5):
    """80 000 reads for ONE workgroup (st 0): 70 000 on one feature, every third of them with one substitution, 10 000
    spread over the library; shuffled, no 'N', tails from a small pool"""
    rng = random.Random(seed)
    assert lib.parts == 1
    tails = [rand_seq(rng, rng.randrange(1, 13)) for _ in range(64)]
    g = lib.keys[SKEW_HOT]
    wins = [(g if i % 3 else change(rng, g, rng.randrange(lib.L))) for i in range(70000)] + [rng.choice(lib.keys) for _ in range(10000)]
    rng.shuffle(wins)
    recs = []
    for w in wins:
        s = w + rng.choice(tails)
        recs.append((s, "I" * len(s)))
    return Case(lib, recs, None, (0,), lib.L, PHRED)


# ---- what must happen to a block --------------------------------------------------------------------------------------

def _on(env, k):
    return (env or {}).get(k, "")[:1] == "1"


def _clean(case, s, q):
    """the packer's rule for fixed-window Counter runs against an all-ACGT library (read_is_clean):
    a quality line as long as the sequence, no quality byte >= 128 under the stored bases; non-ACGT symbols and lower
    case travel in band.  Several windows: the tiles hold the windows only, so a read that ends before the end of the
    last window is not packed (one window: its clipped window is)."""
    if len(s) != len(q):
        return False
    end = max(case.starts) + case.l
    if len(case.starts) > 1:
        if len(s) < end:
            return False
        stored = [st + k for st in case.starts for k in range(case.l)]
    else:
        stored = range(case.starts[0], min(len(s), end))
    return not any(ord(q[j]) >= 128 for j in stored)


def general_reads(case, run, env=None):
    """reads of the block that must leave the packed tiles"""
    if _on(env, "F2Q_FORCE_GENERAL"):
        return case.n
    return sum(not _clean(case, s, q) for s, q in case.recs)


def expected_path(case, run, env=None):
    """the kernel family choose_path must pick for the packed tiles of the block (0: no packed tiles)"""
    lib, miss, W = case.lib, run["miss"], len(case.starts)
    if _on(env, "F2Q_FORCE_GENERAL"):
        return PATH_NONE
    lt_built = lib.lt and miss <= 1 and 14 <= lib.L <= 21                       # build_lt
    lt = lt_built and not _on(env, "F2Q_NO_LT") and len(lib) <= HIST_MAX
    if W > 1:
        return PATH_MULTI_LDS if lt and lib.singles == 0 and lib.parts == W else PATH_MULTI
    if _on(env, "F2Q_FORCE_V1"):
        return PATH_FIXED_V1
    st, L = case.starts[0], case.l
    assert L == lib.L and lib.parts == 1
    # the tiles hold every row under the window: they are as wide as the longest stored read, and a read is stored up to
    # the end of the window
    stored = [min(len(s), st + L) for s, q in case.recs if _clean(case, s, q)]
    rows = miss <= 1 and bool(stored) and -(-max(stored) // 4) >= -(-(st + L) // 4) and -(-max(stored) // 16) >= -(-(st + L) // 16)
    forced = int((env or {}).get("F2Q_PT_PARTS", "0") or 0)
    pt_built = lib.pt and miss <= 1 and 14 <= L <= 21 and (forced > 0 or not lt_built)      # build_pt
    use_lt = rows and lt
    n_tiles = -(-len(stored) // TILE)
    min_reads = int((env or {}).get("F2Q_PT_MIN_READS", PT_MIN_READS))
    if rows and pt_built and not _on(env, "F2Q_NO_PT") and (forced > 0 or (not use_lt and n_tiles * TILE >= min_reads)):
        return PATH_FIXED_PART
    return PATH_FIXED_LDS if use_lt else PATH_FIXED_PACKED


def run_key(run):
    return tuple(sorted((k, str(v)) for k, v in run.items()))


@functools.lru_cache(maxsize=None)
def _oracle(cases, rk, threads):
    run = {k: (v if k == "start" else int(v)) for k, v in rk}
    o = O.count_fastq_parallel(b"".join(c.fq for c in cases), threads, features=feats(cases[0].lib.feats), **run)
    return o.counts(), o.stats()


def expect(cases, **run):
    """(counts, stats) of the oracle over the blocks of one case or of several (of one library), concatenated"""
    cases = cases if isinstance(cases, tuple) else (cases,)
    return _oracle(cases, run_key(run), 4 if sum(c.n for c in cases) > 20000 else 1)


def verdict_of(case, i, **run):
    """(counts as {feature: n}, the five statistics) of the oracle for read i of the block alone"""
    o = O.Oracle(features=feats(case.lib.feats), **run)
    o.count_fastq(fastq_of([case.recs[i]]))
    counts, st = o.counts(), o.stats()
    o.close()
    return {f: c for f, c in enumerate(counts) if c}, st


# ---- the instances, as data -------------------------------------------------------------------------------------------
# Every row names the template instance it must reach and gives a run that reaches it; test_fixed_cases_cpu.py checks
# the restated selection (fixed_variant, part_waves, expected_path) against the name, and the set of names against the
# list of instances the launchers can pick.

# k_count_fixed4_lds<NQ NB, NEAR, A20, MW>: (variant, near, mw, st or starts, L, phred, miss, env)
MATRIX_LDS = [(variant, miss > 0, False, st, L, phred, miss, {})
              for miss in (1, 0)
              for variant, st, L, phred in (("a20", 0, 20, 30), ("a20", 16, 20, 30),
                                            ("spec52", 4, 20, 30), ("spec52", 3, 17, 30), ("spec52", 1, 16, 30), ("spec52", 4, 18, 30),
                                            ("generic", 3, 20, 30), ("generic", 5, 14, 30), ("generic", 2, 21, 30), ("generic", 0, 20, 1))]
MATRIX_LDS += [(variant, miss > 0, True, starts, L, 30, miss, {})
               for miss in (1, 0)
               for variant, starts, L in (("a20", (2, 15), 20), ("spec52", (0, 9), 18), ("generic", (12, 1), 16))]

# k_part_scatter<NQ NB, A20, PW> x k_part_count<NEAR>: (variant, pw, near, st, L, phred, miss, parts)
MATRIX_PART = [(variant, pw, miss > 0, st, L, 30, miss, parts)
               for pw, parts in ((16, 3), (8, 12), (4, 20))
               for variant, st, L in (("a20", 0, 20), ("spec52", 4, 20), ("generic", 3, 20))
               for miss in (1, 0)]
PART_CHUNK = "1024"                    # F2Q_PT_CHUNK: the 18 tiles of a block in five rounds of at most four

# k_count_fixed4<LDS, NQ NB>: (lds, variant, st, L, miss, big): F2Q_NO_LT=1 F2Q_NO_PT=1; big: F2Q_HIST_MAX + 1 features
PACKED_ENV = {"F2Q_NO_LT": "1", "F2Q_NO_PT": "1"}
MATRIX_PACKED = [(not big, variant, st, L, miss, big)
                 for big in (False, True) for variant, st, L in (("spec52", 4, 20), ("generic", 3, 20)) for miss in (0, 1, 2, 3)]

# k_count_multi4<LDS>: (lds, library, starts, L, miss)
MATRIX_MULTI = [(True, "mixed", (2, 15), 20, 1), (True, "mixed", (2, 15), 20, 0), (True, "pairs", (12, 1), 16, 2),
                (False, "big", (2, 15), 20, 1)]

# k_count_fixed<LDS>: (lds, st, L, miss, big): F2Q_FORCE_V1=1
V1_ENV = {"F2Q_FORCE_V1": "1"}
MATRIX_V1 = [(True, 0, 20, 1, False), (True, 3, 17, 0, False), (True, 5, 14, 2, False), (False, 0, 20, 1, True)]

@functools.lru_cache(maxsize=None)
def big_library(L=20, pairs=False):
    """a library of more than F2Q_HIST_MAX features: the histogram leaves the LDS (hit_buf + k_hist_ranges, global
    atomics).  Too large for the LDS tables; the partitioned tables can hold it."""
    lib = _library(L, HIST_MAX + 1, LIB_SEED + 2, 3, parts=2 if pairs else 1, lt=False, pt=True)
    assert len(lib) > HIST_MAX
    return lib


def multi_library(name, L):
    return {"mixed": lambda: pair_library(L, singles=40), "pairs": lambda: pair_library(L), "big": lambda: big_library(L, pairs=True)}[name]()
