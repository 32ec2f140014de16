"""The raw-record modes of a Counter context exclude each other: UMIs (f2q_set_umi / _header / _paired), sample barcodes,
a strand mode, a stagger, indel reads, parts.  Every ordered pair of them is tried here, with f2q_set_mate2 and the calls
that share a file among ranks: the second call is refused with F2Q_ESTATE, its message names the mode in place, and the
context counts afterwards exactly what a context does that was only ever given the first.  A stagger and the indel flag can
be taken back: the context is plain again, packed tiles included, and takes another mode.

Everything is tiny (8 features of 10 bases, 300 reads: five workgroups of a raw-record kernel) and compares contexts with
each other; what each mode counts is checked against its expectation in the mode's own test file."""
import importlib

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
binding = importlib.import_module("2fast2q_amd.binding")
ESTATE = -7
L, N_READS = 10, 300
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def P():
    return pkg()


def _words(rng, n, length):
    """n distinct words, any two of them at least three bases apart"""
    out = []
    while len(out) < n:
        w = bytes(rng.choice(list(b"ACGT"), length).tolist())
        if all(sum(a != b for a, b in zip(w, o)) >= 3 for o in out):
            out.append(w)
    return out


def _rand(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).tolist())


def _subst(rng, w):
    i = int(rng.integers(len(w)))
    return w[:i] + bytes([b"ACGT"[(b"ACGT".index(w[i]) + 1 + int(rng.integers(3))) % 4]]) + w[i + 1:]


RNG = np.random.default_rng(0x30DE)
PARTS1, PARTS2 = _words(RNG, 4, L), _words(RNG, 4, L)
LIB = [w.decode() for w in _words(RNG, 8, L)]                                     # one window
PAIRS = [(i, (i + k) % 4) for i in range(4) for k in (0, 1)]                      # 8 of the 16 pairs
LIB2 = [f"{PARTS1[i].decode()}:{PARTS2[j].decode()}" for i, j in PAIRS]           # two windows, "A:B"
BCS = [b"ACGTACGT", b"TTGCAAGC"]
ONE, TWO = dict(start="0", length=L), dict(start="0,20", length=L)


def _fastq(reads):
    return b"".join(b"@r%d_%s\n%s\n+\n%s\n" % (i, umi, seq, b"I" * len(seq)) for i, (umi, seq) in enumerate(reads))


def _tail(rng, i):
    """what follows base 30 of a read: the UMI at [30, 38), a sample barcode at [40, 48) (every seventh with a substitution)"""
    bc = BCS[i % 2] if i % 7 else _subst(rng, BCS[i % 2])
    return _rand(rng, 8) + b"GA" + bc + b"CT"


def reads_one():
    """the feature at [0, 10): as it is, with a substitution, reverse-complemented (the whole read), 1 .. 8 bases late, with
    one base deleted, or not at all"""
    rng, out = np.random.default_rng(1), []
    for i in range(N_READS):
        f = LIB[i % 8].encode()
        kind = i % 6
        head = {0: f, 1: _subst(rng, f), 3: _rand(rng, 1 + i % 8) + f, 4: f[:4] + f[5:], 5: _rand(rng, L)}.get(kind, f)
        seq = (head + _rand(rng, 30))[:30] + _tail(rng, i)
        if kind == 2:
            seq = seq.translate(COMP)[::-1]
        out.append((_rand(rng, 8), seq))
    return out


def reads_two(split=False):
    """part 1 at [0, 10) and part 2 at [20, 30): pairs of the library, pairs that are not (recombinants), a substitution in
    either part, a part that is none.  split: part 2 moves to the start of a second mate"""
    rng, out1, out2 = np.random.default_rng(2), [], []
    for i in range(N_READS):
        a, b = PARTS1[i % 4], PARTS2[(i // 4 + (i % 3 == 0)) % 4]
        if i % 5 == 1:
            a = _subst(rng, a)
        if i % 5 == 2:
            b = _subst(rng, b)
        if i % 11 == 3:
            b = _rand(rng, L)
        umi = _rand(rng, 8)
        if split:
            out1.append((umi, a + _rand(rng, 10) + b"ACGTACGTAC" + _tail(rng, i)))
            out2.append((umi, b + _rand(rng, 40)))
        else:
            out1.append((umi, a + _rand(rng, 10) + b + _tail(rng, i)))
    return (_fastq(out1), _fastq(out2)) if split else _fastq(out1)


FQ1, FQ2 = _fastq(reads_one()), reads_two()
FQ_M1, FQ_M2 = reads_two(split=True)

# the modes: how a context is given one (Counter's keywords), the word every message about it carries, its own read-back
MODES = {
    "umi":         (dict(umi=(30, 8)), "UMI", lambda c: c.read_umis()),
    "umi_header":  (dict(umi_header=("_", 8)), "UMI", lambda c: c.read_umis()),
    "demux":       (dict(sample_barcodes=(40, BCS), barcode_mismatch=1), "demultiplexing", lambda c: c.read_demux()),
    "strand_rev":  (dict(strand="rev"), "strand", lambda c: c.read_strands()),
    "strand_both": (dict(strand="both"), "strand", lambda c: c.read_strands()),
    "stagger":     (dict(stagger=8), "stagger", lambda c: c.read_stagger()),
    "indel":       (dict(indel=True), "indel", lambda c: c.read_indels()),
    "parts":       (dict(parts=True), "parts", lambda c: c.read_parts()),
    "umi_paired":  (dict(umi_paired=((30, 8), None)), "UMI", lambda c: c.read_umis()),
}
# the setters: the family each belongs to (a setter is tried against every other family) and the call
SETTERS = {
    "set_umi":            ("umi", lambda c: c.set_umi(30, 8)),
    "set_umi_header":     ("umi", lambda c: c.set_umi_header("_", 8)),
    "set_umi_paired":     ("umi", lambda c: c.set_umi_paired((0, 8), None)),
    "set_sample_barcodes": ("demux", lambda c: c.set_sample_barcodes(40, BCS)),
    "set_strand":         ("strand", lambda c: c.set_strand("both")),
    "set_stagger":        ("stagger", lambda c: c.set_stagger(8)),
    "set_indel":          ("indel", lambda c: c.set_indel(True)),
    "set_parts":          ("parts", lambda c: c.set_parts()),
}
FAMILY = {"umi": "umi", "umi_header": "umi", "umi_paired": "umi", "demux": "demux", "strand_rev": "strand", "strand_both": "strand",
          "stagger": "stagger", "indel": "indel", "parts": "parts"}


def _refused(words, call):
    with pytest.raises(binding.F2QError) as exc:
        call()
    assert exc.value.code == ESTATE and all(w in str(exc.value) for w in words), str(exc.value)


def _count(c, fq):
    if isinstance(fq, tuple):
        assert c.count_block_paired(*fq) == (len(fq[0]), len(fq[1]))
    else:
        assert c.count_block(fq) == len(fq)


def _result(c, mode):
    counts, stats = c.read_counts()
    return [np.asarray(a) for a in (counts, stats, *MODES[mode][2](c))]


_FRESH = {}


def _fresh(P, mode, lib, fq, run):
    """what a context counts that was only ever given `mode`: computed once per mode and run"""
    key = (mode, tuple(sorted(run.items())))
    if key not in _FRESH:
        with P.Counter(features=lib, **MODES[mode][0], **run) as c:
            _count(c, fq)
            _FRESH[key] = _result(c, mode)
        assert _FRESH[key][1][0] == N_READS and _FRESH[key][0].sum() > 0             # (the reads do meet the library)
    return _FRESH[key]


def _refused_then_counts_alike(P, tmp_path, mode, lib, fq, run, name_it, estate_only=()):
    """a context with `mode` in place: f2q_set_mate2, every setter of another family and the calls for several ranks are
    refused (name_it: the message names the mode; estate_only: the code alone is checked), then it counts as a fresh one"""
    kw, word, _ = MODES[mode]
    paired = "start2" in run
    with P.Counter(**kw, **run) as c:                                                # no library yet: f2q_set_mate2 gets as far as the mode
        _refused([] if paired else [word], lambda: c.set_mate2("0"))
        for name, (family, call) in SETTERS.items():
            if family == FAMILY[mode] or (name not in name_it and name not in estate_only):
                continue
            _refused([word] if name in name_it else [], lambda: call(c))
        c.set_features(lib)
        if not paired:
            path = tmp_path / f"{mode}.fastq"
            path.write_bytes(fq)
            _refused([word, "ranks"], lambda: c.count_file_shard(str(path), 0, 2))
            n, _ = c.file_pieces(str(path), 1 << 16)
            census = c.census_pieces(str(path), 0, 2, 1 << 16, n)
            _refused([word, "ranks"], lambda: c.count_pieces(str(path), 0, 2, 1 << 16, census))
        _count(c, fq)
        got, want = _result(c, mode), _fresh(P, mode, lib, fq, run)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), (mode, g, w)


SINGLE = ["set_umi", "set_umi_header", "set_umi_paired", "set_sample_barcodes", "set_strand", "set_stagger", "set_indel"]


@pytest.mark.parametrize("mode", ["umi", "umi_header", "demux", "strand_rev", "strand_both", "stagger", "indel"])
def test_one_window_every_other_setter_is_refused_and_changes_nothing(P, tmp_path, mode):
    # (f2q_set_parts wants two windows and may say so first: the code alone)
    _refused_then_counts_alike(P, tmp_path, mode, LIB, FQ1, ONE, name_it=SINGLE, estate_only=["set_parts"])


def test_two_windows_parts_first(P, tmp_path):
    # (f2q_set_stagger and f2q_set_indel want one window and may say so first: the code alone)
    _refused_then_counts_alike(P, tmp_path, "parts", LIB2, FQ2, TWO, name_it=SINGLE[:5], estate_only=["set_stagger", "set_indel"])


@pytest.mark.parametrize("mode", ["umi", "umi_header", "demux", "strand_both"])
def test_two_windows_parts_second(P, tmp_path, mode):
    _refused_then_counts_alike(P, tmp_path, mode, LIB2, FQ2, TWO, name_it=["set_parts"])


def test_pairs_of_mates_umis_and_parts_in_both_orders(P, tmp_path):
    run = dict(start="0", start2="0", length=L)
    _refused_then_counts_alike(P, tmp_path, "umi_paired", LIB2, (FQ_M1, FQ_M2), run, name_it=["set_parts"])
    _refused_then_counts_alike(P, tmp_path, "parts", LIB2, (FQ_M1, FQ_M2), run, name_it=["set_umi_paired"])


def test_a_stagger_and_the_indel_flag_taken_back_leave_a_plain_context(P):
    with P.Counter(features=LIB, **ONE) as c:
        used, want_t = c.count_block(FQ1, want_timing=True)
        want = [np.asarray(a) for a in c.read_counts()]
    assert used == len(FQ1) and 0 < want_t["fast_reads"] and want_t["general_reads"] < want_t["reads"] == N_READS   # packed tiles
    for first in (True, False):                                                      # the library before / after the round trip
        with P.Counter(features=LIB if first else None, **ONE) as c:
            c.set_stagger(8)
            c.set_stagger(0)
            c.set_indel(True)
            c.set_indel(False)
            if not first:
                c.set_features(LIB)
            used, t = c.count_block(FQ1, want_timing=True)
            got = [np.asarray(a) for a in c.read_counts()]
            assert used == len(FQ1) and all(np.array_equal(g, w) for g, w in zip(got, want))
            assert [t[k] for k in ("path", "fast_reads", "general_reads", "reads")] == [want_t[k] for k in ("path", "fast_reads", "general_reads", "reads")]
            _refused(["f2q_set_stagger"], c.read_stagger)
            _refused(["f2q_set_indel"], c.read_indels)
    # ... and it takes another mode, which then counts as on a fresh context
    for leave, mode in ((lambda c: (c.set_stagger(8), c.set_stagger(0)), "indel"), (lambda c: (c.set_indel(True), c.set_indel(False)), "stagger"),
                        (lambda c: (c.set_stagger(8), c.set_stagger(0)), "umi"), (lambda c: (c.set_indel(True), c.set_indel(False)), "demux")):
        with P.Counter(features=LIB, **ONE) as c:
            leave(c)
            kw = MODES[mode][0]
            {"indel": lambda: c.set_indel(True), "stagger": lambda: c.set_stagger(8), "umi": lambda: c.set_umi(*kw["umi"]),
             "demux": lambda: c.set_sample_barcodes(*kw["sample_barcodes"], kw["barcode_mismatch"])}[mode]()
            _count(c, FQ1)
            got, want_m = _result(c, mode), _fresh(P, mode, LIB, FQ1, ONE)
        assert len(got) == len(want_m) and all(np.array_equal(g, w) for g, w in zip(got, want_m)), mode
