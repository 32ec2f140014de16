"""Low-complexity samples for the file readers: text that gzip shrinks 100 : 1 and more (adapter dimers, poly-G tails,
an amplicon library where a handful of records make up most of the file).  A speculative chunk of the parallel gzip
decoder (2fast2q_amd/csrc/f2q_pargz.h) may emit only so many symbols (a memory bound, F2Q_GZ_SYM_KB); on such text it
reaches that cap, and the chunk has to be decoded again by a later round, not reported as damage.  Shared by
tests/test_reader_cpu.py (the reader alone) and tests/test_low_complexity_files_gpu.py (file to counts)."""
import random
import re
import zlib

CAPPED = re.compile(r"\[\d+: L start")          # a chunk of an F2Q_GZ_TRACE round line that stopped at the cap
ROUND = re.compile(r"^\[pargz\] round ", re.M)


def capped_chunks(stderr_text):
    """chunks the F2Q_GZ_TRACE lines on stderr show as stopped at the symbol cap"""
    return len(CAPPED.findall(stderr_text))


def ordinary(n, seed):
    """FASTQ-like text of n reads that compresses 3-4 : 1"""
    rng = random.Random(seed)
    rec = []
    for i in range(n):
        L = rng.randint(30, 151)
        q = "".join(rng.choice("IIIIIIII?5+#FF:,") for _ in range(L))
        rec.append("@inst:%d:%d %d/1\n%s\n+\n%s\n" % (seed, i, rng.randint(0, 9), "".join(rng.choice("ACGT") for _ in range(L)), q))
    return "".join(rec).encode()


def byte_runs(n_bytes, seed, lo=1 << 20, hi=8 << 20):
    """runs of one byte each, lo..hi bytes long, n_bytes in all: deflate's best case, about 1000 : 1"""
    rng = random.Random(seed)
    out, left = [], n_bytes
    while left:
        k = min(left, rng.randint(lo, hi))
        out.append(bytes([rng.choice(b"ACGTNI#\n")]) * k)
        left -= k
    return b"".join(out)


def few_records(n_bytes, seed, n_rec=5, max_run=2000):
    """n_rec distinct FASTQ records in runs of random length, about n_bytes in all: about 150 : 1"""
    rng = random.Random(seed)
    recs = []
    for r in range(n_rec):
        L = rng.randint(100, 151)
        recs.append(("@amplicon:%d:%d\n%s\n+\n%s\n" % (seed, r, "".join(rng.choice("ACGT") for _ in range(L)), "I" * L)).encode())
    out, n = [], 0
    while n < n_bytes:
        b = recs[rng.randrange(n_rec)] * rng.randint(1, max_run)
        out.append(b); n += len(b)
    return b"".join(out)


def ratio_steps(seed=11):
    """one member's text whose ratio steps up and down: ordinary, 24 MB of five records (150 : 1), ordinary, 500 KB of
    random bytes (stored blocks), low-complexity again, ordinary"""
    rng = random.Random(seed)
    return b"".join([ordinary(3000, seed), few_records(24 << 20, seed + 1), ordinary(2500, seed + 2), rng.randbytes(500_000),
                     few_records(5 << 20, seed + 3, n_rec=3), ordinary(2000, seed + 4)])


def gz_member(data, level=6):
    """one gzip member (RFC 1952, no optional fields)"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush()
    return b"\x1f\x8b\x08\0\0\0\0\0\x00\x03" + body + (zlib.crc32(data) & 0xFFFFFFFF).to_bytes(4, "little") + (len(data) & 0xFFFFFFFF).to_bytes(4, "little")


def zlib_prefix(raw, step=4096):
    """the text zlib delivers from a (damaged) gzip file before it gives up, fed `step` bytes at a time, all members"""
    out, pos = [], 0
    while pos < len(raw):
        while pos < len(raw) and raw[pos] == 0:
            pos += 1
        if raw[pos:pos + 2] != b"\x1f\x8b":
            break
        d = zlib.decompressobj(31)
        try:
            while pos < len(raw) and not d.eof:
                piece = raw[pos:pos + step]
                out.append(d.decompress(piece))
                pos += len(piece) - len(d.unused_data)
        except zlib.error:
            break
        if not d.eof:
            break
    return b"".join(out)


# ---- a whole sample of that shape, for the road from file to counts ---------------------------------------------------
import functools

import synth

UP, DOWN = "GTTTAAGAGCTA", "CGTTACCAGGTT"
UMI = (20, 8)                                    # --umi 20,8
FIXED = dict(start="0", length=20, phred=30)     # the fixed window: the first 20 bases
# F2Q_GZ_SYM_KB=64: 64 KiB of this sample's hot stretch hold 13 Mi symbols, 64 KiB of its ordinary reads 0.2 Mi
GZ_ENV = {"F2Q_GZ_PAR_MIN_KB": "16", "F2Q_GZ_CHUNK_KB": "64", "F2Q_GZ_SYM_KB": "64", "F2Q_GZ_TRACE": "1", "F2Q_IO_THREADS": "4"}


def library():
    return synth.make_library(600, 20, 0x0A11)


def _mut(s, pos):
    return s[:pos] + "ACGT"[("ACGT".index(s[pos]) + 1) & 3] + s[pos + 1:]


def hot_records():
    """[(record, run lengths)]: 100-base reads, a guide in the fixed window [0, 20), a UMI at [20, 28), and a second guide
    between the anchors UP and DOWN at 40.  Feature 5 carries most of the sample under two UMIs one base apart
    (25 000 : 3 000 reads: one molecule under both rules) and a one-mismatch read; feature 40 two UMIs one base apart with
    2 500 : 2 000 reads (one cluster, two directional molecules); feature 77 a UMI with a low-quality base"""
    lib = library()
    fill, tail = "TTGACCTGATCA", "ACCATTGGCAGTACGT"
    q = "I" * 100

    def rec(g, umi, g2, qual=q):
        return ("@hot\n%s\n+\n%s\n" % (g + umi + fill + UP + g2 + DOWN + tail, qual)).encode()
    return [(rec(lib[5], "ACGTACGT", lib[7]), (9000, 7000, 6000)),
            (rec(lib[5], "ACGTACGA", lib[7]), (3000,)),
            (rec(_mut(lib[5], 11), "TTGGCCAA", _mut(lib[9], 3)), (2500, 1500)),
            (rec(lib[40], "GGATCCAT", lib[41]), (2500,)),
            (rec(lib[40], "GGATCCAA", lib[41]), (2000,)),
            (rec(lib[77], "CATCATCA", lib[78], q[:23] + "#" + q[24:]), (1500,))]


@functools.lru_cache(maxsize=None)
def file_sample():
    """(library, text, records), about 8 MB: 800 ordinary reads of 250 bases (window at 0), the hot records in long runs of
    different lengths, 300 ordinary reads with the cassette UP + guide + DOWN.  A reader that loses the tail of the hot
    stretch, or anything behind it, changes the counts of features 5, 40, 77 or of the cassette reads.  At gzip level 6
    the head takes 66 KiB and the hot stretch 30 KiB: with chunks of 64 KiB the second chunk starts inside the hot stretch"""
    lib = library()
    hot = hot_records()
    runs = [(r, n) for k in range(3) for r, ns in hot if k < len(ns) for n in (ns[k],)]
    head = synth.make_fastq(synth.Spec(seed=91, n_reads=800, read_len=250), lib)
    tail = synth.make_fastq(synth.Spec(seed=92, n_reads=300, read_len=100, cassette=True, up=UP, down=DOWN, max_offset=40), lib)
    text = head + b"".join(r * n for r, n in runs) + tail
    return lib, text, 1100 + sum(n for _, n in runs)


@functools.lru_cache(maxsize=None)
def paired_sample():
    """(library, st1, st2, length, R1 text, R2 text, pairs): 1100 ordinary pairs of 250 + 250 bases, five of them also in
    long runs behind the first 800 (7 MB a mate; the same geometry as file_sample's)"""
    import paired_cases as PC
    st1, st2, length = (5,), (30,), 10
    lib = PC.pair_library(300, length, 1, 1, 9)
    fq = PC.make_pairs_uniform(lib, length, list(st1), list(st2), True, 1100, seed=4, len1=250, len2=250)
    out = []
    for text in fq:
        lines = text.split(b"\n")
        recs = [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, 4400, 4)]
        runs = b"".join(recs[k] * n for k, n in ((0, 5000), (1, 3000), (2, 2000), (0, 2500), (3, 1000), (4, 500)))
        out.append(b"".join(recs[:800]) + runs + b"".join(recs[800:]))
    return lib, st1, st2, length, out[0], out[1], 1100 + 14000
