"""ctypes binding of libf2q_hip.so (include/f2q.h).

This is the only way the Python harness reaches the GPU: there is no Python or
CPU implementation of the counting path in this package.  If the shared library
is missing or no HIP device is usable, construction raises ``F2QError``.
"""
import ctypes as C
import os

import numpy as np

MAX_ITER = 16
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("F2Q_LIB_PATH") or os.path.join(_HERE, "lib", "libf2q_hip.so")   # override: diagnostic builds
STAT_NAMES = ("reads", "perfect_counter", "imperfect_counter", "non_aligned_counter", "quality_failed")

EXPORTS = (
    "f2q_version", "f2q_build_id", "f2q_create", "f2q_destroy", "f2q_last_error", "f2q_set_features", "f2q_count_block",
    "f2q_count_file", "f2q_count_file_shard", "f2q_file_pieces", "f2q_census_pieces", "f2q_count_pieces", "f2q_synth_create", "f2q_block_from_fastq", "f2q_count_resident", "f2q_count_resident_queued", "f2q_queued_times", "f2q_block_info",
    "f2q_block_free", "f2q_synth_fastq", "f2q_synth_library", "f2q_reset_counts", "f2q_read_counts",
    "f2q_counts_device_ptr", "f2q_stream", "f2q_ec_size", "f2q_ec_fetch", "f2q_set_read_base", "f2q_synth_guides",
    "f2q_text_upload", "f2q_count_text", "f2q_text_free", "f2q_text_from_bgzf", "f2q_text_read",
    "f2q_set_mate2", "f2q_count_block_paired", "f2q_block_from_fastq_paired", "f2q_count_file_paired",
    "f2q_set_assign_library", "f2q_ec_assign", "f2q_ec_fetch_assigned",
    "f2q_ec_collapse", "f2q_ec_fetch_collapsed",
    "f2q_set_umi", "f2q_read_umis", "f2q_umi_collapse",
    "f2q_set_umi_reads", "f2q_umi_collapse_directional", "f2q_umi_pairs",
    "f2q_set_umi_paired", "f2q_set_umi_header",
    "f2q_set_sample_barcodes", "f2q_read_demux",
    "f2q_set_strand", "f2q_read_strands",
    "f2q_set_parts", "f2q_parts_info", "f2q_read_parts", "f2q_parts_recombinants",
    "f2q_set_stagger", "f2q_read_stagger",
    "f2q_set_indel", "f2q_read_indels",
)

STRANDS = ("fwd", "rev", "both")            # F2Q_STRAND_FWD / _REV / _BOTH
PARTS_CLASSES = ("pair_perfect", "pair_imperfect", "recombinant", "part1_only", "part2_only", "neither")   # F2Q_PARTS_*

ERRORS = {-1: "EINVAL", -2: "ENODEVICE", -3: "EHIP", -4: "ENOMEM", -5: "EIO", -6: "ETRUNCATED", -7: "ESTATE",
          -8: "EUNSUPPORTED", -9: "EPAIRING"}
F2Q_ETRUNCATED = -6
F2Q_EPAIRING = -9


class F2QError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libf2q_hip: {ERRORS.get(code, code)}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [
        ("mode", C.c_int32), ("miss", C.c_int32), ("phred", C.c_int32), ("length", C.c_int32),
        ("n_start", C.c_int32), ("start", C.c_int32 * MAX_ITER),
        ("n_upstream", C.c_int32), ("n_downstream", C.c_int32),
        ("upstream", C.c_char_p * MAX_ITER), ("downstream", C.c_char_p * MAX_ITER),
        ("miss_search_up", C.c_int32), ("miss_search_down", C.c_int32),
        ("qual_up", C.c_int32), ("qual_down", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32 * 7),
    ]


class Synth(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64), ("n_reads", C.c_uint64), ("first_read", C.c_uint64),
        ("read_len", C.c_int32), ("start", C.c_int32), ("cassette", C.c_int32), ("max_offset", C.c_int32),
        ("up", C.c_char_p), ("down", C.c_char_p),
        ("t_sub", C.c_uint32), ("t_rand", C.c_uint32), ("t_n", C.c_uint32), ("t_lowq", C.c_uint32),
        ("t_q29", C.c_uint32), ("t_q28", C.c_uint32), ("reserved", C.c_int32 * 4),
    ]


class Timing(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("reads", C.c_uint64),
                ("fast_reads", C.c_uint64), ("general_reads", C.c_uint64), ("launches", C.c_uint32),
                ("path", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


def make_params(mode="C", miss=1, phred=30, length=20, start="0", upstream=None, downstream=None,
                miss_search_up=0, miss_search_down=0, qual_up=30, qual_down=30, device=0):
    """Build an f2q_params from the reference's ``param`` keys (fast2q.py:1246-1309).
    Returns (struct, keepalive list)."""
    p = Params()
    keep = []
    p.mode = 0 if str(mode).upper() == "C" else 1
    p.miss, p.phred, p.length = int(miss), int(phred), int(length)
    p.miss_search_up, p.miss_search_down = int(miss_search_up), int(miss_search_down)
    p.qual_up, p.qual_down, p.device = int(qual_up), int(qual_down), int(device)

    def split(x):
        if x is None:
            return []
        return list(x) if isinstance(x, (list, tuple)) else str(x).split(",")

    ups, downs = split(upstream), split(downstream)
    if not ups and not downs:
        starts = [int(n) for n in str(start).split(",")]            # fast2q.py:539
        if len(starts) > MAX_ITER:
            raise ValueError("at most 16 start positions")
        p.n_start = len(starts)
        for i, s in enumerate(starts):
            p.start[i] = s
    else:
        if len(ups) > MAX_ITER or len(downs) > MAX_ITER:
            raise ValueError("at most 16 search sequences")
        p.n_upstream, p.n_downstream = len(ups), len(downs)
        for i, s in enumerate(ups):
            b = s.encode(); keep.append(b); p.upstream[i] = b
        for i, s in enumerate(downs):
            b = s.encode(); keep.append(b); p.downstream[i] = b
    return p, keep


def make_synth(seed=0xF2A5, n_reads=1000, first_read=0, read_len=150, start=0, cassette=False, up="", down="",
               max_offset=100, p_sub=0.10, p_rand=0.05, p_n=0.005, p_lowq=0.06, p_q29=0.01, p_q28=0.01):
    """f2q_synth from the keyword set of tests/synth.py Spec."""
    def p32(x):
        return min(int(round(x * 4294967296.0)), 0xFFFFFFFF)
    s = Synth()
    s.seed, s.n_reads, s.first_read = seed, n_reads, first_read
    s.read_len, s.start, s.cassette, s.max_offset = read_len, start, 1 if cassette else 0, max_offset
    keep = [up.encode(), down.encode()]
    s.up, s.down = keep[0], keep[1]
    s.t_sub, s.t_rand, s.t_n = p32(p_sub), p32(p_sub + p_rand), p32(p_n)
    s.t_lowq, s.t_q29, s.t_q28 = p32(p_lowq), p32(p_lowq + p_q29), p32(p_lowq + p_q29 + p_q28)
    return s, keep


_lib = None


def load(path=None):
    """dlopen libf2q_hip.so and declare the prototypes.  Raises F2QError when it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise F2QError(-2, f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(path)
    vp, u64p, i64p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
    L.f2q_version.restype = C.c_int
    L.f2q_build_id.restype = C.c_char_p
    L.f2q_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.f2q_destroy.argtypes = [vp]; L.f2q_destroy.restype = None
    L.f2q_last_error.argtypes = [vp]; L.f2q_last_error.restype = C.c_char_p
    L.f2q_set_features.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32]
    L.f2q_count_block.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(Timing)]
    L.f2q_count_file.argtypes = [vp, C.c_char_p, C.POINTER(Timing)]
    L.f2q_text_upload.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
    L.f2q_count_text.argtypes = [vp, vp, C.POINTER(C.c_size_t), C.POINTER(Timing)]
    L.f2q_text_free.argtypes = [vp, vp]; L.f2q_text_free.restype = None
    L.f2q_text_from_bgzf.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
    L.f2q_text_read.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.f2q_count_file_shard.argtypes = [vp, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(Timing)]
    L.f2q_file_pieces.argtypes = [C.c_char_p, C.c_uint64, u64p, C.POINTER(C.c_int)]
    L.f2q_census_pieces.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, u64p, C.c_uint64]
    L.f2q_count_pieces.argtypes = [vp, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, u64p, C.c_uint64, C.POINTER(Timing)]
    L.f2q_set_mate2.argtypes = [vp, C.POINTER(C.c_int32), C.c_int32, C.c_int32]
    L.f2q_count_block_paired.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(Timing)]
    L.f2q_block_from_fastq_paired.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(vp)]
    L.f2q_count_file_paired.argtypes = [vp, C.c_char_p, C.c_char_p, C.POINTER(Timing)]
    L.f2q_synth_create.argtypes = [vp, C.POINTER(Synth), C.POINTER(vp)]
    L.f2q_block_from_fastq.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
    L.f2q_count_resident.argtypes = [vp, vp, C.POINTER(Timing)]
    L.f2q_count_resident_queued.argtypes = [vp, vp]
    L.f2q_queued_times.argtypes = [vp, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]
    L.f2q_block_info.argtypes = [vp, u64p, u64p, u64p]
    L.f2q_block_free.argtypes = [vp, vp]; L.f2q_block_free.restype = None
    L.f2q_synth_fastq.argtypes = [vp, C.POINTER(Synth), C.c_uint64, C.c_uint64, vp, C.POINTER(C.c_size_t)]
    L.f2q_synth_library.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_char_p]
    L.f2q_synth_guides.argtypes = [vp, C.c_char_p, C.c_uint32, C.c_uint32]
    L.f2q_reset_counts.argtypes = [vp]
    L.f2q_set_read_base.argtypes = [vp, C.c_uint64]
    L.f2q_read_counts.argtypes = [vp, i64p, i64p]
    L.f2q_counts_device_ptr.argtypes = [vp, C.POINTER(vp), u64p]
    L.f2q_stream.argtypes = [vp]; L.f2q_stream.restype = vp
    L.f2q_ec_size.argtypes = [vp, u64p, u64p]
    L.f2q_ec_fetch.argtypes = [vp, C.c_char_p, u64p, i64p, u64p]
    L.f2q_set_assign_library.argtypes = [vp, C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32]
    L.f2q_ec_assign.argtypes = [vp, i64p, i64p, C.POINTER(Timing)]
    L.f2q_ec_fetch_assigned.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.f2q_ec_collapse.argtypes = [vp, C.c_int32, C.c_int32, i64p, C.POINTER(Timing)]
    L.f2q_ec_fetch_collapsed.argtypes = [vp, u64p, i64p]
    L.f2q_set_umi.argtypes = [vp, C.c_int32, C.c_int32]
    L.f2q_set_umi_paired.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.f2q_set_umi_header.argtypes = [vp, C.c_int32, C.c_int32]
    L.f2q_read_umis.argtypes = [vp, i64p, i64p]
    L.f2q_umi_collapse.argtypes = [vp, C.c_int32, i64p, i64p]
    L.f2q_set_umi_reads.argtypes = [vp, C.c_int32]
    L.f2q_umi_collapse_directional.argtypes = [vp, i64p, i64p]
    L.f2q_set_sample_barcodes.argtypes = [vp, C.c_char_p, C.c_uint32, C.c_int32, C.c_int32, C.c_int32]
    L.f2q_read_demux.argtypes = [vp, i64p, i64p, i64p]
    L.f2q_set_strand.argtypes = [vp, C.c_int32]
    L.f2q_read_strands.argtypes = [vp, i64p, i64p]
    u32p = C.POINTER(C.c_uint32)
    L.f2q_umi_pairs.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint64), u32p, u32p, u32p]
    L.f2q_set_parts.argtypes = [vp]
    L.f2q_set_stagger.argtypes = [vp, C.c_int32]
    L.f2q_read_stagger.argtypes = [vp, i64p, i64p, C.c_int32]
    L.f2q_set_indel.argtypes = [vp, C.c_int32]
    L.f2q_read_indels.argtypes = [vp, i64p, i64p, i64p, i64p, C.c_int32, i64p]
    L.f2q_parts_info.argtypes = [vp, u32p, u32p]
    L.f2q_read_parts.argtypes = [vp, i64p, i64p, i64p, i64p]
    L.f2q_parts_recombinants.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint64), u32p, u32p, u32p]
    if path == LIB_PATH:
        _lib = L
    return L


def build_id():
    """the source hash the loaded library was compiled from (include/f2q.h: f2q_build_id)"""
    return (load().f2q_build_id() or b"").decode()


def synth_library(seed, n, length):
    """n unique uniform ACGT strings (host helper of the library; == tests/synth.py make_library)."""
    L = load()
    buf = C.create_string_buffer(n * length)
    rc = L.f2q_synth_library(seed, n, length, buf)
    if rc:
        raise F2QError(rc, "f2q_synth_library")
    raw = buf.raw
    return [raw[i * length:(i + 1) * length].decode() for i in range(n)]


class DeviceText:
    """FASTQ text resident in device memory (f2q_text)"""
    def __init__(self, counter, h):
        self._c, self._h = counter, h

    def free(self):
        if self._h:
            self._c._L.f2q_text_free(self._c._h, self._h)
            self._h = None

    def read(self):
        """the text's bytes, copied back to the host"""
        n = C.c_size_t(0)
        self._c._check(self._c._L.f2q_text_read(self._c._h, self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        self._c._check(self._c._L.f2q_text_read(self._c._h, self._h, C.cast(buf, C.c_void_p), n.value, C.byref(n)))
        return buf.raw[:n.value]


class Block:
    """A device-resident block of reads."""

    def __init__(self, owner, handle):
        self._o, self._h = owner, handle

    def info(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._o._L.f2q_block_info(self._h, C.byref(a), C.byref(b), C.byref(c))
        return {"n_reads": a.value, "n_general": b.value, "device_bytes": c.value}

    def free(self):
        if self._h:
            self._o._L.f2q_block_free(self._o._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Counter:
    """One counting context (f2q_ctx) bound to one GPU.

    ``features``: ordered list of sequences as features_loader leaves them
    (upper-case, blanks removed, unique); row i of the count vector is feature i.

    ``umi=(S, L)`` counts distinct UMIs per feature (f2q_set_umi): the UMI is read positions [S, S + L); Counter mode,
    single reads; ``read_umis()`` returns them, ``collapse_umis()`` the molecules left when UMIs of one feature at Hamming
    distance 1 are joined.  ``umi_reads=True`` also keeps the reads of every (feature, UMI) pair (f2q_set_umi_reads):
    ``collapse_umis(rule="directional")`` and ``umi_pairs()`` need them.

    ``start2`` ("b[,b...]" or a list) makes it a paired context (f2q_set_mate2): ``start`` names the windows in mate 1,
    ``start2`` those in mate 2, ``rc2`` takes mate 2 reverse-complemented; such a context counts with the *_paired calls.
    ``umi_paired=((S1, L1) or None, (S2, L2) or None)`` makes a paired context a UMI context (f2q_set_umi_paired): the UMI
    is mate 1's [S1, S1 + L1) followed by [S2, S2 + L2) of mate 2 as sequenced, whatever ``rc2`` says; ``umi_length`` is
    the total number of bases, and everything ``umi=`` offers works on it (``umi=`` itself stays single-read only).
    ``umi_header=(sep, L)`` takes the UMI from the read header instead (f2q_set_umi_header): the L bases behind the last
    ``sep`` (one character, or its byte value) of the read id, mate 1's on a paired context; ``umi_length`` answers L.

    ``sample_barcodes=(S, [seq, ...])`` demultiplexes a pooled sample by an inline barcode (f2q_set_sample_barcodes): every
    read carries one of the barcodes (all of one length, 1 .. 16 bases, at most 1024) at read positions [S, S + L);
    ``barcode_mismatch`` 0 / 1 is the number of substitutions allowed.  Counter mode, single reads, no UMIs;
    ``read_demux()`` returns the count matrix per sample, the five counters per sample and the five barcode verdicts.

    ``strand="fwd" | "rev" | "both"`` is the orientation single reads are counted in (f2q_set_strand): as written, as their
    reverse complement, or as written first and as the reverse complement when that assigned no feature.  Counter mode,
    single reads, no UMIs, no sample barcodes; ``read_strands()`` returns the reads assigned on the reverse strand per
    feature and the four strand counters.

    ``parts=True`` matches each part of a pair library alone (f2q_set_parts): Counter mode, exactly two fixed windows
    (``start="a,b"``, or one window per mate with ``start2``), every feature "A:B".  ``parts_info()`` gives the sizes of
    the two part libraries (ids in first-occurrence order over the features), ``read_parts()`` the counts per feature by
    the part rule, the two marginals and the six read classes, ``parts_recombinants()`` the recombinant pairs.

    ``stagger=N`` (1 .. 32) tries the one fixed window at the starts s .. s + N (f2q_set_stagger): the earliest exact start
    wins, else the earliest start within ``miss``.  Counter mode, single reads, one ``start``, no UMIs, sample barcodes,
    strand mode or parts; ``read_stagger()`` returns the reads assigned perfectly / imperfectly at each offset.  0: a plain
    context.

    ``indel=True`` reports the reads whose feature carries one inserted or deleted base (f2q_set_indel): a read the plain rule
    assigns nothing is tried as a one-base deletion and as a one-base insertion of every feature of exactly ``length`` bases.
    Counts and the five counters stay what they are without it.  Counter mode, single reads, one ``start``, ``length`` 2 .. 31,
    no UMIs, sample barcodes, strand mode, parts or stagger; ``read_indels()`` returns the deletion and insertion reads per
    feature and per position and the four totals.
    """

    def __init__(self, features=None, lib_path=None, start2=None, rc2=False, umi=None, umi_reads=False, umi_paired=None, umi_header=None,
                 sample_barcodes=None, barcode_mismatch=0, strand="fwd", parts=False, stagger=0, indel=False, **params):
        self._L = load(lib_path)
        self._p, self._keep = make_params(**params)
        self.mode = "C" if self._p.mode == 0 else "EC"
        h = C.c_void_p()
        rc = self._L.f2q_create(C.byref(self._p), C.byref(h))
        if rc:
            raise F2QError(rc, (self._L.f2q_last_error(None) or b"").decode())
        self._h = h
        self.n_features = 0
        self.n_assign = 0
        self.paired = False
        self.umi = None
        self.umi_paired = None
        self.umi_header = None
        self.umi_length = 0              # bases of a UMI (set_umi / set_umi_paired), 0: no UMI context
        self.umi_reads = False
        self.sample_barcodes = None      # (start, [barcodes]) of a demultiplexing context
        self.barcode_mismatch = 0
        self.strand = "fwd"              # the strand mode of the context (set_strand)
        self.parts = False               # each part of a pair library matched alone (set_parts)
        self.stagger = 0                 # extra starts the window is tried at (set_stagger)
        self.indel = False               # one-base insertions and deletions are reported (set_indel)
        try:
            self.set_strand(strand)
            if sample_barcodes is not None:
                self.set_sample_barcodes(sample_barcodes[0], sample_barcodes[1], barcode_mismatch)
            elif barcode_mismatch:
                raise ValueError("barcode_mismatch needs sample_barcodes")
            if start2 is not None:
                self.set_mate2(start2, rc2)
            if umi is not None:
                self.set_umi(*umi)
            if umi_paired is not None:
                self.set_umi_paired(*umi_paired)
            if umi_header is not None:
                self.set_umi_header(*umi_header)
            if umi_reads:
                self.set_umi_reads(True)
            if parts:
                self.set_parts()
            if stagger:
                self.set_stagger(stagger)
            if indel:
                self.set_indel(True)
        except BaseException:
            self.close()
            raise
        if features is not None:
            self.set_features(features)

    # -- helpers --
    def _check(self, rc):
        if rc:
            raise F2QError(rc, (self._L.f2q_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.f2q_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- library --
    @staticmethod
    def _blob(seqs):
        enc = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
        offs = np.zeros(len(enc) + 1, dtype=np.uint32)
        if enc:
            offs[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64).astype(np.uint32)
        return b"".join(enc), offs, len(enc)

    def set_features(self, seqs):
        blob, offs, n = self._blob(seqs)
        self._check(self._L.f2q_set_features(self._h, blob, offs.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        self.n_features = n

    def set_assign_library(self, seqs):
        """Extract+Count contexts: the library ec_assign matches the extracted keys against (once per context)"""
        blob, offs, n = self._blob(seqs)
        self._check(self._L.f2q_set_assign_library(self._h, blob, offs.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        self.n_assign = n

    def set_mate2(self, start2, rc2=False):
        """windows of mate 2 (paired-end samples); before set_features"""
        st = [int(x) for x in (start2 if isinstance(start2, (list, tuple)) else str(start2).split(","))]
        arr = (C.c_int32 * max(len(st), 1))(*st)
        self._check(self._L.f2q_set_mate2(self._h, arr, len(st), 1 if rc2 else 0))
        self.paired = True

    def set_umi(self, start, length):
        """the UMI window of every read (f2q_set_umi); before counting"""
        self._check(self._L.f2q_set_umi(self._h, int(start), int(length)))
        self.umi = (int(start), int(length))
        self.umi_length = int(length)

    def set_umi_paired(self, part1, part2):
        """the UMI of every pair (f2q_set_umi_paired): part1 = (S1, L1) in mate 1 or None, part2 = (S2, L2) in mate 2 as
        sequenced or None; after set_mate2, before counting"""
        p1, p2 = [(0, 0) if p is None else (int(p[0]), int(p[1])) for p in (part1, part2)]
        self._check(self._L.f2q_set_umi_paired(self._h, p1[0], p1[1], p2[0], p2[1]))
        self.umi_paired = (p1 if p1[1] else None, p2 if p2[1] else None)
        self.umi_length = p1[1] + p2[1]

    def set_umi_header(self, sep, length):
        """the UMI of every read (pair: of mate 1) is in its header (f2q_set_umi_header): ``length`` bases behind the last
        ``sep`` of the read id; in place of set_umi / set_umi_paired, before counting"""
        if isinstance(sep, (bytes, str)):
            if len(sep) != 1:
                raise ValueError(f"the header UMI separator is one character, not {sep!r}")
            sep = ord(sep)
        self._check(self._L.f2q_set_umi_header(self._h, int(sep), int(length)))
        self.umi_header = (chr(int(sep)), int(length))
        self.umi_length = int(length)

    def set_umi_reads(self, on=True):
        """keep the reads of every (feature, UMI) pair (f2q_set_umi_reads); after set_umi, before counting"""
        self._check(self._L.f2q_set_umi_reads(self._h, 1 if on else 0))
        self.umi_reads = bool(on)

    def set_sample_barcodes(self, start, seqs, mismatch=0):
        """the inline sample barcodes of a pooled sample (f2q_set_sample_barcodes); before counting"""
        enc = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
        if len({len(b) for b in enc}) > 1:
            raise ValueError("the sample barcodes must all have one length")
        length = len(enc[0]) if enc else 0
        self._check(self._L.f2q_set_sample_barcodes(self._h, b"".join(enc), len(enc), length, int(start), int(mismatch)))
        self.sample_barcodes = (int(start), [b.decode("latin-1").upper() for b in enc])
        self.barcode_mismatch = int(mismatch)

    def set_strand(self, strand):
        """the orientation single reads are counted in: "fwd", "rev" or "both" (f2q_set_strand); before counting"""
        if strand not in STRANDS:
            raise ValueError(f"strand is one of {', '.join(STRANDS)}, not {strand!r}")
        self._check(self._L.f2q_set_strand(self._h, STRANDS.index(strand)))
        if strand != "fwd":
            self.strand = strand

    def set_parts(self):
        """match each part of a pair library alone and count recombinants (f2q_set_parts); after set_mate2, before counting"""
        self._check(self._L.f2q_set_parts(self._h))
        self.parts = True

    def set_stagger(self, n):
        """try the one fixed window at the starts s .. s + n, 0 <= n <= 32 (f2q_set_stagger); before counting; 0 clears it"""
        self._check(self._L.f2q_set_stagger(self._h, int(n)))
        self.stagger = int(n)

    def read_stagger(self):
        """(perfect[n + 1], imperfect[n + 1]) as int64 arrays (f2q_read_stagger): reads assigned at each offset"""
        out = [np.zeros(self.stagger + 1, dtype=np.int64) for _ in range(2)]
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.f2q_read_stagger(self._h, out[0].ctypes.data_as(i64p), out[1].ctypes.data_as(i64p), self.stagger + 1))
        return tuple(out)

    def set_indel(self, on=True):
        """report reads whose feature carries one inserted or deleted base (f2q_set_indel); before counting; False clears it"""
        self._check(self._L.f2q_set_indel(self._h, 1 if on else 0))
        self.indel = bool(on)

    def read_indels(self):
        """(del_counts[n_features], ins_counts[n_features], del_pos[L], ins_pos[L], totals[4]) as int64 arrays
        (f2q_read_indels); totals = reads tried, deletion reads, insertion reads, ambiguous reads"""
        L = int(self._p.length)
        out = [np.zeros(n, dtype=np.int64) for n in (self.n_features, self.n_features, L, L, 4)]
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.f2q_read_indels(self._h, *(a.ctypes.data_as(i64p) for a in out[:4]), L, out[4].ctypes.data_as(i64p)))
        return tuple(out)

    def parts_info(self):
        """(n1, n2): the sizes of the two part libraries (f2q_parts_info)"""
        n1, n2 = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.f2q_parts_info(self._h, C.byref(n1), C.byref(n2)))
        return n1.value, n2.value

    def read_parts(self):
        """(parts_counts[n_features], part1_reads[n1], part2_reads[n2], classes[6]) as int64 arrays (f2q_read_parts);
        classes in the order of PARTS_CLASSES"""
        n1, n2 = self.parts_info()
        i64p = C.POINTER(C.c_int64)
        out = [np.zeros(max(n, 1), dtype=np.int64) for n in (self.n_features, n1, n2, 6)]
        self._check(self._L.f2q_read_parts(self._h, *[a.ctypes.data_as(i64p) for a in out]))
        return out[0][:self.n_features], out[1][:n1], out[2][:n2], out[3]

    def parts_recombinants(self):
        """(part1[n], part2[n], reads[n]) as uint32 arrays sorted by (part1, part2): every recombinant pair the set holds
        (f2q_parts_recombinants)"""
        u32p = C.POINTER(C.c_uint32)
        n = C.c_uint64(0)
        self._check(self._L.f2q_parts_recombinants(self._h, 0, C.byref(n), None, None, None))
        out = [np.zeros(max(n.value, 1), dtype=np.uint32) for _ in range(3)]
        self._check(self._L.f2q_parts_recombinants(self._h, max(n.value, 1), C.byref(n), *[a.ctypes.data_as(u32p) for a in out]))
        return tuple(a[:n.value] for a in out)

    # -- counting: paired-end --
    @staticmethod
    def _ptr(data):
        data = data if isinstance(data, bytes) else bytes(data)
        return data, C.cast(C.c_char_p(data), C.c_void_p)

    def count_block_paired(self, data1, data2, want_timing=False):
        """fastq_parser over two FASTQ buffers in lockstep; returns (bytes consumed of each) (and timing)"""
        d1, p1 = self._ptr(data1)
        d2, p2 = self._ptr(data2)
        u1, u2, t = C.c_size_t(0), C.c_size_t(0), Timing()
        self._check(self._L.f2q_count_block_paired(self._h, p1, len(d1), p2, len(d2), C.byref(u1), C.byref(u2), C.byref(t)))
        return ((u1.value, u2.value), t.as_dict()) if want_timing else (u1.value, u2.value)

    def block_from_fastq_paired(self, data1, data2):
        d1, p1 = self._ptr(data1)
        d2, p2 = self._ptr(data2)
        h = C.c_void_p()
        self._check(self._L.f2q_block_from_fastq_paired(self._h, p1, len(d1), p2, len(d2), C.byref(h)))
        return Block(self, h)

    def count_file_paired(self, path1, path2):
        """Counts the two files of a paired sample.  Returns (timing dict, truncated flag); F2QError with code
        F2Q_EPAIRING when one file holds records beyond the other's last (the common pairs are counted)."""
        t = Timing()
        rc = self._L.f2q_count_file_paired(self._h, os.fsencode(path1), os.fsencode(path2), C.byref(t))
        if rc == F2Q_ETRUNCATED:
            return t.as_dict(), True
        self._check(rc)
        return t.as_dict(), False

    # -- counting --
    def count_block(self, data, want_timing=False):
        """fastq_parser over a bytes-like FASTQ buffer; returns bytes consumed (and timing)."""
        mv = memoryview(data)
        n = mv.nbytes
        if isinstance(data, bytes):
            ptr = C.cast(C.c_char_p(data), C.c_void_p)          # the bytes object's own buffer, no copy
        elif isinstance(data, bytearray):
            buf = (C.c_char * n).from_buffer(data)
            ptr = C.cast(buf, C.c_void_p)
        else:
            arr = np.frombuffer(mv, dtype=np.uint8)
            ptr = C.c_void_p(arr.ctypes.data)
        used, t = C.c_size_t(0), Timing()
        self._check(self._L.f2q_count_block(self._h, ptr, n, C.byref(used), C.byref(t)))
        return (used.value, t.as_dict()) if want_timing else used.value

    def text_upload(self, data):
        """copy at most 1 GiB of FASTQ text into device memory once -> DeviceText (count_text takes it from there)"""
        data = bytes(data)
        h = C.c_void_p()
        self._check(self._L.f2q_text_upload(self._h, C.cast(C.c_char_p(data), C.c_void_p), len(data), C.byref(h)))
        return DeviceText(self, h)

    def text_from_bgzf(self, data):
        """inflate an in-memory BGZF buffer on the device -> (DeviceText, truncated); truncated: a member is damaged and
        the text holds the members before it"""
        data = bytes(data)
        h = C.c_void_p()
        rc = self._L.f2q_text_from_bgzf(self._h, C.cast(C.c_char_p(data), C.c_void_p), len(data), C.byref(h))
        if rc == F2Q_ETRUNCATED and h.value:
            return DeviceText(self, h), True
        self._check(rc)
        return DeviceText(self, h), False

    def count_text(self, text, want_timing=False):
        """frame, pack and count FASTQ text that already sits in device memory; returns bytes consumed (and timing)"""
        used, t = C.c_size_t(0), Timing()
        self._check(self._L.f2q_count_text(self._h, text._h, C.byref(used), C.byref(t)))
        return (used.value, t.as_dict()) if want_timing else used.value

    def count_file(self, path):
        """Counts a whole .fastq / .gz file.  Returns (timing dict, truncated flag)."""
        t = Timing()
        rc = self._L.f2q_count_file(self._h, os.fsencode(path), C.byref(t))
        if rc == F2Q_ETRUNCATED:
            return t.as_dict(), True
        self._check(rc)
        return t.as_dict(), False

    def count_file_shard(self, path, rank, world):
        """This rank's share of a file that `world` processes count together.  Returns (timing dict, truncated flag)."""
        t = Timing()
        rc = self._L.f2q_count_file_shard(self._h, os.fsencode(path), rank, world, C.byref(t))
        if rc == F2Q_ETRUNCATED:
            return t.as_dict(), True
        self._check(rc)
        return t.as_dict(), False

    # -- a plain or BGZF file shared out by pieces: nobody reads or inflates foreign bytes (include/f2q.h, f2q_file_pieces ...) --
    def file_pieces(self, path, piece_bytes):
        """(number of pieces, shardable)"""
        n, ok = C.c_uint64(), C.c_int()
        rc = self._L.f2q_file_pieces(os.fsencode(path), piece_bytes, C.byref(n), C.byref(ok))
        if rc:
            raise F2QError(rc, (self._L.f2q_last_error(None) or b"").decode())
        return n.value, bool(ok.value)

    def census_pieces(self, path, rank, world, piece_bytes, n_pieces):
        """uint64[2 * n_pieces]: newline count and ends-with-newline flag of this rank's pieces (zeros elsewhere)"""
        census = np.zeros(2 * n_pieces, dtype=np.uint64)
        rc = self._L.f2q_census_pieces(os.fsencode(path), rank, world, piece_bytes, census.ctypes.data_as(C.POINTER(C.c_uint64)), n_pieces)
        if rc:
            raise F2QError(rc, (self._L.f2q_last_error(None) or b"").decode())
        return census

    def count_pieces(self, path, rank, world, piece_bytes, census):
        """counts the records that start in this rank's pieces; census = the ranks' census vectors summed"""
        census = np.ascontiguousarray(census, dtype=np.uint64)
        t = Timing()
        self._check(self._L.f2q_count_pieces(self._h, os.fsencode(path), rank, world, piece_bytes,
                                             census.ctypes.data_as(C.POINTER(C.c_uint64)), len(census) // 2, C.byref(t)))
        return t.as_dict()

    def block_from_fastq(self, data):
        data = bytes(data)
        h = C.c_void_p()
        self._check(self._L.f2q_block_from_fastq(self._h, C.cast(C.c_char_p(data), C.c_void_p), len(data), C.byref(h)))
        return Block(self, h)

    def synth_guides(self, guides):
        """guide set for the synthetic generator (needed by Extract+Count contexts, which take no library)"""
        glen = len(guides[0])
        self._check(self._L.f2q_synth_guides(self._h, "".join(guides).encode(), len(guides), glen))

    def synth_create(self, guides=None, **spec):
        if guides is not None:
            self.synth_guides(guides)
        s, keep = make_synth(**spec)
        h = C.c_void_p()
        self._check(self._L.f2q_synth_create(self._h, C.byref(s), C.byref(h)))
        return Block(self, h)

    def synth_fastq(self, lo=0, hi=None, guides=None, **spec):
        if guides is not None:
            self.synth_guides(guides)
        s, keep = make_synth(**spec)
        hi = s.n_reads if hi is None else hi
        n = C.c_size_t(0)
        self._check(self._L.f2q_synth_fastq(self._h, C.byref(s), lo, hi, None, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        self._check(self._L.f2q_synth_fastq(self._h, C.byref(s), lo, hi, C.c_void_p(buf.ctypes.data), C.byref(n)))
        return buf[:n.value]

    def count_resident(self, block):
        t = Timing()
        self._check(self._L.f2q_count_resident(self._h, block._h, C.byref(t)))
        return t.as_dict()

    def count_resident_queued(self, block):
        """queue the hot path over a resident block on the context's stream without waiting (see queued_times)"""
        self._check(self._L.f2q_count_resident_queued(self._h, block._h))

    def queued_times(self, cap=4096):
        """wait for the stream; kernel time (ms) of every step queued since the last call"""
        buf = (C.c_float * cap)()
        n = C.c_uint32()
        self._check(self._L.f2q_queued_times(self._h, buf, cap, C.byref(n)))
        return [float(buf[i]) for i in range(min(n.value, cap))]

    def set_read_base(self, first_read_index):
        self._check(self._L.f2q_set_read_base(self._h, int(first_read_index)))

    # -- results --
    def reset(self):
        self._check(self._L.f2q_reset_counts(self._h))

    def read_counts(self):
        counts = np.zeros(max(self.n_features, 1), dtype=np.int64)
        stats = np.zeros(5, dtype=np.int64)
        self._check(self._L.f2q_read_counts(self._h, counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                            stats.ctypes.data_as(C.POINTER(C.c_int64))))
        return counts[:self.n_features], stats

    def read_demux(self):
        """(matrix[nb + 1, n_features], sample_stats[nb + 1, 5], verdicts[5]) as int64 arrays (f2q_read_demux): row b is
        barcode b, row nb the unassigned reads; verdicts = exact, one mismatch, ambiguous, no match, unreadable"""
        nb = len(self.sample_barcodes[1]) if self.sample_barcodes else 0
        matrix = np.zeros((nb + 1, max(self.n_features, 1)), dtype=np.int64)
        sstats = np.zeros((nb + 1, 5), dtype=np.int64)
        verdicts = np.zeros(5, dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.f2q_read_demux(self._h, matrix.ctypes.data_as(i64p) if self.n_features else None,
                                           sstats.ctypes.data_as(i64p), verdicts.ctypes.data_as(i64p)))
        return matrix[:, :self.n_features], sstats, verdicts

    def read_strands(self):
        """(rev_counts[n_features], extra[4]) as int64 arrays (f2q_read_strands): reads assigned on the reverse strand per
        feature; extra = assigned forward, reverse perfect, reverse imperfect, reverse strands examined"""
        rev = np.zeros(max(self.n_features, 1), dtype=np.int64)
        extra = np.zeros(4, dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        self._check(self._L.f2q_read_strands(self._h, rev.ctypes.data_as(i64p), extra.ctypes.data_as(i64p)))
        return rev[:self.n_features], extra

    def read_umis(self):
        """(umis[n_features], umi_reads, umi_failed): distinct UMIs per feature, assigned reads with a valid / an invalid UMI"""
        umis = np.zeros(max(self.n_features, 1), dtype=np.int64)
        extra = np.zeros(2, dtype=np.int64)
        self._check(self._L.f2q_read_umis(self._h, umis.ctypes.data_as(C.POINTER(C.c_int64)),
                                          extra.ctypes.data_as(C.POINTER(C.c_int64))))
        return umis[:self.n_features], int(extra[0]), int(extra[1])

    def collapse_umis(self, dist=1, rule="cluster"):
        """(molecules[n_features], pairs, edges): the UMIs of a feature that differ in one base joined, the groups counted
        (f2q_umi_collapse); pairs = (feature, UMI) pairs held, edges = joined pairs of them.  dist=0: read_umis()'s array.
        rule="directional" (dist 1 only; needs umi_reads=True): a UMI absorbs a neighbour only when it has at least
        2 * reads - 1 of the neighbour's reads (f2q_umi_collapse_directional); edges = pairs of UMIs one base apart"""
        if rule == "directional":
            if int(dist) != 1:
                raise ValueError("the directional rule collapses at distance 1")
            return self.collapse_umis_directional()[:3]
        if rule != "cluster":
            raise ValueError("rule is 'cluster' or 'directional'")
        molecules = np.zeros(max(self.n_features, 1), dtype=np.int64)
        extra = np.zeros(2, dtype=np.int64)
        self._check(self._L.f2q_umi_collapse(self._h, int(dist), molecules.ctypes.data_as(C.POINTER(C.c_int64)),
                                             extra.ctypes.data_as(C.POINTER(C.c_int64))))
        return molecules[:self.n_features], int(extra[0]), int(extra[1])

    def collapse_umis_directional(self):
        """(molecules[n_features], pairs, edges, dominated, reads): f2q_umi_collapse_directional with all of its extra[4]"""
        molecules = np.zeros(max(self.n_features, 1), dtype=np.int64)
        extra = np.zeros(4, dtype=np.int64)
        self._check(self._L.f2q_umi_collapse_directional(self._h, molecules.ctypes.data_as(C.POINTER(C.c_int64)),
                                                         extra.ctypes.data_as(C.POINTER(C.c_int64))))
        return (molecules[:self.n_features],) + tuple(int(x) for x in extra)

    def umi_pairs(self):
        """(feature[n], codes[n], reads[n]) of every (feature, UMI) pair held, sorted by (feature, codes); codes: base j of
        the UMI in bits 2j .. 2j+1, A C G T = 0 .. 3 (f2q_umi_pairs; needs umi_reads=True)"""
        n = C.c_uint64()
        self._check(self._L.f2q_umi_pairs(self._h, 0, C.byref(n), None, None, None))
        arrs = [np.zeros(max(n.value, 1), dtype=np.uint32) for _ in range(3)]
        got = C.c_uint64()
        self._check(self._L.f2q_umi_pairs(self._h, n.value, C.byref(got), *[a.ctypes.data_as(C.POINTER(C.c_uint32)) for a in arrs]))
        return tuple(a[:got.value] for a in arrs)

    def counts_device_ptr(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._L.f2q_counts_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def stream(self):
        return self._L.f2q_stream(self._h)

    def ec_results(self):
        """[(key, count, first_read)] in first-occurrence order (== the reference's dict order)."""
        nk, nb = C.c_uint64(), C.c_uint64()
        self._check(self._L.f2q_ec_size(self._h, C.byref(nk), C.byref(nb)))
        n = nk.value
        keys = C.create_string_buffer(max(nb.value, 1))
        offs = np.zeros(n + 1, dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.int64)
        first = np.zeros(max(n, 1), dtype=np.uint64)
        self._check(self._L.f2q_ec_fetch(self._h, keys, offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                         first.ctypes.data_as(C.POINTER(C.c_uint64))))
        raw = keys.raw
        rows = [(raw[int(offs[i]):int(offs[i + 1])].decode("latin-1"), int(counts[i]), int(first[i])) for i in range(n)]
        rows.sort(key=lambda r: r[2])
        return rows

    def ec_assign(self, want_timing=False):
        """match every key the Extract+Count tables hold against the assign library: (counts, stats) as Counter mode
        would have returned them for the same reads (and the timing)"""
        counts = np.zeros(max(self.n_assign, 1), dtype=np.int64)
        stats = np.zeros(5, dtype=np.int64)
        t = Timing()
        self._check(self._L.f2q_ec_assign(self._h, counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                          stats.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(t)))
        return (counts[:self.n_assign], stats, t.as_dict()) if want_timing else (counts[:self.n_assign], stats)

    def ec_assigned(self):
        """[(key, count, first_read, feature, mismatches)] of the last ec_assign in first-occurrence order; feature is
        an index into the assign library, -1 (with mismatches -1) for a key assigned to none"""
        nk, nb = C.c_uint64(), C.c_uint64()
        self._check(self._L.f2q_ec_size(self._h, C.byref(nk), C.byref(nb)))
        n = nk.value
        keys = C.create_string_buffer(max(nb.value, 1))
        offs = np.zeros(n + 1, dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.int64)
        first = np.zeros(max(n, 1), dtype=np.uint64)
        feat = np.zeros(max(n, 1), dtype=np.int32)
        dist = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self._L.f2q_ec_fetch_assigned(self._h, feat.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  dist.ctypes.data_as(C.POINTER(C.c_int32))))
        self._check(self._L.f2q_ec_fetch(self._h, keys, offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                         first.ctypes.data_as(C.POINTER(C.c_uint64))))
        raw = keys.raw
        rows = [(raw[int(offs[i]):int(offs[i + 1])].decode("latin-1"), int(counts[i]), int(first[i]), int(feat[i]), int(dist[i]))
                for i in range(n)]
        rows.sort(key=lambda r: r[2])
        return rows

    ECC_EXTRA = ("eligible_keys", "absorbed_keys", "absorbed_reads", "longest_chain")

    def ec_collapse(self, dist=1, ratio=5, want_timing=False):
        """fold every plain extracted key of at most 29 bases into its neighbour one substitution away with the most
        reads, when that one has at least `ratio` times its reads (f2q_ec_collapse; dist 0: every key stays its own
        centroid): the four counters as a dict (and the timing)"""
        extra = np.zeros(4, dtype=np.int64)
        t = Timing()
        self._check(self._L.f2q_ec_collapse(self._h, int(dist), int(ratio), extra.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(t)))
        out = dict(zip(self.ECC_EXTRA, (int(x) for x in extra)))
        return (out, t.as_dict()) if want_timing else out

    def ec_collapsed(self):
        """[(key, reads, first_read, centroid_key, cluster_reads)] of the last ec_collapse in first-occurrence order;
        cluster_reads is 0 for a key that is no centroid"""
        nk, nb = C.c_uint64(), C.c_uint64()
        self._check(self._L.f2q_ec_size(self._h, C.byref(nk), C.byref(nb)))
        n = nk.value
        keys = C.create_string_buffer(max(nb.value, 1))
        offs = np.zeros(n + 1, dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.int64)
        first = np.zeros(max(n, 1), dtype=np.uint64)
        cent = np.zeros(max(n, 1), dtype=np.uint64)
        cluster = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self._L.f2q_ec_fetch_collapsed(self._h, cent.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   cluster.ctypes.data_as(C.POINTER(C.c_int64))))
        self._check(self._L.f2q_ec_fetch(self._h, keys, offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         counts.ctypes.data_as(C.POINTER(C.c_int64)),
                                         first.ctypes.data_as(C.POINTER(C.c_uint64))))
        raw = keys.raw
        text = [raw[int(offs[i]):int(offs[i + 1])].decode("latin-1") for i in range(n)]
        rows = [(text[i], int(counts[i]), int(first[i]), text[int(cent[i])], int(cluster[i])) for i in range(n)]
        rows.sort(key=lambda r: r[2])
        return rows
