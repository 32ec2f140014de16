"""Host harness of the MI355X-native 2FAST2Q counting path.

This module mirrors the reference's interface for the path (afombravo/2FAST2Q v2.8.1,
fast2q/fast2q.py) -- same function names, argument meaning, return shapes, output files -- so that
an existing ``2fast2q -c ...`` command line, features CSV and ``compiled.csv`` consumer keep working:

    features_loader (:125)   reads_counter (:514, the drop-in seam)   aligner (:752)
    csv_writer (:803)        compiling (:1316)   run_stats (:1386)    input_parser (:1171)
    initializer (:1082)      file_sizer_split (:1657)   main (:1691)

What is different: reads_counter() does no per-read work in Python.  It hands the file to
libf2q_hip.so (include/f2q.h) through ctypes; FASTQ framing, Phred masking, window / anchored
extraction, <= m mismatch matching and count accumulation all run in the library (HIP kernels on
gfx950).  The reference's Numba helpers, multiprocessing pools, memo caches and chunk splitter
have no counterpart here (--cp = samples in flight, as threads; --fs is accepted and ignored).  There is no CPU fallback: without
the library or a GPU, reads_counter raises.

Multi-GPU: when launched with one process per GPU (torchrun; RANK/WORLD_SIZE set) every rank
counts its share of each file's record blocks and the int64 count vector is summed with one
all-reduce (sharding.py).
"""
import argparse
import atexit
import csv
import datetime
import glob
import os
import re
import sys
import threading
import time
from collections import namedtuple
from dataclasses import dataclass, field
from pathlib import Path

from . import binding, sharding

version = "2.8.1+mi355x.0.1"


@dataclass
class Features:
    """name / read count of one feature; instances live in a dict keyed by sequence (:21-44)"""
    name: str
    counts: int


def colourful_errors(warning_type, error):
    """timestamped INFO / WARNING / FATAL line (:46-67); no colour codes (colorama is optional upstream only)"""
    print(f" {datetime.datetime.now().strftime('%c')} [{warning_type}] {error}")


def path_finder(folder_path, extension):
    found = []
    for ext in extension:
        for filename in glob.glob(os.path.join(folder_path, ext)):
            found.append([filename, os.path.getsize(filename)])
    return found


def path_parser(folder_path, extension):
    """files of the given patterns, by size; the *reads.csv temporaries by name (:91-123)"""
    pathing = path_finder(folder_path, extension)
    if extension != ['*reads.csv']:
        ordered = sorted(pathing, key=lambda e: e[-1])
        if not ordered:
            colourful_errors("FATAL", f"Check the path to the {extension} files folder. No files of this type found.\n")
            sys.exit()
        return ordered
    return [p[0] for p in sorted(pathing)]


def features_loader(guides):
    """{SEQUENCE: Features(name, 0)} from a 2-column csv (:125-186): separators ',' ';' tab are tried in
    turn; sequences are upper-cased with blanks removed; a repeated sequence keeps its first name."""
    colourful_errors("INFO", "Loading Features")
    if not os.path.isfile(guides):
        colourful_errors("FATAL", f"Check the path to the features file.\nNo .csv file found in the following path: {guides}\n")
        sys.exit()
    features = {}
    for sep in (",", ";", "\t"):
        names = set()
        try:
            with open(guides) as handle:
                for line in handle:
                    cols = line.rstrip().split(sep)
                    sequence = cols[1].upper().replace(" ", "")
                    name = cols[0]
                    if name in names:
                        colourful_errors("WARNING", f"The name {name} seems to appear at least twice. This MIGHT result in unexpected behaviour. Please have only unique name entries in your features.csv file.")
                    if sequence not in features:
                        features[sequence] = Features(name, 0)
                        names.add(name)
                    else:
                        colourful_errors("WARNING", f"{features[sequence].name} and {name} share the same sequence. Only {features[sequence].name} will be considered valid. {name} will be ignored.")
        except IndexError:
            pass
    if not features:
        colourful_errors("FATAL", "The given .csv file doesn't seem to be comma, semicolon, or tab separated. Please double check that the file's column separation\n")
        sys.exit()
    colourful_errors("INFO", f"{len(features)} different features were provided.")
    return features


def sample_barcodes_loader(path):
    """(names, barcodes) of a --sb file: rows `name,barcode`, read as features_loader reads --g -- ',' ';' tab tried in turn,
    the first two columns taken, barcodes upper-cased with blanks removed -- but stricter where --g is lenient: the first
    separator that splits EVERY non-blank line is the file's (features_loader keeps the rows before the first short line and
    adds up what the three separators give), blank lines are skipped, and nothing repeated is dropped: it is refused.
    A string that says what is wrong with the file otherwise."""
    if not os.path.isfile(path):
        return f"no .csv file found in the following path: {path}"
    rows = []
    for sep in (",", ";", "\t"):
        try:
            with open(path) as handle:
                rows = [(cols[0], cols[1].upper().replace(" ", "")) for cols in (line.rstrip().split(sep) for line in handle if line.strip())]
        except IndexError:
            rows = []
        if rows:
            break
    if not rows:
        return "the file doesn't seem to be comma, semicolon, or tab separated rows of name,barcode"
    names, barcodes = [r[0] for r in rows], [r[1] for r in rows]
    if len(rows) > 1024:
        return f"{len(rows)} barcodes: at most 1024 are taken"
    for name, barcode in rows:
        if name == "unassigned":
            return "the name unassigned is taken by the reads that carry no barcode"
        if names.count(name) > 1:
            return f"the name {name} appears at least twice"
        if not 1 <= len(barcode) <= 16:
            return f"the barcode of {name} ({barcode}) has {len(barcode)} bases: between 1 and 16 are taken"
        if set(barcode) - set("ACGT"):
            return f"the barcode of {name} ({barcode}) holds a symbol that is not A/C/G/T"
        if len(barcode) != len(barcodes[0]):
            return f"the barcode of {name} ({barcode}) has {len(barcode)} bases, that of {names[0]} has {len(barcodes[0])}: all barcodes have one length"
        if barcodes.count(barcode) > 1:
            return f"the barcode {barcode} appears at least twice ({', '.join(n for n, b in rows if b == barcode)})"
    return names, barcodes


def _counter_kwargs(param):
    """the keyword arguments of the run's context: the core ones, then what every option of the run adds"""
    kwargs = dict(mode=param['Running Mode'], miss=param['miss'], phred=param['phred'], length=param['length'],
                  start=param['start'], upstream=param['upstream'], downstream=param['downstream'],
                  miss_search_up=param['miss_search_up'], miss_search_down=param['miss_search_down'],
                  qual_up=param['qual_up'], qual_down=param['qual_down'],
                  device=int(param.get('device', os.environ.get("F2Q_DEVICE", os.environ.get("LOCAL_RANK", 0)))))
    for opt in _options_of(param):
        kwargs.update(opt.kwargs(param))
    return kwargs


def part_libraries(seqs):
    """(parts of position 1, parts of position 2) of a pair library, each in first-occurrence order over the features: the
    ids f2q_set_parts gives them (include/f2q.h)"""
    firsts, seconds = {}, {}
    for seq in seqs:
        a, _, b = seq.partition(":")
        firsts.setdefault(a, len(firsts))
        seconds.setdefault(b, len(seconds))
    return list(firsts), list(seconds)


def check_parts_library(features):
    """--parts: every feature is two non-empty parts joined by ':'; a sentence that names the first row that is not, else None"""
    for seq, feature in features.items():
        parts = seq.split(":")
        if len(parts) != 2 or not parts[0] or not parts[1]:
            return f"the feature {feature.name} ({seq}) is not two non-empty parts joined by ':'"
    return None


# ---- contexts are kept between samples ----------------------------------------------------------------------------
# A run counts many samples against ONE library with ONE set of parameters.  Creating a context per sample would build and
# upload the library index and allocate (and pin) the staging buffers every time -- 50 ms to several hundred per sample, as
# much as counting a small sample takes.  Each worker thread keeps its context; it is reset between samples
# (f2q_reset_counts: accumulators, Extract+Count tables, read numbering) and closed when the run ends.
_CTX_LOCK = threading.Lock()
_CTX_ALL = []
_CTX_TLS = threading.local()
_CTX_GEN = [0]


def _context_for(seqs, kwargs, assign=None):
    """assign: the library an Extract+Count context matches its keys against (--as), set once when the context is made"""
    key = (tuple(sorted((k, str(v)) for k, v in kwargs.items())), None if seqs is None else tuple(seqs))      # (compared by value: a few ms for 100 k features)
    if assign is not None:
        key = (key, tuple(assign))
    cur = getattr(_CTX_TLS, "entry", None)
    if os.environ.get("F2Q_NO_CTX_CACHE") == "1":              # A/B runs: a fresh context per sample
        key = (key, object())
    if cur is not None and cur[0] == _CTX_GEN[0] and cur[1] == key:
        cur[2].reset()
        return cur[2]
    if cur is not None and cur[0] == _CTX_GEN[0]:
        _drop_context(cur[2])
    ctx = binding.Counter(features=seqs, **kwargs)
    if assign is not None:
        ctx.set_assign_library(assign)
    _CTX_TLS.entry = (_CTX_GEN[0], key, ctx)
    with _CTX_LOCK:
        _CTX_ALL.append(ctx)
    return ctx


def _drop_context(ctx):
    with _CTX_LOCK:
        if ctx in _CTX_ALL:
            _CTX_ALL.remove(ctx)
    _CTX_TLS.entry = None
    ctx.close()


def close_contexts():
    """close every context kept by reads_counter (end of a run; also registered with atexit)"""
    with _CTX_LOCK:
        ctxs, _CTX_ALL[:] = list(_CTX_ALL), []
        _CTX_GEN[0] += 1
    for c in ctxs:
        c.close()


atexit.register(close_contexts)


_EXTENSIONS = re.compile(r"(\.(fastq|fq|gz|bgz))+$", re.IGNORECASE)


def mate_token(path):
    """(key, mate) of a paired-end file name: mate is 1 or 2, key the name with the mate token masked, equal for the two
    files of a sample; (None, 0) for a name that carries no token.  The token is the last _R1 / _R2 that is followed by
    '_', '.' or the end of the stem (Illumina: x_S1_L001_R1_001.fastq.gz), else _1 / _2 directly before the extension(s)."""
    name = os.path.basename(path)
    stem = _EXTENSIONS.sub("", name)
    found = list(re.finditer(r"_R([12])(?=_|\.|$)", stem))
    if found:
        m = found[-1]
        return name[:m.start(1)] + "*" + name[m.end(1):], int(m.group(1))
    m = re.search(r"_([12])$", stem)
    if m:
        return name[:m.start(1)] + "*" + name[m.end(1):], int(m.group(1))
    return None, 0


def pair_files(files):
    """[(R1 path, R2 path)] of a --pe run, in the order of the R1 files; ValueError names a file without its mate"""
    mates = {}
    for path in files:
        key, mate = mate_token(path)
        if not mate:
            raise ValueError(f"{path} carries no _R1/_R2 (or _1/_2) token: with --pe every file of --s needs its mate")
        if (os.path.dirname(path), key, mate) in mates:
            raise ValueError(f"{path} and {mates[(os.path.dirname(path), key, mate)]} claim the same mate of one sample")
        mates[(os.path.dirname(path), key, mate)] = path
    pairs = []
    for path in files:
        key, mate = mate_token(path)
        other = mates.get((os.path.dirname(path), key, 3 - mate))
        if other is None:
            raise ValueError(f"{path} has no mate file (--pe pairs _R1 with _R2, or _1 with _2)")
        if mate == 1:
            pairs.append((path, other))
    return pairs


def reads_counter(i, raw, features, param, reads_stats, preprocess=False):
    """Counts one FASTQ(.gz) file (:514-582).  Returns (features, reads_stats, local_read_stats) -- the reference's
    contract.  A paired-end run (param['paired']) counts `raw` together with its mate file param['mates'][raw].  A cut-off or damaged .gz gives the counts of every complete record before the damage plus the
    reference's warning (its parser keeps what it counted when readline raises, :405-407).  `features` is updated in
    place: Counter mode adds to Features.counts, Extract+Count mode adds the de-novo keys in first-occurrence order."""
    return _count_sample(i, raw, features, param, reads_stats, preprocess)[:3]


def _count_sample(i, raw, features, param, reads_stats, preprocess=False):
    """reads_counter, and next to its three values what every option of the run read from the context while it held the
    sample: {option name: Option.read()'s record}.  aligner() calls this one."""
    if (param['upstream'] is not None) and (param['downstream'] is not None):
        if len(str(param['upstream']).split(",")) != len(str(param['downstream']).split(",")):
            colourful_errors("FATAL", "Up and Downstream sequences must be submitted in concurrent pairs, separated by ,.")
            sys.exit()
    local_read_stats = dict.fromkeys(binding.STAT_NAMES, 0)
    if preprocess:                                  # memo warm-up (:1593-1617) has nothing to warm here
        return features, reads_stats, local_read_stats, {}
    options = _options_of(param)
    world = sharding.world()
    for opt in reversed(options):                   # (as file_sizer_split, for a caller that gets past it)
        if world.size > 1 and opt.one_rank(param):
            raise RuntimeError(opt.one_rank(param))
    counter_mode = param['Running Mode'] == 'C'
    seqs = list(features) if counter_mode else None
    kwargs = _counter_kwargs(param)
    assign = kwargs.pop('assign_library', None)     # (not an argument of the context: given to it once it is made)
    ctx = _context_for(seqs, kwargs, assign)
    try:
        if param.get('paired'):
            try:
                _, truncated = ctx.count_file_paired(raw, param['mates'][raw])
            except binding.F2QError as exc:
                if exc.code != binding.F2Q_EPAIRING:
                    raise
                truncated = False                   # the common pairs are counted
                colourful_errors("WARNING", f"{exc}. Only the pairs both files hold were counted.")
            counts, stats = ctx.read_counts()
            ec_rows = None if counter_mode else ctx.ec_results()
        elif world.size > 1:
            truncated = sharding.count_file_sharded(ctx, raw, world)
            counts, stats, ec_rows = sharding.reduce_results(ctx, world)
        else:
            _, truncated = ctx.count_file(raw)
            counts, stats = ctx.read_counts()
            ec_rows = None if counter_mode else ctx.ec_results()
        extras = {}
        for opt in options:
            record = opt.read(ctx, param)
            if record is not None:
                extras[opt.name] = record
                stats = record.get('stats', stats)  # (--as: the counters Counter mode gives for the same reads)
    except BaseException:
        _drop_context(ctx)                          # whatever state the failure left: the next sample starts afresh
        raise
    if truncated:
        colourful_errors("WARNING", f"{raw} is an incomplete or corrupted gzip file. Only partial processing might have occurred.")
    if counter_mode:
        for seq, n in zip(seqs, counts):
            features[seq].counts += int(n)
    else:
        for key, n, _first in ec_rows:
            if key in features:
                features[key].counts += n
            else:
                features[key] = Features(key, n)
    for k, v in zip(binding.STAT_NAMES, stats):
        local_read_stats[k] = int(v)
    return features, reads_stats, local_read_stats, extras


@dataclass
class SampleResult:
    """What one sample contributes to the run's tables: kept in memory from aligner() to compiling()
    (the reference round-trips this through <sample>_reads.csv and an English sentence, :785-799, :1316-1406)."""
    name: str            # file stem without .fastq / .gz (:779-783)
    time_value: str      # "0.52" / "1.03" ...
    time_unit: str       # seconds / minutes / hours
    rows: list           # [feature name, reads] in the sample's row order (numeric or alphabetical, :790-793)
    stats: dict          # the five counters of reads_counter (:310-316)
    extras: dict = field(default_factory=dict)   # what the run's options add: {option name: Option.sample()'s record}

    def sentence(self):
        """first line of <sample>_reads.csv, as upstream words it (:785)"""
        st = self.stats
        return (f'#script ran in {self.time_value} {self.time_unit} for file {self.name}. '
                f'{st["perfect_counter"] + st["imperfect_counter"]} reads out of {st["reads"]} were aligned. '
                f'{st["perfect_counter"]} were perfectly aligned. '
                f'{st["imperfect_counter"]} were aligned with mismatch. '
                f'{st["non_aligned_counter"]} passed quality filtering but were not aligned. '
                f'{st["quality_failed"]} did not pass quality filtering.')

    def reads_csv_rows(self):
        return [[self.sentence()], ["#Feature", "Reads"]] + [list(r) for r in self.rows]


def _sample_name(raw):
    name = Path(raw).stem
    return Path(name).stem if ".fastq" in name else name


def _elapsed_text(seconds):
    """(value, unit) of aligner's running time (:771-777)"""
    if seconds > 3600:
        return str(round(seconds / 3600, 2)), "hours"
    if seconds > 60:
        return str(round(seconds / 60, 2)), "minutes"
    return str(round(seconds, 2)), "seconds"


def aligner(i, raw, features, param, reads_stats):
    """One sample (:752-801): count it, order its rows, and keep the result for compiling() in param["samples"] -- what the
    run's options add to it travels in its extras.  <sample>_reads.csv is only written when the temporaries are kept
    (--k): nothing reads it back."""
    started = time.perf_counter()
    packed = _count_sample(i, raw, features, param, reads_stats)
    if packed is None:
        return reads_stats
    features, reads_stats, local, records = packed
    rows = _sample_rows([f.name, f.counts] for f in features.values())
    value, unit = _elapsed_text(time.perf_counter() - started)
    sample = SampleResult(_sample_name(raw), value, unit, rows, dict(local))
    sample.extras.update((opt.name, opt.sample(records[opt.name], sample, features, param)) for opt in OPTIONS if opt.name in records)
    if not param['Progress bar']:
        colourful_errors("INFO", f"Sample {sample.name} was processed in {value} {unit}")
    param.setdefault("samples", {})[sample.name] = sample     # a later file of the same name replaces the earlier one,
    if not param.get("delete", True) and sharding.world().rank == 0:   # as its _reads.csv would upstream
        csv_writer(os.path.join(param["directory"], sample.name + "_reads.csv"), sample.reads_csv_rows())
    return reads_stats


def _sample_file(param, sample, suffix, rows):
    """<sample><suffix> of one option, written by rank 0"""
    if sharding.world().rank == 0:
        os.makedirs(param["directory"], exist_ok=True)
        csv_writer(os.path.join(param["directory"], sample.name + suffix), rows)


def _column(sample, pairs, stats=None, tag=""):
    """a column of one of the options' tables: [name, number] pairs in the sample's row order, under the sample's name
    (+ tag) and running time, with the counters that go with them (the sample's own unless given)"""
    return SampleResult(sample.name + tag, sample.time_value, sample.time_unit, _sample_rows(pairs), dict(sample.stats if stats is None else stats))


def _sample_rows(pairs):
    """[name, reads] rows in a sample's order: numeric when every name is a number, else alphabetical (:790-793)"""
    rows = [[name, reads] for name, reads in pairs]
    try:
        rows.sort(key=lambda row: int(row[0]))       # all names numeric: numerical order
    except ValueError:
        rows.sort(key=lambda row: row[0])
    return rows


def csv_writer(path, outfile):
    """csv.writer rows (CRLF line ends, like the reference :803-809)"""
    with open(path, "w", newline='') as output:
        csv.writer(output).writerows(outfile)


def initializer(cmd):
    """banner-less counterpart of :1082-1169: coerces the Phred inputs, creates the output directory name"""
    param = cmd
    if param is None:
        colourful_errors("FATAL", "Only the command line mode (-c) is provided by this build; the tkinter dialog of the reference is not.")
        sys.exit(2)
    print(f"\n 2FAST2Q (MI355X counting path)  Version: {version}")
    if param["test_mode"]:
        colourful_errors("WARNING", "Running test mode!\n")
    param["version"] = version
    for key in ("phred", "qual_up", "qual_down"):
        if int(param[key]) <= 0:            # :1118-1125
            param[key] = 1
    current_time = datetime.datetime.now().strftime('%Y_%m_%d_%H_%M_%S')
    param["directory"] = os.path.join(param['out'], f"2FAST2Q_output_{current_time}")
    print("\n -- Parameters -- ")
    if param['Running Mode'] == 'C':
        print("\n Mode: Align and count")
        print(f" Allowed mismatches per alignement: {param['miss']}")
    else:
        print("\n Mode: Extract and count")
    print(f" Minimal Phred Score per bp >= {param['phred']}")
    if param['upstream'] is not None:
        print(f" Upstream search sequence: {param['upstream']}")
        print(f" Mismatches allowed in the upstream search sequence: {param['miss_search_up']}")
        print(f" Minimal Phred-score in the upstream search sequence: {param['qual_up']}")
    if param['downstream'] is not None:
        print(f" Downstream search sequence: {param['downstream']}")
        print(f" Mismatches allowed in the downstream search sequence: {param['miss_search_down']}")
        print(f" Minimal Phred-score in the downstream search sequence: {param['qual_down']}")
    if (param['upstream'] is None) or (param['downstream'] is None):
        print(f" Finding features with the folowing length: {param['length']}bp")
    if (param['upstream'] is None) and (param['downstream'] is None):
        print(f" Read alignment start position: {param['start']}")
    for opt in _options_of(param):
        for line in opt.banner(param):
            print(f" {line}")
    print(f" All data will be saved into {param['directory']}")
    print("\n ---- ")
    param["cpu"] = param["cpu"] if isinstance(param["cpu"], int) and param["cpu"] > 0 else (os.cpu_count() or 1)
    return param


def _package_data(name):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", name)


def ensure_example_fastq():
    """The upstream demo FASTQ is not redistributed (.MISSING_LARGE_BLOBS); test mode synthesises a
    stand-in of 20,000 reads from the packaged D39V library with the §8(d) generator."""
    import gzip
    path = _package_data("example.fastq.gz")
    if os.path.exists(path):
        return path
    feats = {}
    with open(_package_data("D39V_guides.csv")) as h:
        for line in h:
            cols = line.rstrip().split(",")
            feats.setdefault(cols[1].upper().replace(" ", ""), cols[0])
    with binding.Counter(features=list(feats), miss=1) as ctx:
        fq = bytes(ctx.synth_fastq(seed=0xD39, n_reads=20000, read_len=75))
    try:
        with gzip.open(path, "wb", compresslevel=6) as f:
            f.write(fq)
    except OSError:
        import tempfile
        path = os.path.join(tempfile.mkdtemp(prefix="f2q_demo_"), "example.fastq.gz")
        with gzip.open(path, "wb", compresslevel=6) as f:
            f.write(fq)
    return path


def umi_text(codes, length):
    """the bases of a UMI held as 2-bit codes, base j in bits 2j .. 2j+1 (f2q_umi_pairs)"""
    return "".join("ACGT"[(codes >> (2 * j)) & 3] for j in range(length))


def umi_length(param):
    """bases of the run's UMI (--umi, --umih, or --umi1 and --umi2 together), 0 without one"""
    if param.get('umi'):
        return param['umi'][1]
    if param.get('umi_header'):
        return param['umi_header'][1]
    return sum(part[1] for part in param.get('umi_paired') or () if part)


# the line each of these options adds to the parameter print-out and to the head of <name>_stats.csv
INDEL_HEADER, PARTS_HEADER = "#Indel reads reported: 1", "#Parts matched independently: 2"


def sample_barcodes_header(param):
    sb = param['sample_barcodes']
    return f"#Sample barcodes, start, length, mismatches: {sb['start']},{len(sb['barcodes'][0])},{sb['miss']}"


def stagger_header(param):
    return f"#Stagger: {param['stagger']}"


def strand_header(param):
    return f"#Strand: {param['strand']}"


def ec_collapse_header(param):
    return "#Extracted sequences collapsed, mismatches, ratio: %d,%d" % param['ec_collapse']


def parse_umih(text):
    """(separator, L) of a --umih value SEP,L, split at the last comma; a string that says what is wrong with it otherwise"""
    sep, comma, length = str(text).rpartition(",")
    if not comma or len(sep) != 1 or not re.fullmatch(r"\s*\d+\s*", length):
        return "expected SEP,L: one separator character, a comma, the number of bases"
    if not 33 <= ord(sep) <= 126 or sep.isalnum() or sep == "+":
        return f"the separator {sep!r} must be one printable ASCII character that is not a letter, a digit or '+'"
    if not 1 <= int(length) <= 16:
        return "the length L must be between 1 and 16"
    return sep, int(length)


def parse_umi(text):
    """(S, L) of a --umi value, None for a malformed or out-of-range one"""
    m = re.fullmatch(r"\s*(\d+)\s*,\s*(\d+)\s*", str(text))
    if not m or int(m.group(1)) > 0x3FFFFFFF or not 1 <= int(m.group(2)) <= 16:
        return None
    return int(m.group(1)), int(m.group(2))


# ---- the command-line options beyond the reference's ---------------------------------------------------------------------
@dataclass
class Option:
    """What one command-line option adds to a run: one row of OPTIONS.  input_parser, _counter_kwargs, file_sizer_split, main,
    _count_sample, aligner, initializer, run_headers, compiling and run_stats are loops over the rows around their option-free
    core; none of them names an option.  Every field but the first three has the default of an option that adds nothing
    there.  `found` is [(sample, the option's record of it)] over the samples that carry one, in <name>.csv's column order;
    tables and stats are asked only when there are any."""
    name: str                    # its key of param (set by parse; the option is on when it holds something) and of SampleResult.extras
    flags: tuple                 # (flag, add_argument's keywords) of each of its flags
    parse: callable              # (args, p), asked when the command line holds one of its flags: sets its keys of p; the sentence that refuses it, else None
    on: callable = None          # (param): where `name` alone does not tell
    library: callable = lambda features, param: None       # main(), once the library is read: checks it or loads beside it; a refusal, else None
    kwargs: callable = lambda param: {}                     # what it adds to the context's keyword arguments (and so to the key contexts are kept under)
    one_rank: callable = lambda param: None                 # what several ranks do not merge, as one sentence
    banner: callable = lambda param: []                     # its lines of the parameter print-out
    header: callable = lambda param: []                     # its '#key: value' lines at the head of <name>_stats.csv
    read: callable = lambda ctx, param: None                # what it fetches from the context that has counted a sample, as a dict
    sample: callable = None      # (got, sample, features, param): read()'s dict shaped for the tables, kept as sample.extras[name]; writes its per-sample files
    tables: callable = lambda param, found: []              # [(suffix, rows)]: every <name><suffix>.csv it adds
    stats: callable = lambda param, found: []               # the rows of its blocks of <name>_stats.csv

    def found(self, ordered):
        return [(s, s.extras[self.name]) for s in ordered if self.name in s.extras]


def _options_of(param):
    return [opt for opt in OPTIONS if (opt.on(param) if opt.on else param.get(opt.name))]


def _counter_mode_only(flag, p):
    """the refusal of an option that reads the library while it counts, in an Extract+Count run"""
    return None if p['Running Mode'] == "C" else f"{flag} only has a meaning in Counter mode: it cannot be combined with --mo EC."


def _cannot_combine(flag, args, p, others, why):
    """the refusal of `flag` next to any of `others`, named as the command line gives them.  --strand counts when it is a
    strand mode (fwd is a run without it), --stagger when its row took it (0 is a run without it)."""
    given = []
    for other in others:
        if other == "--strand":
            given += [f"--strand {args.strand}"] if args.strand in ("rev", "both") else []
        elif other == "--stagger":
            given += [f"--stagger {p['stagger']}"] if p.get('stagger') else []
        elif getattr(args, other.lstrip("-")) is not None:
            given.append(other)
    return f"{flag} cannot be combined with {' / '.join(given)}: {why}." if given else None


def _one_window_start(flag, p):
    if not re.fullmatch(r"[0-9]+", str(p['start']).strip()):
        return f"{flag} needs exactly one window start at or after the first base: --st {p['start']} does not name one."


def _not_merged(flag, what):
    return f"{flag}: {what} not merged across several ranks; run one process"


def _names(features):
    return [f.name for f in features.values()]


def _ints(numbers):
    return [int(n) for n in numbers]


def _table(suffix, columns):
    """(suffix, rows) of <name><suffix>.csv: <name>.csv's layout over these columns"""
    head, table = _table_of(columns)
    return suffix, [head] + [[feature] + counts for feature, counts in table.items()]


def _parse_paired(args, p):
    if args.pe is None:
        return f"{'--st2' if args.st2 is not None else '--rc2'} only has a meaning with --pe."
    if args.t is not None:
        return "--pe cannot be combined with -t: the test mode runs on one packaged single-end sample."
    if args.us is not None or args.ds is not None:
        return "--pe takes fixed positions only (--st / --st2): it cannot be combined with --us / --ds."
    if args.st2 is None:
        return "--pe needs --st2: the start position(s) of the feature part(s) within mate 2."
    p['paired'], p['start2'], p['rc2'] = True, args.st2, args.rc2 is not None


PAIRED = Option(
    'paired', parse=_parse_paired,
    flags=(("--pe", dict(nargs='?', const=True, help="Paired-end: the files of --s are paired by name (_R1/_R2, else _1/_2); --st names the feature parts in mate 1, --st2 those in mate 2")),
           ("--st2", dict(help="With --pe: the start position(s) of the feature part(s) within mate 2")),
           ("--rc2", dict(nargs='?', const=True, help="With --pe: mate 2 is reverse-complemented before its parts are taken"))),
    kwargs=lambda param: dict(start2=param['start2'], rc2=bool(param.get('rc2'))),      # the windows of mate 2 and its direction (f2q_set_mate2)
    one_rank=lambda param: "--pe: paired files are not shared out over several ranks; run one process",
    banner=lambda param: [f"Paired-end: mate 2 start position: {param['start2']}" + (" (mate 2 reverse-complemented)" if param['rc2'] else "")],
    header=lambda param: [f"#Paired-end, feature start position in mate 2: {param['start2']}", f"#Mate 2 reverse-complemented: {'yes' if param['rc2'] else 'no'}"])


# ---- --umi, --umi1 / --umi2 or --umih name the run's one source of UMIs (param['umi'], ['umi_paired'], ['umi_header']); --mu 1 and
# --mur directional add a kind of UMI_TABLES each.  A sample's record: {kind: its column of that kind}
def _parse_umi_family(args, p):
    if args.umi is not None:
        if _counter_mode_only("--umi", p):
            return _counter_mode_only("--umi", p)
        if args.pe is not None:
            return "--umi takes single reads: it cannot be combined with --pe. The UMI of a pair is named per mate with --umi1 S,L and / or --umi2 S,L."
        p['umi'] = parse_umi(args.umi)
        if p['umi'] is None:
            return f"--umi {args.umi}: expected S,L with a start S >= 0 and a length 1 <= L <= 16."
    if args.umi1 is not None or args.umi2 is not None:
        given = " / ".join(f for f, v in (("--umi1", args.umi1), ("--umi2", args.umi2)) if v is not None)
        if args.pe is None:
            return f"{given} only has a meaning with --pe: the UMI part of one mate of a pair (single reads: --umi)."
        if args.umi is not None:
            return f"{given} cannot be combined with --umi: --umi names the UMI of single reads."
        if _counter_mode_only(given, p):
            return _counter_mode_only(given, p)
        parts = []
        for flag, value in (("--umi1", args.umi1), ("--umi2", args.umi2)):
            parts.append(None if value is None else parse_umi(value))
            if value is not None and parts[-1] is None:
                return f"{flag} {value}: expected S,L with a start S >= 0 and a length 1 <= L <= 16."
        if sum(part[1] for part in parts if part) > 16:
            return f"--umi1 {args.umi1} --umi2 {args.umi2}: the two parts together hold 16 bases at most."
        p['umi_paired'] = tuple(parts)
    if args.umih is not None:
        refusal = _cannot_combine("--umih", args, p, UMI_FLAGS[:3], "a run has one source of UMIs, the read header or the read") or _counter_mode_only("--umih", p)
        if refusal:
            return refusal
        parsed = parse_umih(args.umih)
        if isinstance(parsed, str):
            return f"--umih {args.umih}: {parsed}."
        p['umi_header'] = parsed
    any_umi = any(getattr(args, flag.lstrip("-")) is not None for flag in UMI_FLAGS)
    if args.mu is not None:
        if not any_umi:
            return "--mu only has a meaning with --umi: the mismatches allowed between two UMIs of one feature."
        if args.mu not in ("0", "1"):
            return f"--mu {args.mu}: expected 0 or 1 (UMIs are collapsed at Hamming distance 1 at most)."
        if args.mu == "1":                                      # (0 is a run without the flag)
            p['umi_mismatch'] = 1
    if args.mur is not None:
        if args.mur not in ("cluster", "directional"):
            return f"--mur {args.mur}: expected cluster or directional."
        if not any_umi or args.mu != "1":
            return "--mur only has a meaning with --umi and --mu 1: the rule UMIs one base apart are collapsed by."
        if args.mur == "directional":
            p['umi_rule'] = 'directional'


def _umi_kwargs(param):
    # f2q_set_umi, f2q_set_umi_paired, f2q_set_umi_header (--mu: collapsing changes no context); --mur directional: it keeps the reads of every pair (f2q_set_umi_reads)
    kwargs = {key: tuple(param[key]) for key in ('umi', 'umi_paired', 'umi_header') if param.get(key)}
    return dict(kwargs, umi_reads=True) if param.get('umi_rule') == 'directional' else kwargs


def _umi_lines(param):
    """[(line of the parameter print-out, line at the head of <name>_stats.csv)]"""
    said, lines = "Distinct UMIs are counted per feature: UMI", []
    if param.get('umi'):
        lines.append((f"{said} start position in the read: {param['umi'][0]}, length: {param['umi'][1]}bp", f"#UMI start position in the read, length: {param['umi'][0]},{param['umi'][1]}"))
    lines += [(f"{said} part in mate {mate}, start position: {part[0]}, length: {part[1]}bp", f"#UMI in mate {mate}, start, length: {part[0]},{part[1]}")
              for mate, part in enumerate(param.get('umi_paired') or (), 1) if part]
    if param.get('umi_header'):
        lines.append((f"{said} in the read header, behind the last '{param['umi_header'][0]}' of the read id, length: {param['umi_header'][1]}bp",
                      f"#UMI in read header, separator, length: {param['umi_header'][0]},{param['umi_header'][1]}"))
    if param.get('umi_mismatch'):
        lines.append((f"UMIs of one feature that differ in one base are collapsed (--mu {param['umi_mismatch']})", f"#UMI mismatches collapsed: {param['umi_mismatch']}"))
    if param.get('umi_rule') == 'directional':
        lines.append(("Molecules are also counted by the directional rule: a UMI absorbs a neighbour with at most (its reads + 1) / 2 reads (--mur directional)",
                      "#UMI collapse rule: directional"))
    return lines


def _umi_read(ctx, param):
    """per kind of UMI_TABLES that was computed: (a number per feature, the sample-level counters); --mur directional with
    --k: the (feature, UMI, reads) table too"""
    umis, umi_reads, umi_failed = ctx.read_umis()           # distinct UMIs per feature and the two sample-level counters (f2q_read_umis)
    got = {"umis": (_ints(umis), dict(umi_reads=umi_reads, umi_failed=umi_failed))}
    if param.get('umi_mismatch'):                           # --mu 1: UMIs of a feature one base apart joined (f2q_umi_collapse)
        molecules, pairs, edges = ctx.collapse_umis(param['umi_mismatch'])
        got["molecules"] = (_ints(molecules), dict(umi_pairs=pairs, umi_edges=edges, umi_molecules=int(sum(molecules))))
    if param.get('umi_rule') == 'directional':              # --mur directional: the directional rule on the same set, and its pairs
        molecules, pairs, edges, dominated, reads = ctx.collapse_umis_directional()
        got["directional"] = (_ints(molecules), dict(umi_pairs=pairs, umi_edges=edges, umi_dominated=dominated, umi_molecules=int(sum(molecules)), umi_pair_reads=reads))
        got["pair_table"] = ctx.umi_pairs() if not param.get("delete", True) else None
    return got


def _umi_sample(got, sample, features, param):
    """the sample's rows once per kind, holding UMIs / molecules instead of reads"""
    got = dict(got)
    pair_table = got.pop("pair_table", None)
    if not param.get("delete", True):                       # the temporaries of --k
        kinds = [t for t in UMI_TABLES if t[0] in got]
        both = _sample_rows((f.name, (f.counts,) + tuple(ns)) for f, ns in zip(features.values(), zip(*(got[t[0]][0] for t in kinds))))  # (the order of sample.rows)
        _sample_file(param, sample, "_umi_reads.csv", [["#Feature", "Reads"] + [t[2] for t in kinds]] + [[name, *ns] for name, ns in both])
    if pair_table is not None:                              # every (feature, UMI) pair with its reads, in f2q_umi_pairs' order
        length = umi_length(param)                          # (--umi1 + --umi2: the concatenation as sequenced)
        _sample_file(param, sample, "_umi_pairs.csv", [["#Feature", "UMI", "Reads"]] + [[_names(features)[f], umi_text(int(c), length), int(n)] for f, c, n in zip(*pair_table)])
    return {kind: _column(sample, zip(_names(features), column), dict(sample.stats, **stats)) for kind, (column, stats) in got.items()}


def _umi_stats(param, found):
    """per kind: its head, then one line of counters per sample"""
    rows = []
    for kind, _, _, stats_head, counters in UMI_TABLES:
        lines = [[s.name] + [rec[kind].stats[c] for c in counters] for s, rec in found if kind in rec]
        rows += [stats_head] + lines if lines else []
    return rows


UMI = Option(
    'umi', parse=_parse_umi_family, on=lambda param: umi_length(param) > 0,
    flags=(("--umi", dict(help="S,L: every read carries a UMI of L bases (1-16) at position S; Counter mode also reports the distinct UMIs per feature (<name>_umi.csv)")),
           ("--umi1", dict(help="With --pe, S,L: the UMI (or its first part) is L bases at position S of mate 1")),
           ("--umi2", dict(help="With --pe, S,L: the UMI (or its second part) is L bases at position S of mate 2 as sequenced (whatever --rc2 says); --umi1 and --umi2 together hold 16 bases at most")),
           ("--umih", dict(help="SEP,L: the UMI of every read is in its header, the L bases (1-16) behind the last SEP of the read id, e.g. _,8 after umi_tools extract / fastp --umi, :,8 for an Illumina index-read UMI; with --pe: mate 1's header. Takes the place of --umi / --umi1 / --umi2")),
           ("--mu", dict(help="With --umi (or --umih, --umi1 / --umi2): mismatches in the UMI, 0 or 1 (default 0). 1: UMIs of one feature that differ in one base count as one molecule (<name>_umi_collapsed.csv)")),
           ("--mur", dict(help="With --umi and --mu 1: the rule UMIs are collapsed by, cluster (default) or directional. directional: a UMI absorbs a neighbouring UMI only when it has at least twice its reads minus one (<name>_umi_directional.csv)"))),
    kwargs=_umi_kwargs, read=_umi_read, sample=_umi_sample, stats=_umi_stats,
    one_rank=lambda param: _not_merged("--umi" if param.get('umi') else "--umih" if param.get('umi_header') else "--umi1 / --umi2", "the UMI sets are"),
    banner=lambda param: [said for said, _ in _umi_lines(param)],
    header=lambda param: [line for _, line in _umi_lines(param)],
    tables=lambda param, found: [_table(suffix, [rec[kind] for _, rec in found if kind in rec])             # <name>.csv's layout and row order per kind
                                 for kind, suffix, _, _, _ in UMI_TABLES if any(kind in rec for _, rec in found)])


# ---- --sb.  A sample's record: a column per barcode, then the unassigned reads; the five verdict counters
DemuxSample = namedtuple("DemuxSample", "columns verdicts")


def _parse_sample_barcodes(args, p):
    if args.sb is None:
        return f"{'--sbs' if args.sbs is not None else '--sbm'} only has a meaning with --sb: the .csv file with the sample barcodes."
    refusal = _counter_mode_only("--sb", p) or _cannot_combine("--sb", args, p, ("--pe",) + UMI_FLAGS, "sample barcodes are taken from single reads without UMIs")
    if refusal:
        return refusal
    if args.sbs is not None and not (args.sbs.isascii() and args.sbs.isdigit() and int(args.sbs) <= 0x3FFFFFFF):
        return f"--sbs {args.sbs}: expected the start position of the sample barcode within the read, a number >= 0."
    if args.sbm is not None and args.sbm not in ("0", "1"):
        return f"--sbm {args.sbm}: expected 0 or 1 (sample barcodes are matched at Hamming distance 1 at most)."
    loaded = sample_barcodes_loader(args.sb)
    if isinstance(loaded, str):
        return f"--sb {args.sb}: {loaded}."
    p['sample_barcodes'] = dict(path=args.sb, names=loaded[0], barcodes=loaded[1], start=int(args.sbs or 0), miss=int(args.sbm or 0))


def _demux_sample(got, sample, features, param):
    columns = [_column(sample, zip(_names(features), _ints(got["matrix"][b])), dict(zip(binding.STAT_NAMES, _ints(got["sample_stats"][b]))), f":{bname}")
               for b, bname in enumerate(param['sample_barcodes']['names'] + ["unassigned"])]
    return DemuxSample(columns, _ints(got["verdicts"]))


def _demux_stats(param, found):
    """the verdicts per file, then the counters per (file, barcode)"""
    return ([DEMUX_VERDICT_STATS_HEAD] + [[s.name] + rec.verdicts for s, rec in found] + [DEMUX_SAMPLE_STATS_HEAD] +
            [[c.name, c.stats["reads"], c.stats["perfect_counter"] + c.stats["imperfect_counter"], c.stats["perfect_counter"],
              c.stats["imperfect_counter"], c.stats["non_aligned_counter"], c.stats["quality_failed"]] for _, rec in found for c in rec.columns])


SAMPLE_BARCODES = Option(
    'sample_barcodes', parse=_parse_sample_barcodes, sample=_demux_sample, stats=_demux_stats,
    flags=(("--sb", dict(help="The full path to a .csv file with rows name,barcode: the reads of every file are demultiplexed by an inline sample barcode (1-16 bases, at most 1024 barcodes of one length) while they are counted (<name>_demux.csv). Counter mode, single reads, one process")),
           ("--sbs", dict(help="With --sb: the start position of the sample barcode within the read (default = 0)")),
           ("--sbm", dict(help="With --sb: mismatches allowed in the sample barcode, 0 or 1 (default = 0)"))),
    kwargs=lambda param: dict(sample_barcodes=(param['sample_barcodes']['start'], tuple(param['sample_barcodes']['barcodes'])),     # a demultiplexing context
                              barcode_mismatch=param['sample_barcodes']['miss']),                                                  # (f2q_set_sample_barcodes)
    one_rank=lambda param: _not_merged("--sb", "the demultiplexed counts are"),
    banner=lambda param: [f"Reads are demultiplexed by {len(param['sample_barcodes']['barcodes'])} inline sample barcodes of {param['sample_barcodes']['path']}",
                          sample_barcodes_header(param)[1:]],
    header=lambda param: [sample_barcodes_header(param)],
    read=lambda ctx, param: dict(zip(("matrix", "sample_stats", "verdicts"), ctx.read_demux())),     # the count matrix, the counters per barcode, the verdicts (f2q_read_demux)
    tables=lambda param, found: [_table("_demux", [column for _, rec in found for column in rec.columns])])


# ---- --strand rev / both.  A sample's record: its column split by the strand a read was counted on; the four strand counters
StrandSample = namedtuple("StrandSample", "columns counters")


def _parse_strand(args, p):
    if args.strand not in ("fwd", "rev", "both"):
        return f"--strand {args.strand}: expected fwd, rev or both."
    if args.strand != "fwd":                                     # (fwd is a run without the flag)
        flag = f"--strand {args.strand}"
        refusal = _counter_mode_only(flag, p) or _cannot_combine(flag, args, p, ("--pe",) + UMI_FLAGS + ("--sb",),
                                                                 "the reverse strand is read from single reads without UMIs or sample barcodes")
        if refusal:
            return refusal
        p['strand'] = args.strand


def _strand_sample(got, sample, features, param):
    split = [(f.name, int(f.counts) - int(n), int(n)) for f, n in zip(features.values(), got["rev_counts"])]
    return StrandSample([_column(sample, ((name, fwd) for name, fwd, _ in split), {}, ":fwd"), _column(sample, ((name, rev) for name, _, rev in split), {}, ":rev")],
                        _ints(got["counters"]))


STRAND = Option(
    'strand', parse=_parse_strand, sample=_strand_sample,
    flags=(("--strand", dict(help="fwd (default), rev or both: the orientation the reads are counted in. rev: every read is reverse-complemented first; both: a read that is assigned no feature as sequenced is tried reverse-complemented (<name>_strand.csv). Counter mode, single reads, one process")),),
    kwargs=lambda param: dict(strand=param['strand']),                                              # (f2q_set_strand)
    one_rank=lambda param: _not_merged("--strand", "the reverse-strand counts are"),
    banner=lambda param: [f"Reads are counted on {'the reverse strand' if param['strand'] == 'rev' else 'the forward strand, else on the reverse strand'}", strand_header(param)[1:]],
    header=lambda param: [strand_header(param)],
    read=lambda ctx, param: dict(zip(("rev_counts", "counters"), ctx.read_strands())),              # reads assigned on the reverse strand per feature, the strand counters (f2q_read_strands)
    tables=lambda param, found: [_table("_strand", [column for _, rec in found for column in rec.columns])],
    stats=lambda param, found: [STRAND_STATS_HEAD] + [[s.name] + rec.counters for s, rec in found])


# ---- --stagger N.  A sample's record: its reads assigned without / with mismatches at each offset
StaggerSample = namedtuple("StaggerSample", "perfect imperfect")


def _parse_stagger(args, p):
    if not re.fullmatch(r"[0-9]{1,3}", str(args.stagger)) or int(args.stagger) > 32:
        return f"--stagger {args.stagger}: expected a number of extra starts, 0 to 32."
    if int(args.stagger):                                        # (0 is a run without the flag)
        flag = f"--stagger {args.stagger}"
        refusal = (_counter_mode_only(flag, p) or
                   _cannot_combine(flag, args, p, ("--pe", "--us", "--ds") + UMI_FLAGS + ("--sb", "--parts", "--strand"),
                                   "one fixed window of single reads is tried at several starts, without anchors, UMIs, sample barcodes, a strand mode or parts") or
                   _one_window_start(flag, p))
        if refusal:
            return refusal
        p['stagger'] = int(args.stagger)


def _stagger_stats(param, found):
    """where the reads of each file were assigned"""
    rows = [STAGGER_STATS_HEAD]
    for s, rec in found:
        both = [a + b for a, b in zip(rec.perfect, rec.imperfect)]
        rows.append([s.name, both[0], sum(both[1:]), both.index(max(both))])
    return rows


STAGGER = Option(
    'stagger', parse=_parse_stagger, stats=_stagger_stats,
    flags=(("--stagger", dict(help="N (0-32): the one fixed window (--st s --l L) is tried at the starts s .. s+N; a read counts at the earliest start that reads a feature exactly, else at the earliest one within --m (<name>_stagger.csv). 0 (default): off. Counter mode, single reads, one --st value, one process")),),
    kwargs=lambda param: dict(stagger=param['stagger']),                                            # the window tried at N + 1 starts (f2q_set_stagger)
    one_rank=lambda param: _not_merged("--stagger", "the offset histograms are"),
    banner=lambda param: [f"The feature window is tried at the starts {param['start']} .. {int(param['start']) + param['stagger']}: the earliest exact one counts, else the earliest within --m",
                          stagger_header(param)[1:]],
    header=lambda param: [stagger_header(param)],
    read=lambda ctx, param: dict(zip(("perfect", "imperfect"), ctx.read_stagger())),                # (f2q_read_stagger)
    sample=lambda got, sample, features, param: StaggerSample(_ints(got["perfect"]), _ints(got["imperfect"])),
    tables=lambda param, found: [("_stagger", [["#Offset", "Start"] + [f"{s.name}:{kind}" for s, _ in found for kind in ("perfect", "imperfect")]] +     # a row per offset
                                  [[d, int(param['start']) + d] + [n for _, rec in found for n in (rec.perfect[d], rec.imperfect[d])] for d in range(param['stagger'] + 1)])])


# ---- --indel.  A sample's record: its deletion and its insertion column, the reads of either per position, the four totals
IndelSample = namedtuple("IndelSample", "columns del_pos ins_pos totals")


def _parse_indel(args, p):
    if args.indel is not True:
        return f"--indel takes no value: --indel {args.indel} is not understood."
    refusal = (_counter_mode_only("--indel", p) or
               _cannot_combine("--indel", args, p, ("--pe", "--us", "--ds") + UMI_FLAGS + ("--sb", "--parts", "--strand", "--stagger"),
                               "the unassigned reads of one fixed window of single reads are examined, without anchors, UMIs, sample barcodes, a strand mode, parts or a stagger") or
               _one_window_start("--indel", p))
    if refusal:
        return refusal
    if not 2 <= p['length'] <= 31:
        return f"--indel needs a window of 2 to 31 bases: --l {p['length']} is outside that range."
    p['indel'] = True


INDEL = Option(
    'indel', parse=_parse_indel,
    flags=(("--indel", dict(nargs='?', const=True, help="Reads that the one fixed window (--st s --l L, L 2-31) assigns to no feature are tried as a one-base deletion and as a one-base insertion of every feature of L bases; they are reported per feature and per position (<name>_indel.csv, <name>_indel_positions.csv) and change no count. Counter mode, single reads, one --st value, one process")),),
    kwargs=lambda param: dict(indel=True),                                                          # one-base insertions and deletions reported (f2q_set_indel)
    one_rank=lambda param: _not_merged("--indel", "the indel counts are"),
    banner=lambda param: ["Reads that are assigned no feature are tried as one-base deletions and insertions of every feature; they are reported, not counted", INDEL_HEADER[1:]],
    header=lambda param: [INDEL_HEADER],
    read=lambda ctx, param: dict(zip(("dels", "inss", "del_pos", "ins_pos", "totals"), ctx.read_indels())),     # per feature and per position, the four totals (f2q_read_indels)
    sample=lambda got, sample, features, param: IndelSample([_column(sample, zip(_names(features), _ints(got["dels"])), {}, ":del"),
                                                             _column(sample, zip(_names(features), _ints(got["inss"])), {}, ":ins")],
                                                            _ints(got["del_pos"]), _ints(got["ins_pos"]), _ints(got["totals"])),
    tables=lambda param, found: [_table("_indel", [column for _, rec in found for column in rec.columns]),
                                 ("_indel_positions", [["#Position"] + [f"{s.name}:{kind}" for s, _ in found for kind in ("del", "ins")]] +              # a row per position
                                  [[at] + [n for _, rec in found for n in (rec.del_pos[at], rec.ins_pos[at])] for at in range(param['length'])])],
    stats=lambda param, found: [INDEL_STATS_HEAD] + [[s.name] + rec.totals for s, rec in found])


# ---- --parts.  A sample's record: its rows by the part rule, {(part 1, part 2): reads} of its recombinant pairs, its six read classes by name
PartsSample = namedtuple("PartsSample", "table recombinants classes")


def _parse_parts(args, p):
    refusal = _counter_mode_only("--parts", p) or _cannot_combine("--parts", args, p, ("--us", "--ds") + UMI_FLAGS + ("--sb", "--strand"),
                                                                  "the parts are matched at fixed positions, without UMIs, sample barcodes or a strand mode")
    if refusal:
        return refusal
    windows = [len(str(p['start']).split(","))] + ([len(str(args.st2).split(","))] if args.pe is not None else [])
    if windows not in ([2], [1, 1]):
        return (f"--parts needs exactly two windows: --st a,b for single reads, or one window per mate with --pe (--st a --st2 b); "
                f"--st {p['start']}" + (f" --st2 {args.st2}" if args.pe is not None else "") + f" names {' + '.join(str(n) for n in windows)}.")
    p['parts'] = True


def _parts_library(features, param):
    wrong = check_parts_library(features)
    return f"--parts takes a library of pairs, --g {param['feature']}: {wrong}." if wrong else None


def _parts_sample(got, sample, features, param):
    firsts, seconds = part_libraries(list(features))
    if not param.get("delete", True):
        _sample_file(param, sample, "_parts_marginals.csv", [["#position", "part", "reads"]] + [[1, part, int(n)] for part, n in zip(firsts, got["part1"])] +
                     [[2, part, int(n)] for part, n in zip(seconds, got["part2"])])
    return PartsSample(_column(sample, zip(_names(features), _ints(got["parts_counts"]))), {(firsts[a], seconds[b]): int(n) for a, b, n in zip(*got["recombinants"])},
                       dict(zip(binding.PARTS_CLASSES, _ints(got["classes"]))))


def _parts_tables(param, found):
    """<name>.csv's layout and row order holding parts_counts; the recombinant pairs of any sample, those with the most reads first"""
    columns = [rec.recombinants for _, rec in found]
    pairs = sorted({pair for column in columns for pair in column}, key=lambda pair: (-sum(column.get(pair, 0) for column in columns), pair))
    return [_table("_parts", [rec.table for _, rec in found]),
            ("_recombinants", [["#Part1", "Part2"] + [s.name for s, _ in found]] + [[a, b] + [column.get((a, b), 0) for column in columns] for a, b in pairs])]


PARTS = Option(
    'parts', parse=_parse_parts, library=_parts_library, sample=_parts_sample, tables=_parts_tables,
    flags=(("--parts", dict(nargs='?', const=True, help="Pair libraries (features A:B over exactly two windows: --st a,b, or --pe --st a --st2 b): each part is also matched on its own with --m mismatches per part; reads whose two parts the library does not pair are counted as recombinants (<name>_parts.csv, <name>_recombinants.csv). Counter mode, one process")),),
    kwargs=lambda param: dict(parts=True),                                                          # each part of a pair library matched alone (f2q_set_parts)
    one_rank=lambda param: _not_merged("--parts", "the part tables and recombinant sets are"),
    banner=lambda param: ["Each of the two feature parts is also matched on its own; recombinant reads are counted per pair of parts", PARTS_HEADER[1:]],
    header=lambda param: [PARTS_HEADER],
    read=lambda ctx, param: dict(zip(("parts_counts", "part1", "part2", "classes"), ctx.read_parts()), recombinants=ctx.parts_recombinants()),      # (f2q_read_parts, f2q_parts_recombinants)
    stats=lambda param, found: [PARTS_STATS_HEAD] + [                                               # the six read classes per file, the distinct recombinant pairs next to their reads
        [s.name, c["pair_perfect"], c["pair_imperfect"], c["recombinant"], len(rec.recombinants), c["part1_only"], c["part2_only"], c["neither"]] for s, rec in found for c in [rec.classes]])


# ---- --as.  A sample's record: the column Counter mode would have given for it
def _parse_assign(args, p):
    if args.g is None or args.t is not None:
        return "--as needs --g: the .csv file with the features the extracted sequences are assigned to."
    if p['Running Mode'] != "EC":
        return "--as only has a meaning with --mo EC: Counter mode assigns every read already."
    p['assign'] = True


def _assign_read(ctx, param):
    """one match per distinct key on the device: the Counter-mode count vector and counters of the same reads (they take the
    place of the sample's own), and every key's feature (f2q_ec_assign)"""
    counts, stats = ctx.ec_assign()
    return dict(counts=_ints(counts), stats=stats, rows=ctx.ec_assigned())


def _assign_sample(got, sample, features, param):
    names = _names(param['assign_features'])
    _sample_file(param, sample, "_assigned.csv", [["#key", "reads", "feature_name", "mismatches"]] + [[key, n, names[f] if f >= 0 else "", d] for key, n, _first, f, d in got["rows"]])
    return _column(sample, zip(names, got["counts"]))


ASSIGN = Option(
    'assign', parse=_parse_assign, read=_assign_read, sample=_assign_sample,
    flags=(("--as", dict(dest="assign", nargs='?', const=True, help="With --mo EC and --g: every extracted sequence is also assigned to its feature (--m mismatches), giving the Counter mode table of the same run")),),
    library=lambda features, param: param.update(assign_features=features_loader(param["feature"])),
    kwargs=lambda param: dict(assign_library=list(param['assign_features'])),                       # the library the context matches its keys against, given to it once it is made
    one_rank=lambda param: _not_merged("--as", "assignments are"),
    banner=lambda param: [f"Extracted sequences are assigned to the features of {param['feature']} ({param['miss']} mismatches allowed)"],
    tables=lambda param, found: [_table("_features", [rec for _, rec in found])])                   # the table Counter mode would have written for the same samples


# ---- --ecm 1 / --ecr.  A sample's record: its centroids with their cluster reads, the six numbers of EC_COLLAPSE_STATS_HEAD
CollapseSample = namedtuple("CollapseSample", "table counters")


def _parse_ec_collapse(args, p):
    ecm = None if args.ecm is None else args.ecm.strip()
    if ecm == "0" and args.ecr is None:
        args.ecm = None                                         # --ecm 0 is a run without the flag: the recorded command line leaves it out
        return None
    if ecm not in (None, "0", "1"):
        return f"--ecm takes 0 or 1 (mismatches among the extracted sequences): --ecm {args.ecm} is not understood."
    if ecm != "1":
        return f"--ecr {args.ecr} only has a meaning with --ecm 1: without it the extracted sequences are not collapsed."
    if args.ecr is not None and not (re.fullmatch(r"[0-9]{1,4}", args.ecr.strip()) and 2 <= int(args.ecr) <= 255):
        return f"--ecr takes a whole number from 2 to 255: --ecr {args.ecr} is not one."
    if p['Running Mode'] != "EC":
        return "--ecm 1 only has a meaning with --mo EC: Counter mode extracts no sequences to collapse."
    if args.pe is not None:
        return "--ecm 1 cannot be combined with --pe: the joined keys of a pair are not collapsed."
    anchored = args.us is not None or args.ds is not None
    if anchored and max(len(str(x).split(",")) for x in (args.us, args.ds) if x is not None) > 1:
        return "--ecm 1 needs one --us/--ds pair: with several pairs every extracted sequence is a ':'-joined key and none could be collapsed."
    if not anchored and len(str(p['start']).split(",")) > 1:
        return f"--ecm 1 needs one window: with --st {p['start']} every extracted sequence is a ':'-joined key and none could be collapsed."
    if not (args.us is not None and args.ds is not None) and p['length'] > 29:
        return f"--ecm 1 collapses sequences of at most 29 bases: with --l {p['length']} none could be collapsed."
    p['ec_collapse'] = (1, int(args.ecr) if args.ecr is not None else 5)


def _collapse_sample(got, sample, features, param):
    counters, rows = got["counters"], got["rows"]
    _sample_file(param, sample, "_clusters.csv", [["#key", "reads", "centroid", "cluster_reads"]] + [[key, n, cent, cluster] for key, n, _first, cent, cluster in rows])
    centroids = [(key, cluster) for key, _n, _first, cent, cluster in rows if cent == key]
    return CollapseSample(_column(sample, centroids), [len(rows), counters["eligible_keys"], counters["absorbed_keys"], len(centroids), counters["absorbed_reads"], counters["longest_chain"]])


EC_COLLAPSE = Option(
    'ec_collapse', parse=_parse_ec_collapse, sample=_collapse_sample,
    flags=(("--ecm", dict(help="With --mo EC: mismatches among the extracted sequences, 0 (default) or 1. 1: per sample, every plain sequence of at most 29 bases is folded into the sequence one substitution away with the most reads, when that one has at least --ecr times its reads (<sample>_clusters.csv, <name>_collapsed.csv). One fixed window of at most 29 bases or one --us/--ds pair, single reads, one process")),
           ("--ecr", dict(help="With --ecm 1: the reads a sequence needs, as a multiple of another's, to absorb it: 2-255 (default = 5)"))),
    one_rank=lambda param: "--ecm 1: the merged tables of several ranks live on the host and are not collapsed; run one process",
    banner=lambda param: ["Extracted sequences of one sample that differ in one base are collapsed into the one with the most reads", ec_collapse_header(param)[1:]],
    header=lambda param: [ec_collapse_header(param)],
    read=lambda ctx, param: dict(counters=ctx.ec_collapse(*param['ec_collapse']), rows=ctx.ec_collapsed()),    # the sample's plain keys one base apart folded on the device (f2q_ec_collapse)
    tables=lambda param, found: [_table("_collapsed", [rec.table for _, rec in found])],            # <name>.csv's layout over the samples' centroids and their cluster reads
    stats=lambda param, found: [EC_COLLAPSE_STATS_HEAD] + [[s.name] + rec.counters for s, rec in found])


UMI_FLAGS = ("--umi", "--umi1", "--umi2", "--umih")
# in the order of the '#key: value' lines and of the blocks of <name>_stats.csv
OPTIONS = (PAIRED, UMI, SAMPLE_BARCODES, STRAND, STAGGER, INDEL, PARTS, ASSIGN, EC_COLLAPSE)
# the order the command line is examined in, which decides what a command line that is wrong twice is told: the order the
# options came to the program in (--parts before --stagger and --indel)
PARSE_ORDER = (PAIRED, UMI, SAMPLE_BARCODES, STRAND, PARTS, STAGGER, INDEL, ASSIGN, EC_COLLAPSE)


def input_parser(argv=None):
    """the reference's flag set (:1193-1216) and defaults (:1246-1309), plus --gpu (device ordinal)"""
    ap = argparse.ArgumentParser(prog="2fast2q")
    ap.add_argument("-c", nargs='?', const=True, help="cmd line mode.")
    ap.add_argument("-t", nargs='?', const=True, help="Runs 2FAST2Q in test mode with example data.")
    ap.add_argument("-v", nargs='?', const=True, help="Prints the current version.")
    ap.add_argument("--s", help="The full path to the directory with the sequencing files OR file.")
    ap.add_argument("--g", help="The full path to the .csv file with the sgRNAs.")
    ap.add_argument("--o", help="The full path to the output directory")
    ap.add_argument("--fn", nargs='?', const="compiled", help="Specify an output compiled file name (default is called compiled)")
    ap.add_argument("--pb", nargs='?', const=False, help="Adds progress bars (default is enabled)")
    ap.add_argument("--m", help="The number of allowed mismatches per feature (default = 1). Ignored in extract + Count mode.")
    ap.add_argument("--ph", help="Minimal Phred-score (default=30).")
    ap.add_argument("--st", help="The start position of the feature within the read (default = 0).")
    ap.add_argument("--l", help="The length of the feature in bp (default = 20).")
    ap.add_argument("--us", help="Upstream search sequence.")
    ap.add_argument("--ds", help="Downstream search sequence.")
    ap.add_argument("--msu", help="Upstream search sequence mismatches (default is 0).")
    ap.add_argument("--msd", help="Downstream search sequence mismatches (default is 0).")
    ap.add_argument("--qsu", help="Minimal Phred-score (default=30) in the upstream search sequence")
    ap.add_argument("--qsd", help="Minimal Phred-score (default=30) in the downstream search sequence")
    ap.add_argument("--mo", help="Running Mode (default=C) [Counter (C) / Extractor + Counter (EC)].")
    ap.add_argument("--cp", help="Number of cpus (accepted for compatibility; the counting runs on the GPU)")
    ap.add_argument("--fs", nargs='?', const=False, help="File Split mode (accepted for compatibility; ignored)")
    ap.add_argument("--k", nargs='?', const=False, help="If enabled, keeps all temporary files (default is disabled)")
    ap.add_argument("--gpu", help="HIP device ordinal (default: LOCAL_RANK or 0)")
    for opt in OPTIONS:
        for flag, keywords in opt.flags:
            ap.add_argument(flag, **keywords)
    args = ap.parse_args(argv)
    if args.v is not None:
        print(f"\nVersion: {version}\n")
        sys.exit()
    if args.c is None:
        return None
    p = {"cmd": True, "big_file_split": args.fs is not None}
    p['Running Mode'] = "EC" if (args.mo is not None and "EC" in args.mo.upper()) else "C"
    p['out_file_name'] = args.fn if args.fn is not None else "compiled"
    p['length'] = int(args.l) if args.l is not None else 20
    p['Progress bar'] = args.pb is None
    p['start'] = args.st if args.st is not None else "0"
    p['phred'] = int(args.ph) if args.ph is not None else 30
    p['miss'] = int(args.m) if args.m is not None else 1
    p['upstream'], p['downstream'] = args.us, args.ds
    p['miss_search_up'] = int(args.msu) if args.msu is not None else 0
    p['miss_search_down'] = int(args.msd) if args.msd is not None else 0
    p['qual_up'] = int(args.qsu) if args.qsu is not None else 30
    p['qual_down'] = int(args.qsd) if args.qsd is not None else 30
    p['delete'] = args.k is None
    p['cpu'] = int(args.cp) if args.cp is not None else False
    if args.gpu is not None:
        p['device'] = int(args.gpu)
    for opt in PARSE_ORDER:                                    # before any output directory exists
        given = any(getattr(args, keywords.get("dest", flag.lstrip("-"))) is not None for flag, keywords in opt.flags)
        refusal = opt.parse(args, p) if given else None
        if refusal:
            colourful_errors("FATAL", refusal)
            sys.exit(2)
    p['used_cmd'] = " ".join(f"--{k}" if isinstance(v, bool) and v else f"--{k} {v}"
                             for k, v in ((("as" if k == "assign" else k), v) for k, v in vars(args).items()) if v is not None)
    p["test_mode"] = args.t is not None
    if args.t is None:
        paths = [[args.s, 'seq_files'], [args.g, 'feature'], [args.o, 'out']]
    else:                                                       # (after the refusals: the packaged sample is made on the GPU)
        paths = [[ensure_example_fastq(), 'seq_files'], [_package_data('D39V_guides.csv'), 'feature'], [os.getcwd(), 'out']]
    for value, key in paths:                                   # :1178-1191
        if value is None:
            p[key] = os.getcwd()
            if key == 'feature':
                found = path_finder(os.getcwd(), ["*.csv"])
                if p['Running Mode'] != "EC":
                    if len(found) > 1:
                        colourful_errors("FATAL", "There is more than one .csv in the current directory. If not directly indicating a path for the features .csv, please have only 1 .csv file in the directory.\n")
                        sys.exit()
                    if len(found) == 1:
                        p[key] = found[0][0]
        else:
            p[key] = value
    return p


def file_sizer_split(param):
    """sample discovery (:1657-1689): *.gz and *.fastq of the --s directory, smallest first"""
    if param["test_mode"]:
        param["sequencing_files"] = {"len_files": 1, "preprocess_files": [param["seq_files"]], "files": [param["seq_files"]]}
        return param
    files = [p[0] for p in path_parser(param["seq_files"], ["*.gz", "*.fastq"])]
    for opt in reversed(_options_of(param)):                     # (the last row that refuses speaks: --umih or --parts, not the --pe it came with)
        if sharding.world().size > 1 and opt.one_rank(param):
            colourful_errors("FATAL", opt.one_rank(param) + ".")
            sys.exit(2)
    if param.get('paired'):                                      # one sample per pair, named after its R1 file
        try:
            pairs = pair_files(files)
        except ValueError as exc:
            colourful_errors("FATAL", str(exc))
            sys.exit(2)
        param['mates'] = dict(pairs)
        files = [r1 for r1, _ in pairs]
    param["sequencing_files"] = {"len_files": len(files), "preprocess_files": files[:1], "files": files}
    return param


def aligner_mp_dispenser(features, param, start=0):
    """every sample through aligner() (:1619-1655); samples are independent, one GPU pass each"""
    if sharding.world().rank == 0:
        os.makedirs(param["directory"], exist_ok=True)
    sharding.barrier()
    reads_stats = {"failed_reads": set(), "passed_reads": {}}
    colourful_errors("INFO", f"Processing {param['sequencing_files']['len_files']} files. Please hold.")

    def one(i, raw):
        # Counter mode: each sample starts from zeroed counts, as the per-process `features` copy does upstream
        per_sample = {k: Features(v.name, 0) for k, v in features.items()} if param['Running Mode'] == 'C' else {}
        aligner(i, raw, per_sample, param, reads_stats)

    files = list(enumerate(param['sequencing_files']['files']))
    # samples in flight: two.  The GPU counts a sample faster than the host reads it, the file reader brings its own
    # worker pool (parallel pread / BGZF / gzip chunks), and every worker thread owns a context with pinned staging
    # buffers: more threads only add allocations and contention (16 samples of 1 M reads, --cp 1 / 2 / 4 / 16: 1.7 / 1.7 /
    # 2.1 / 2.4 s whole run; .gz: 2.4 / 2.0 / 2.4 / 3.1 s -- scripts/samples_threads.py).  F2Q_SAMPLES_IN_FLIGHT overrides.
    cap = int(os.environ.get("F2Q_SAMPLES_IN_FLIGHT", "2") or 2)
    workers = max(1, min(int(param.get("cpu") or 1), len(files), cap, 16))
    try:
        _dispense(files, workers, one)
    finally:
        close_contexts()                            # (the worker threads' contexts outlive the threads otherwise)


def _dispense(files, workers, one):
    if workers > 1 and sharding.world().size == 1:
        # --cp samples in flight, as upstream (:1646-1655) -- threads, not processes: the per-read work is in the
        # library (ctypes drops the GIL), each sample has its own context and HIP stream, and for .gz input the
        # single-threaded inflate of one file overlaps with the inflate and the GPU work of the others
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=workers) as pool:
            for fut in [pool.submit(one, i, raw) for i, raw in files]:
                fut.result()
    else:
        for i, raw in files:
            one(i, raw)


def _samples_from_directory(directory):
    """SampleResults of the <sample>_reads.csv files of a directory (a run whose temporaries were kept, or made by the
    reference itself): the file layout of aligner() read back, for callers that have no in-memory results."""
    found = {}
    for path in path_parser(directory, ['*reads.csv']):
        name = Path(path).stem[:-len("_reads")]
        with open(path, newline='') as handle:
            table = list(csv.reader(handle))
        words = table[0][0].split()
        numbers = [w for w in words if w.isdigit()]        # aligned, reads, perfect, imperfect, non aligned, failed
        stats = dict(zip(("reads", "perfect_counter", "imperfect_counter", "non_aligned_counter", "quality_failed"),
                         (int(numbers[-5]), int(numbers[-4]), int(numbers[-3]), int(numbers[-2]), int(numbers[-1]))))
        found[name] = SampleResult(name, words[3], words[4], [[r[0], int(r[1])] for r in table[2:]], stats)
    return found


def run_headers(param):
    """the '#key: value' lines that open <name>_stats.csv (:1323-1337)"""
    lines = [f"#2FAST2Q version: {param['version']}"]
    if "used_cmd" in param:
        lines.append(f"#cmd used: {param['used_cmd']}")
    lines += [f"#Mismatch: {param['miss']}",
              f"#Phred Score: {param['phred']}",
              f"#Feature Length: {param['length']}",
              f"#Feature start position in the read: {param['start']}",
              f"#Running mode: {param['Running Mode']}",
              f"#Upstream search sequence: {param['upstream']}",
              f"#Downstream search sequence: {param['downstream']}",
              f"#Mismatches in the upstream search sequence: {param['miss_search_up']}",
              f"#Mismatches in the downstream search sequence: {param['miss_search_down']}",
              f"#Minimal Phred-score in the upstream search sequence: {param['qual_up']}",
              f"#Minimal Phred-score in the downstream search sequence: {param['qual_down']}"]
    for opt in _options_of(param):
        lines += opt.header(param)
    return lines


def compile_table(samples):
    """(head, {feature: [reads per sample]}) of the run (:1341-1364).  Samples in the order upstream meets their
    <sample>_reads.csv files (sorted by that file name); features in first-met order, a feature a sample lacks counts 0
    there (Extract+Count samples have different key sets).  A feature name holding '#' is left out of the table, as
    upstream's line filter does (:1350)."""
    ordered = sorted(samples.values(), key=lambda s: s.name + "_reads.csv")
    return (ordered,) + _table_of(ordered)


def _table_of(ordered):
    """compile_table's head and rows for columns that are in their order already"""
    table = {}
    for column, sample in enumerate(ordered):
        for name, reads in sample.rows:
            name = str(name)
            if "#" in name:
                continue
            table.setdefault(name, [0] * column).append(int(reads))
        for counts in table.values():
            counts.extend([0] * (column + 1 - len(counts)))
    return ["#Feature"] + [s.name for s in ordered], table


def compiling(param):
    """<name>.csv and <name>_stats.csv (+ plots) from the samples aligner() collected (:1316-1384); without in-memory
    results the <sample>_reads.csv files of the output directory are read instead."""
    samples = param.get("samples") or _samples_from_directory(param["directory"])
    ordered, head, table = compile_table(samples)
    run_stats(run_headers(param), param, table, head, ordered)
    tables = [_table("", ordered)] + [t for opt in OPTIONS if opt.found(ordered) for t in opt.tables(param, opt.found(ordered))]
    for suffix, rows in tables:                      # <name>.csv, then <name><suffix>.csv of every option that has numbers of these samples
        csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}{suffix}.csv"), rows)
    if param["delete"]:
        for path in path_finder(param["directory"], ['*reads.csv']):
            os.remove(path[0])
    colourful_errors("INFO", "Analysis successfully completed")
    print("\n If you find 2FAST2Q useful, please consider citing:\n Bravo AM, Typas A, Veening J. 2022. \n 2FAST2Q: a general-purpose sequence search and counting program for FASTQ files. PeerJ 10:e14041\n DOI: 10.7717/peerj.14041\n")
    if param["test_mode"]:
        colourful_errors("WARNING", "Test successful. 2FAST2Q is working as intended!\n")


STATS_HEAD = ["#Sample name", "Running Time", "Running Time unit", "Total number of reads in sample",
              "Total number of reads that were aligned", "Number of reads that were aligned without mismatches",
              "Number of reads that were aligned with mismatches",
              "Number of reads that passed quality filtering but were not aligned",
              'Number of reads that did not pass quality filtering.']


# the heads of the options' blocks of <name>_stats.csv
UMI_STATS_HEAD = ["#Sample name (UMI)", "Number of aligned reads with a valid UMI", "Number of aligned reads with an invalid UMI"]
UMI_COLLAPSE_STATS_HEAD = ["#Sample name (UMI collapsed)", "Number of distinct (feature, UMI) pairs", "Number of pairs of them that differ in one base", "Number of molecules"]
UMI_DIRECTIONAL_STATS_HEAD = ["#Sample name (UMI directional)", "Number of distinct (feature, UMI) pairs", "Number of pairs of them that differ in one base", "Number of pairs a neighbour absorbs directly", "Number of molecules", "Number of reads of all pairs"]
# what a UMI run reports, one column per sample (sample.extras['umi'][kind], a SampleResult): kind, suffix of the run's
# table, column of <sample>_umi_reads.csv, head and counters of its block of <name>_stats.csv.  --umi gives the first,
# --mu 1 the second, --mur directional the third
UMI_TABLES = (("umis", "_umi", "UMIs", UMI_STATS_HEAD, ("umi_reads", "umi_failed")),
              ("molecules", "_umi_collapsed", "Molecules", UMI_COLLAPSE_STATS_HEAD, ("umi_pairs", "umi_edges", "umi_molecules")),
              ("directional", "_umi_directional", "Directional", UMI_DIRECTIONAL_STATS_HEAD,
               ("umi_pairs", "umi_edges", "umi_dominated", "umi_molecules", "umi_pair_reads")))
DEMUX_VERDICT_STATS_HEAD = ["#Sample name (sample barcodes)", "Number of reads with a barcode read without mismatches", "Number of reads with a barcode read with one mismatch", "Number of reads one mismatch away from several barcodes", "Number of reads that match no barcode",
                            "Number of reads whose barcode is cut off or did not pass quality filtering"]
DEMUX_SAMPLE_STATS_HEAD = ["#Sample name:sample barcode"] + STATS_HEAD[3:]
STRAND_STATS_HEAD = ["#Sample name (strands)", "Number of reads assigned on the forward strand", "Number of reads assigned on the reverse strand without mismatches", "Number of reads assigned on the reverse strand with mismatches", "Number of reads whose reverse strand was examined"]
STAGGER_STATS_HEAD = ["#Sample name (stagger)", "Number of reads assigned at offset 0", "Number of reads assigned at a later offset", "Offset with the most assigned reads"]
INDEL_STATS_HEAD = ["#Sample name (indel)", "Number of reads that were assigned no feature and tried", "Number of reads with a one-base deletion of a feature", "Number of reads with a one-base insertion into a feature", "Number of reads that fit two or more features with one indel"]
PARTS_STATS_HEAD = ["#Sample name (parts)", "Number of reads whose two parts are a library pair, both without mismatches", "Number of reads whose two parts are a library pair, at least one with mismatches", "Number of recombinant reads (two assigned parts the library does not pair)",
                    "Number of distinct recombinant pairs", "Number of reads with part 1 assigned only", "Number of reads with part 2 assigned only",
                    "Number of reads with no part assigned"]
EC_COLLAPSE_STATS_HEAD = ["#Sample name (collapsed sequences)", "Number of distinct sequences", "Number of sequences that can be collapsed", "Number of sequences absorbed by another", "Number of centroids", "Number of reads of the absorbed sequences",
                          "Longest chain of absorbed sequences"]


def run_stats(headers, param, compiled, head, ordered):
    """<name>_stats.csv -- the run's '#key: value' lines, the column names, one row of numbers per sample (:1386-1412,
    taken from the counters themselves) -- plus the four overview plots (:1414-1527)"""
    rows = [[s.name, s.time_value, s.time_unit, s.stats["reads"], s.stats["perfect_counter"] + s.stats["imperfect_counter"],
             s.stats["perfect_counter"], s.stats["imperfect_counter"], s.stats["non_aligned_counter"],
             s.stats["quality_failed"]] for s in ordered]
    global_stat = [[line] for line in headers] + [STATS_HEAD] + rows
    for opt in OPTIONS:                                          # its blocks: a head, then a row per sample (or column) it has numbers of
        global_stat += opt.stats(param, opt.found(ordered)) if opt.found(ordered) else []
    csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}_stats.csv"), global_stat)
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        import numpy as np
    except Exception as exc:                                     # plots are cosmetic; say so and go on
        colourful_errors("WARNING", f"matplotlib unavailable ({exc}); plots skipped")
        return
    base = os.path.join(param["directory"], param['out_file_name'])
    labels = [r[0] for r in rows]

    def bars(relative, path, xlabel, legend):
        fig, ax = plt.subplots(figsize=(12, max(1, int(len(global_stat) / 4))))
        for i, r in enumerate(rows):
            total, aligned, not_aligned, qfail = int(r[3]), int(r[4]), int(r[7]), int(r[8])
            if relative:
                tot = max(total, 1)
                a, n, q = aligned / tot * 100, not_aligned / tot * 100, qfail / tot * 100
                ax.barh(i, a, .75, color="#6290C3", hatch="\\", edgecolor="black", linewidth=.7)
                ax.barh(i, n, .75, left=a, color="#F1FFE7", hatch="//", edgecolor="black", linewidth=.7)
                ax.barh(i, q, .75, left=a + n, color="#FB5012", hatch="||", edgecolor="black", linewidth=.7)
            else:
                ax.barh(i, total, .75, color="#FFD25A", hatch="//", edgecolor="black", linewidth=.7)
                ax.barh(i, aligned, .75, color="#FFAA5A", hatch="\\", edgecolor="black", linewidth=.7)
                ax.barh(i, not_aligned, .75, color="#F56416", hatch="x", edgecolor="black", linewidth=.7)
        ax.set_yticks(np.arange(len(labels)))
        ax.set_yticklabels(labels)
        ax.tick_params(axis='both', which='both', labelsize=16)
        ax.set_xlabel(xlabel, size=20)
        ax.spines['top'].set_visible(False)
        ax.spines['right'].set_visible(False)
        ax.set_xlim(xmin=1)
        ax.legend(legend, loc='right', bbox_to_anchor=(1.1, 1), ncol=3, prop={'size': 12})
        fig.tight_layout()
        fig.savefig(path, dpi=300, bbox_inches='tight')
        plt.close(fig)

    bars(False, base + "_reads_plot.png", 'Number of reads',
         ["Total reads in sample", "Aligned reads", "Reads that passed quality filtering but failed to align"])
    bars(True, base + "_reads_plot_percentage.png", '% of reads per sample',
         ["Aligned reads", "Reads that passed quality filtering but failed to align", "Reads that did not pass quality filtering"])

    per_sample = [[compiled[f][k] for f in compiled] for k in range(len(head) - 1)]

    def violin(data, path, title):
        fig, ax = plt.subplots(figsize=(12, max(1.0, len(global_stat) / 2)))
        ax.set_title(title, size=20)
        ax.set_xlabel('Reads per feature', size=20)
        if data and all(len(d) for d in data):
            parts = ax.violinplot(data, points=200, widths=1, showmeans=False, showmedians=False, showextrema=False, vert=False)
            for pc in parts['bodies']:
                pc.set_facecolor('#D43F3A'); pc.set_edgecolor('black'); pc.set_alpha(1)
            q1, med, q3 = np.percentile(np.array(data, dtype=float), [25, 50, 75], axis=1)
            inds = np.arange(1, len(med) + 1)
            ax.scatter(med, inds, marker='o', color='white', s=40, zorder=3)
            ax.hlines(inds, q1, q3, color='k', linestyle='-', lw=8)
        ax.set_yticks(np.arange(len(head[1:])) + 1)
        ax.set_yticklabels(head[1:])
        ax.tick_params(axis='both', which='major', labelsize=20)
        ax.spines['top'].set_visible(False)
        ax.spines['right'].set_visible(False)
        ax.set_xlim(xmin=1)
        fig.savefig(path, dpi=300, bbox_inches='tight')
        plt.close(fig)

    violin(per_sample, base + "_distribution_plot.png", 'Reads per feature distribution')
    totals = [sum(d) for d in per_sample]                      # (once per sample: the inner sum made this step quadratic in the library size)
    rpm = [[v / t * 1000000 for v in d] for d, t in zip(per_sample, totals) if t > 0]
    violin(rpm if len(rpm) == len(per_sample) else [], base + "_distribution_normalized_RPM_plot.png",
           'Reads per feature (RPM normalized) distribution')


def main(argv=None):
    param = file_sizer_split(initializer(input_parser(argv)))
    features = features_loader(param["feature"]) if param['Running Mode'] == 'C' else {}
    for opt in _options_of(param):                   # refused before the output directory exists
        refusal = opt.library(features, param)
        if refusal:
            colourful_errors("FATAL", refusal)
            sys.exit(2)
    aligner_mp_dispenser(features, param)
    sharding.barrier()
    if sharding.world().rank == 0:
        compiling(param)
    sharding.barrier()


if __name__ == "__main__":
    main()
