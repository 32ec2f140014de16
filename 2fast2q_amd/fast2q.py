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
from dataclasses import dataclass
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
    if param.get('paired'):                         # a paired context: the windows of mate 2 and its direction (f2q_set_mate2)
        plain = {k: v for k, v in param.items() if k != 'paired'}
        kwargs = dict(_counter_kwargs(plain), start2=param['start2'], rc2=bool(param.get('rc2')))
        if param.get('umi_paired'):                 # --umi1 / --umi2: a paired UMI context (f2q_set_umi_paired), part of the key too
            kwargs['umi_paired'] = tuple(param['umi_paired'])
            if param.get('umi_rule') == 'directional':
                kwargs['umi_reads'] = True
        return kwargs                               # (--umih: the plain keys carry it; the UMI of a pair is in mate 1's header)
    kwargs = dict(mode=param['Running Mode'], miss=param['miss'], phred=param['phred'], length=param['length'],
                  start=param['start'], upstream=param['upstream'], downstream=param['downstream'],
                  miss_search_up=param['miss_search_up'], miss_search_down=param['miss_search_down'],
                  qual_up=param['qual_up'], qual_down=param['qual_down'],
                  device=int(param.get('device', os.environ.get("F2Q_DEVICE", os.environ.get("LOCAL_RANK", 0)))))
    if param.get('umi'):                            # a UMI context (f2q_set_umi); part of the key contexts are kept under
        kwargs['umi'] = tuple(param['umi'])         # (--mu is not: collapsing changes no context)
        if param.get('umi_rule') == 'directional':  # --mur directional: the context keeps the reads of every pair (f2q_set_umi_reads)
            kwargs['umi_reads'] = True
    if param.get('umi_header'):                     # --umih: the UMI is in the read header (f2q_set_umi_header)
        kwargs['umi_header'] = tuple(param['umi_header'])
        if param.get('umi_rule') == 'directional':
            kwargs['umi_reads'] = True
    if param.get('sample_barcodes'):                # --sb: a demultiplexing context (f2q_set_sample_barcodes); part of the key too
        sb = param['sample_barcodes']
        kwargs['sample_barcodes'] = (sb['start'], tuple(sb['barcodes']))
        kwargs['barcode_mismatch'] = sb['miss']
    if param.get('strand'):                         # --strand rev / both (f2q_set_strand); part of the key too
        kwargs['strand'] = param['strand']
    if param.get('parts'):                          # --parts: each part of a pair library matched alone (f2q_set_parts); part of the key too
        kwargs['parts'] = True
    if param.get('stagger'):                        # --stagger N: the window tried at N + 1 starts (f2q_set_stagger); part of the key too
        kwargs['stagger'] = param['stagger']
    if param.get('indel'):                          # --indel: one-base insertions and deletions reported (f2q_set_indel); part of the key too
        kwargs['indel'] = True
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
    if (param['upstream'] is not None) and (param['downstream'] is not None):
        if len(str(param['upstream']).split(",")) != len(str(param['downstream']).split(",")):
            colourful_errors("FATAL", "Up and Downstream sequences must be submitted in concurrent pairs, separated by ,.")
            sys.exit()
    local_read_stats = dict.fromkeys(binding.STAT_NAMES, 0)
    if preprocess:                                  # memo warm-up (:1593-1617) has nothing to warm here
        return features, reads_stats, local_read_stats
    counter_mode = param['Running Mode'] == 'C'
    seqs = list(features) if counter_mode else None
    assign = list(param['assign_features']) if param.get('assign') and not counter_mode else None
    if assign is not None and sharding.world().size > 1:
        raise RuntimeError("--as: assignments are not merged across several ranks; run one process")
    if param.get('umi') and sharding.world().size > 1:
        raise RuntimeError("--umi: the UMI sets are not merged across several ranks; run one process")
    if param.get('ec_collapse') and sharding.world().size > 1:
        raise RuntimeError("--ecm 1: the merged tables of several ranks are not collapsed; run one process")
    if param.get('umi_paired') and sharding.world().size > 1:
        raise RuntimeError("--umi1 / --umi2: the UMI sets are not merged across several ranks; run one process")
    if param.get('umi_header') and sharding.world().size > 1:
        raise RuntimeError("--umih: the UMI sets are not merged across several ranks; run one process")
    if param.get('sample_barcodes') and sharding.world().size > 1:
        raise RuntimeError("--sb: the demultiplexed counts are not merged across several ranks; run one process")
    if param.get('strand') and sharding.world().size > 1:
        raise RuntimeError("--strand: the reverse-strand counts are not merged across several ranks; run one process")
    if param.get('parts') and sharding.world().size > 1:
        raise RuntimeError("--parts: the part tables and recombinant sets are not merged across several ranks; run one process")
    if param.get('stagger') and sharding.world().size > 1:
        raise RuntimeError("--stagger: the offset histograms are not merged across several ranks; run one process")
    if param.get('indel') and sharding.world().size > 1:
        raise RuntimeError("--indel: the indel counts are not merged across several ranks; run one process")
    ctx =_context_for(seqs, _counter_kwargs(param)) if assign is None else _context_for(seqs, _counter_kwargs(param), assign)
    try:
        world = sharding.world()
        if param.get('paired'):
            if world.size > 1:
                raise RuntimeError("--pe: paired files are not shared out over several ranks; run one process")
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
        if assign is not None:
            # one match per distinct key on the device: the Counter-mode count vector and counters of the same reads, and
            # every key's feature (f2q_ec_assign)
            acounts, stats = ctx.ec_assign()
            param.setdefault('assigned', {})[raw] = ([int(n) for n in acounts], ctx.ec_assigned())
        if param.get('ec_collapse') and not counter_mode:
            # the sample's plain keys one base apart folded on the device (f2q_ec_collapse): the counters, every key's centroid
            dist, ratio = param['ec_collapse']
            extra = ctx.ec_collapse(dist, ratio)
            param.setdefault('collapsed', {})[raw] = (extra, ctx.ec_collapsed())
        if umi_length(param):                       # distinct UMIs per feature and the two sample-level counters (f2q_read_umis)
            umis, umi_reads, umi_failed = ctx.read_umis()
            # the sample's record: per kind of UMI_TABLES that was computed, a number per feature and the sample-level counters
            rec = param.setdefault('umi_counted', {})[raw] = {"umis": ([int(n) for n in umis], dict(umi_reads=umi_reads, umi_failed=umi_failed))}
            if param.get('umi_mismatch'):           # --mu 1: UMIs of a feature one base apart joined (f2q_umi_collapse)
                molecules, pairs, edges = ctx.collapse_umis(param['umi_mismatch'])
                rec["molecules"] = ([int(n) for n in molecules], dict(umi_pairs=pairs, umi_edges=edges, umi_molecules=int(sum(molecules))))
            if param.get('umi_rule') == 'directional':      # --mur directional: the directional rule on the same set, and its pairs
                molecules, pairs, edges, dominated, reads = ctx.collapse_umis_directional()
                rec["directional"] = ([int(n) for n in molecules], dict(umi_pairs=pairs, umi_edges=edges, umi_dominated=dominated,
                                                                        umi_molecules=int(sum(molecules)), umi_pair_reads=reads))
                rec["pair_table"] = ctx.umi_pairs() if not param.get("delete", True) else None
        if param.get('sample_barcodes'):            # --sb: the count matrix, the counters per sample barcode, the verdicts (f2q_read_demux)
            param.setdefault('demux_counted', {})[raw] = ctx.read_demux()
        if param.get('strand'):                     # --strand rev / both: reads assigned on the reverse strand, the strand counters (f2q_read_strands)
            param.setdefault('strand_counted', {})[raw] = ctx.read_strands()
        if param.get('stagger'):                    # --stagger N: reads assigned without / with mismatches at each offset (f2q_read_stagger)
            param.setdefault('stagger_counted', {})[raw] = ctx.read_stagger()
        if param.get('indel'):                      # --indel: deletion and insertion reads per feature and per position, the four totals (f2q_read_indels)
            param.setdefault('indel_counted', {})[raw] = ctx.read_indels()
        if param.get('parts'):                      # --parts: counts by the part rule, the marginals, the six classes (f2q_read_parts) and the recombinant pairs
            param.setdefault('parts_counted', {})[raw] = (ctx.read_parts(), ctx.parts_recombinants())
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
    return features, reads_stats, local_read_stats


@dataclass
class SampleResult:
    """What one sample contributes to the run's tables: kept in memory from aligner() to compiling()
    (the reference round-trips this through <sample>_reads.csv and an English sentence, :785-799, :1316-1406)."""
    name: str            # file stem without .fastq / .gz (:779-783)
    time_value: str      # "0.52" / "1.03" ...
    time_unit: str       # seconds / minutes / hours
    rows: list           # [feature name, reads] in the sample's row order (numeric or alphabetical, :790-793)
    stats: dict          # the five counters of reads_counter (:310-316)

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
    """One sample (:752-801): count it, order its rows, and keep the result for compiling() in param["samples"].
    <sample>_reads.csv is only written when the temporaries are kept (--k): nothing reads it back."""
    started = time.perf_counter()
    packed = reads_counter(i, raw, features, param, reads_stats)
    if packed is None:
        return reads_stats
    features, reads_stats, local = packed
    rows = _sample_rows([f.name, f.counts] for f in features.values())
    value, unit = _elapsed_text(time.perf_counter() - started)
    sample = SampleResult(_sample_name(raw), value, unit, rows, dict(local))
    if raw in param.get('assigned', {}):             # --as: the table Counter mode would have given, and every key's feature
        acounts, arows = param['assigned'].pop(raw)
        names = [f.name for f in param['assign_features'].values()]
        param.setdefault("assign_samples", {})[sample.name] = SampleResult(sample.name, value, unit, _sample_rows(zip(names, acounts)), dict(local))
        if sharding.world().rank == 0:
            os.makedirs(param["directory"], exist_ok=True)
            csv_writer(os.path.join(param["directory"], sample.name + "_assigned.csv"),
                       [["#key", "reads", "feature_name", "mismatches"]] +
                       [[key, n, names[f] if f >= 0 else "", d] for key, n, _first, f, d in arows])
    if raw in param.get('collapsed', {}):            # --ecm 1: every key's centroid; the sample's column of <name>_collapsed.csv
        extra, crows = param['collapsed'].pop(raw)
        centroids = [(key, cluster) for key, _n, _first, cent, cluster in crows if cent == key]
        param.setdefault("collapse_samples", {})[sample.name] = (
            SampleResult(sample.name, value, unit, _sample_rows(centroids), dict(local)),
            [len(crows), extra["eligible_keys"], extra["absorbed_keys"], len(centroids), extra["absorbed_reads"], extra["longest_chain"]])
        if sharding.world().rank == 0:
            os.makedirs(param["directory"], exist_ok=True)
            csv_writer(os.path.join(param["directory"], sample.name + "_clusters.csv"),
                       [["#key", "reads", "centroid", "cluster_reads"]] + [[key, n, cent, cluster] for key, n, _first, cent, cluster in crows])
    if raw in param.get('umi_counted', {}):          # --umi: the same rows once per kind, holding UMIs / molecules instead of reads
        rec = param['umi_counted'].pop(raw)
        pair_table = rec.pop("pair_table", None)
        names = [f.name for f in features.values()]
        param.setdefault("umi_samples", {})[sample.name] = {
            kind: SampleResult(sample.name, value, unit, _sample_rows(zip(names, column)), dict(local, **stats)) for kind, (column, stats) in rec.items()}
        if not param.get("delete", True) and sharding.world().rank == 0:
            os.makedirs(param["directory"], exist_ok=True)
            kinds = [t for t in UMI_TABLES if t[0] in rec]
            both = _sample_rows((f.name, (f.counts,) + tuple(ns)) for f, ns in zip(features.values(), zip(*(rec[t[0]][0] for t in kinds))))  # (the order of `rows`)
            csv_writer(os.path.join(param["directory"], sample.name + "_umi_reads.csv"),
                       [["#Feature", "Reads"] + [t[2] for t in kinds]] + [[name, *ns] for name, ns in both])
            if pair_table is not None:               # every (feature, UMI) pair with its reads, in f2q_umi_pairs' order
                length = umi_length(param)          # (--umi1 + --umi2: the concatenation as sequenced)
                csv_writer(os.path.join(param["directory"], sample.name + "_umi_pairs.csv"),
                           [["#Feature", "UMI", "Reads"]] + [[names[f], umi_text(int(c), length), int(n)] for f, c, n in zip(*pair_table)])
    if raw in param.get('demux_counted', {}):        # --sb: the same rows once per sample barcode, then the unassigned reads
        matrix, sstats, verdicts = param['demux_counted'].pop(raw)
        names = [f.name for f in features.values()]
        columns = [SampleResult(f"{sample.name}:{bname}", value, unit, _sample_rows(zip(names, (int(n) for n in matrix[b]))),
                                dict(zip(binding.STAT_NAMES, (int(n) for n in sstats[b]))))
                   for b, bname in enumerate(param['sample_barcodes']['names'] + ["unassigned"])]
        param.setdefault("demux_samples", {})[sample.name] = (columns, [int(n) for n in verdicts])
    if raw in param.get('strand_counted', {}):       # --strand rev / both: the sample's column split by the strand a read was counted on
        rev_counts, extra = param['strand_counted'].pop(raw)
        split = [(f.name, int(f.counts) - int(n), int(n)) for f, n in zip(features.values(), rev_counts)]
        columns = [SampleResult(f"{sample.name}:fwd", value, unit, _sample_rows((name, fwd) for name, fwd, _ in split), {}),
                   SampleResult(f"{sample.name}:rev", value, unit, _sample_rows((name, rev) for name, _, rev in split), {})]
        param.setdefault("strand_samples", {})[sample.name] = (columns, [int(n) for n in extra])
    if raw in param.get('stagger_counted', {}):      # --stagger N: the sample's two columns of <name>_stagger.csv
        perfect, imperfect = param['stagger_counted'].pop(raw)
        param.setdefault("stagger_samples", {})[sample.name] = ([int(n) for n in perfect], [int(n) for n in imperfect])
    if raw in param.get('indel_counted', {}):        # --indel: the sample's two columns of <name>_indel.csv and of <name>_indel_positions.csv, its totals
        dels, inss, del_pos, ins_pos, totals = param['indel_counted'].pop(raw)
        names = [f.name for f in features.values()]
        columns = [SampleResult(f"{sample.name}:del", value, unit, _sample_rows(zip(names, (int(n) for n in dels))), {}),
                   SampleResult(f"{sample.name}:ins", value, unit, _sample_rows(zip(names, (int(n) for n in inss))), {})]
        param.setdefault("indel_samples", {})[sample.name] = (columns, [int(n) for n in del_pos], [int(n) for n in ins_pos], [int(n) for n in totals])
    if raw in param.get('parts_counted', {}):        # --parts: the same rows holding parts_counts; the recombinant pairs by their texts; the classes
        (parts_counts, part1, part2, classes), (i1, i2, reads) = param['parts_counted'].pop(raw)
        names = [f.name for f in features.values()]
        firsts, seconds = part_libraries(list(features))
        recombinants = {(firsts[a], seconds[b]): int(n) for a, b, n in zip(i1, i2, reads)}
        param.setdefault("parts_samples", {})[sample.name] = (
            SampleResult(sample.name, value, unit, _sample_rows(zip(names, (int(n) for n in parts_counts))), dict(local)),
            recombinants, dict(zip(binding.PARTS_CLASSES, (int(n) for n in classes))))
        if not param.get("delete", True) and sharding.world().rank == 0:
            os.makedirs(param["directory"], exist_ok=True)
            csv_writer(os.path.join(param["directory"], sample.name + "_parts_marginals.csv"),
                       [["#position", "part", "reads"]] + [[1, part, int(n)] for part, n in zip(firsts, part1)] + [[2, part, int(n)] for part, n in zip(seconds, part2)])
    if not param['Progress bar']:
        colourful_errors("INFO", f"Sample {sample.name} was processed in {value} {unit}")
    param.setdefault("samples", {})[sample.name] = sample     # a later file of the same name replaces the earlier one,
    if not param.get("delete", True) and sharding.world().rank == 0:   # as its _reads.csv would upstream
        csv_writer(os.path.join(param["directory"], sample.name + "_reads.csv"), sample.reads_csv_rows())
    return reads_stats


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
    if param.get('assign'):
        print(f" Extracted sequences are assigned to the features of {param['feature']} ({param['miss']} mismatches allowed)")
    if param.get('paired'):
        print(f" Paired-end: mate 2 start position: {param['start2']}" + (" (mate 2 reverse-complemented)" if param['rc2'] else ""))
    if param.get('umi'):
        print(f" Distinct UMIs are counted per feature: UMI start position in the read: {param['umi'][0]}, length: {param['umi'][1]}bp")
    for mate, part in enumerate(param.get('umi_paired') or (), 1):
        if part:
            print(f" Distinct UMIs are counted per feature: UMI part in mate {mate}, start position: {part[0]}, length: {part[1]}bp")
    if param.get('umi_header'):
        print(f" Distinct UMIs are counted per feature: UMI in the read header, behind the last '{param['umi_header'][0]}' of the read id, length: {param['umi_header'][1]}bp")
    if param.get('sample_barcodes'):
        sb = param['sample_barcodes']
        print(f" Reads are demultiplexed by {len(sb['barcodes'])} inline sample barcodes of {sb['path']}")
        print(f" {sample_barcodes_header(param)[1:]}")
    if param.get('strand'):
        print(f" Reads are counted on {'the reverse strand' if param['strand'] == 'rev' else 'the forward strand, else on the reverse strand'}")
        print(f" {strand_header(param)[1:]}")
    if param.get('stagger'):
        print(f" The feature window is tried at the starts {param['start']} .. {int(param['start']) + param['stagger']}: the earliest exact one counts, else the earliest within --m")
        print(f" {stagger_header(param)[1:]}")
    if param.get('indel'):
        print(" Reads that are assigned no feature are tried as one-base deletions and insertions of every feature; they are reported, not counted")
        print(f" {INDEL_HEADER[1:]}")
    if param.get('parts'):
        print(" Each of the two feature parts is also matched on its own; recombinant reads are counted per pair of parts")
        print(f" {PARTS_HEADER[1:]}")
    if param.get('ec_collapse'):
        print(" Extracted sequences of one sample that differ in one base are collapsed into the one with the most reads")
        print(f" {ec_collapse_header(param)[1:]}")
    if param.get('umi_mismatch'):
        print(f" UMIs of one feature that differ in one base are collapsed (--mu {param['umi_mismatch']})")
    if param.get('umi_rule') == 'directional':
        print(" Molecules are also counted by the directional rule: a UMI absorbs a neighbour with at most (its reads + 1) / 2 reads (--mur directional)")
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


def sample_barcodes_header(param):
    """the line a --sb run adds to the parameter print-out and to the head of <name>_stats.csv"""
    sb = param['sample_barcodes']
    return f"#Sample barcodes, start, length, mismatches: {sb['start']},{len(sb['barcodes'][0])},{sb['miss']}"


def stagger_header(param):
    """the line a --stagger N run (N > 0) adds to the parameter print-out and to the head of <name>_stats.csv"""
    return f"#Stagger: {param['stagger']}"


INDEL_HEADER = "#Indel reads reported: 1"      # the line an --indel run adds to the parameter print-out and to the head of <name>_stats.csv


def strand_header(param):
    """the line a --strand rev / both run adds to the parameter print-out and to the head of <name>_stats.csv"""
    return f"#Strand: {param['strand']}"


# the line a --parts run adds to the parameter print-out and to the head of <name>_stats.csv
PARTS_HEADER = "#Parts matched independently: 2"


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
    ap.add_argument("--pe", nargs='?', const=True, help="Paired-end: the files of --s are paired by name (_R1/_R2, else _1/_2); --st names the feature parts in mate 1, --st2 those in mate 2")
    ap.add_argument("--st2", help="With --pe: the start position(s) of the feature part(s) within mate 2")
    ap.add_argument("--rc2", nargs='?', const=True, help="With --pe: mate 2 is reverse-complemented before its parts are taken")
    ap.add_argument("--umi", help="S,L: every read carries a UMI of L bases (1-16) at position S; Counter mode also reports the distinct UMIs per feature (<name>_umi.csv)")
    ap.add_argument("--umi1", help="With --pe, S,L: the UMI (or its first part) is L bases at position S of mate 1")
    ap.add_argument("--umi2", help="With --pe, S,L: the UMI (or its second part) is L bases at position S of mate 2 as sequenced (whatever --rc2 says); --umi1 and --umi2 together hold 16 bases at most")
    ap.add_argument("--umih", help="SEP,L: the UMI of every read is in its header, the L bases (1-16) behind the last SEP of the read id, e.g. _,8 after umi_tools extract / fastp --umi, :,8 for an Illumina index-read UMI; with --pe: mate 1's header. Takes the place of --umi / --umi1 / --umi2")
    ap.add_argument("--mu", help="With --umi (or --umih, --umi1 / --umi2): mismatches in the UMI, 0 or 1 (default 0). 1: UMIs of one feature that differ in one base count as one molecule (<name>_umi_collapsed.csv)")
    ap.add_argument("--mur", help="With --umi and --mu 1: the rule UMIs are collapsed by, cluster (default) or directional. directional: a UMI absorbs a neighbouring UMI only when it has at least twice its reads minus one (<name>_umi_directional.csv)")
    ap.add_argument("--sb", help="The full path to a .csv file with rows name,barcode: the reads of every file are demultiplexed by an inline sample barcode (1-16 bases, at most 1024 barcodes of one length) while they are counted (<name>_demux.csv). Counter mode, single reads, one process")
    ap.add_argument("--sbs", help="With --sb: the start position of the sample barcode within the read (default = 0)")
    ap.add_argument("--sbm", help="With --sb: mismatches allowed in the sample barcode, 0 or 1 (default = 0)")
    ap.add_argument("--strand", help="fwd (default), rev or both: the orientation the reads are counted in. rev: every read is reverse-complemented first; both: a read that is assigned no feature as sequenced is tried reverse-complemented (<name>_strand.csv). Counter mode, single reads, one process")
    ap.add_argument("--stagger", help="N (0-32): the one fixed window (--st s --l L) is tried at the starts s .. s+N; a read counts at the earliest start that reads a feature exactly, else at the earliest one within --m (<name>_stagger.csv). 0 (default): off. Counter mode, single reads, one --st value, one process")
    ap.add_argument("--indel", nargs='?', const=True, help="Reads that the one fixed window (--st s --l L, L 2-31) assigns to no feature are tried as a one-base deletion and as a one-base insertion of every feature of L bases; they are reported per feature and per position (<name>_indel.csv, <name>_indel_positions.csv) and change no count. Counter mode, single reads, one --st value, one process")
    ap.add_argument("--parts", nargs='?', const=True, help="Pair libraries (features A:B over exactly two windows: --st a,b, or --pe --st a --st2 b): each part is also matched on its own with --m mismatches per part; reads whose two parts the library does not pair are counted as recombinants (<name>_parts.csv, <name>_recombinants.csv). Counter mode, one process")
    ap.add_argument("--as", dest="assign", nargs='?', const=True, help="With --mo EC and --g: every extracted sequence is also assigned to its feature (--m mismatches), giving the Counter mode table of the same run")
    ap.add_argument("--ecm", help="With --mo EC: mismatches among the extracted sequences, 0 (default) or 1. 1: per sample, every plain sequence of at most 29 bases is folded into the sequence one substitution away with the most reads, when that one has at least --ecr times its reads (<sample>_clusters.csv, <name>_collapsed.csv). One fixed window of at most 29 bases or one --us/--ds pair, single reads, one process")
    ap.add_argument("--ecr", help="With --ecm 1: the reads a sequence needs, as a multiple of another's, to absorb it: 2-255 (default = 5)")
    args = ap.parse_args(argv)
    if args.ecm is not None and args.ecm.strip() == "0" and args.ecr is None:
        args.ecm = None                                         # --ecm 0 is a run without the flag
    if args.v is not None:
        print(f"\nVersion: {version}\n")
        sys.exit()
    if args.c is None:
        return None
    if args.pe is not None and args.t is not None:
        colourful_errors("FATAL", "--pe cannot be combined with -t: the test mode runs on one packaged single-end sample.")
        sys.exit(2)
    if args.assign is not None and (args.g is None or args.t is not None):
        colourful_errors("FATAL", "--as needs --g: the .csv file with the features the extracted sequences are assigned to.")
        sys.exit(2)
    p = {"cmd": True, "big_file_split": args.fs is not None}
    p['used_cmd'] = " ".join(f"--{k}" if isinstance(v, bool) and v else f"--{k} {v}"
                             for k, v in ((("as" if k == "assign" else k), v) for k, v in vars(args).items()) if v is not None)
    p['Running Mode'] = "EC" if (args.mo is not None and "EC" in args.mo.upper()) else "C"
    if args.t is None:
        p["test_mode"] = False
        paths = [[args.s, 'seq_files'], [args.g, 'feature'], [args.o, 'out']]
    else:
        p["test_mode"] = True
        paths = [[ensure_example_fastq(), 'seq_files'], [_package_data('D39V_guides.csv'), 'feature'], [os.getcwd(), 'out']]
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
    if args.pe is not None:
        if args.us is not None or args.ds is not None:
            colourful_errors("FATAL", "--pe takes fixed positions only (--st / --st2): it cannot be combined with --us / --ds.")
            sys.exit(2)
        if args.st2 is None:
            colourful_errors("FATAL", "--pe needs --st2: the start position(s) of the feature part(s) within mate 2.")
            sys.exit(2)
        p['paired'], p['start2'], p['rc2'] = True, args.st2, args.rc2 is not None
    elif args.st2 is not None or args.rc2 is not None:
        colourful_errors("FATAL", f"{'--st2' if args.st2 is not None else '--rc2'} only has a meaning with --pe.")
        sys.exit(2)
    if args.umi is not None:
        if p['Running Mode'] != "C":
            colourful_errors("FATAL", "--umi only has a meaning in Counter mode: it cannot be combined with --mo EC.")
            sys.exit(2)
        if args.pe is not None:
            colourful_errors("FATAL", "--umi takes single reads: it cannot be combined with --pe. The UMI of a pair is named per mate with --umi1 S,L and / or --umi2 S,L.")
            sys.exit(2)
        p['umi'] = parse_umi(args.umi)
        if p['umi'] is None:
            colourful_errors("FATAL", f"--umi {args.umi}: expected S,L with a start S >= 0 and a length 1 <= L <= 16.")
            sys.exit(2)
    if args.umi1 is not None or args.umi2 is not None:
        given = " / ".join(f for f, v in (("--umi1", args.umi1), ("--umi2", args.umi2)) if v is not None)
        if args.pe is None:
            colourful_errors("FATAL", f"{given} only has a meaning with --pe: the UMI part of one mate of a pair (single reads: --umi).")
            sys.exit(2)
        if args.umi is not None:
            colourful_errors("FATAL", f"{given} cannot be combined with --umi: --umi names the UMI of single reads.")
            sys.exit(2)
        if p['Running Mode'] != "C":
            colourful_errors("FATAL", f"{given} only has a meaning in Counter mode: it cannot be combined with --mo EC.")
            sys.exit(2)
        parts = []
        for flag, value in (("--umi1", args.umi1), ("--umi2", args.umi2)):
            parts.append(None if value is None else parse_umi(value))
            if value is not None and parts[-1] is None:
                colourful_errors("FATAL", f"{flag} {value}: expected S,L with a start S >= 0 and a length 1 <= L <= 16.")
                sys.exit(2)
        if sum(part[1] for part in parts if part) > 16:
            colourful_errors("FATAL", f"--umi1 {args.umi1} --umi2 {args.umi2}: the two parts together hold 16 bases at most.")
            sys.exit(2)
        p['umi_paired'] = tuple(parts)
    if args.umih is not None:
        others = [f for f, v in (("--umi", args.umi), ("--umi1", args.umi1), ("--umi2", args.umi2)) if v is not None]
        if others:
            colourful_errors("FATAL", f"--umih cannot be combined with {' / '.join(others)}: a run has one source of UMIs, the read header or the read.")
            sys.exit(2)
        if p['Running Mode'] != "C":
            colourful_errors("FATAL", "--umih only has a meaning in Counter mode: it cannot be combined with --mo EC.")
            sys.exit(2)
        parsed = parse_umih(args.umih)
        if isinstance(parsed, str):
            colourful_errors("FATAL", f"--umih {args.umih}: {parsed}.")
            sys.exit(2)
        p['umi_header'] = parsed
    any_umi = args.umi is not None or args.umi1 is not None or args.umi2 is not None or args.umih is not None
    if args.mu is not None:
        if not any_umi:
            colourful_errors("FATAL", "--mu only has a meaning with --umi: the mismatches allowed between two UMIs of one feature.")
            sys.exit(2)
        if args.mu not in ("0", "1"):
            colourful_errors("FATAL", f"--mu {args.mu}: expected 0 or 1 (UMIs are collapsed at Hamming distance 1 at most).")
            sys.exit(2)
        if args.mu == "1":
            p['umi_mismatch'] = 1
    if args.mur is not None:
        if args.mur not in ("cluster", "directional"):
            colourful_errors("FATAL", f"--mur {args.mur}: expected cluster or directional.")
            sys.exit(2)
        if not any_umi or args.mu != "1":
            colourful_errors("FATAL", "--mur only has a meaning with --umi and --mu 1: the rule UMIs one base apart are collapsed by.")
            sys.exit(2)
        if args.mur == "directional":
            p['umi_rule'] = 'directional'
    if args.sb is None and (args.sbs is not None or args.sbm is not None):
        colourful_errors("FATAL", f"{'--sbs' if args.sbs is not None else '--sbm'} only has a meaning with --sb: the .csv file with the sample barcodes.")
        sys.exit(2)
    if args.sb is not None:
        if p['Running Mode'] != "C":
            colourful_errors("FATAL", "--sb only has a meaning in Counter mode: it cannot be combined with --mo EC.")
            sys.exit(2)
        others = [f for f, v in (("--pe", args.pe), ("--umi", args.umi), ("--umi1", args.umi1), ("--umi2", args.umi2), ("--umih", args.umih)) if v is not None]
        if others:
            colourful_errors("FATAL", f"--sb cannot be combined with {' / '.join(others)}: sample barcodes are taken from single reads without UMIs.")
            sys.exit(2)
        if args.sbs is not None and not (args.sbs.isascii() and args.sbs.isdigit() and int(args.sbs) <= 0x3FFFFFFF):
            colourful_errors("FATAL", f"--sbs {args.sbs}: expected the start position of the sample barcode within the read, a number >= 0.")
            sys.exit(2)
        if args.sbm is not None and args.sbm not in ("0", "1"):
            colourful_errors("FATAL", f"--sbm {args.sbm}: expected 0 or 1 (sample barcodes are matched at Hamming distance 1 at most).")
            sys.exit(2)
        loaded = sample_barcodes_loader(args.sb)
        if isinstance(loaded, str):
            colourful_errors("FATAL", f"--sb {args.sb}: {loaded}.")
            sys.exit(2)
        p['sample_barcodes'] = dict(path=args.sb, names=loaded[0], barcodes=loaded[1], start=int(args.sbs or 0), miss=int(args.sbm or 0))
    if args.strand is not None:
        if args.strand not in ("fwd", "rev", "both"):
            colourful_errors("FATAL", f"--strand {args.strand}: expected fwd, rev or both.")
            sys.exit(2)
        if args.strand != "fwd":                                 # (fwd is a run without the flag)
            if p['Running Mode'] != "C":
                colourful_errors("FATAL", f"--strand {args.strand} only has a meaning in Counter mode: it cannot be combined with --mo EC.")
                sys.exit(2)
            others = [f for f, v in (("--pe", args.pe), ("--umi", args.umi), ("--umi1", args.umi1), ("--umi2", args.umi2), ("--umih", args.umih), ("--sb", args.sb)) if v is not None]
            if others:
                colourful_errors("FATAL", f"--strand {args.strand} cannot be combined with {' / '.join(others)}: the reverse strand is read from single reads without UMIs or sample barcodes.")
                sys.exit(2)
            p['strand'] = args.strand
    if args.parts is not None:
        if p['Running Mode'] != "C":
            colourful_errors("FATAL", "--parts only has a meaning in Counter mode: it cannot be combined with --mo EC.")
            sys.exit(2)
        others = [f for f, v in (("--us", args.us), ("--ds", args.ds), ("--umi", args.umi), ("--umi1", args.umi1), ("--umi2", args.umi2), ("--umih", args.umih), ("--sb", args.sb)) if v is not None]
        if args.strand in ("rev", "both"):
            others.append(f"--strand {args.strand}")
        if others:
            colourful_errors("FATAL", f"--parts cannot be combined with {' / '.join(others)}: the parts are matched at fixed positions, without UMIs, sample barcodes or a strand mode.")
            sys.exit(2)
        windows = [len(str(p['start']).split(","))] + ([len(str(args.st2).split(","))] if args.pe is not None else [])
        if windows not in ([2], [1, 1]):
            colourful_errors("FATAL", f"--parts needs exactly two windows: --st a,b for single reads, or one window per mate with --pe (--st a --st2 b); "
                                      f"--st {p['start']}" + (f" --st2 {args.st2}" if args.pe is not None else "") + f" names {' + '.join(str(n) for n in windows)}.")
            sys.exit(2)
        p['parts'] = True
    if args.stagger is not None:
        if not re.fullmatch(r"[0-9]{1,3}", str(args.stagger)) or int(args.stagger) > 32:
            colourful_errors("FATAL", f"--stagger {args.stagger}: expected a number of extra starts, 0 to 32.")
            sys.exit(2)
        if int(args.stagger):                                    # (0 is a run without the flag)
            if p['Running Mode'] != "C":
                colourful_errors("FATAL", f"--stagger {args.stagger} only has a meaning in Counter mode: it cannot be combined with --mo EC.")
                sys.exit(2)
            others = [f for f, v in (("--pe", args.pe), ("--us", args.us), ("--ds", args.ds), ("--umi", args.umi), ("--umi1", args.umi1), ("--umi2", args.umi2),
                                     ("--umih", args.umih), ("--sb", args.sb), ("--parts", args.parts)) if v is not None]
            if args.strand in ("rev", "both"):
                others.append(f"--strand {args.strand}")
            if others:
                colourful_errors("FATAL", f"--stagger {args.stagger} cannot be combined with {' / '.join(others)}: one fixed window of single reads is tried at "
                                          "several starts, without anchors, UMIs, sample barcodes, a strand mode or parts.")
                sys.exit(2)
            if not re.fullmatch(r"[0-9]+", str(p['start']).strip()):
                colourful_errors("FATAL", f"--stagger {args.stagger} needs exactly one window start at or after the first base: --st {p['start']} does not name one.")
                sys.exit(2)
            p['stagger'] = int(args.stagger)
    if args.indel is not None:
        if args.indel is not True:
            colourful_errors("FATAL", f"--indel takes no value: --indel {args.indel} is not understood.")
            sys.exit(2)
        if p['Running Mode'] != "C":
            colourful_errors("FATAL", "--indel only has a meaning in Counter mode: it cannot be combined with --mo EC.")
            sys.exit(2)
        others = [f for f, v in (("--pe", args.pe), ("--us", args.us), ("--ds", args.ds), ("--umi", args.umi), ("--umi1", args.umi1), ("--umi2", args.umi2),
                                 ("--umih", args.umih), ("--sb", args.sb), ("--parts", args.parts)) if v is not None]
        if args.strand in ("rev", "both"):
            others.append(f"--strand {args.strand}")
        if p.get('stagger'):
            others.append(f"--stagger {p['stagger']}")
        if others:
            colourful_errors("FATAL", f"--indel cannot be combined with {' / '.join(others)}: the unassigned reads of one fixed window of single reads are "
                                      "examined, without anchors, UMIs, sample barcodes, a strand mode, parts or a stagger.")
            sys.exit(2)
        if not re.fullmatch(r"[0-9]+", str(p['start']).strip()):
            colourful_errors("FATAL", f"--indel needs exactly one window start at or after the first base: --st {p['start']} does not name one.")
            sys.exit(2)
        if not 2 <= p['length'] <= 31:
            colourful_errors("FATAL", f"--indel needs a window of 2 to 31 bases: --l {p['length']} is outside that range.")
            sys.exit(2)
        p['indel'] = True
    if args.assign is not None:
        if p['Running Mode'] != "EC":
            colourful_errors("FATAL", "--as only has a meaning with --mo EC: Counter mode assigns every read already.")
            sys.exit(2)
        p['assign'] = True
    if args.ecm is not None or args.ecr is not None:
        refusal = ec_collapse_refusal(args, p)
        if refusal:
            colourful_errors("FATAL", refusal)
            sys.exit(2)
        p['ec_collapse'] = (1, int(args.ecr) if args.ecr is not None else 5)
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


def ec_collapse_refusal(args, p):
    """why --ecm / --ecr cannot be taken as given, else None (input_parser: before any output directory exists)"""
    ecm = None if args.ecm is None else args.ecm.strip()
    if ecm not in (None, "0", "1"):
        return f"--ecm takes 0 or 1 (mismatches among the extracted sequences): --ecm {args.ecm} is not understood."
    if ecm != "1":                                              # (--ecm 0 alone never gets here)
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
    return None


def file_sizer_split(param):
    """sample discovery (:1657-1689): *.gz and *.fastq of the --s directory, smallest first"""
    if param["test_mode"]:
        param["sequencing_files"] = {"len_files": 1, "preprocess_files": [param["seq_files"]], "files": [param["seq_files"]]}
        return param
    files = [p[0] for p in path_parser(param["seq_files"], ["*.gz", "*.fastq"])]
    if param.get('umi_paired') and sharding.world().size > 1:
        colourful_errors("FATAL", "--umi1 / --umi2: the UMI sets are not merged across several ranks; run one process.")
        sys.exit(2)
    if param.get('umi_header') and sharding.world().size > 1:
        colourful_errors("FATAL", "--umih: the UMI sets are not merged across several ranks; run one process.")
        sys.exit(2)
    if param.get('sample_barcodes') and sharding.world().size > 1:
        colourful_errors("FATAL", "--sb: the demultiplexed counts are not merged across several ranks; run one process.")
        sys.exit(2)
    if param.get('strand') and sharding.world().size > 1:
        colourful_errors("FATAL", "--strand: the reverse-strand counts are not merged across several ranks; run one process.")
        sys.exit(2)
    if param.get('stagger') and sharding.world().size > 1:
        colourful_errors("FATAL", "--stagger: the offset histograms are not merged across several ranks; run one process.")
        sys.exit(2)
    if param.get('indel') and sharding.world().size > 1:
        colourful_errors("FATAL", "--indel: the indel counts are not merged across several ranks; run one process.")
        sys.exit(2)
    if param.get('parts') and sharding.world().size > 1:
        colourful_errors("FATAL", "--parts: the part tables and recombinant sets are not merged across several ranks; run one process.")
        sys.exit(2)
    if param.get('paired'):                                      # one sample per pair, named after its R1 file
        if sharding.world().size > 1:
            colourful_errors("FATAL", "--pe: paired files are not shared out over several ranks; run one process.")
            sys.exit(2)
        try:
            pairs = pair_files(files)
        except ValueError as exc:
            colourful_errors("FATAL", str(exc))
            sys.exit(2)
        param['mates'] = dict(pairs)
        files = [r1 for r1, _ in pairs]
    if param.get('assign') and sharding.world().size > 1:
        colourful_errors("FATAL", "--as: assignments are not merged across several ranks; run one process.")
        sys.exit(2)
    if param.get('umi') and sharding.world().size > 1:
        colourful_errors("FATAL", "--umi: the UMI sets are not merged across several ranks; run one process.")
        sys.exit(2)
    if param.get('ec_collapse') and sharding.world().size > 1:
        colourful_errors("FATAL", "--ecm 1: the merged tables of several ranks live on the host and are not collapsed; run one process.")
        sys.exit(2)
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


def ec_collapse_header(param):
    return "#Extracted sequences collapsed, mismatches, ratio: %d,%d" % param['ec_collapse']


EC_COLLAPSE_STATS_HEAD = ["#Sample name (collapsed sequences)", "Number of distinct sequences", "Number of sequences that can be collapsed",
                          "Number of sequences absorbed by another", "Number of centroids", "Number of reads of the absorbed sequences",
                          "Longest chain of absorbed sequences"]


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
    if param.get('paired'):
        lines += [f"#Paired-end, feature start position in mate 2: {param['start2']}",
                  f"#Mate 2 reverse-complemented: {'yes' if param['rc2'] else 'no'}"]
    if param.get('umi'):
        lines.append(f"#UMI start position in the read, length: {param['umi'][0]},{param['umi'][1]}")
    for mate, part in enumerate(param.get('umi_paired') or (), 1):
        if part:
            lines.append(f"#UMI in mate {mate}, start, length: {part[0]},{part[1]}")
    if param.get('umi_header'):
        lines.append(f"#UMI in read header, separator, length: {param['umi_header'][0]},{param['umi_header'][1]}")
    if param.get('umi_mismatch'):
        lines.append(f"#UMI mismatches collapsed: {param['umi_mismatch']}")
    if param.get('umi_rule') == 'directional':
        lines.append("#UMI collapse rule: directional")
    if param.get('sample_barcodes'):
        lines.append(sample_barcodes_header(param))
    if param.get('strand'):
        lines.append(strand_header(param))
    if param.get('stagger'):
        lines.append(stagger_header(param))
    if param.get('indel'):
        lines.append(INDEL_HEADER)
    if param.get('parts'):
        lines.append(PARTS_HEADER)
    if param.get('ec_collapse'):
        lines.append(ec_collapse_header(param))
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
    csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}.csv"),
               [head] + [[feature] + counts for feature, counts in table.items()])
    if param.get("assign_samples"):                  # --as: the table Counter mode would have written for the same samples
        _, ahead, atable = compile_table(param["assign_samples"])
        csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}_features.csv"),
                   [ahead] + [[feature] + counts for feature, counts in atable.items()])
    if param.get("collapse_samples"):                # --ecm 1: <name>.csv's layout over the samples' centroids and their cluster reads
        _, chead, ctable = compile_table({name: rec[0] for name, rec in param["collapse_samples"].items()})
        csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}_collapsed.csv"),
                   [chead] + [[feature] + counts for feature, counts in ctable.items()])
    for kind, suffix, _, _, _ in UMI_TABLES:         # --umi / --mu 1 / --mur directional: <name>.csv's layout and row order per kind
        per_sample = {name: rec[kind] for name, rec in param.get("umi_samples", {}).items() if kind in rec}
        if per_sample:
            _, uhead, utable = compile_table(per_sample)
            csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}{suffix}.csv"),
                       [uhead] + [[feature] + counts for feature, counts in utable.items()])
    if param.get("demux_samples"):                   # --sb: per file, in <name>.csv's column order, a column per barcode, then the unassigned reads
        dhead, dtable = _table_of([column for s in ordered for column in param["demux_samples"].get(s.name, ((), ()))[0]])
        csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}_demux.csv"),
                   [dhead] + [[feature] + counts for feature, counts in dtable.items()])
    if param.get("strand_samples"):                  # --strand rev / both: per file, in <name>.csv's column order, the forward and the reverse column
        shead, stable = _table_of([column for s in ordered for column in param["strand_samples"].get(s.name, ((), ()))[0]])
        csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}_strand.csv"),
                   [shead] + [[feature] + counts for feature, counts in stable.items()])
    if param.get("stagger_samples"):                 # --stagger N: a row per offset; per file, in <name>.csv's column order, its perfect and its imperfect reads
        stag = param["stagger_samples"]
        names = [s.name for s in ordered if s.name in stag]
        csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}_stagger.csv"),
                   [["#Offset", "Start"] + [f"{name}:{kind}" for name in names for kind in ("perfect", "imperfect")]] +
                   [[d, int(param['start']) + d] + [stag[name][k][d] for name in names for k in (0, 1)] for d in range(param['stagger'] + 1)])
    if param.get("indel_samples"):                   # --indel: per file, in <name>.csv's column order, its deletion and its insertion column; a row per position
        ind = param["indel_samples"]
        ihead, itable = _table_of([column for s in ordered for column in ind.get(s.name, ((),))[0]])
        csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}_indel.csv"),
                   [ihead] + [[feature] + counts for feature, counts in itable.items()])
        names = [s.name for s in ordered if s.name in ind]
        csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}_indel_positions.csv"),
                   [["#Position"] + [f"{name}:{kind}" for name in names for kind in ("del", "ins")]] +
                   [[p] + [ind[name][k][p] for name in names for k in (1, 2)] for p in range(param['length'])])
    if param.get("parts_samples"):                   # --parts: <name>.csv's layout and row order holding parts_counts; the recombinant pairs of any sample
        parts = param["parts_samples"]
        _, phead, ptable = compile_table({name: rec[0] for name, rec in parts.items()})
        csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}_parts.csv"),
                   [phead] + [[feature] + counts for feature, counts in ptable.items()])
        columns = [parts[s.name][1] for s in ordered if s.name in parts]
        pairs = sorted({pair for column in columns for pair in column}, key=lambda pair: (-sum(column.get(pair, 0) for column in columns), pair))
        csv_writer(os.path.join(param["directory"], f"{param['out_file_name']}_recombinants.csv"),
                   [["#Part1", "Part2"] + [s.name for s in ordered if s.name in parts]] + [[a, b] + [column.get((a, b), 0) for column in columns] for a, b in pairs])
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


UMI_STATS_HEAD = ["#Sample name (UMI)", "Number of aligned reads with a valid UMI", "Number of aligned reads with an invalid UMI"]
UMI_COLLAPSE_STATS_HEAD = ["#Sample name (UMI collapsed)", "Number of distinct (feature, UMI) pairs", "Number of pairs of them that differ in one base",
                           "Number of molecules"]
UMI_DIRECTIONAL_STATS_HEAD = ["#Sample name (UMI directional)", "Number of distinct (feature, UMI) pairs", "Number of pairs of them that differ in one base",
                              "Number of pairs a neighbour absorbs directly", "Number of molecules", "Number of reads of all pairs"]
# what a UMI run reports, one record per sample (param["umi_samples"][name][kind], a SampleResult): kind, suffix of the run's
# table, column of <sample>_umi_reads.csv, head and counters of its block of <name>_stats.csv.  --umi gives the first,
# --mu 1 the second, --mur directional the third
UMI_TABLES = (("umis", "_umi", "UMIs", UMI_STATS_HEAD, ("umi_reads", "umi_failed")),
              ("molecules", "_umi_collapsed", "Molecules", UMI_COLLAPSE_STATS_HEAD, ("umi_pairs", "umi_edges", "umi_molecules")),
              ("directional", "_umi_directional", "Directional", UMI_DIRECTIONAL_STATS_HEAD,
               ("umi_pairs", "umi_edges", "umi_dominated", "umi_molecules", "umi_pair_reads")))


DEMUX_VERDICT_STATS_HEAD = ["#Sample name (sample barcodes)", "Number of reads with a barcode read without mismatches", "Number of reads with a barcode read with one mismatch",
                            "Number of reads one mismatch away from several barcodes", "Number of reads that match no barcode",
                            "Number of reads whose barcode is cut off or did not pass quality filtering"]
DEMUX_SAMPLE_STATS_HEAD = ["#Sample name:sample barcode"] + STATS_HEAD[3:]


STRAND_STATS_HEAD = ["#Sample name (strands)", "Number of reads assigned on the forward strand", "Number of reads assigned on the reverse strand without mismatches",
                     "Number of reads assigned on the reverse strand with mismatches", "Number of reads whose reverse strand was examined"]


STAGGER_STATS_HEAD = ["#Sample name (stagger)", "Number of reads assigned at offset 0", "Number of reads assigned at a later offset", "Offset with the most assigned reads"]


INDEL_STATS_HEAD = ["#Sample name (indel)", "Number of reads that were assigned no feature and tried", "Number of reads with a one-base deletion of a feature",
                    "Number of reads with a one-base insertion into a feature", "Number of reads that fit two or more features with one indel"]


PARTS_STATS_HEAD = ["#Sample name (parts)", "Number of reads whose two parts are a library pair, both without mismatches",
                    "Number of reads whose two parts are a library pair, at least one with mismatches", "Number of recombinant reads (two assigned parts the library does not pair)",
                    "Number of distinct recombinant pairs", "Number of reads with part 1 assigned only", "Number of reads with part 2 assigned only",
                    "Number of reads with no part assigned"]


def run_stats(headers, param, compiled, head, ordered):
    """<name>_stats.csv -- the run's '#key: value' lines, the column names, one row of numbers per sample (:1386-1412,
    taken from the counters themselves) -- plus the four overview plots (:1414-1527)"""
    rows = [[s.name, s.time_value, s.time_unit, s.stats["reads"], s.stats["perfect_counter"] + s.stats["imperfect_counter"],
             s.stats["perfect_counter"], s.stats["imperfect_counter"], s.stats["non_aligned_counter"],
             s.stats["quality_failed"]] for s in ordered]
    global_stat = [[line] for line in headers] + [STATS_HEAD] + rows
    umi = param.get("umi_samples", {})
    for kind, _, _, stats_head, columns in UMI_TABLES:       # per kind: its head, then one line of counters per sample
        if any(kind in rec for rec in umi.values()):
            global_stat += [stats_head] + [[s.name] + [umi[s.name][kind].stats[c] for c in columns] for s in ordered if kind in umi.get(s.name, {})]
    demux = param.get("demux_samples", {})
    if demux:                                                    # --sb: the verdicts per file, then the counters per (file, barcode)
        global_stat += [DEMUX_VERDICT_STATS_HEAD] + [[s.name] + demux[s.name][1] for s in ordered if s.name in demux]
        global_stat += [DEMUX_SAMPLE_STATS_HEAD] + [
            [c.name, c.stats["reads"], c.stats["perfect_counter"] + c.stats["imperfect_counter"], c.stats["perfect_counter"],
             c.stats["imperfect_counter"], c.stats["non_aligned_counter"], c.stats["quality_failed"]]
            for s in ordered if s.name in demux for c in demux[s.name][0]]
    strands = param.get("strand_samples", {})
    if strands:                                                  # --strand rev / both: the four strand counters per file
        global_stat += [STRAND_STATS_HEAD] + [[s.name] + strands[s.name][1] for s in ordered if s.name in strands]
    stag = param.get("stagger_samples", {})
    if stag:                                                     # --stagger N: where the reads of each file were assigned
        global_stat.append(STAGGER_STATS_HEAD)
        for s in ordered:
            if s.name in stag:
                both = [a + b for a, b in zip(*stag[s.name])]
                global_stat.append([s.name, both[0], sum(both[1:]), both.index(max(both))])
    ind = param.get("indel_samples", {})
    if ind:                                                      # --indel: the four totals per file
        global_stat += [INDEL_STATS_HEAD] + [[s.name] + ind[s.name][3] for s in ordered if s.name in ind]
    parts = param.get("parts_samples", {})
    if parts:                                                    # --parts: the six read classes per file, the distinct recombinant pairs next to their reads
        global_stat += [PARTS_STATS_HEAD] + [
            [s.name, c["pair_perfect"], c["pair_imperfect"], c["recombinant"], len(parts[s.name][1]), c["part1_only"], c["part2_only"], c["neither"]]
            for s in ordered if s.name in parts for c in [parts[s.name][2]]]
    coll = param.get("collapse_samples", {})
    if coll:                                                     # --ecm 1: the collapse of each file
        global_stat += [EC_COLLAPSE_STATS_HEAD] + [[s.name] + coll[s.name][1] for s in ordered if s.name in coll]
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
    features = {}
    if param['Running Mode'] == 'C':
        features = features_loader(param["feature"])
        if param.get('parts'):                       # refused before the output directory exists
            wrong = check_parts_library(features)
            if wrong:
                colourful_errors("FATAL", f"--parts takes a library of pairs, --g {param['feature']}: {wrong}.")
                sys.exit(2)
    elif param.get('assign'):
        param['assign_features'] = features_loader(param["feature"])
    aligner_mp_dispenser(features, param)
    sharding.barrier()
    if sharding.world().rank == 0:
        compiling(param)
    sharding.barrier()


if __name__ == "__main__":
    main()
