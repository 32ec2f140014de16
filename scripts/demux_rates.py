"""Cost of demultiplexing by an inline sample barcode (--sb; f2q_set_sample_barcodes)
(python scripts/demux_rates.py [n_reads] [out_file] [parent_checkout]; out_file defaults to profiles/r14_demux_rates.txt):
one JSON line over 150-base reads (10 k features of 20 bases, --st 0 --l 20 --m 1) that carry one of the sample barcodes at
[20, 28) -- 85 % as it is, 10 % with one substitution, 5 % random --, 2 M reads by default.
  (a) the block made once (f2q_block_from_fastq) and counted from there: the HIP-event time of k_count_demux with 96 and 384
      barcodes, --sbm 0 and 1, the barcode table in LDS and in global memory (F2Q_DEMUX_TABLE; a table of more than 4096
      slots stays in global memory whatever the switch says -- the line says which instance ran)
  (b) k_count_general<false> on the same block, a plain context under F2Q_FORCE_GENERAL=1: this tree's, and -- when
      parent_checkout names a built checkout of the parent commit -- the parent's
  (c) f2q_count_text on the same text uploaded once, and f2q_count_file on it as a plain file, each with (96 barcodes,
      --sbm 1) and without the barcodes: wall time of the call
Every figure comes from a process of its own (this file with --one) under a time limit, the kinds taking turns, twice;
nothing more is started after a failure."""
import importlib, json, os, re, subprocess, sys, tempfile, time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
START, LENGTH, BC = 0, 20, (20, 8)
CHUNK = 250_000
DEMUX_KINDS = tuple(f"demux_{nb}_{m}_{where}" for nb in (96, 384) for m in (0, 1) for where in ("lds", "global"))
GENERAL_KINDS = ("general", "general_parent")
INGEST_KINDS = ("text_plain", "text_demux", "file_plain", "file_demux")
TRACE = re.compile(r"\[f2q trace\] sample barcodes: .* table (\d+) slots, (\d+) entries, (\d+) ambiguous, (LDS|global)")


def library(n=10000, seed=0xF2A5):
    rng = np.random.default_rng(seed)
    rows = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (2 * n, LENGTH))]
    return sorted({r.tobytes().decode() for r in rows})[:n]


def barcodes(nb, seed=0xBC):
    """the first nb of one list of distinct 8-mers: the 96 are among the 384"""
    rng = np.random.default_rng(seed)
    rows = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (2048, BC[1]))]
    return list(dict.fromkeys(r.tobytes().decode() for r in rows))[:nb]


def make_reads(lib, n, first, seed=0xBEEF, length=150, p_sub=0.02, p_rand=0.1, p_lowq=0.004, p_n=0.005):
    """n reads of 150 bases, numbered from `first`: a feature at START, substitutions, random reads, low quality bytes and
    'N's anywhere; at BC one of the 96 barcodes (a subset of the 384), one base substituted in 10 %, a random window in 5 %"""
    rng = np.random.default_rng(seed + first)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    feats = np.array([list(f.encode()) for f in lib], np.uint8)
    bcs = np.array([list(b.encode()) for b in barcodes(96)], np.uint8)
    s = acgt[rng.integers(0, 4, (n, length))]
    seg = feats[rng.integers(0, len(lib), n)]
    sub = rng.random(seg.shape) < p_sub
    seg[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    planted = rng.random(n) >= p_rand
    s[planted, START:START + LENGTH] = seg[planted]
    w = bcs[rng.integers(0, len(bcs), n)]
    kind = rng.random(n)
    one = np.flatnonzero(kind < 0.10)
    w[one, rng.integers(0, BC[1], len(one))] = acgt[rng.integers(0, 4, len(one))]
    rand = kind >= 0.95
    w[rand] = acgt[rng.integers(0, 4, (int(rand.sum()), BC[1]))]
    s[:, BC[0]:BC[0] + BC[1]] = w
    s[rng.random(s.shape, dtype=np.float32) < p_n] = ord("N")
    q = np.full((n, length), ord("I"), np.uint8)
    low = rng.random(q.shape, dtype=np.float32) < p_lowq
    q[low] = np.frombuffer(b"!#+5:>?@", np.uint8)[rng.integers(0, 8, int(low.sum()))]
    head = np.frombuffer(b"".join(b"@r%08d" % (first + i) for i in range(n)), np.uint8).reshape(n, 10)
    nl = np.full((n, 1), 10, np.uint8)
    plus = np.tile(np.frombuffer(b"\n+\n", np.uint8), (n, 1))
    return np.concatenate([head, nl, s, plus, q, nl], axis=1).tobytes()


def one(kind, path, tree):
    """one context; the block (or the text) made once and counted REPS + 1 times, the first pass not reported; file kinds: the
    file streamed REPS times.  `tree`: the checkout whose package and library are used"""
    sys.path.insert(0, tree)
    extra, out = {}, dict(kind=kind)
    if kind.startswith("demux_"):
        _, nb, m, where = kind.split("_")
        os.environ["F2Q_DEMUX_TABLE"] = where
        os.environ["F2Q_TRACE"] = "1"
        extra = dict(sample_barcodes=(BC[0], barcodes(int(nb))), barcode_mismatch=int(m))
    elif kind.endswith("_demux"):
        extra = dict(sample_barcodes=(BC[0], barcodes(96)), barcode_mismatch=1)
    elif kind.startswith("general"):
        os.environ["F2Q_FORCE_GENERAL"] = "1"
    pkg = importlib.import_module("2fast2q_amd")
    with pkg.Counter(features=library(), miss=1, phred=30, length=LENGTH, start=str(START), **extra) as c:
        if kind.startswith("file_"):
            ms = []
            for rep in range(REPS):
                c.reset()
                t0 = time.perf_counter()
                c.count_file(path)
                ms.append((time.perf_counter() - t0) * 1e3)
            out.update(wall_ms=ms)
        elif kind.startswith("text_"):
            text = c.text_upload(open(path, "rb").read())
            ms = []
            for rep in range(REPS + 1):
                c.reset()
                t0 = time.perf_counter()
                c.count_text(text)
                c.read_counts()                                      # (waits for the stream)
                ms.append((time.perf_counter() - t0) * 1e3)
            text.free()
            out.update(wall_ms=ms[1:])
        else:
            blk = c.block_from_fastq(open(path, "rb").read())
            info = blk.info()
            assert info["n_general"] == info["n_reads"], info        # every read on the raw-record road
            ms = []
            for rep in range(REPS + 1):
                c.reset()
                ms.append(c.count_resident(blk)["kernel_ms"])
            blk.free()
            out.update(kernel_ms=ms[1:])
        counts, stats = c.read_counts()
        out.update(reads=int(stats[0]), assigned=int(stats[1] + stats[2]))
        if extra:
            matrix, sstats, verdicts = c.read_demux()
            assert (matrix.sum(axis=0) == counts).all() and (sstats.sum(axis=0) == stats).all() and verdicts.sum() == stats[0]
            out.update(verdicts=[int(v) for v in verdicts])
    print(json.dumps(out), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    out_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "profiles", "r14_demux_rates.txt")
    parent = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else None
    kinds = list(DEMUX_KINDS) + [k for k in GENERAL_KINDS if parent or k != "general_parent"] + list(INGEST_KINDS)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fastq")
        lib = library()
        with open(path, "wb") as h:
            for first in range(0, n, CHUNK):
                h.write(make_reads(lib, min(CHUNK, n - first), first))
        runs, tables = {}, {}
        for kind in kinds * 2:
            print(f"[demux_rates] {kind}", file=sys.stderr, flush=True)
            tree = parent if kind == "general_parent" else HERE
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, path, tree], capture_output=True, text=True, timeout=300)
            if done.returncode:                                      # nothing more is started after a failure
                sys.exit(f"{kind}: exit status {done.returncode}\n{done.stderr[-2000:]}")
            runs.setdefault(kind, []).append(json.loads(done.stdout.strip().splitlines()[-1]))
            m = TRACE.search(done.stderr)
            if m:
                tables[kind] = dict(slots=int(m.group(1)), entries=int(m.group(2)), ambiguous=int(m.group(3)), instance=m.group(4))
    row = dict(workload="reads_150_10k_m1_barcode8_at_20", reads=n, order_of_processes=kinds * 2)
    rate = lambda ms: n / ms / 1e6
    assert len({(runs[k][0]["reads"], runs[k][0]["assigned"]) for k in runs}) == 1           # every context decided the reads alike
    for kind in kinds:
        key = "wall_ms" if kind in INGEST_KINDS else "kernel_ms"
        best = min(min(r[key]) for r in runs[kind])
        row[kind] = {key: [r[key] for r in runs[kind]], "best_ms": best, "greads_s": rate(best), **tables.get(kind, {}),
                     **({"verdicts": runs[kind][0]["verdicts"]} if "verdicts" in runs[kind][0] else {})}
    for nb in (96, 384):
        for m in (0, 1):
            a, b = row[f"demux_{nb}_{m}_lds"], row[f"demux_{nb}_{m}_global"]
            assert a["verdicts"] == b["verdicts"]
            row[f"lds_to_global_{nb}_{m}"] = a["best_ms"] / b["best_ms"] if a["instance"] == "LDS" else None
    base = "general_parent" if parent else "general"
    ingest = row["text_plain"]["greads_s"]
    row.update(baseline=base,
               demux_to_general={k: row[k]["best_ms"] / row[base]["best_ms"] for k in DEMUX_KINDS},
               text_demux_to_text_plain=row["text_demux"]["best_ms"] / row["text_plain"]["best_ms"],
               file_demux_to_file_plain=row["file_demux"]["best_ms"] / row["file_plain"]["best_ms"],
               kernel_above_text_ingest={k: row[k]["greads_s"] > ingest for k in DEMUX_KINDS},
               kernel_above_file_ingest={k: row[k]["greads_s"] > row["file_plain"]["greads_s"] for k in DEMUX_KINDS})
    if parent:
        row.update(general_to_general_parent=row["general"]["best_ms"] / row["general_parent"]["best_ms"])
    with open(out_file, "w") as h:
        h.write(json.dumps(row) + "\n")
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        main()
