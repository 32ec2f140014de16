"""Cost of counting reads of either orientation (--strand; f2q_set_strand)
(python scripts/strand_rates.py [n_reads] [out_file] [parent_checkout]; out_file defaults to profiles/r15_strand_rates.txt):
one JSON line over 150-base reads (10 k features of 20 bases, --st 0 --l 20 --m 1), 2 M reads by default, as three texts:
every read as made ("forward"), every read mirrored ("mirrored": reverse-complemented, the quality line reversed), and every
second read mirrored ("mixed").
  (a) the block made once (f2q_block_from_fastq) and counted from there: the HIP-event time of k_count_strand<true> (both)
      on the forward, the mixed and the mirrored block, and of k_count_strand<false> (rev) on the mirrored block
  (b) k_count_general<false> on the forward block, a plain context under F2Q_FORCE_GENERAL=1: this tree's, and -- when
      parent_checkout names a built checkout of the parent commit -- the parent's
  (c) f2q_count_text on the forward text uploaded once (a plain context), and f2q_count_file on the mixed text as a plain
      file with and without --strand both: wall time of the call
Every figure comes from a process of its own (this file with --one) under a time limit, the kinds taking turns, twice;
nothing more is started after a failure."""
import importlib, json, os, subprocess, sys, tempfile, time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
START, LENGTH = 0, 20
CHUNK = 250_000
# kind -> (text, strand mode)
STRAND_KINDS = {"both_forward": ("forward", "both"), "both_mixed": ("mixed", "both"), "both_mirrored": ("mirrored", "both"), "rev_mirrored": ("mirrored", "rev")}
GENERAL_KINDS = ("general", "general_parent")
INGEST_KINDS = {"text_plain": ("forward", "fwd"), "file_plain": ("mixed", "fwd"), "file_both": ("mixed", "both")}
COMP = np.arange(256, dtype=np.uint8)
COMP[list(b"ACGTacgt")] = list(b"TGCAtgca")


def library(n=10000, seed=0xF2A5):
    rng = np.random.default_rng(seed)
    rows = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (2 * n, LENGTH))]
    return sorted({r.tobytes().decode() for r in rows})[:n]


def make_reads(lib, n, first, which, seed=0xBEEF, length=150, p_sub=0.02, p_rand=0.1, p_lowq=0.004, p_n=0.005):
    """n reads of 150 bases, numbered from `first`: a feature at START, substitutions, random reads, low quality bytes and
    'N's anywhere; which = "forward" / "mirrored" / "mixed" (the odd-numbered reads mirrored) -- the same reads in all three"""
    rng = np.random.default_rng(seed + first)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    feats = np.array([list(f.encode()) for f in lib], np.uint8)
    s = acgt[rng.integers(0, 4, (n, length))]
    seg = feats[rng.integers(0, len(lib), n)]
    sub = rng.random(seg.shape) < p_sub
    seg[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    planted = rng.random(n) >= p_rand
    s[planted, START:START + LENGTH] = seg[planted]
    s[rng.random(s.shape, dtype=np.float32) < p_n] = ord("N")
    q = np.full((n, length), ord("I"), np.uint8)
    low = rng.random(q.shape, dtype=np.float32) < p_lowq
    q[low] = np.frombuffer(b"!#+5:>?@", np.uint8)[rng.integers(0, 8, int(low.sum()))]
    flip = np.zeros(n, bool) if which == "forward" else np.ones(n, bool) if which == "mirrored" else (first + np.arange(n)) % 2 == 1
    s[flip] = COMP[s[flip][:, ::-1]]
    q[flip] = q[flip][:, ::-1]
    head = np.frombuffer(b"".join(b"@r%08d" % (first + i) for i in range(n)), np.uint8).reshape(n, 10)
    nl = np.full((n, 1), 10, np.uint8)
    plus = np.tile(np.frombuffer(b"\n+\n", np.uint8), (n, 1))
    return np.concatenate([head, nl, s, plus, q, nl], axis=1).tobytes()


def one(kind, path, tree):
    """one context; the block (or the text) made once and counted REPS + 1 times, the first pass not reported; file kinds: the
    file streamed REPS times.  `tree`: the checkout whose package and library are used"""
    sys.path.insert(0, tree)
    extra, out = {}, dict(kind=kind)
    mode = dict(STRAND_KINDS, **INGEST_KINDS).get(kind, (None, "fwd"))[1]
    if mode != "fwd":
        extra = dict(strand=mode)
    if kind.startswith("general"):
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
            rev, ext = c.read_strands()
            assert rev.sum() == ext[1] + ext[2] and ext[:3].sum() == stats[1] + stats[2] and (rev <= counts).all()
            out.update(strands=[int(v) for v in ext])
    print(json.dumps(out), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    out_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "profiles", "r15_strand_rates.txt")
    parent = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else None
    kinds = list(STRAND_KINDS) + [k for k in GENERAL_KINDS if parent or k != "general_parent"] + list(INGEST_KINDS)
    with tempfile.TemporaryDirectory() as tmp:
        lib = library()
        paths = {which: os.path.join(tmp, which + ".fastq") for which in ("forward", "mirrored", "mixed")}
        for which, path in paths.items():
            with open(path, "wb") as h:
                for first in range(0, n, CHUNK):
                    h.write(make_reads(lib, min(CHUNK, n - first), first, which))
        runs = {}
        for kind in kinds * 2:
            print(f"[strand_rates] {kind}", file=sys.stderr, flush=True)
            tree = parent if kind == "general_parent" else HERE
            path = paths[dict(STRAND_KINDS, **INGEST_KINDS).get(kind, ("forward",))[0]]
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, path, tree], capture_output=True, text=True, timeout=300)
            if done.returncode:                                      # nothing more is started after a failure
                sys.exit(f"{kind}: exit status {done.returncode}\n{done.stderr[-2000:]}")
            runs.setdefault(kind, []).append(json.loads(done.stdout.strip().splitlines()[-1]))
    row = dict(workload="reads_150_10k_m1_st0", reads=n, order_of_processes=kinds * 2)
    rate = lambda ms: n / ms / 1e6
    # the same reads whichever way round they lie: every strand context assigns what the plain context assigns on the forward
    # text, but for the few random windows that happen to lie within one base of a feature on the other strand
    assigned = [runs[k][0]["assigned"] for k in runs if k != "file_plain"]
    assert {runs[k][0]["reads"] for k in runs} == {n} and max(assigned) - min(assigned) <= 20, {k: runs[k][0] for k in runs}
    for kind in kinds:
        key = "wall_ms" if kind in INGEST_KINDS else "kernel_ms"
        best = min(min(r[key]) for r in runs[kind])
        row[kind] = {key: [r[key] for r in runs[kind]], "best_ms": best, "greads_s": rate(best),
                     **({"strands": runs[kind][0]["strands"]} if "strands" in runs[kind][0] else {})}
    base = "general_parent" if parent else "general"
    ingest = row["text_plain"]["greads_s"]
    row.update(baseline=base,
               strand_to_general={k: row[k]["best_ms"] / row[base]["best_ms"] for k in STRAND_KINDS},
               file_both_to_file_plain=row["file_both"]["best_ms"] / row["file_plain"]["best_ms"],
               kernel_above_text_ingest={k: row[k]["greads_s"] > ingest for k in STRAND_KINDS},
               kernel_above_file_ingest={k: row[k]["greads_s"] > row["file_plain"]["greads_s"] for k in STRAND_KINDS})
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
