"""Cost of reporting one-base insertions and deletions (--indel; f2q_set_indel)
(python scripts/indel_rates.py [n_reads] [out_file] [parent_checkout]; out_file defaults to profiles/r18_indel_rates.txt):
one JSON line over 150-base reads (10 k features of 20 bases, --st 12 --l 20 --m 1), 2 M reads by default, as three texts of
the same reads: "none" (no read edited), "five" and "twenty" (about 5 % / 20 % of the reads with one base of their feature
deleted or one base inserted into it, half and half).
  (a) each text's block made once (f2q_block_from_fastq) and counted from there: the HIP-event time of k_count_indel
  (b) k_count_general<false> on the same blocks, a plain context under F2Q_FORCE_GENERAL=1: this tree's, and -- when
      parent_checkout names a built checkout of the parent commit -- the parent's (the yardstick)
  (c) f2q_count_text on the texts uploaded once, with and without the flag, and f2q_count_file on the "five" text as a plain
      file with and without it: wall time of the call
  (d) the size of the deletion-variant table, as F2Q_TRACE=1 prints it
Every figure comes from a process of its own (this file with --one) under a time limit, the kinds taking turns, twice;
nothing more is started after a failure."""
import importlib, json, os, re, subprocess, sys, tempfile, time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
START, LENGTH = 12, 20
CHUNK = 250_000
TEXTS = {"none": 0.0, "five": 0.05, "twenty": 0.20}
# kind -> (text, the flag)
INDEL_KINDS = {f"indel_{t}": (t, True) for t in TEXTS}
GENERAL_KINDS = {f"general_{t}": (t, False) for t in TEXTS}
PARENT_KINDS = {f"general_parent_{t}": (t, False) for t in TEXTS}
INGEST_KINDS = dict([(f"text_plain_{t}", (t, False)) for t in TEXTS] + [(f"text_indel_{t}", (t, True)) for t in TEXTS] +
                    [("file_plain", ("five", False)), ("file_indel", ("five", True))])
ALL = dict(INDEL_KINDS, **GENERAL_KINDS, **PARENT_KINDS, **INGEST_KINDS, table=("none", True))


def library(n=10000, seed=0xF2A5):
    rng = np.random.default_rng(seed)
    rows = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (2 * n, LENGTH))]
    return sorted({r.tobytes().decode() for r in rows})[:n]


def make_reads(lib, n, first, share, seed=0xBEEF, length=150, p_sub=0.02, p_rand=0.1, p_lowq=0.004, p_n=0.005):
    """n reads of 150 bases, numbered from `first`: a feature at --st 12, substitutions, random reads, low quality bytes and
    'N's anywhere; then `share` of the reads lose one base of the feature or gain one inside it (the bases behind move; the
    line keeps its length).  The same reads in every text: the edit is drawn from a generator of its own"""
    rng = np.random.default_rng(seed + first)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    feats = np.array([list(f.encode()) for f in lib], np.uint8)
    s = acgt[rng.integers(0, 4, (n, length))]
    seg = feats[rng.integers(0, len(lib), n)]
    sub = rng.random(seg.shape) < p_sub
    seg[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    planted = rng.random(n) >= p_rand
    s[planted, START:START + LENGTH] = seg[planted]
    edit = np.random.default_rng(seed + first + 1)
    roll, pos, extra = edit.random(n), edit.integers(0, LENGTH, n), acgt[edit.integers(0, 4, n)]
    for i in np.nonzero(roll < share)[0]:
        at = START + int(pos[i])
        if roll[i] < share / 2:                                      # a deletion: the bases behind move up, a fresh one ends the line
            s[i, at:-1] = s[i, at + 1:].copy()
            s[i, -1] = extra[i]
        else:                                                        # an insertion: the bases behind move down, the last one leaves
            s[i, at + 1:] = s[i, at:-1].copy()
            s[i, at] = extra[i]
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
    out = dict(kind=kind)
    _, flag = ALL[kind]
    if kind.startswith("general"):
        os.environ["F2Q_FORCE_GENERAL"] = "1"
    pkg = importlib.import_module("2fast2q_amd")
    with pkg.Counter(features=library(), miss=1, phred=30, start=str(START), length=LENGTH, **(dict(indel=True) if flag else {})) as c:
        if kind == "table":                                          # (F2Q_TRACE=1 set by the caller: the line is on stderr by now)
            print(json.dumps(out), flush=True)
            return
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
            out.update(kernel_ms=ms[1:], n_general=int(info["n_general"]))
            blk.free()
        counts, stats = c.read_counts()
        out.update(reads=int(stats[0]), assigned=int(stats[1] + stats[2]), unassigned=int(stats[3] + stats[4]))
        if flag:
            dels, inss, del_pos, ins_pos, totals = c.read_indels()
            assert dels.sum() == del_pos.sum() == totals[1] and inss.sum() == ins_pos.sum() == totals[2] and totals[0] == stats[3] + stats[4]
            out.update(totals=[int(v) for v in totals])
    print(json.dumps(out), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    out_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "profiles", "r18_indel_rates.txt")
    parent = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else None
    kinds = list(INDEL_KINDS) + list(GENERAL_KINDS) + (list(PARENT_KINDS) if parent else []) + list(INGEST_KINDS)
    with tempfile.TemporaryDirectory() as tmp:
        lib = library()
        paths = {which: os.path.join(tmp, which + ".fastq") for which in TEXTS}
        for which, path in paths.items():
            with open(path, "wb") as h:
                for first in range(0, n, CHUNK):
                    h.write(make_reads(lib, min(CHUNK, n - first), first, TEXTS[which]))
        said = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "table", paths["none"], HERE], capture_output=True, text=True, timeout=300,
                              env=dict(os.environ, F2Q_TRACE="1"))
        if said.returncode:
            sys.exit(f"table: exit status {said.returncode}\n{said.stderr[-2000:]}")
        table = re.search(r"deletion-variant table (\d+) slots \((\d+) variants of (\d+) candidates, (\d+) shared\)", said.stderr)
        runs = {}
        for kind in kinds * 2:
            print(f"[indel_rates] {kind}", file=sys.stderr, flush=True)
            tree = parent if kind in PARENT_KINDS else HERE
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, paths[ALL[kind][0]], tree], capture_output=True, text=True, timeout=300)
            if done.returncode:                                      # nothing more is started after a failure
                sys.exit(f"{kind}: exit status {done.returncode}\n{done.stderr[-2000:]}")
            runs.setdefault(kind, []).append(json.loads(done.stdout.strip().splitlines()[-1]))
    slots, variants, candidates, shared = (int(x) for x in table.groups())
    row = dict(workload="reads_150_10k_m1_st12_indel_0_5_20_percent", reads=n, order_of_processes=kinds * 2,
               variant_table=dict(slots=slots, bytes=16 * slots, variants=variants, candidates=candidates, shared=shared))
    rate = lambda ms: n / ms / 1e6
    assert {runs[k][0]["reads"] for k in runs} == {n}, {k: runs[k][0] for k in runs}
    for t in TEXTS:                                                  # the flag changes no count
        assert runs[f"indel_{t}"][0]["assigned"] == runs[f"general_{t}"][0]["assigned"] == runs[f"text_plain_{t}"][0]["assigned"], t
        assert runs[f"indel_{t}"][0]["totals"] == runs[f"text_indel_{t}"][0]["totals"], t
    for kind in kinds:
        key = "wall_ms" if kind in INGEST_KINDS else "kernel_ms"
        best = min(min(r[key]) for r in runs[kind])
        row[kind] = {key: [r[key] for r in runs[kind]], "best_ms": best, "greads_s": rate(best), "assigned": runs[kind][0]["assigned"],
                     "unassigned": runs[kind][0]["unassigned"], **({"totals": runs[kind][0]["totals"]} if "totals" in runs[kind][0] else {})}
    base = "general_parent_" if parent else "general_"
    row.update(baseline=base + "<text>",
               indel_to_general={t: row[f"indel_{t}"]["best_ms"] / row[base + t]["best_ms"] for t in TEXTS},
               text_indel_to_text_plain={t: row[f"text_indel_{t}"]["best_ms"] / row[f"text_plain_{t}"]["best_ms"] for t in TEXTS},
               file_indel_to_file_plain=row["file_indel"]["best_ms"] / row["file_plain"]["best_ms"],
               kernel_above_text_ingest_of_the_same_run={t: row[f"indel_{t}"]["greads_s"] > row[f"text_indel_{t}"]["greads_s"] for t in TEXTS},
               kernel_above_plain_text_ingest={t: row[f"indel_{t}"]["greads_s"] > row[f"text_plain_{t}"]["greads_s"] for t in TEXTS},
               kernel_above_file_ingest=row["indel_five"]["greads_s"] > row["file_indel"]["greads_s"])
    if parent:
        row.update(general_to_general_parent={t: row[f"general_{t}"]["best_ms"] / row[f"general_parent_{t}"]["best_ms"] for t in TEXTS})
    with open(out_file, "w") as h:
        h.write(json.dumps(row) + "\n")
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        main()
