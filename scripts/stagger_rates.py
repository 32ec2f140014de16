"""Cost of trying one fixed window at a range of starts (--stagger; f2q_set_stagger)
(python scripts/stagger_rates.py [n_reads] [out_file] [parent_checkout]; out_file defaults to profiles/r17_stagger_rates.txt):
one JSON line over 150-base reads (10 k features of 20 bases, --st 12 --l 20 --m 1), 2 M reads by default, as two texts: the
feature at offset i % 9 behind a 12-base flank ("staggered"), and the same reads with every feature at offset 0 ("at0").
  (a) the staggered block made once (f2q_block_from_fastq) and counted from there: the HIP-event time of k_count_stagger at
      N = 8 and N = 32, in the span layout and under F2Q_STAGGER_WALK=1
  (b) k_count_general<false> on the at0 block, a plain context under F2Q_FORCE_GENERAL=1: this tree's, and -- when
      parent_checkout names a built checkout of the parent commit -- the parent's (the baseline)
  (c) the anchored tile path on the staggered block: --us with the 12-base flank, today's way to count such a sample
  (d) f2q_count_text on the texts uploaded once (a plain context on at0; N = 8 and N = 32 on staggered), and f2q_count_file
      on the staggered text as a plain file with and without --stagger 8: wall time of the call
Every figure comes from a process of its own (this file with --one) under a time limit, the kinds taking turns, twice;
nothing more is started after a failure."""
import importlib, json, os, subprocess, sys, tempfile, time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
START, LENGTH = 12, 20
FLANK = b"GTTTAAGAGCTA"
CHUNK = 250_000
# kind -> (text, N, walk layout)
STAGGER_KINDS = {"stagger8_span": ("staggered", 8, False), "stagger8_walk": ("staggered", 8, True),
                 "stagger32_span": ("staggered", 32, False), "stagger32_walk": ("staggered", 32, True)}
GENERAL_KINDS = ("general", "general_parent")
INGEST_KINDS = {"text_plain": ("at0", 0, False), "text_stagger8": ("staggered", 8, False), "text_stagger32": ("staggered", 32, False),
                "file_plain": ("staggered", 0, False), "file_stagger8": ("staggered", 8, False)}
ALL = dict(STAGGER_KINDS, **INGEST_KINDS, anchored=("staggered", 0, False), general=("at0", 0, False), general_parent=("at0", 0, False))


def library(n=10000, seed=0xF2A5):
    rng = np.random.default_rng(seed)
    rows = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (2 * n, LENGTH))]
    return sorted({r.tobytes().decode() for r in rows})[:n]


def make_reads(lib, n, first, which, seed=0xBEEF, length=150, p_sub=0.02, p_rand=0.1, p_lowq=0.004, p_n=0.005):
    """n reads of 150 bases, numbered from `first`: the flank and a feature behind it at offset (read number) % 9 -- "at0": at
    offset 0 --, substitutions, random reads, low quality bytes and 'N's anywhere; the same reads in both texts"""
    rng = np.random.default_rng(seed + first)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    feats = np.array([list(f.encode()) for f in lib], np.uint8)
    s = acgt[rng.integers(0, 4, (n, length))]
    seg = feats[rng.integers(0, len(lib), n)]
    sub = rng.random(seg.shape) < p_sub
    seg[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    planted = rng.random(n) >= p_rand
    offs = (first + np.arange(n)) % 9 if which == "staggered" else np.zeros(n, np.int64)
    body = np.concatenate([np.tile(np.frombuffer(FLANK, np.uint8), (n, 1)), seg], axis=1)
    for d in range(9):
        rows = planted & (offs == d)
        s[rows, d:d + len(FLANK) + LENGTH] = body[rows]
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
    _, n, walk = ALL[kind]
    if walk:
        os.environ["F2Q_STAGGER_WALK"] = "1"
    if kind.startswith("general"):
        os.environ["F2Q_FORCE_GENERAL"] = "1"
    pkg = importlib.import_module("2fast2q_amd")
    run = dict(upstream=FLANK.decode(), length=LENGTH) if kind == "anchored" else dict(start=str(START), length=LENGTH)
    with pkg.Counter(features=library(), miss=1, phred=30, **run, **(dict(stagger=n) if n else {})) as c:
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
            assert kind == "anchored" or info["n_general"] == info["n_reads"], info      # every read on the raw-record road
            ms = []
            for rep in range(REPS + 1):
                c.reset()
                ms.append(c.count_resident(blk)["kernel_ms"])
            out.update(kernel_ms=ms[1:], n_general=int(info["n_general"]))
            blk.free()
        counts, stats = c.read_counts()
        out.update(reads=int(stats[0]), assigned=int(stats[1] + stats[2]))
        if n:
            perfect, imperfect = c.read_stagger()
            assert perfect.sum() == stats[1] and imperfect.sum() == stats[2]
            out.update(perfect=[int(v) for v in perfect], imperfect=[int(v) for v in imperfect])
    print(json.dumps(out), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    out_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "profiles", "r17_stagger_rates.txt")
    parent = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else None
    kinds = list(STAGGER_KINDS) + [k for k in GENERAL_KINDS if parent or k != "general_parent"] + ["anchored"] + list(INGEST_KINDS)
    with tempfile.TemporaryDirectory() as tmp:
        lib = library()
        paths = {which: os.path.join(tmp, which + ".fastq") for which in ("staggered", "at0")}
        for which, path in paths.items():
            with open(path, "wb") as h:
                for first in range(0, n, CHUNK):
                    h.write(make_reads(lib, min(CHUNK, n - first), first, which))
        runs = {}
        for kind in kinds * 2:
            print(f"[stagger_rates] {kind}", file=sys.stderr, flush=True)
            tree = parent if kind == "general_parent" else HERE
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, paths[ALL[kind][0]], tree], capture_output=True, text=True, timeout=300)
            if done.returncode:                                      # nothing more is started after a failure
                sys.exit(f"{kind}: exit status {done.returncode}\n{done.stderr[-2000:]}")
            runs.setdefault(kind, []).append(json.loads(done.stdout.strip().splitlines()[-1]))
    row = dict(workload="reads_150_10k_m1_st12_offsets_0_8", reads=n, order_of_processes=kinds * 2)
    rate = lambda ms: n / ms / 1e6
    # the same reads wherever their feature lies: a stagger context on the staggered text assigns what the plain context assigns
    # on the at0 text, but for the few windows that happen to lie within one base of a feature at another start
    assert {runs[k][0]["reads"] for k in runs} == {n}, {k: runs[k][0] for k in runs}
    at0 = runs["general"][0]["assigned"]
    for k in STAGGER_KINDS:
        assert abs(runs[k][0]["assigned"] - at0) <= n // 1000, (k, runs[k][0]["assigned"], at0)
    assert runs["stagger8_span"][0]["perfect"] == runs["stagger8_walk"][0]["perfect"] and runs["stagger32_span"][0]["imperfect"] == runs["stagger32_walk"][0]["imperfect"]
    for kind in kinds:
        key = "wall_ms" if kind in INGEST_KINDS else "kernel_ms"
        best = min(min(r[key]) for r in runs[kind])
        row[kind] = {key: [r[key] for r in runs[kind]], "best_ms": best, "greads_s": rate(best), "assigned": runs[kind][0]["assigned"],
                     **({"perfect": runs[kind][0]["perfect"], "imperfect": runs[kind][0]["imperfect"]} if "perfect" in runs[kind][0] else {})}
    base = "general_parent" if parent else "general"
    row.update(baseline=base,
               stagger_to_general={k: row[k]["best_ms"] / row[base]["best_ms"] for k in STAGGER_KINDS},
               span_to_walk={n_: row[f"stagger{n_}_span"]["best_ms"] / row[f"stagger{n_}_walk"]["best_ms"] for n_ in (8, 32)},
               stagger_to_anchored={k: row[k]["best_ms"] / row["anchored"]["best_ms"] for k in STAGGER_KINDS},
               file_stagger8_to_file_plain=row["file_stagger8"]["best_ms"] / row["file_plain"]["best_ms"],
               kernel_above_text_ingest_of_the_same_run={"stagger8_span": row["stagger8_span"]["greads_s"] > row["text_stagger8"]["greads_s"],
                                                         "stagger32_span": row["stagger32_span"]["greads_s"] > row["text_stagger32"]["greads_s"]},
               kernel_above_plain_text_ingest={k: row[k]["greads_s"] > row["text_plain"]["greads_s"] for k in STAGGER_KINDS})
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
