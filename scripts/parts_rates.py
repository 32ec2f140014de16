"""Cost of matching each part of a pair library alone (--parts; f2q_set_parts)
(python scripts/parts_rates.py [n_reads] [out_file] [parent_checkout]; out_file defaults to profiles/r16_parts_rates.txt):
one JSON line over a 10 k-feature combinatorial library of 10 + 10 bases (a quarter of the 200 x 200 pairs of two part
lists), --l 10 --m 1, about 20 % planted recombinants, 2 M records by default, in two shapes: single reads of 150 bases
with --st 0,20, and 2 x 150 pairs with --st 0 --st2 0 --rc2.
  (a) the block made once (f2q_block_from_fastq / _paired) and counted from there: the HIP-event time of
      k_count_parts<false> / k_count_parts<true>
  (b) k_count_general<false> / <true> on the same block, a plain context under F2Q_FORCE_GENERAL=1: this tree's, and -- when
      parent_checkout names a built checkout of the parent commit -- the parent's; the ratio (a) / (b)
  (c) f2q_count_text on the single-read text uploaded once, with and without the flag: wall time of the call -- the rate at
      which text already in device memory is ingested, which the kernel rate of (a) is compared with
  (d) f2q_count_file on the same text as a plain file, with and without the flag, later passes
Every figure comes from a process of its own (this file with --one) under a time limit, the kinds taking turns, twice, five
timed passes each (ten per kind); nothing more is started after a failure."""
import importlib, json, os, subprocess, sys, tempfile, time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
L, NP = 10, 200
CHUNK = 250_000
COMP = bytes.maketrans(b"ACGT", b"TGCA")
KERNEL_KINDS = ("parts_single", "parts_paired", "general_single", "general_paired")
PARENT_KINDS = ("general_parent_single", "general_parent_paired")
INGEST_KINDS = ("text_plain", "text_parts", "file_plain", "file_parts")


def parts(seed):
    rng = np.random.default_rng(seed)
    rows = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (4 * NP, L))]
    return list(dict.fromkeys(r.tobytes().decode() for r in rows))[:NP]


def library(n=10000, seed=0x9A27):
    """n of the NP x NP pairs of two part lists, in a random order: every part is shared by about n / NP features"""
    a, b = parts(seed), parts(seed + 1)
    rng = np.random.default_rng(seed + 2)
    picks = rng.permutation(NP * NP)
    assert n < NP * NP
    return [a[k // NP] + ":" + b[k % NP] for k in picks[:n]]


def make_reads(lib, n, first, paired, seed=0xBEEF, length=150, p_sub=0.02, p_rec=0.2, p_rand=0.08, p_lowq=0.004, p_n=0.005):
    """n records numbered from `first`: a library pair (or, in p_rec of them, two parts the library does not pair; in p_rand
    random windows) at 0 and 20 of a single read, or at 0 of either mate (mate 2 then written reverse-complemented);
    substitutions, low quality bytes and 'N's anywhere.  Returns (text 1, text 2 or None)"""
    rng = np.random.default_rng(seed + first)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    held = set(lib)
    pa, pb = parts(0x9A27), parts(0x9A28)
    A = np.array([list(p.encode()) for p in pa], np.uint8)
    B = np.array([list(p.encode()) for p in pb], np.uint8)
    ia = np.array([pa.index(f.split(":")[0]) for f in lib])
    ib = np.array([pb.index(f.split(":")[1]) for f in lib])
    pick = rng.integers(0, len(lib), n)
    i1, i2 = ia[pick], ib[pick]
    kind = rng.random(n)
    rec = np.flatnonzero(kind < p_rec)
    for k in rec:                                                # a pair of parts the library does not hold
        while True:
            x, y = int(rng.integers(0, NP)), int(rng.integers(0, NP))
            if pa[x] + ":" + pb[y] not in held:
                i1[k], i2[k] = x, y
                break
    out = []
    texts = [[(A[i1], 0)], [(B[i2], 0)]] if paired else [[(A[i1], 0), (B[i2], 20)]]      # per text: (window bytes, position)
    rand = kind >= 1.0 - p_rand
    for mate, ws in enumerate(texts):
        s = acgt[rng.integers(0, 4, (n, length))]
        for seg, at in ws:
            seg = seg.copy()
            sub = rng.random(seg.shape) < p_sub
            seg[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
            s[~rand, at:at + L] = seg[~rand]
        s[rng.random(s.shape, dtype=np.float32) < p_n] = ord("N")
        q = np.full((n, length), ord("I"), np.uint8)
        low = rng.random(q.shape, dtype=np.float32) < p_lowq
        q[low] = np.frombuffer(b"!#+5:>?@", np.uint8)[rng.integers(0, 8, int(low.sum()))]
        if mate == 1:                                            # mate 2 as the sequencer wrote it: --rc2 takes it back
            s = np.frombuffer(s.tobytes().translate(COMP), np.uint8).reshape(s.shape)[:, ::-1]
            q = q[:, ::-1]
        head = np.frombuffer(b"".join(b"@%c%08d" % (b"ab"[mate], first + i) for i in range(n)), np.uint8).reshape(n, 10)
        nl = np.full((n, 1), 10, np.uint8)
        plus = np.tile(np.frombuffer(b"\n+\n", np.uint8), (n, 1))
        out.append(np.concatenate([head, nl, s, plus, q, nl], axis=1).tobytes())
    return out[0], (out[1] if paired else None)


def one(kind, path, tree):
    """one context; the block (or the text) made once and counted REPS + 1 times, the first pass not reported; file kinds: the
    file streamed REPS + 1 times, the first pass not reported.  `tree`: the checkout whose package and library are used"""
    sys.path.insert(0, tree)
    out = dict(kind=kind)
    paired = kind.endswith("_paired")
    with_parts = kind.startswith("parts_") or kind.endswith("_parts")
    if kind.startswith("general"):
        os.environ["F2Q_FORCE_GENERAL"] = "1"
    pkg = importlib.import_module("2fast2q_amd")
    run = dict(start="0", start2="0", rc2=True) if paired else dict(start="0,20")
    extra = dict(parts=True) if with_parts else {}
    with pkg.Counter(features=library(), miss=1, phred=30, length=L, **run, **extra) as c:
        if kind.startswith("file_"):
            ms = []
            for rep in range(REPS + 1):
                c.reset()
                t0 = time.perf_counter()
                c.count_file(path + ".single")
                ms.append((time.perf_counter() - t0) * 1e3)
            out.update(wall_ms=ms[1:])
        elif kind.startswith("text_"):
            text = c.text_upload(open(path + ".single", "rb").read())
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
            if paired:
                blk = c.block_from_fastq_paired(open(path + ".r1", "rb").read(), open(path + ".r2", "rb").read())
            else:
                blk = c.block_from_fastq(open(path + ".single", "rb").read())
            info = blk.info()
            assert info["n_general"] == info["n_reads"], info        # every record on the raw-record road
            ms = []
            for rep in range(REPS + 1):
                c.reset()
                ms.append(c.count_resident(blk)["kernel_ms"])
            blk.free()
            out.update(kernel_ms=ms[1:])
        counts, stats = c.read_counts()
        out.update(reads=int(stats[0]), assigned=int(stats[1] + stats[2]))
        if with_parts:
            pc, m1, m2, cls = c.read_parts()
            i1, i2, reads = c.parts_recombinants()
            assert cls.sum() == stats[0] and pc.sum() == cls[0] + cls[1] and int(reads.sum()) == cls[2]
            out.update(classes=[int(v) for v in cls], recombinant_pairs=int(len(reads)))
    print(json.dumps(out), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    out_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "profiles", "r16_parts_rates.txt")
    parent = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else None
    kinds = list(KERNEL_KINDS) + (list(PARENT_KINDS) if parent else []) + list(INGEST_KINDS)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fastq")
        lib = library()
        with open(path + ".single", "wb") as hs, open(path + ".r1", "wb") as h1, open(path + ".r2", "wb") as h2:
            for first in range(0, n, CHUNK):
                hs.write(make_reads(lib, min(CHUNK, n - first), first, False)[0])
                a, b = make_reads(lib, min(CHUNK, n - first), first, True)
                h1.write(a); h2.write(b)
        runs = {}
        for kind in kinds * 2:
            print(f"[parts_rates] {kind}", file=sys.stderr, flush=True)
            tree = parent if kind in PARENT_KINDS else HERE
            one_kind = kind.replace("_parent", "")
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", one_kind, path, tree], capture_output=True, text=True, timeout=300)
            if done.returncode:                                      # nothing more is started after a failure
                sys.exit(f"{kind}: exit status {done.returncode}\n{done.stderr[-2000:]}")
            runs.setdefault(kind, []).append(json.loads(done.stdout.strip().splitlines()[-1]))
    row = dict(workload="150_bases_10k_pairs_of_200x200_parts_l10_m1_20pct_recombinants", reads=n, order_of_processes=kinds * 2)
    rate = lambda ms: n / ms / 1e6
    for shape in ("single", "paired"):                               # every context decided the records alike by the joined rule
        assert len({(runs[k][0]["reads"], runs[k][0]["assigned"]) for k in runs if k.endswith(shape)}) == 1
    for kind in kinds:
        key = "wall_ms" if kind in INGEST_KINDS else "kernel_ms"
        best = min(min(r[key]) for r in runs[kind])
        row[kind] = {key: [r[key] for r in runs[kind]], "best_ms": best, "greads_s": rate(best),
                     **({"classes": runs[kind][0]["classes"], "recombinant_pairs": runs[kind][0]["recombinant_pairs"]} if "classes" in runs[kind][0] else {})}
    base = "general_parent_" if parent else "general_"
    ingest = row["text_plain"]["greads_s"]
    row.update(baseline=base.rstrip("_"),
               parts_to_general={s: row["parts_" + s]["best_ms"] / row[base + s]["best_ms"] for s in ("single", "paired")},
               text_parts_to_text_plain=row["text_parts"]["best_ms"] / row["text_plain"]["best_ms"],
               file_parts_to_file_plain=row["file_parts"]["best_ms"] / row["file_plain"]["best_ms"],
               kernel_above_text_ingest={s: row["parts_" + s]["greads_s"] > ingest for s in ("single", "paired")},
               kernel_above_file_ingest={s: row["parts_" + s]["greads_s"] > row["file_plain"]["greads_s"] for s in ("single", "paired")})
    if parent:
        row.update(general_to_general_parent={s: row["general_" + s]["best_ms"] / row["general_parent_" + s]["best_ms"] for s in ("single", "paired")})
    with open(out_file, "w") as h:
        h.write(json.dumps(row) + "\n")
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        main()
