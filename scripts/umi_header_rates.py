"""Cost of UMIs in read headers (--umih; f2q_set_umi_header)
(python scripts/umi_header_rates.py [n_reads] [out_file] [parent_checkout]; out_file defaults to
profiles/r13_umi_header_rates.txt): one JSON line over 150-base reads whose 8-base UMI stands both in the header
(@r<number>_<UMI>) and at [20, 28) of the read (10 k features of 20 bases, --st 0 --l 20 --m 1), 2 M reads by default.
  (a) the text uploaded once (f2q_text_upload) and counted from there on a header context (F2Q_TRACE=1: the HIP-event
      times of k_classify, k_header_umi and k_pack of every pass over the same text) -- k_header_umi next to k_classify +
      k_pack -- and the HIP-event time of the counting kernel, k_count_umi<false, true>
  (b) the same on an inline context (--umi 20,8): k_count_umi<false>, the instance with the decode, on the same block
  (c) f2q_count_file on that text as a plain file with --umih, with --umi 20,8, and -- when parent_checkout names a built
      checkout of the parent commit -- with the parent's --umi 20,8
Every figure comes from a process of its own (this file with --one) under a time limit, the kinds taking turns, twice;
nothing more is started after a failure."""
import importlib, json, os, re, subprocess, sys, tempfile, time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
START, LENGTH, UMI = 0, 20, (20, 8)
SEP = "_"
KINDS = ("header", "inline")
FILE_KINDS = ("file_header", "file_inline", "file_parent_inline")
CHUNK = 250_000
TRACE = re.compile(r"\[f2q trace\] ingest kernels: (\d+) records, k_classify ([\d.]+) ms, k_header_umi ([\d.]+) ms, k_pack ([\d.]+) ms")


def library(n=10000, seed=0xF2A5):
    rng = np.random.default_rng(seed)
    rows = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (2 * n, LENGTH))]
    return sorted({r.tobytes().decode() for r in rows})[:n]


def make_reads(lib, n, first, seed=0xBEEF, length=150, p_sub=0.02, p_rand=0.1, p_lowq=0.004, p_n=0.005, pool=64):
    """n reads of 150 bases, numbered from `first`: a feature at START, substitutions, random reads, low quality bytes and
    'N's anywhere; one of `pool` UMIs at UMI of the read (quality 'I' there, so both sources are valid alike unless an 'N'
    fell on it) and the same eight bytes behind the '_' of the header"""
    rng = np.random.default_rng(seed + first)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    feats = np.array([list(f.encode()) for f in lib], np.uint8)
    umis = acgt[np.random.default_rng(seed).integers(0, 4, (pool, UMI[1]))]
    s = acgt[rng.integers(0, 4, (n, length))]
    seg = feats[rng.integers(0, len(lib), n)]
    sub = rng.random(seg.shape) < p_sub
    seg[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    planted = rng.random(n) >= p_rand
    s[planted, START:START + LENGTH] = seg[planted]
    s[:, UMI[0]:UMI[0] + UMI[1]] = umis[rng.integers(0, pool, n)]
    s[rng.random(s.shape, dtype=np.float32) < p_n] = ord("N")
    q = np.full((n, length), ord("I"), np.uint8)
    low = rng.random(q.shape, dtype=np.float32) < p_lowq
    q[low] = np.frombuffer(b"!#+5:>?@", np.uint8)[rng.integers(0, 8, int(low.sum()))]
    q[:, UMI[0]:UMI[0] + UMI[1]] = ord("I")
    head = np.frombuffer(b"".join(b"@r%08d_" % (first + i) for i in range(n)), np.uint8).reshape(n, 11)
    nl = np.full((n, 1), 10, np.uint8)
    plus = np.tile(np.frombuffer(b"\n+\n", np.uint8), (n, 1))
    return np.concatenate([head, s[:, UMI[0]:UMI[0] + UMI[1]], nl, s, plus, q, nl], axis=1).tobytes()


def one(kind, path, tree):
    """the text uploaded once and counted REPS + 1 times (the first pass sizes the set and is not reported); file kinds: the
    file streamed REPS times instead.  `tree`: the checkout whose package and library are used"""
    sys.path.insert(0, tree)
    if not kind.startswith("file_"):                                 # (the trace waits for the stream here and there: not on the file runs)
        os.environ["F2Q_TRACE"] = "1"
    pkg = importlib.import_module("2fast2q_amd")
    lib = library()
    source = dict(umi_header=(SEP, UMI[1])) if kind.endswith("header") else dict(umi=UMI)
    out = dict(kind=kind)
    with pkg.Counter(features=lib, miss=1, phred=30, length=LENGTH, start=str(START), **source) as c:
        if kind.startswith("file_"):
            ms = []
            for rep in range(REPS):
                c.reset()
                t0 = time.perf_counter()
                c.count_file(path)
                ms.append((time.perf_counter() - t0) * 1e3)
            out.update(file_wall_ms=ms)
        else:
            text = c.text_upload(open(path, "rb").read())
            ms = []
            for rep in range(REPS + 1):
                c.reset()
                ms.append(c.count_text(text, want_timing=True)[1]["kernel_ms"])
            text.free()
            out.update(kernel_ms=ms[1:])
        counts, stats = c.read_counts()
        umis, ok, bad = c.read_umis()
        out.update(reads=int(stats[0]), assigned=int(stats[1] + stats[2]), set_pairs=int(umis.sum()), umi_reads=ok, umi_failed=bad)
    print(json.dumps(out), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    out_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "profiles", "r13_umi_header_rates.txt")
    parent = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else None
    file_kinds = [k for k in FILE_KINDS if parent or k != "file_parent_inline"]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fastq")
        lib = library()
        with open(path, "wb") as h:
            for first in range(0, n, CHUNK):
                h.write(make_reads(lib, min(CHUNK, n - first), first))
        runs, ingest = {}, {}
        for kind in list(KINDS) * 2 + file_kinds * 2:
            print(f"[umi_header_rates] {kind}", file=sys.stderr, flush=True)
            tree = parent if kind == "file_parent_inline" else HERE
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, path, tree], capture_output=True, text=True, timeout=600)
            if done.returncode:                                      # nothing more is started after a failure
                sys.exit(f"{kind}: exit status {done.returncode}\n{done.stderr[-2000:]}")
            runs.setdefault(kind, []).append(json.loads(done.stdout.strip().splitlines()[-1]))
            if kind in KINDS:                                        # the ingest kernels of every pass but the first
                rows = [tuple(map(float, m.groups()[1:])) for m in TRACE.finditer(done.stderr)][1:]
                ingest.setdefault(kind, []).append(rows)
    row = dict(workload="reads_150_10k_m1_umi8_header_and_inline_20_8", reads=n, order_of_processes=list(KINDS) * 2 + file_kinds * 2)
    rate = lambda ms: n / ms / 1e6
    for kind in KINDS:
        best = min(min(r["kernel_ms"]) for r in runs[kind])
        passes = [p for rows in ingest[kind] for p in rows]
        row[kind] = dict(count_kernel_ms=[r["kernel_ms"] for r in runs[kind]], count_best_ms=best, count_greads_s=rate(best),
                         k_classify_ms=sorted(p[0] for p in passes), k_header_umi_ms=sorted(p[1] for p in passes), k_pack_ms=sorted(p[2] for p in passes),
                         **{k: runs[kind][0][k] for k in ("reads", "assigned", "set_pairs", "umi_reads", "umi_failed")})
    for kind in file_kinds:
        best = min(min(r["file_wall_ms"]) for r in runs[kind])
        row[kind] = dict(wall_ms=[r["file_wall_ms"] for r in runs[kind]], best_ms=best, greads_s=rate(best))
    assert len({(runs[k][0]["reads"], runs[k][0]["assigned"]) for k in runs}) == 1       # every context decided the reads alike
    assert len({(runs[k][0]["set_pairs"], runs[k][0]["umi_reads"], runs[k][0]["umi_failed"]) for k in runs}) == 1, "the two sources disagree"
    h = row["header"]
    row.update(k_header_umi_to_k_classify=min(h["k_header_umi_ms"]) / min(h["k_classify_ms"]),
               k_header_umi_to_classify_plus_pack=min(h["k_header_umi_ms"]) / (min(h["k_classify_ms"]) + min(h["k_pack_ms"])),
               count_header_to_count_inline=h["count_best_ms"] / row["inline"]["count_best_ms"],
               file_header_to_file_inline=row["file_header"]["best_ms"] / row["file_inline"]["best_ms"])
    if parent:
        p = row["file_parent_inline"]["wall_ms"]
        row.update(file_header_to_file_parent_inline=row["file_header"]["best_ms"] / row["file_parent_inline"]["best_ms"],
                   parent_inline_spread_ms=[min(min(w) for w in p), max(max(w) for w in p)],
                   file_header_inside_parent_spread=row["file_header"]["best_ms"] <= max(max(w) for w in p))
    with open(out_file, "w") as h:
        h.write(json.dumps(row) + "\n")
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        main()
