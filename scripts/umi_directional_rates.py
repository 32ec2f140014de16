"""Cost of keeping reads per (feature, UMI) pair and of --mur directional
(python scripts/umi_directional_rates.py [n_reads] [parent_checkout] [out_file]; out_file defaults to
profiles/r11_umi_directional_rates.txt): one JSON line per UMI window (8 and 4 flank bases) over the config-3 resident
block of scripts/umi_rates.py (50 M reads of 150 bases by default, 10 k guides, --st 0 --l 20 --m 1), HIP events throughout.
  (a) k_count_umi<true>: reads kept (f2q_set_umi_reads)
  (b) k_count_umi<false>: the instance every run without the call takes
  (c) the parent commit's k_count_umi, from `parent_checkout` (a built checkout of the parent commit next to the tree;
      without one (c) and the comparisons with it are left out)
  (d) f2q_umi_collapse_directional per launch next to f2q_umi_collapse on the same set (the F2Q_TRACE=1 lines)
Every counting figure comes from a process of its own (this file with --count), the three kinds taking turns -- c b a, four
times, and c -- so that the parent's run-to-run spread is taken in the same session: (b) must sit inside it.  (a) is given as a ratio
to (c) and against the text-already-in-HBM ingest rate of README (1.21 Greads/s): above it a --mur directional file run
stays ingest-bound."""
import importlib, json, os, re, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, REPS = 0xBEEF, 5
INGEST_GREADS_S = 1.21
WINDOWS = ((20, 8), (20, 4))


def setup(root, n):
    sys.path.insert(0, root)
    pkg = importlib.import_module("2fast2q_amd")
    guides = pkg.binding.synth_library(0xF2A5 + 3, 10000, 20)
    spec = dict(seed=SEED, n_reads=n, first_read=0, read_len=150, p_n=0.005)
    run = dict(features=guides, miss=1, phred=30, length=20, start="0")
    return pkg, spec, run


def count_only(root, n, keep):
    """k_count_umi's time per pass for both windows; the first pass (it sizes the set) is not among them"""
    pkg, spec, run = setup(root, n)
    out = {}
    for start, length in WINDOWS:
        with pkg.Counter(umi=(start, length), **(dict(run, umi_reads=True) if keep else run)) as c:
            blk = c.synth_create(**spec)
            ms = []
            for rep in range(REPS + 1):
                c.reset()
                ms.append(c.count_resident(blk)["kernel_ms"])
            umis, ok, bad = c.read_umis()
            blk.free()
        out[f"{start},{length}"] = dict(ms=ms[1:], pairs=int(umis.sum()), umi_reads=ok)
    print(json.dumps(out), flush=True)


def traced(call):
    """the library's stderr while `call` runs"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            out = call()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return out, tmp.read().decode()


CLUSTER = re.compile(r"UMI collapse: (\d+) pairs, (\d+) edges, (\d+) molecules, ([\d.]+) ms \(union-find init ([\d.]+), link ([\d.]+), roots ([\d.]+);")
DIRECTIONAL = re.compile(r"UMI collapse directional: (\d+) pairs, (\d+) edges, (\d+) dominated, (\d+) molecules, (\d+) reads, ([\d.]+) ms "
                         r"\(union-find init ([\d.]+), link ([\d.]+), spread ([\d.]+), roots ([\d.]+);")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
    parent = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] else None
    out_file = sys.argv[3] if len(sys.argv) > 3 else os.path.join(HERE, "profiles", "r11_umi_directional_rates.txt")
    turns = list("cbacbacbacbac") if parent else list("babababa")
    runs = {"a": [], "b": [], "c": []}
    for kind in turns:                                               # each in a fresh process: one library, one first set
        root = parent if kind == "c" else HERE
        got = subprocess.run([sys.executable, os.path.abspath(__file__), "--count", root, str(n), "1" if kind == "a" else "0"],
                             check=True, capture_output=True, text=True, timeout=900).stdout
        runs[kind].append(json.loads(got.strip().splitlines()[-1]))
    os.environ["F2Q_TRACE"] = "1"
    pkg, spec, run = setup(HERE, n)
    rows = []
    for start, length in WINDOWS:
        key = f"{start},{length}"
        best = {k: [min(r[key]["ms"]) for r in v] for k, v in runs.items()}
        row = dict(workload="cfg3_50M_10k_m1", reads=n, umi=[start, length], order_of_processes="".join(turns),
                   a_reads_kept_ms=[r[key]["ms"] for r in runs["a"]], b_reads_off_ms=[r[key]["ms"] for r in runs["b"]],
                   c_parent_ms=[r[key]["ms"] for r in runs["c"]] if parent else "not measured",
                   a_best_ms=min(best["a"]), b_best_ms=min(best["b"]), a_greads_s=n / min(best["a"]) / 1e6, b_greads_s=n / min(best["b"]) / 1e6,
                   ingest_greads_s=INGEST_GREADS_S, a_above_ingest_rate=n / min(best["a"]) / 1e6 > INGEST_GREADS_S, a_to_b=min(best["a"]) / min(best["b"]))
        if parent:
            lo, hi = min(best["c"]), max(best["c"])
            row.update(c_best_ms_per_process=best["c"], c_spread=(hi - lo) / lo, b_best_ms_per_process=best["b"],
                       b_to_c=min(best["b"]) / lo, b_within_parent_spread=all(x <= hi for x in best["b"]), a_to_c=min(best["a"]) / lo)
        with pkg.Counter(umi=(start, length), umi_reads=True, **run) as c:
            blk = c.synth_create(**spec)
            c.count_resident(blk)
            umis, ok, bad = c.read_umis()
            cl, di = [], []
            for rep in range(REPS + 1):
                (molecules, pairs, edges), said = traced(lambda: c.collapse_umis(1))
                m = CLUSTER.search(said)
                assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (pairs, edges, int(molecules.sum())), said
                cl.append([float(m.group(i)) for i in (5, 6, 7)])
                (dmol, dpairs, dedges, dominated, reads), said = traced(c.collapse_umis_directional)
                m = DIRECTIONAL.search(said)
                assert m and [int(m.group(i)) for i in range(1, 6)] == [dpairs, dedges, dominated, int(dmol.sum()), reads], said
                di.append([float(m.group(i)) for i in (7, 8, 9, 10)])
                assert (dpairs, dedges, reads) == (pairs, edges, ok) and bool((molecules <= dmol).all()) and bool((dmol <= umis).all())
            blk.free()
        cbest, dbest = [min(r[i] for r in cl[1:]) for i in range(3)], [min(r[i] for r in di[1:]) for i in range(4)]
        row.update(pairs=pairs, edges=edges, umi_reads=ok, cluster_molecules=int(molecules.sum()), directional_molecules=int(dmol.sum()),
                   dominated=dominated, cluster_init_link_roots_ms=cl[1:], directional_init_link_spread_roots_ms=di[1:],
                   cluster_best_ms=cbest, directional_best_ms=dbest, directional_to_cluster=sum(dbest) / sum(cbest),
                   directional_pairs_per_s=pairs / (sum(dbest) / 1e3), directional_to_a=sum(dbest) / min(best["a"]))
        rows.append(row)
    with open(out_file, "w") as h:
        for row in rows:
            h.write(json.dumps(row) + "\n")
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--count":
        count_only(sys.argv[2], int(sys.argv[3]), sys.argv[4] == "1")
    else:
        main()
