"""Cost of collapsing the extracted keys of an Extract+Count sample (--ecm 1; f2q_ec_collapse)
(python scripts/ec_collapse_rates.py [n_reads] [n_small] [out_file] [parent_checkout]; out_file defaults to
profiles/r19_ec_collapse_rates.txt): one JSON line over the README's anchored Extract+Count workload (150-base reads, the
cassette of a 10 k-guide library between --us/--ds at a varying offset, --msu 1 --msd 1), made resident on the device by
f2q_synth_create: n_reads (50 M by default: the largest block this script makes resident) and a second, smaller table
(n_small, 2 M by default).
  (a) f2q_ec_collapse at ratio 5 on the table of each block: HIP-event time of k_ec_parent and of k_ec_roots (F2Q_TRACE=1
      prints both) in the wave-cooperative layout and under F2Q_ECC_LINK=lane
  (b) the counting time of the same blocks (HIP events): this tree's, and -- when parent_checkout names a built checkout of
      the parent commit -- the parent's; no counting kernel differs, so the ratio should be 1.00 within the spread
  (c) f2q_ec_assign on the large table against the 10 k guides: the one other per-key pass there is
  (d) f2q_count_text on the text of the smaller block uploaded once: wall time of the call, the ingest the collapse of that
      sample has to stay below for a file run to remain ingest-bound
Every figure comes from a process of its own (this file with --one) under a time limit, five passes after one that is not
reported, the kinds taking turns, twice: ten passes in two processes per kind.  Nothing more is started after a failure."""
import importlib, json, os, re, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
UP, DOWN, SEED, LIB_SEED = "GTTTAAGAGCTA", "CGTTACCAGGTT", 0xBEEF, 0xF2A5 + 5
RUN = dict(upstream=UP, downstream=DOWN, miss_search_up=1, miss_search_down=1)
TRACE = re.compile(r"Extract\+Count collapse .*: (\d+) keys, (\d+) eligible, (\d+) absorbed with (\d+) reads, longest chain (\d+), .*"
                   r"k_ec_parent ([0-9.]+), k_ec_roots ([0-9.]+); (\w+), (\d+) slots")
KINDS = ("collapse_wave_big", "collapse_lane_big", "collapse_wave_small", "collapse_lane_small", "count_big", "count_small",
         "count_parent_big", "count_parent_small", "assign_big", "text_small")


def one(kind, n, tree):
    sys.path.insert(0, tree)
    what, size = kind.rsplit("_", 1)
    if what.startswith("collapse"):
        os.environ["F2Q_TRACE"] = "1"
        os.environ["F2Q_ECC_LINK"] = "lane" if "lane" in what else "wave"
    pkg = importlib.import_module("2fast2q_amd")
    guides = pkg.binding.synth_library(LIB_SEED, 10000, 20)
    spec = dict(seed=SEED, n_reads=n, first_read=0, read_len=150, p_n=0.005, cassette=True, up=UP, down=DOWN, max_offset=100)
    out = dict(kind=kind, reads=n)
    with pkg.Counter(mode="EC", miss=1, phred=30, **RUN) as c:
        if what == "text":
            text = c.text_upload(bytes(c.synth_fastq(guides=guides, **spec)))
            ms = []
            for rep in range(REPS + 1):
                c.reset()
                t0 = time.perf_counter()
                c.count_text(text)
                c.read_counts()                                     # (waits for the stream)
                ms.append((time.perf_counter() - t0) * 1e3)
            text.free()
            out.update(wall_ms=ms[1:])
        else:
            if what == "assign":
                c.set_assign_library(guides)
            blk = c.synth_create(guides=guides, **spec)
            ms = []
            for rep in range(REPS + 1 if what.startswith("count") else 1):
                c.reset()
                ms.append(c.count_resident(blk)["kernel_ms"])
            if what.startswith("count"):
                out.update(kernel_ms=ms[1:])
            elif what == "assign":
                out.update(kernel_ms=[c.ec_assign(want_timing=True)[2]["kernel_ms"] for rep in range(REPS + 1)][1:])
            else:
                both = [c.ec_collapse(1, 5, want_timing=True) for rep in range(REPS + 1)]
                assert all(b[0] == both[0][0] for b in both)
                out.update(kernel_ms=[b[1]["kernel_ms"] for b in both][1:], extra=both[0][0])
            blk.free()
        out.update(counted=int(c.read_counts()[1][0]))
    print(json.dumps(out), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
    n_small = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
    out_file = sys.argv[3] if len(sys.argv) > 3 else os.path.join(HERE, "profiles", "r19_ec_collapse_rates.txt")
    parent = os.path.abspath(sys.argv[4]) if len(sys.argv) > 4 else None
    kinds = [k for k in KINDS if parent or "parent" not in k]
    runs = {}
    for kind in kinds * 2:
        print(f"[ec_collapse_rates] {kind}", file=sys.stderr, flush=True)
        size = n if kind.endswith("_big") else n_small
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, str(size), parent if "parent" in kind else HERE],
                              capture_output=True, text=True, timeout=600)
        if done.returncode:                                          # nothing more is started after a failure
            sys.exit(f"{kind}: exit status {done.returncode}\n{done.stderr[-2000:]}")
        r = json.loads(done.stdout.strip().splitlines()[-1])
        if kind.startswith("collapse"):
            lines = [m.groups() for m in map(TRACE.search, done.stderr.splitlines()) if m][1:]      # (the first pass is not reported)
            assert len(lines) == REPS and all(g[7] == kind.split("_")[1] for g in lines), done.stderr[-2000:]
            r.update(parent_ms=[float(g[5]) for g in lines], roots_ms=[float(g[6]) for g in lines], keys=int(lines[0][0]), slots=int(lines[0][8]))
        runs.setdefault(kind, []).append(r)
    row = dict(workload="cfg5b_anchor_ec_150bp_10k_guides", reads_big=n, reads_small=n_small, ratio=5, order_of_processes=kinds * 2)
    for size in ("big", "small"):
        a, b = runs[f"collapse_wave_{size}"][0], runs[f"collapse_lane_{size}"][0]
        assert a["extra"] == b["extra"] and a["keys"] == b["keys"], (a, b)           # both layouts give one answer
    for kind in kinds:
        key = "wall_ms" if kind.startswith("text") else "kernel_ms"
        row[kind] = {key: [r[key] for r in runs[kind]], "best_ms": min(min(r[key]) for r in runs[kind])}
        if kind.startswith("collapse"):
            row[kind].update(parent_ms=[r["parent_ms"] for r in runs[kind]], roots_ms=[r["roots_ms"] for r in runs[kind]],
                             best_parent_ms=min(min(r["parent_ms"]) for r in runs[kind]), best_roots_ms=min(min(r["roots_ms"]) for r in runs[kind]),
                             keys=runs[kind][0]["keys"], slots=runs[kind][0]["slots"], extra=runs[kind][0]["extra"])
    best = lambda k: row[k]["best_ms"]
    row.update(wave_to_lane={s: best(f"collapse_wave_{s}") / best(f"collapse_lane_{s}") for s in ("big", "small")},
               collapse_to_count={s: best(f"collapse_wave_{s}") / best(f"count_{s}") for s in ("big", "small")},
               collapse_to_assign_big=best("collapse_wave_big") / best("assign_big"),
               collapse_small_to_text_ingest_small=best("collapse_wave_small") / best("text_small"),
               collapse_below_ingest_of_its_sample=best("collapse_wave_small") < best("text_small"))
    if parent:
        row.update(count_to_count_parent={s: best(f"count_{s}") / best(f"count_parent_{s}") for s in ("big", "small")})
    with open(out_file, "w") as h:
        h.write(json.dumps(row) + "\n")
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    else:
        main()
