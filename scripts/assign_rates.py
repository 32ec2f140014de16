"""Cost of Extract+Count with a library (python scripts/assign_rates.py [n_reads] > profiles/<name>.txt): per workload
one JSON line with the HIP-event time of f2q_ec_assign next to the Extract+Count counting time of the same resident
block, and -- the alternative without it -- a full Counter pass over the same reads against the same library (--m 1),
kernel and wall time; BASELINE configs 5b (anchored) and 3b (fixed window), 50 M reads by default."""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("2fast2q_amd")
UP, DOWN, SEED = "GTTTAAGAGCTA", "CGTTACCAGGTT", 0xBEEF
N = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
for name, lib_seed, anchored in (("cfg5b_50M_anchor_ec", 0xF2A5 + 5, True), ("cfg3b_50M_fixed_ec", 0xF2A5 + 3, False)):
    guides = pkg.binding.synth_library(lib_seed, 10000, 20)
    run = dict(upstream=UP, downstream=DOWN, miss_search_up=1, miss_search_down=1) if anchored else dict(length=20, start="0")
    spec = dict(seed=SEED, n_reads=N, first_read=0, read_len=150, p_n=0.005)
    if anchored:
        spec.update(cassette=True, up=UP, down=DOWN, max_offset=100)
    with pkg.Counter(mode="EC", miss=1, phred=30, **run) as c:
        c.set_assign_library(guides)
        blk = c.synth_create(guides=guides, **spec)
        count_ms, assign_ms, assign_wall = [], [], []
        for rep in range(4):
            c.reset()
            count_ms.append(c.count_resident(blk)["kernel_ms"])
            for again in range(2):
                t0 = time.perf_counter()
                counts, stats, t = c.ec_assign(want_timing=True)
                assign_wall.append((time.perf_counter() - t0) * 1e3)
                assign_ms.append(t["kernel_ms"])
        nk = len(c.ec_assigned())
        blk.free()
    with pkg.Counter(features=guides, miss=1, phred=30, **run) as cc:
        blk = cc.synth_create(**spec)
        counter_ms, counter_wall = [], []
        for rep in range(4):
            cc.reset()
            t0 = time.perf_counter()
            counter_ms.append(cc.count_resident(blk)["kernel_ms"])
            ccounts, cstats = cc.read_counts()
            counter_wall.append((time.perf_counter() - t0) * 1e3)
        blk.free()
    same = list(ccounts) == list(counts) and list(cstats) == list(stats)
    row = dict(workload=name, reads=N, distinct_keys=nk, ec_count_kernel_ms=count_ms, assign_kernel_ms=assign_ms, assign_wall_ms=assign_wall,
               counter_pass_kernel_ms=counter_ms, counter_pass_wall_ms=counter_wall, assign_equals_counter_pass=same, stats=[int(x) for x in stats])
    print(json.dumps(row), flush=True)
