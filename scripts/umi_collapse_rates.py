"""Cost of --mu 1 (python scripts/umi_collapse_rates.py [n_reads] > profiles/<name>.txt): one JSON line per UMI window
(8 and 4 bases) over the config-3 resident block of scripts/umi_rates.py (50 M reads of 150 bases by default, 10 k guides,
--st 0 --l 20 --m 1): k_count_umi's HIP-event time on the reads, then f2q_umi_collapse on the set they leave -- pairs,
edges, molecules and the HIP-event time of each of its three launches (the F2Q_TRACE=1 line of the library, a warm-up and
REPS repeats per geometry), for the default geometry and the alternatives: workgroup size, workgroups per CU, and the
lane-per-slot layout against the wave-cooperative one.  The 4-base run checks itself: every feature holds all 256 UMIs,
so every feature is one molecule and the edges are 10 000 x 256 x 12 / 2."""
import importlib, json, os, re, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["F2Q_TRACE"] = "1"
pkg = importlib.import_module("2fast2q_amd")
SEED, REPS = 0xBEEF, 5
N = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
guides = pkg.binding.synth_library(0xF2A5 + 3, 10000, 20)
spec = dict(seed=SEED, n_reads=N, first_read=0, read_len=150, p_n=0.005)
run = dict(features=guides, miss=1, phred=30, length=20, start="0")
LINE = re.compile(r"UMI collapse: (\d+) pairs, (\d+) edges, (\d+) molecules, ([\d.]+) ms \(union-find init ([\d.]+), link ([\d.]+), roots ([\d.]+); (\w+), (\d+) x (\d+)\)")
GEOMETRIES = [dict(), dict(F2Q_UMI_LINK_WG="64", F2Q_UMI_LINK_GRID="32"), dict(F2Q_UMI_LINK_WG="128", F2Q_UMI_LINK_GRID="16"),
              dict(F2Q_UMI_LINK_GRID="4"), dict(F2Q_UMI_LINK_GRID="16"), dict(F2Q_UMI_LINK_GRID="64"), dict(F2Q_UMI_LINK="lane"),
              dict(F2Q_UMI_LINK="lane", F2Q_UMI_LINK_WG="64", F2Q_UMI_LINK_GRID="32"), dict()]


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


for start, length in ((20, 8), (20, 4)):
    with pkg.Counter(umi=(start, length), **run) as c:
        blk = c.synth_create(**spec)
        count_ms = []
        for rep in range(3):
            c.reset()
            count_ms.append(c.count_resident(blk)["kernel_ms"])
        umis, ok, bad = c.read_umis()
        row = dict(workload="cfg3_50M_10k_m1", reads=N, umi=[start, length], k_count_umi_ms=count_ms, umi_reads=ok, geometries=[])
        for env in GEOMETRIES:
            os.environ.update(env)
            reps = []
            for rep in range(REPS + 1):
                (molecules, pairs, edges), said = traced(lambda: c.collapse_umis(1))
                m = LINE.search(said)
                assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (pairs, edges, int(molecules.sum())), said
                reps.append([float(m.group(i)) for i in (5, 6, 7)])
            for k in env:
                del os.environ[k]
            best = [min(r[i] for r in reps[1:]) for i in range(3)]
            row["geometries"].append(dict(env=env, layout=m.group(8), grid=int(m.group(9)), workgroup=int(m.group(10)), init_link_roots_ms=reps[1:],
                                          best_ms=best, pairs_per_s=pairs / (sum(best) / 1e3), ratio_to_k_count_umi=sum(best) / min(count_ms[1:])))
            row.update(pairs=pairs, edges=edges, molecules=int(molecules.sum()), pairs_equal_umis=pairs == int(umis.sum()))
            if length == 4:
                row["self_check"] = bool((molecules == 1).all()) and pairs == 2_560_000 and edges == 15_360_000 if N == 50_000_000 else None
        blk.free()
    print(json.dumps(row), flush=True)
