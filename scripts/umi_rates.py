"""Cost of --umi (python scripts/umi_rates.py [n_reads] > profiles/<name>.txt): one JSON line with the HIP-event time of
f2q_count_resident over the config-3 resident block (50 M reads of 150 bases by default, 10 k guides, --st 0 --l 20 --m 1)
on the raw-record road without the (feature, UMI) set (F2Q_FORCE_GENERAL=1: k_count_general) and with it (k_count_umi),
for a UMI window of 8 bases (random flank: nearly every assigned read brings a new pair) and of 4 bases (256 UMIs per
feature: most reads repeat a pair); the first pass of each UMI context includes sizing the set, the later ones reuse it."""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("2fast2q_amd")
SEED = 0xBEEF
N = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
guides = pkg.binding.synth_library(0xF2A5 + 3, 10000, 20)
spec = dict(seed=SEED, n_reads=N, first_read=0, read_len=150, p_n=0.005)
run = dict(features=guides, miss=1, phred=30, length=20, start="0")


def passes(c, reps=4):
    blk = c.synth_create(**spec)
    assert blk.info()["n_general"] == N
    ms = []
    for rep in range(reps):
        c.reset()
        ms.append(c.count_resident(blk)["kernel_ms"])
    counts, stats = c.read_counts()
    blk.free()
    return ms, list(counts), list(stats)


os.environ["F2Q_FORCE_GENERAL"] = "1"
with pkg.Counter(**run) as c:
    plain_ms, counts, stats = passes(c)
del os.environ["F2Q_FORCE_GENERAL"]
row = dict(workload="cfg3_50M_10k_m1", reads=N, stats=[int(x) for x in stats], general_kernel_ms=plain_ms,
           general_greads_s=N / min(plain_ms) / 1e6)
for start, length in ((20, 8), (20, 4)):
    with pkg.Counter(umi=(start, length), **run) as c:
        ms, ucounts, ustats = passes(c)
        umis, ok, bad = c.read_umis()
    row[f"umi_{start}_{length}"] = dict(kernel_ms=ms, greads_s=N / min(ms[1:]) / 1e6, ratio_to_general=min(ms[1:]) / min(plain_ms),
                                        pairs=int(umis.sum()), umi_reads=ok, umi_failed=bad,
                                        counts_equal_general=ucounts == counts and ustats == stats)
print(json.dumps(row), flush=True)
