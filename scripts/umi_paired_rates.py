"""Cost of the (feature, UMI) set on paired-end samples (--umi1 / --umi2 with --pe; f2q_set_umi_paired)
(python scripts/umi_paired_rates.py [n_pairs] [out_file]; out_file defaults to profiles/r12_umi_paired_rates.txt): one JSON
line over resident 2 x 150 pairs (10 k features of 10 + 10 bases, --st 5 --st2 0 --l 10 --m 1 --rc2, UMI 12,8 in mate 2),
HIP events throughout.  A resident block of pairs holds less than 1 GiB of text per mate, so the block has 2 M pairs by
default (at most 3.3 M fit), not the 50 M reads of scripts/umi_directional_rates.py.
  (a) k_count_umi_pair under both layouts (F2Q_UMI_PAIR_STAGE=1: the merged lines staged in LDS, =0: read from global
      memory), each with and without reads per pair (f2q_set_umi_reads)
  (b) the same pairs on a paired context WITHOUT the call (tiles for clean pairs, k_count_general<true> for the rest): the
      cost of the feature is (a) against (b); and with F2Q_FORCE_GENERAL=1 (every pair through k_count_general<true>: the
      same road without the set)
  (c) for scale, the single-end k_count_umi<false> rate of profiles/r11_umi_directional_rates.txt (8-base UMI, 50 M reads)
  (d) f2q_count_file_paired on the same pairs as two plain FASTQ files, with and without the call: the paired file-ingest
      rate the resident rates are to be read against
Every figure comes from a process of its own (this file with --one), the kinds taking turns, twice."""
import importlib, json, os, subprocess, sys, tempfile, time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 5
ST1, ST2, LENGTH, UMI2 = 5, 0, 10, (12, 8)
KINDS = {"stage0": dict(stage="0", keep=False), "stage0_reads": dict(stage="0", keep=True), "stage1": dict(stage="1", keep=False),
         "stage1_reads": dict(stage="1", keep=True), "no_umi": dict(), "no_umi_general": dict(general=True)}
FILE_KINDS = {"umi": dict(stage=None, keep=False), "umi_reads": dict(stage=None, keep=True), "no_umi": dict()}      # (the default layout)
CHUNK = 250_000


def library(n=10000, seed=0xF2A5):
    rng = np.random.default_rng(seed)
    parts = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (2 * n, 2, LENGTH))]
    return sorted({a.tobytes().decode() + ":" + b.tobytes().decode() for a, b in parts})[:n]


def make_pairs(lib, n, first, seed=0xBEEF, length=150, p_sub=0.02, p_rand=0.1, p_lowq=0.004, p_n=0.005, pool=64):
    """n uniform 2 x 150 pairs, numbered from `first`: the parts of a feature at ST1 of mate 1 and at ST2 of mate 2 as the run
    takes it (mate 2 is written reverse-complemented), substitutions, random pairs, low quality bytes and 'N's anywhere;
    positions UMI2 of mate 2 as written hold one of `pool` UMIs, so a (feature, UMI) pair has about three reads"""
    rng = np.random.default_rng(seed + first)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    parts = np.array([[list(p.encode()) for p in f.split(":")] for f in lib], np.uint8)
    umis = acgt[np.random.default_rng(seed).integers(0, 4, (pool, UMI2[1]))]
    pick, planted = rng.integers(0, len(lib), n), rng.random(n) >= p_rand
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    out = []
    for mate, st in enumerate((ST1, ST2)):
        s = acgt[rng.integers(0, 4, (n, length))]
        seg = parts[pick, mate].copy()
        sub = rng.random(seg.shape) < p_sub
        seg[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
        s[planted, st:st + LENGTH] = seg[planted]
        s[rng.random(s.shape, dtype=np.float32) < p_n] = ord("N")
        q = np.full((n, length), ord("I"), np.uint8)
        low = rng.random(q.shape, dtype=np.float32) < p_lowq
        q[low] = np.frombuffer(b"!#+5:>?@", np.uint8)[rng.integers(0, 8, int(low.sum()))]
        if mate == 1:
            s, q = np.frombuffer(s.tobytes().translate(comp), np.uint8).reshape(s.shape)[:, ::-1].copy(), q[:, ::-1]
            s[:, UMI2[0]:UMI2[0] + UMI2[1]] = umis[rng.integers(0, pool, n)]
        head = np.frombuffer(b"".join(b"@%c%08d\n" % (b"ab"[mate], first + i) for i in range(n)), np.uint8).reshape(n, 11)
        plus = np.tile(np.frombuffer(b"\n+\n", np.uint8), (n, 1))
        out.append(np.concatenate([head, s, plus, q, np.full((n, 1), 10, np.uint8)], axis=1).tobytes())
    return out


def context(pkg, lib, kind):
    spec = KINDS.get(kind) or FILE_KINDS[kind]
    for key in ("F2Q_UMI_PAIR_STAGE", "F2Q_FORCE_GENERAL"):
        os.environ.pop(key, None)
    if "stage" in spec:
        if spec["stage"] is not None:
            os.environ["F2Q_UMI_PAIR_STAGE"] = spec["stage"]
        return pkg.Counter(features=lib, miss=1, phred=30, length=LENGTH, start=str(ST1), start2=str(ST2), rc2=True, umi_paired=(None, UMI2),
                           umi_reads=spec["keep"])
    if spec.get("general"):
        os.environ["F2Q_FORCE_GENERAL"] = "1"
    return pkg.Counter(features=lib, miss=1, phred=30, length=LENGTH, start=str(ST1), start2=str(ST2), rc2=True)


def one(kind, path1, path2, files):
    """a resident block counted REPS + 1 times (the first pass sizes the set and is not reported); files: the two files
    streamed REPS times instead"""
    sys.path.insert(0, HERE)
    pkg = importlib.import_module("2fast2q_amd")
    lib = library()
    out = dict(kind=kind)
    with context(pkg, lib, kind) as c:
        if files:
            ms = []
            for rep in range(REPS):
                c.reset()
                t0 = time.perf_counter()
                c.count_file_paired(path1, path2)
                ms.append((time.perf_counter() - t0) * 1e3)
            out.update(file_wall_ms=ms)
        else:
            blk = c.block_from_fastq_paired(open(path1, "rb").read(), open(path2, "rb").read())
            info, ms = blk.info(), []
            for rep in range(REPS + 1):
                c.reset()
                ms.append(c.count_resident(blk)["kernel_ms"])
            blk.free()
            out.update(kernel_ms=ms[1:], general=info["n_general"])
        counts, stats = c.read_counts()
        out.update(pairs=int(stats[0]), assigned=int(stats[1] + stats[2]))
        if c.umi_length:
            umis, ok, bad = c.read_umis()
            out.update(set_pairs=int(umis.sum()), umi_reads=ok, umi_failed=bad)
    print(json.dumps(out), flush=True)


def single_end_figure():
    try:
        row = json.loads(open(os.path.join(HERE, "profiles", "r11_umi_directional_rates.txt")).readline())
        return dict(reads=row["reads"], umi=row["umi"], k_count_umi_false_best_ms=row["b_best_ms"], greads_s=row["b_greads_s"])
    except (OSError, ValueError, KeyError):
        return "not found"


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    out_file = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "profiles", "r12_umi_paired_rates.txt")
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, f"pairs_R{k}.fastq") for k in (1, 2)]
        lib = library()
        with open(paths[0], "wb") as h1, open(paths[1], "wb") as h2:
            for first in range(0, n, CHUNK):
                t1, t2 = make_pairs(lib, min(CHUNK, n - first), first)
                h1.write(t1); h2.write(t2)
        runs = {}
        for files, kinds in ((False, list(KINDS) * 2), (True, list(FILE_KINDS) * 2)):
            for kind in kinds:
                print(f"[umi_paired_rates] {'files' if files else 'resident'} {kind}", file=sys.stderr, flush=True)
                done = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, paths[0], paths[1], "1" if files else "0"],
                                      capture_output=True, text=True, timeout=900)
                if done.returncode:                                  # nothing more is started after a failure
                    sys.exit(f"{kind}: exit status {done.returncode}\n{done.stderr[-2000:]}")
                runs.setdefault(("file_" if files else "") + kind, []).append(json.loads(done.stdout.strip().splitlines()[-1]))
    row = dict(workload="pairs_2x150_10k_m1_rc2_umi2_12_8", pairs=n, order_of_processes=list(KINDS) * 2)
    rate = lambda ms: n / ms / 1e6
    for kind in KINDS:
        best = min(min(r["kernel_ms"]) for r in runs[kind])
        row[kind] = dict(kernel_ms=[r["kernel_ms"] for r in runs[kind]], best_ms=best, gpairs_s=rate(best), general_pairs=runs[kind][0]["general"],
                         **{k: runs[kind][0][k] for k in ("pairs", "assigned", "set_pairs", "umi_reads", "umi_failed") if k in runs[kind][0]})
    for kind in FILE_KINDS:
        best = min(min(r["file_wall_ms"]) for r in runs["file_" + kind])
        row["file_" + kind] = dict(wall_ms=[r["file_wall_ms"] for r in runs["file_" + kind]], best_ms=best, gpairs_s=rate(best))
    same = {(runs[k][0]["pairs"], runs[k][0]["assigned"]) for k in runs}
    assert len(same) == 1, same                                      # every context decided the pairs alike
    assert len({(runs[k][0]["set_pairs"], runs[k][0]["umi_reads"]) for k in runs if "set_pairs" in runs[k][0]}) == 1
    row.update(stage1_to_stage0=row["stage1"]["best_ms"] / row["stage0"]["best_ms"],
               stage1_reads_to_stage0_reads=row["stage1_reads"]["best_ms"] / row["stage0_reads"]["best_ms"],
               faster_layout="stage1" if row["stage1"]["best_ms"] < row["stage0"]["best_ms"] else "stage0",
               umi_to_no_umi=min(row["stage0"]["best_ms"], row["stage1"]["best_ms"]) / row["no_umi"]["best_ms"],
               umi_to_no_umi_general=min(row["stage0"]["best_ms"], row["stage1"]["best_ms"]) / row["no_umi_general"]["best_ms"],
               file_umi_to_file_no_umi=row["file_umi"]["best_ms"] / row["file_no_umi"]["best_ms"],
               resident_above_file_ingest_rate=max(row["stage0"]["gpairs_s"], row["stage1"]["gpairs_s"]) > row["file_no_umi"]["gpairs_s"],
               single_end_for_scale=single_end_figure())
    with open(out_file, "w") as h:
        h.write(json.dumps(row) + "\n")
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] == "1")
    else:
        main()
