"""Rates of the paired-end path (python scripts/paired_rates.py [n_pairs] > profiles/<name>.txt).
With --ingest-only: three calls of each ingest entry point and nothing else, for
    rocprofv3 --kernel-trace --stats -d <dir> -o pair -f csv -- python scripts/paired_rates.py 3000000 --ingest-only

Counting: a resident block of pairs (f2q_block_from_fastq_paired) beside the resident block of the merged reads of the same
pairs counted single-end with two windows (f2q_block_from_fastq), both through f2q_count_resident_queued: the tiles are
the same bytes, so the times should agree within the spread of the repeats.
Ingest: f2q_count_block_paired on the two texts beside f2q_count_block on the merged text (same build: that entry point
and its kernels are unchanged by the paired path), with the ratio of the text sizes.
Files: f2q_count_file_paired on plain and BGZF pairs beside f2q_count_file on the merged file."""
import importlib
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import paired_cases as PC                                             # noqa: E402
from conftest import bgzf_bytes                                       # noqa: E402

P = importlib.import_module("2fast2q_amd")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 3000000                              # a block of pairs holds < 1 GiB of text per mate and call
    ingest_only = "--ingest-only" in sys.argv
    print(f"# python scripts/paired_rates.py {n}{' --ingest-only' if ingest_only else ''}   (150 + 150-base mates, 10 k A:B features of 10 + 10 bases, --m 1, rc2)")
    st1, st2, length = [5], [30], 10
    lib = PC.pair_library(10000, length, 1, 1, 3)
    fq1, fq2 = PC.make_pairs_uniform(lib, length, st1, st2, True, n, seed=1)
    (start, merged), = PC.merged_groups(fq1, fq2, st1, st2, length, True)[0].items()
    pe = P.Counter(features=lib, miss=1, length=length, start="5", start2="30", rc2=True)
    se = P.Counter(features=lib, miss=1, length=length, start=start)
    if ingest_only:
        for _ in range(3):
            pe.count_block_paired(fq1, fq2); se.count_block(merged)
        print(f"text bytes: paired {len(fq1) + len(fq2)}, merged {len(merged)}")
        pe.close(); se.close()
        return
    # ---- counting (a resident block of pairs holds less than 1 GiB of text per mate: the first 3 M pairs at most)
    nc = min(n, 3000000)
    c1, c2 = fq1[:len(fq1) // n * nc], fq2[:len(fq2) // n * nc]           # (every record of a mate is as long)
    (_, cm), = PC.merged_groups(c1, c2, st1, st2, length, True)[0].items()
    bp, bs = pe.block_from_fastq_paired(c1, c2), se.block_from_fastq(cm)
    n_all, n = n, nc
    for name, c, b in (("paired", pe, bp), ("merged single-end", se, bs)):
        for _ in range(5):
            c.count_resident_queued(b)
        c.queued_times()
        for _ in range(40):
            c.count_resident_queued(b)
        ms = c.queued_times()
        t = c.count_resident(b)
        print(f"counting, {name}: median {statistics.median(ms):.4f} ms, min {min(ms):.4f}, max {max(ms):.4f} per {n} reads "
              f"({n / statistics.median(ms) / 1e6:.1f} Greads/s); path {t['path']}, general reads {t['general_reads']}, block {b.info()['device_bytes']} bytes")
    bp.free(); bs.free()
    n = n_all
    # ---- ingest
    times = {}
    for name, call in (("paired", lambda: pe.count_block_paired(fq1, fq2)), ("merged single-end", lambda: se.count_block(merged))):
        call()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter(); call(); ts.append((time.perf_counter() - t0) * 1e3)
        times[name] = ts
        print(f"ingest, {name}: median {statistics.median(ts):.1f} ms, min {min(ts):.1f}, max {max(ts):.1f} ({n / statistics.median(ts) / 1e3:.1f} Mreads/s)")
    ratio = (len(fq1) + len(fq2)) / len(merged)
    print(f"ingest: text bytes paired / merged = {ratio:.4f}; merged time x ratio = {statistics.median(times['merged single-end']) * ratio:.1f} ms")
    # ---- files
    with tempfile.TemporaryDirectory() as d:
        for kind in ("plain", "bgzf"):
            enc = (lambda x: x) if kind == "plain" else bgzf_bytes
            ext = ".fastq" if kind == "plain" else ".fastq.gz"
            paths = [os.path.join(d, f"{kind}_R1{ext}"), os.path.join(d, f"{kind}_R2{ext}"), os.path.join(d, f"{kind}_merged{ext}")]
            for p, data in zip(paths, (fq1, fq2, merged)):
                with open(p, "wb") as f:
                    f.write(enc(data))
            for name, call in (("paired", lambda: pe.count_file_paired(paths[0], paths[1])), ("merged single-end", lambda: se.count_file(paths[2]))):
                call()
                t0 = time.perf_counter(); call(); ms = (time.perf_counter() - t0) * 1e3
                print(f"file, {kind}, {name}: {ms:.1f} ms ({n / ms / 1e3:.1f} Mreads/s)")
    pe.close(); se.close()


if __name__ == "__main__":
    main()
