"""Wall-clock rate of f2q_count_file on BGZF FASTQ, host inflater against device inflater (F2Q_DEVICE_INFLATE=1).

An n-read x 150 bp synthetic file (default 8 M reads) is written as BGZF at zlib level 1 and at level 6.  Each file is
counted with the switch off and on, the arms alternating `repeats` times, every count in a fresh child process; prints
Mreads/s of the f2q_count_file call and its F2Q_TRACE split.  usage: bgzf_rate.py [n_reads] [repeats] [dir]"""
import concurrent.futures
import importlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def guides(pkg):
    return pkg.binding.synth_library(0xF2A5 + 3, 10000, 20)


def bgzf_member(args):
    data, level = args
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = co.compress(data) + co.flush()
    bsize = 18 + len(body) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1) + body
            + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def write_bgzf(path, fq, level, block=0xFF00):
    jobs = [(fq[i:i + block], level) for i in range(0, len(fq), block)] + [(b"", level)]     # bgzip's empty end marker
    with concurrent.futures.ThreadPoolExecutor(16) as ex, open(path, "wb") as f:            # (zlib lets go of the GIL)
        for m in ex.map(bgzf_member, jobs, chunksize=64):
            f.write(m)


def child(path):
    pkg = importlib.import_module("2fast2q_amd")
    with pkg.Counter(features=guides(pkg), miss=1) as c:
        t0 = time.perf_counter()
        t, trunc = c.count_file(path)
        dt = time.perf_counter() - t0
    print(json.dumps({"s": dt, "reads": t["reads"], "truncated": trunc}), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    d = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp()
    pkg = importlib.import_module("2fast2q_amd")
    with pkg.Counter(features=guides(pkg), miss=1) as c:
        fq = bytes(c.synth_fastq(seed=1, n_reads=n, read_len=150))
    files = {}
    for lv in (1, 6):
        p = os.path.join(d, f"b{lv}.fastq.gz")
        t0 = time.perf_counter()
        write_bgzf(p, fq, lv)
        files[lv] = p
        print(f"level {lv}: {len(fq) / 1e9:.2f} GB of text, {os.path.getsize(p) / 1e9:.3f} GB BGZF (written in {time.perf_counter() - t0:.0f} s)", flush=True)
    del fq
    for lv, p in files.items():
        for rep in range(reps):
            for arm in ("host", "device"):
                env = dict(os.environ, F2Q_TRACE="1")
                env.pop("F2Q_DEVICE_INFLATE", None)
                if arm == "device":
                    env["F2Q_DEVICE_INFLATE"] = "1"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", p], env=env, stdout=subprocess.PIPE,
                                   stderr=subprocess.PIPE, text=True, timeout=600)
                if r.returncode:
                    print(f"level {lv} {arm}: child exited {r.returncode}\n{r.stderr[-3000:]}", flush=True)
                    sys.exit(1)
                res = json.loads(r.stdout.strip().splitlines()[-1])
                trace = [x.split(" (", 1)[-1] for x in r.stderr.splitlines() if x.startswith("[f2q trace]") and " io threads)" in x]
                print(f"level {lv} {arm:6s} #{rep}: {res['reads'] / res['s'] / 1e6:6.1f} Mreads/s ({res['s']:.2f} s, {res['reads']} reads"
                      f"{', truncated' if res['truncated'] else ''}) {trace[-1] if trace else ''}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
