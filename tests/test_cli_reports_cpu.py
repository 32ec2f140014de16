"""Every report file of the command line, without a GPU: fast2q.main() over a counter that returns seeded values of the shapes
binding.Counter documents, one run per option (and the combinations the options allow), with and without --k, with feature
names that are all numbers and that are not.  The set of files of the output directory, every .csv byte for byte and
run_headers(param) are compared with tests/golden/cli_reports.json, which tests/golden/make_golden_cli_reports.py recorded
from this project's own output.  The GPU command-line tests check that the numbers are right; this one checks that no
table, block or line of a report moves."""
import glob
import importlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

from conftest import GOLDEN
from test_abi_and_host import _Clock

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")
GOLDEN_FILE = os.path.join(GOLDEN, "cli_reports.json")

SEQS = ["ACGTACGTACGTACGTACGT", "TTTTACGTACGTACGTAAAA", "GGGGACGTACGTACGTCCCC", "CATGCATGCATGCATGCATG", "GATTACAGATTACAGATTAC"]
NAMES = {"text": ["geneB", "geneA", "zeta", "alpha", "mid"], "numeric": ["10", "9", "100", "1", "25"]}
PAIRS = [(0, 0), (1, 1), (2, 0), (0, 1), (3, 2)]               # the pair library of --parts: (part 1, part 2) of each feature
PART1 = ["ACGTACGTAC", "TTTTACGTAC", "GGGGACGTAC", "CATGCATGCA"]
PART2 = ["GTACGTACGT", "GTACGTAAAA", "TGCATGCATG"]
EC_KEYS = ["ACGTACGTACGTACGTACGT", "ACGTACGTACGTACGTACGA", "TTTTACGTACGTACGTAAAA", "CCCCCCCCCCGGGGGGGGGG", "GATTACAGATTACAGATTAC",
           "GATTACAGATTACAGATTAG", "AAAAAAAAAATTTTTTTTTT"]

# name, flags, the namings it runs with, the --k settings it runs with
BOTH, KEPT, DROPPED = (True, False), (True,), (False,)
CASES = [
    ("plain_counter", [], ("text", "numeric"), BOTH),
    ("plain_ec", ["--mo", "EC"], ("text",), BOTH),
    ("paired", ["--pe", "--st2", "0", "--rc2"], ("text", "numeric"), BOTH),
    ("umi", ["--umi", "20,8"], ("text", "numeric"), BOTH),
    ("umi_mu1", ["--umi", "20,8", "--mu", "1"], ("text", "numeric"), BOTH),
    ("umi_directional", ["--umi", "20,8", "--mu", "1", "--mur", "directional"], ("text", "numeric"), BOTH),
    ("umih", ["--umih", "_,8"], ("text", "numeric"), BOTH),
    ("sample_barcodes", ["--sb", "sb.csv", "--sbs", "2", "--sbm", "1"], ("text", "numeric"), BOTH),
    ("strand", ["--strand", "both"], ("text", "numeric"), BOTH),
    ("stagger", ["--stagger", "3", "--st", "2"], ("text", "numeric"), BOTH),
    ("indel", ["--indel"], ("text", "numeric"), BOTH),
    ("parts", ["--parts", "--st", "0,30", "--l", "10"], ("text", "numeric"), BOTH),
    ("assign", ["--mo", "EC", "--as"], ("text", "numeric"), BOTH),
    ("ec_collapse", ["--mo", "EC", "--ecm", "1", "--ecr", "3"], ("text",), BOTH),
    ("pe_umi12_directional", ["--pe", "--st2", "0", "--umi1", "0,4", "--umi2", "0,4", "--mu", "1", "--mur", "directional"], ("text", "numeric"), KEPT),
    ("pe_parts", ["--pe", "--st2", "0", "--parts", "--l", "10"], ("text", "numeric"), DROPPED),
    ("ec_as_ecm", ["--mo", "EC", "--as", "--ecm", "1"], ("text", "numeric"), DROPPED),
]
RUNS = [(name, naming, keep) for name, _, namings, keeps in CASES for naming in namings for keep in keeps]
FLAGS = {name: flags for name, flags, _, _ in CASES}


def run_id(name, naming, keep):
    return f"{name}-{naming}-{'keep' if keep else 'delete'}"


def _vals(seed, tag, n, hi):
    """n numbers 0 .. hi that depend on the sample (seed) and on what they stand for (tag)"""
    x, out = zlib.crc32(tag.encode(), seed), []
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append((x >> 8) % (hi + 1))
    return out


def _i64(values):
    return np.array(values, dtype=np.int64)


class FakeCounter:
    """binding.Counter's readers over seeded values: every array has the shape and type the binding documents, the values
    derive from the name of the file that was counted, and they agree where the command line combines them"""

    def __init__(self, seqs, kwargs, assign=None):
        self.seqs, self.kw, self.assign, self.seed, self.did = seqs, kwargs, assign, None, set()
        self.n = len(seqs) if seqs is not None else 0

    def reset(self):
        self.seed, self.did = None, set()

    def close(self):
        pass

    def count_file(self, path):
        assert "start2" not in self.kw
        self.seed = zlib.crc32(os.path.basename(path).encode())
        return None, False

    def count_file_paired(self, path1, path2):
        assert "start2" in self.kw and fast2q.mate_token(path1)[0] == fast2q.mate_token(path2)[0]
        self.seed = zlib.crc32(os.path.basename(path1).encode())
        return None, False

    def _counts(self):
        return [10 + v for v in _vals(self.seed, "counts", self.n, 90)]

    def _stats(self, assigned):
        imperfect = assigned // 4
        unaligned, failed = _vals(self.seed, "stats", 2, 40)
        return _i64([assigned + unaligned + failed, assigned - imperfect, imperfect, unaligned, failed])

    def _ec(self):
        """[(key, reads, first read)]: the first four keys and a seeded choice of the others, in first-read order"""
        keep = [True] * 4 + [v == 1 for v in _vals(self.seed, "ec_keep", len(EC_KEYS) - 4, 1)]
        keys = [k for k, on in zip(EC_KEYS, keep) if on]
        order = sorted(range(len(keys)), key=lambda i: _vals(self.seed, "ec_order", len(keys), 1000)[i] * 10 + i)
        reads = [3 + v for v in _vals(self.seed, "ec_reads", len(keys), 60)]
        return [(keys[i], reads[i], 5 * at) for at, i in enumerate(order)]

    def read_counts(self):
        if self.seqs is None:
            return _i64([]), self._stats(sum(n for _, n, _ in self._ec()))
        return _i64(self._counts()), self._stats(sum(self._counts()))

    def ec_results(self):
        assert self.seqs is None
        return self._ec()

    def _assigned(self):
        rows = []
        for (key, n, first), f in zip(self._ec(), _vals(self.seed, "as_feature", len(EC_KEYS), len(self.assign))):
            f -= 1                                                  # -1: assigned to no feature
            rows.append((key, n, first, f, -1 if f < 0 else (n + f) % 2))
        return rows

    def ec_assign(self):
        assert self.assign is not None
        self.did.add("ec_assign")
        counts = [0] * len(self.assign)
        for _, n, _, f, _ in self._assigned():
            if f >= 0:
                counts[f] += n
        return _i64(counts), self._stats(sum(counts))

    def ec_assigned(self):
        assert "ec_assign" in self.did
        return self._assigned()

    def _collapsed(self):
        """the second key of the sample is absorbed by its first; every other key is its own centroid"""
        ec = self._ec()
        rows = [(ec[0][0], ec[0][1], ec[0][2], ec[0][0], ec[0][1] + ec[1][1]), (ec[1][0], ec[1][1], ec[1][2], ec[0][0], 0)]
        return rows + [(key, n, first, key, n) for key, n, first in ec[2:]]

    def ec_collapse(self, dist=1, ratio=5):
        assert self.seqs is None and dist == 1 and 2 <= ratio <= 255
        self.did.add("ec_collapse")
        ec = self._ec()
        return dict(zip(binding.Counter.ECC_EXTRA, (len(ec) - ratio % 2, 1, ec[1][1], 1)))

    def ec_collapsed(self):
        assert "ec_collapse" in self.did
        return self._collapsed()

    def _has_umi(self):
        return any(self.kw.get(k) for k in ("umi", "umi_paired", "umi_header"))

    def _umis(self):
        return [1 + v % c for v, c in zip(_vals(self.seed, "umis", self.n, 1000), self._counts())]

    def read_umis(self):
        assert self._has_umi()
        failed = _vals(self.seed, "umi_failed", 1, 9)[0]
        return _i64(self._umis()), sum(self._counts()) - failed, failed

    def collapse_umis(self, dist=1, rule="cluster"):
        assert self._has_umi() and dist == 1 and rule == "cluster"
        molecules = [1 + v % u for v, u in zip(_vals(self.seed, "molecules", self.n, 1000), self._umis())]
        return _i64(molecules), sum(self._umis()), sum(self._umis()) - sum(molecules)

    def collapse_umis_directional(self):
        assert self._has_umi() and self.kw.get("umi_reads")
        molecules = [1 + v % u for v, u in zip(_vals(self.seed, "directional", self.n, 1000), self._umis())]
        absorbed = sum(self._umis()) - sum(molecules)
        return _i64(molecules), sum(self._umis()), absorbed + 2, absorbed, sum(self._counts())

    def umi_pairs(self):
        assert self._has_umi() and self.kw.get("umi_reads")
        rows = sorted({(f, c) for f, c in zip(_vals(self.seed, "pair_feature", 8, self.n - 1), _vals(self.seed, "pair_codes", 8, 0xFFFF))})
        reads = [1 + v for v in _vals(self.seed, "pair_reads", len(rows), 20)]
        return tuple(np.array(col, dtype=np.uint32) for col in ([f for f, _ in rows], [c for _, c in rows], reads))

    def read_demux(self):
        start, barcodes = self.kw["sample_barcodes"]
        rows = len(barcodes) + 1
        matrix = [_vals(self.seed, f"demux{b}", self.n, 30) for b in range(rows)]
        sstats = []
        for b in range(rows):
            imperfect, unaligned, failed = _vals(self.seed, f"demux_stats{b}", 3, 7)
            imperfect = min(imperfect, sum(matrix[b]))
            sstats.append([sum(matrix[b]) + unaligned + failed, sum(matrix[b]) - imperfect, imperfect, unaligned, failed])
        return np.array(matrix, dtype=np.int64).reshape(rows, self.n), _i64(sstats), _i64(_vals(self.seed, "verdicts", 5, 200))

    def read_strands(self):
        assert self.kw["strand"] in ("rev", "both")
        rev = [c // 3 for c in self._counts()]
        return _i64(rev), _i64([sum(self._counts()) - sum(rev), sum(rev) - sum(rev) // 5, sum(rev) // 5, sum(rev) + 17])

    def read_stagger(self):
        n = self.kw["stagger"] + 1
        return _i64(_vals(self.seed, "stagger_perfect", n, 80)), _i64(_vals(self.seed, "stagger_imperfect", n, 20))

    def read_indels(self):
        assert self.kw["indel"] is True
        length = self.kw["length"]
        dels, inss = _vals(self.seed, "dels", self.n, 12), _vals(self.seed, "inss", self.n, 12)
        del_pos, ins_pos = _vals(self.seed, "del_pos", length, 5), _vals(self.seed, "ins_pos", length, 5)
        return _i64(dels), _i64(inss), _i64(del_pos), _i64(ins_pos), _i64([sum(dels) + sum(inss) + 9, sum(dels), sum(inss), 3])

    def _recombinants(self):
        firsts, seconds = fast2q.part_libraries(self.seqs)
        free = [(a, b) for a in range(len(firsts)) for b in range(len(seconds))
                if firsts[a] + ":" + seconds[b] not in self.seqs]
        return [(a, b, n) for (a, b), n in zip(free, _vals(self.seed, "recombinants", len(free), 3)) if n]

    def read_parts(self):
        assert self.kw["parts"] is True
        firsts, seconds = fast2q.part_libraries(self.seqs)
        counts = [c + v for c, v in zip(self._counts(), _vals(self.seed, "parts_counts", self.n, 4))]
        classes = [sum(counts) - sum(counts) // 6, sum(counts) // 6, sum(n for _, _, n in self._recombinants())] + _vals(self.seed, "classes", 3, 25)
        return (_i64(counts), _i64(_vals(self.seed, "part1", len(firsts), 99)), _i64(_vals(self.seed, "part2", len(seconds), 99)), _i64(classes))

    def parts_recombinants(self):
        return tuple(np.array([row[k] for row in self._recombinants()], dtype=np.uint32) for k in range(3))


def write_inputs(name, naming):
    """the two samples (four files for a paired run), the library and the sample barcodes, under the current directory"""
    os.mkdir("in")
    stems = ("s2_R1", "s2_R2", "s10_R1", "s10_R2") if "--pe" in FLAGS[name] else ("s2", "s10")
    for k, stem in enumerate(stems):                                # (sizes differ: the samples are met smallest first)
        with open(os.path.join("in", stem + ".fastq"), "w") as out:
            out.write("@r\nACGT\n+\nIIII\n" * (k + 1))
    seqs = [PART1[a] + ":" + PART2[b] for a, b in PAIRS] if "--parts" in FLAGS[name] else SEQS
    with open("lib.csv", "w") as out:
        out.writelines(f"{n},{s}\n" for n, s in zip(NAMES[naming], seqs))
    with open("sb.csv", "w") as out:
        out.write("x,ACGT\ny,TTTT\nw,GGCC\n")


def run_cli(name, naming, keep, monkeypatch):
    """one run of main() in the current directory: {"files": names under the output directory, "csv": {name: text},
    "headers": run_headers(param)}"""
    write_inputs(name, naming)
    seen = {}
    real_compiling = fast2q.compiling

    def compiling(param):
        seen["headers"] = fast2q.run_headers(param)
        real_compiling(param)

    monkeypatch.setattr(fast2q, "_context_for", lambda seqs, kwargs, assign=None: FakeCounter(seqs, kwargs, assign))
    monkeypatch.setattr(fast2q, "compiling", compiling)
    monkeypatch.setattr(fast2q.time, "perf_counter", _Clock([0.5249, 61.8, 3700.0, 12.0]))
    monkeypatch.setitem(sys.modules, "matplotlib", None)            # the plots are skipped: only the .csv files are compared
    argv = ["-c", "--s", "in", "--o", "out", "--cp", "1"] + FLAGS[name] + (["--k"] if keep else [])
    if name not in ("plain_ec", "ec_collapse"):
        argv += ["--g", "lib.csv"]
    fast2q.main(argv)
    (directory,) = glob.glob(os.path.join("out", "2FAST2Q_output_*"))
    files = sorted(os.listdir(directory))
    assert not [f for f in files if f.endswith(".png")]
    csvs = {}
    for f in files:
        with open(os.path.join(directory, f), "rb") as handle:
            csvs[f] = handle.read().decode("latin-1")
    return {"files": files, "csv": csvs, "headers": seen["headers"]}


def _golden():
    with open(GOLDEN_FILE) as handle:
        return json.load(handle)


def test_the_golden_file_holds_these_runs_and_no_others():
    assert sorted(_golden()) == sorted(run_id(*run) for run in RUNS)


@pytest.mark.parametrize("name,naming,keep", RUNS, ids=[run_id(*run) for run in RUNS])
def test_report_files(name, naming, keep, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    got = run_cli(name, naming, keep, monkeypatch)
    want = _golden()[run_id(name, naming, keep)]
    assert got["files"] == want["files"]
    assert got["headers"] == want["headers"]
    for f in want["files"]:
        assert got["csv"][f] == want["csv"][f], f
    capsys.readouterr()
