"""CPU-side checks of the boundary: the shared library loads and exports every symbol that
include/f2q.h declares (no compute calls), the ctypes structs match the C layout, the product has
no CPU fallback, and the host harness reproduces the reference's file formats."""
import csv
import importlib
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, pkg

binding = importlib.import_module("2fast2q_amd.binding")
fast2q = importlib.import_module("2fast2q_amd.fast2q")


def header_functions():
    text = open(os.path.join(ROOT, "include", "f2q.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(f2q_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    L = binding.load()
    declared = header_functions()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/f2q.h but not exported"
    assert sorted(binding.EXPORTS) == declared
    assert L.f2q_version() == 1
    # the binary on disk is the tree's: its baked-in source hash equals the hash of csrc/ + include/f2q.h now
    assert binding.build_id() == g.source_id()


def test_bgzf_pieces_and_census_on_the_host(tmp_path):
    """f2q_file_pieces / f2q_census_pieces need no device: a BGZF file is cut into runs of whole members from the text
    sizes in the member trailers, and the census of all runs adds up to the newlines of the text"""
    import ctypes as C
    import gzip
    import numpy as np
    from conftest import bgzf_bytes
    import __graft_entry__ as g
    g.build()
    L = binding.load()
    text = b"".join(b"@r%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % i for i in range(30000))
    path = tmp_path / "x.fastq.gz"
    path.write_bytes(bgzf_bytes(text[:400000], block=5000, eof_marker=True) + bgzf_bytes(text[400000:], block=0xFF00))
    for piece in (4096, 100000, 1 << 22):
        n, ok = C.c_uint64(), C.c_int()
        assert L.f2q_file_pieces(os.fsencode(str(path)), piece, C.byref(n), C.byref(ok)) == 0
        assert ok.value == 2 and n.value >= 1
        total = np.zeros(2 * n.value, dtype=np.uint64)
        for world in (1, 3):
            total[:] = 0
            for rank in range(world):
                cen = np.zeros(2 * n.value, dtype=np.uint64)
                assert L.f2q_census_pieces(os.fsencode(str(path)), rank, world, piece, cen.ctypes.data_as(C.POINTER(C.c_uint64)), n.value) == 0
                total += cen
            assert int(total[0::2].sum()) == text.count(b"\n")
    plain = tmp_path / "x.fastq"; plain.write_bytes(text)
    n, ok = C.c_uint64(), C.c_int()
    assert L.f2q_file_pieces(os.fsencode(str(plain)), 1 << 16, C.byref(n), C.byref(ok)) == 0 and ok.value == 1
    other = tmp_path / "y.fastq.gz"; other.write_bytes(gzip.compress(text))
    assert L.f2q_file_pieces(os.fsencode(str(other)), 1 << 16, C.byref(n), C.byref(ok)) == 0 and ok.value == 0 and n.value == 0


def test_bgzf_pieces_follow_the_member_text_sizes(tmp_path):
    """the cut of a BGZF file into pieces is the one the ISIZE fields give by the rule "a new piece when adding the member
    would exceed piece_bytes": about 40 members, some runs filling a piece exactly, two empty members in a row in the
    middle and the EOF marker at the end; and the census of every rank's pieces adds up to the newlines of the text"""
    import ctypes as C
    import struct
    import numpy as np
    from conftest import bgzf_bytes
    import __graft_entry__ as g
    g.build()
    L = binding.load()
    piece = 65536
    text = b"".join(b"@r%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % i for i in range(22000))
    cut = 20 * 16384                                   # four members of 16384 bytes fill a piece to the byte
    data = bgzf_bytes(text[:cut], block=16384) + bgzf_bytes(b"") + bgzf_bytes(text[cut:], block=20480)
    isize, pos = [], 0
    while pos < len(data):                             # (bgzf_bytes: BSIZE - 1 at offset 16 of a member, ISIZE in its last 4 bytes)
        bsize = struct.unpack_from("<H", data, pos + 16)[0] + 1
        isize.append(struct.unpack_from("<I", data, pos + bsize - 4)[0])
        pos += bsize
    assert 38 <= len(isize) <= 42 and isize[-1] == 0 and (0, 0) in zip(isize, isize[1:-1]) and sum(isize) == len(text)
    expect, acc = 0, 0
    for s in isize:
        if expect == 0 or acc + s > piece:
            expect, acc = expect + 1, 0
        acc += s
    path = tmp_path / "x.fastq.gz"
    path.write_bytes(data)
    for world in (1, 3):
        n, ok = C.c_uint64(), C.c_int()
        assert L.f2q_file_pieces(os.fsencode(str(path)), piece, C.byref(n), C.byref(ok)) == 0
        assert ok.value == 2 and n.value == expect
        total = np.zeros(2 * n.value, dtype=np.uint64)
        for rank in range(world):
            cen = np.zeros(2 * n.value, dtype=np.uint64)
            assert L.f2q_census_pieces(os.fsencode(str(path)), rank, world, piece, cen.ctypes.data_as(C.POINTER(C.c_uint64)), n.value) == 0
            total += cen
        assert int(total[0::2].sum()) == text.count(b"\n")


def test_build_sees_every_source_file():
    import __graft_entry__ as g
    deps = {os.path.basename(d) for d in g.hip_deps()}
    on_disk = {f for f in os.listdir(os.path.join(ROOT, "2fast2q_amd", "csrc")) if f.endswith((".h", ".hip"))}
    assert on_disk <= deps and "f2q.h" in deps
    # every header the translation unit includes (directly or not) is a dependency
    for f in on_disk:
        for inc in re.findall(r'#include\s+"([^"]+)"', open(os.path.join(ROOT, "2fast2q_amd", "csrc", f)).read()):
            assert os.path.basename(inc) in deps, (f, inc)


def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "f2q.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(f2q_params),offsetof(f2q_params,upstream),offsetof(f2q_params,device),sizeof(f2q_synth),'
                   'offsetof(f2q_synth,t_sub),sizeof(f2q_timing));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    import ctypes as C
    want = [C.sizeof(binding.Params), binding.Params.upstream.offset, binding.Params.device.offset,
            C.sizeof(binding.Synth), binding.Synth.t_sub.offset, C.sizeof(binding.Timing)]
    assert got == want


def test_no_cpu_fallback_without_gpu():
    # asked in a child process: torch brings its own HIP runtime, and initialising it here, after the product's library
    # has been loaded, would leave the product's runtime without a device for the GPU tests later in this session
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], stdout=subprocess.PIPE,
                           text=True, timeout=240, check=True)
    if probe.stdout.strip().splitlines()[-1] == "True":
        pytest.skip("GPU present")
    with pytest.raises(binding.F2QError) as e:
        binding.Counter(features=["ACGT"], length=4)
    assert e.value.code == -2                     # F2Q_ENODEVICE: the product fails loudly


def test_product_does_not_touch_the_oracle():
    # the oracle is a checker only: nothing under 2fast2q_amd/ may import, load or link it
    bad = re.compile(r"(import\s+oracle|from\s+oracle|libf2q_oracle|oracle/|f2q_oracle|emu_helper|libf2q_emu)")
    for dirpath, _, files in os.walk(os.path.join(ROOT, "2fast2q_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not bad.search(text), f


def test_features_loader_d39v(capsys):
    feats = fast2q.features_loader(os.path.join(ROOT, "2fast2q_amd", "data", "D39V_guides.csv"))
    assert len(feats) == 1498                                     # sgRNA0867 duplicates sgRNA0850
    names = [f.name for f in feats.values()]
    assert "sgRNA0850" in names and "sgRNA0867" not in names
    assert all(set(s) <= set("ACGT") and len(s) == 20 for s in feats)       # row 81's trailing blank is gone
    assert "share the same sequence" in capsys.readouterr().out


def test_features_loader_separators(tmp_path):
    for sep in (",", ";", "\t"):
        p = tmp_path / "f.csv"
        p.write_text(f"a{sep}acgt \nb{sep}AC GT\nc{sep}TTTT\n")
        feats = fast2q.features_loader(str(p))
        assert list(feats) == ["ACGT", "TTTT"] and feats["ACGT"].name == "a"


def test_input_parser_defaults_and_flags():
    p = fast2q.input_parser(["-c", "--s", "/x", "--g", "/g.csv", "--o", "/o"])
    assert (p["length"], p["start"], p["phred"], p["miss"], p["Running Mode"]) == (20, "0", 30, 1, "C")
    assert (p["miss_search_up"], p["miss_search_down"], p["qual_up"], p["qual_down"]) == (0, 0, 30, 30)
    assert p["upstream"] is None and p["downstream"] is None and p["delete"] and p["Progress bar"]
    p = fast2q.input_parser(["-c", "--s", "/x", "--o", "/o", "--mo", "ec", "--us", "ACGT", "--ds", "TTTT", "--msu", "1",
                             "--msd", "2", "--qsu", "20", "--qsd", "10", "--m", "2", "--ph", "25", "--l", "15",
                             "--st", "3,9", "--k", "--pb", "--fn", "out", "--cp", "4", "--fs"])
    assert p["Running Mode"] == "EC" and p["upstream"] == "ACGT" and p["downstream"] == "TTTT"
    assert (p["miss_search_up"], p["miss_search_down"], p["qual_up"], p["qual_down"]) == (1, 2, 20, 10)
    assert (p["miss"], p["phred"], p["length"], p["start"]) == (2, 25, 15, "3,9")
    assert not p["delete"] and not p["Progress bar"] and p["out_file_name"] == "out" and p["cpu"] == 4
    assert fast2q.input_parser([]) is None


def _sentence(name, reads, perfect, imperfect, non_aligned, qfail, timing="0.5 seconds"):
    return (f"#script ran in {timing} for file {name}. {perfect + imperfect} reads out of {reads} were aligned. "
            f"{perfect} were perfectly aligned. {imperfect} were aligned with mismatch. {non_aligned} passed quality "
            f"filtering but were not aligned. {qfail} did not pass quality filtering.")


def test_compiling_formats(tmp_path):
    d = tmp_path / "out"
    d.mkdir()
    fast2q.csv_writer(str(d / "s1_reads.csv"), [[_sentence("s1", 10, 5, 2, 2, 1)], ["#Feature", "Reads"], ["g1", 4], ["g2", 3]])
    fast2q.csv_writer(str(d / "s2_reads.csv"), [[_sentence("s2", 20, 9, 1, 6, 4)], ["#Feature", "Reads"], ["g1", 7], ["g3", 3]])
    param = dict(directory=str(d), version="x", miss=1, phred=30, length=20, start="0", upstream=None, downstream=None,
                 miss_search_up=0, miss_search_down=0, qual_up=30, qual_down=30, out_file_name="compiled", delete=True,
                 test_mode=False, used_cmd="--c")
    param["Running Mode"] = "C"
    fast2q.compiling(param)
    files = sorted(os.listdir(d))
    assert files == ["compiled.csv", "compiled_distribution_normalized_RPM_plot.png", "compiled_distribution_plot.png",
                     "compiled_reads_plot.png", "compiled_reads_plot_percentage.png", "compiled_stats.csv"]   # 6 files
    raw = (d / "compiled.csv").read_bytes()
    assert raw == b"#Feature,s1,s2\r\ng1,4,7\r\ng2,3,0\r\ng3,0,3\r\n"       # CRLF, zero back-fill, first-file order
    rows = list(csv.reader(open(d / "compiled_stats.csv")))
    assert rows[-2] == ["s1", "0.5", "seconds", "10", "7", "5", "2", "2", "1"]
    assert rows[-1] == ["s2", "0.5", "seconds", "20", "10", "9", "1", "6", "4"]
    assert rows[-3][0] == "#Sample name" and any("#Mismatch: 1" in r[0] for r in rows)


def _golden_compiling_cases():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "compiling_cases.json")) as f:
        d = json.load(f)
    return d["cases"], d["elapsed"]


class _Clock:
    """the scripted perf_counter tests/golden/make_golden_compiling.py gave the reference"""

    def __init__(self, elapsed):
        self.t, self.k, self.started, self.elapsed = 100.0, 0, False, elapsed

    def __call__(self):
        if not self.started:
            self.started = True
            return self.t
        self.started = False
        self.t += self.elapsed[self.k % len(self.elapsed)]
        self.k += 1
        return self.t


def golden_param(case, directory, keep=False):
    p = {"cmd": True, "big_file_split": False, "test_mode": False, "out_file_name": "compiled", "length": 20,
         "Progress bar": True, "start": "0", "phred": 30, "miss": 1, "upstream": None, "downstream": None,
         "miss_search_up": 0, "miss_search_down": 0, "qual_up": 30, "qual_down": 30, "Running Mode": "C",
         "delete": not keep, "cpu": 1}
    p.update(case["params"])
    p["version"] = case["expected"]["version"]
    p["directory"] = str(directory)
    return p


@pytest.mark.parametrize("keep", [False, True], ids=["in_memory", "keep_temporaries"])
@pytest.mark.parametrize("case", _golden_compiling_cases()[0], ids=[c["name"] for c in _golden_compiling_cases()[0]])
def test_output_contract_vs_reference(case, keep, tmp_path, monkeypatch):
    """aligner() -> compiling() of the harness against the bytes the REFERENCE's aligner/compiling/run_stats wrote for
    the same samples (tests/golden/compiling_cases.json): compiled.csv and compiled_stats.csv byte for byte, sample
    order, numeric vs alphabetical row order, zero back-fill, and -- with --k -- the <sample>_reads.csv files.
    The counting aligner() calls (_count_sample: reads_counter's three values, then what the options read) is replaced by
    the reference's own per-sample result here (no GPU); tests/test_gpu_cli.py runs the same cases through the device."""
    exp = case["expected"]
    by_file = {s["file"]: s["rows"] for s in exp["samples"]}
    stats_rows = {r[0]: r for r in csv.reader(exp["compiled_stats.csv"].splitlines()) if len(r) == 9 and not r[0].startswith("#")}

    def fake_count_sample(i, raw, features, param, reads_stats, preprocess=False):
        name = fast2q._sample_name(raw)
        r = stats_rows[name]
        for fname, seq, n in by_file[os.path.basename(raw)]:
            if seq in features:
                features[seq].counts += n
            else:
                features[seq] = fast2q.Features(fname, n)
        local = dict(zip(binding.STAT_NAMES, (int(r[3]), int(r[5]), int(r[6]), int(r[7]), int(r[8]))))
        return features, reads_stats, local, {}

    monkeypatch.setattr(fast2q, "_count_sample", fake_count_sample)
    monkeypatch.setattr(fast2q.time, "perf_counter", _Clock(_golden_compiling_cases()[1]))
    param = golden_param(case, tmp_path, keep)
    lib = {}
    if case["features"] is not None:
        for name, seq in case["features"]:
            lib.setdefault(seq.upper().replace(" ", ""), name)
    for i, (fname, _) in enumerate(case["files"]):
        per_sample = {s: fast2q.Features(n, 0) for s, n in lib.items()}
        fast2q.aligner(i, str(tmp_path / "in" / fname), per_sample, param, {})
    if keep:
        for f, text in exp["reads_csv"].items():
            assert (tmp_path / f).read_bytes().decode("latin-1") == text
    else:
        assert not [f for f in os.listdir(tmp_path) if f.endswith("_reads.csv")]      # no temporary files at all
    fast2q.compiling(param)
    assert (tmp_path / "compiled.csv").read_bytes().decode("latin-1") == exp["compiled.csv"]
    assert (tmp_path / "compiled_stats.csv").read_bytes().decode("latin-1") == exp["compiled_stats.csv"]
    left = sorted(os.listdir(tmp_path))
    assert left == (sorted(exp["files_left"] + list(exp["reads_csv"])) if keep else exp["files_left"])


def test_compiling_reads_a_directory_of_reads_csv(tmp_path):
    """without in-memory results compiling() takes the <sample>_reads.csv files of the directory -- e.g. the ones the
    reference itself wrote -- and produces the reference's bytes from them"""
    case = _golden_compiling_cases()[0][2]                       # Extract+Count, different key sets per sample
    for f, text in case["expected"]["reads_csv"].items():
        (tmp_path / f).write_bytes(text.encode("latin-1"))
    fast2q.compiling(golden_param(case, tmp_path))
    assert (tmp_path / "compiled.csv").read_bytes().decode("latin-1") == case["expected"]["compiled.csv"]
    assert (tmp_path / "compiled_stats.csv").read_bytes().decode("latin-1") == case["expected"]["compiled_stats.csv"]
    assert sorted(os.listdir(tmp_path)) == case["expected"]["files_left"]


def test_reference_golden_compiled_format():
    # the reference's own tests/compiled.csv pins the format only (its FASTQ is not redistributed):
    # header '#Feature,<sample>' then one 'name,count' row per unique feature, in library order.
    # Stored verbatim as tests/golden/reference_compiled.csv.
    ref = os.path.join(ROOT, "tests", "golden", "reference_compiled.csv")
    rows = list(csv.reader(open(ref)))
    feats = fast2q.features_loader(os.path.join(ROOT, "2fast2q_amd", "data", "D39V_guides.csv"))
    assert rows[0] == ["#Feature", "example"]
    assert [r[0] for r in rows[1:]] == sorted(f.name for f in feats.values())
    assert sum(int(r[1]) for r in rows[1:]) == 60916
