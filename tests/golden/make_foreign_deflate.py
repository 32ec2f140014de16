#!/usr/bin/env python3
"""Writes tests/golden/foreign_deflate.json: raw deflate members from an encoder other than zlib's, for
tests/deflate_craft.py (family `foreign`).  The encoder is libdeflate (what bgzip / htslib link), loaded with ctypes
from the system's libdeflate.so.0; a machine without it gets a message and no file.  The tests read the fixture only.

  python tests/golden/make_foreign_deflate.py

Levels 1, 6, 9, 12 on six texts.  A member is the deflate payload plus the gzip trailer (CRC-32, ISIZE), base64; equal
members (libdeflate stores random bytes the same way at every level) are kept once under all their names.  Each row
carries the SHA-256 of its text; zlib has decoded every member to that text before it is written."""
import base64
import ctypes
import hashlib
import json
import os
import random
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import inflate_cases as IC   # noqa: E402
import synth                 # noqa: E402

OUT = os.path.join(HERE, "foreign_deflate.json")
LEVELS = (1, 6, 9, 12)


def texts():
    fq = synth.make_fastq(synth.Spec(seed=9, n_reads=1500, read_len=151), synth.make_library(120, 20, 47))
    rng = random.Random(5)
    return {"fastq65280": fq[:65280], "fastq30011": fq[:30011], "random40000": bytes(rng.getrandbits(8) for _ in range(40000)),
            "A65280": b"A" * 65280, "one_byte": fq[:1], "empty": b""}


def main():
    try:
        ld = ctypes.CDLL("libdeflate.so.0")
    except OSError as e:
        print(f"no libdeflate.so.0 on this machine ({e}): nothing written")
        return 1
    ld.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    ld.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    ld.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    ld.libdeflate_deflate_compress.restype = ctypes.c_size_t
    ld.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    rows = {}
    for lv in LEVELS:
        comp = ctypes.c_void_p(ld.libdeflate_alloc_compressor(lv))
        for name, t in texts().items():
            buf = ctypes.create_string_buffer(70000)
            n = ld.libdeflate_deflate_compress(comp, t, len(t), buf, 70000)
            assert n, (lv, name)
            m = buf.raw[:n] + IC.trailer(t)
            assert zlib.decompress(m[:-8], -15) == t and len(m) + 22 <= 65536
            row = rows.setdefault(m, {"names": [], "sha256": hashlib.sha256(t).hexdigest(), "member": base64.b64encode(m).decode()})
            row["names"].append(f"libdeflate{lv}_{name}")
        ld.libdeflate_free_compressor(comp)
    doc = {"encoder": "libdeflate (libdeflate.so.0), libdeflate_deflate_compress", "levels": list(LEVELS), "members": list(rows.values())}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"{OUT}: {len(rows)} members under {sum(len(r['names']) for r in rows.values())} names, {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
