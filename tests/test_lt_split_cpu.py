"""k_count_fixed4_lds decides a read in two stages: an exact stage on table 0 alone for every read, then the full --m 1
decision (lt_probe + lt_decide) on a compacted batch of the reads that need it.  tests/emu/lt_split.cpp runs the
stages' device helpers (f2q_device.h) on the host; these tests check them read by read against the one-stage decision
(lt_decide on every read), and the compaction's lane bookkeeping against every candidate count a tile can have."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import synth

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "lt_split.cpp")
LIB = os.path.join(HERE, "emu", "liblt_split.so")
CSRC = os.path.join(os.path.dirname(HERE), "2fast2q_amd", "csrc")

_L = None


def lib():
    global _L
    if _L is None:
        deps = [SRC] + [os.path.join(CSRC, f) for f in ("f2q_device.h", "f2q_host.h")]
        if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-o", LIB + ".tmp", SRC, "-lz", "-lpthread"])
            os.replace(LIB + ".tmp", LIB)
        L = C.CDLL(LIB)
        P = np.ctypeslib.ndpointer
        L.lts_feature_keys.argtypes = [C.c_char_p, P(np.uint32), C.c_uint32, P(np.uint64)]
        L.lts_check.restype = C.c_int
        L.lts_check.argtypes = [C.c_char_p, P(np.uint32), C.c_uint32, C.c_int, C.c_int, P(np.uint64), P(np.uint32),
                                P(np.uint8), C.c_uint32, P(np.uint64)]
        L.lts_compact.restype = C.c_int
        L.lts_compact.argtypes = [P(np.uint8)]
        _L = L
    return _L


def library(n, glen, seed, n_twins):
    """random guides plus one-substitution twins of the first n_twins (ambiguous nearest neighbours)"""
    guides = synth.make_library(n, glen, seed)
    twins = []
    for i, g in enumerate(guides[:n_twins]):
        p = (i * 7) % glen
        twins.append(g[:p] + "ACGT"[("ACGT".index(g[p]) + 1 + i % 3) % 4] + g[p + 1:])
    return list(dict.fromkeys(guides + twins))


def substitute(rng, keys, glen, n_sub):
    """keys with n_sub distinct bases changed to another base"""
    keys = keys.copy()
    for i in range(len(keys)):
        for p in rng.choice(glen, size=n_sub, replace=False):
            keys[i] ^= np.uint64(int(rng.integers(1, 4)) << (2 * int(p)))
    return keys


@pytest.mark.parametrize("near", [1, 0], ids=["m1", "m0"])
@pytest.mark.parametrize("glen,n_guides", [(20, 10000), (21, 13000), (14, 600), (17, 4000), (19, 8000), (16, 3000)])
def test_two_stages_match_lt_decide(near, glen, n_guides):
    L = lib()
    feats = library(n_guides, glen, 977 * glen + n_guides, 400)
    seqs = "".join(feats).encode()
    offs = np.array([0] + list(np.cumsum([len(f) for f in feats])), dtype=np.uint32)
    fk = np.zeros(len(feats), dtype=np.uint64)
    L.lts_feature_keys(seqs, offs, len(feats), fk)
    rng = np.random.default_rng(glen * 1000 + n_guides + near)
    n = 60000
    pick = fk[rng.integers(0, len(fk), size=n)]
    kind = rng.integers(0, 5, size=n)
    keys = np.where(kind == 0, pick,
           np.where(kind == 1, substitute(rng, pick, glen, 1),
           np.where(kind == 2, substitute(rng, pick, glen, 2),
           np.where(kind == 3, rng.integers(0, 1 << (2 * glen), size=n, dtype=np.uint64), substitute(rng, pick, glen, 1)))))
    # flagged bases: none for most reads, one or two for some (a flagged base keeps whatever its key bits say)
    forced = np.zeros(n, dtype=np.uint32)
    nf = rng.choice(3, size=n, p=[0.8, 0.14, 0.06])
    for i in np.nonzero(nf)[0]:
        for p in rng.choice(glen, size=int(nf[i]), replace=False):
            forced[i] |= np.uint32(1 << int(p))
    cand = (rng.random(n) < 0.9).astype(np.uint8)          # the rest: dead slots, Phred failures, clipped windows
    out = np.zeros(4, dtype=np.uint64)
    assert L.lts_check(seqs, offs, len(feats), glen, near, keys, forced, cand, n, out) == 0
    perfect, imperfect, batch, bad = (int(v) for v in out)
    assert bad == 0
    assert perfect > 0.1 * n and batch > 0.3 * n
    assert (imperfect > 0.05 * n) if near else imperfect == 0


@pytest.mark.parametrize("n_cand", [0, 1, 36, 63, 64, 65, 128, 200, 256])
def test_compaction_places_every_candidate_once(n_cand):
    L = lib()
    rng = np.random.default_rng(n_cand)
    for trial in range(40):
        b = np.zeros(256, dtype=np.uint8)
        if trial % 4 == 0:
            b[:n_cand] = 1                                      # the lowest lanes of slot 0 first, then slot 1, ...
            b = b.reshape(4, 64).T.reshape(-1).copy()
        else:
            b[rng.choice(256, size=n_cand, replace=False)] = 1
        assert L.lts_compact(b) == n_cand
