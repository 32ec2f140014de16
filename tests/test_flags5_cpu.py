"""fixed4_flags_whole5, the flag gather k_count_fixed4_lds<5, 2, ., true> uses (one byte-wise dot product per quality
row), against the general fixed4_flags on random rows: sparse flags, dense flags, every single byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "flags5.cpp")
LIB = os.path.join(HERE, "emu", "libflags5.so")
CSRC = os.path.join(os.path.dirname(HERE), "2fast2q_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    deps = [SRC, os.path.join(CSRC, "f2q_device.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-o", LIB + ".tmp", SRC])
        os.replace(LIB + ".tmp", LIB)
    lib = C.CDLL(LIB)
    lib.fl5_check.restype = C.c_int
    lib.fl5_check.argtypes = [np.ctypeslib.ndpointer(np.uint32), C.c_uint32, C.c_int]
    return lib


@pytest.mark.parametrize("st", [0, 16, 48])
@pytest.mark.parametrize("p_flag", [0.02, 0.5, 1.0])
def test_whole5_equals_general_gather(L, st, p_flag):
    rng = np.random.default_rng(st + int(100 * p_flag))
    n = 4000
    q = rng.integers(0, 128, size=(n, 20, 4), dtype=np.uint32)                   # quality bytes, bit 7 clear
    q |= (rng.random((n, 20, 4)) < p_flag).astype(np.uint32) << 7              # the non-ACGT flag
    words = (q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | (q[..., 3] << 24)).astype(np.uint32)
    assert L.fl5_check(np.ascontiguousarray(words.reshape(-1)), n, st) == 0


def test_whole5_every_single_byte(L):
    words = np.zeros((80, 20), dtype=np.uint32)                                  # lane i: one flagged byte of read i % 4
    for i in range(80):
        r, k = divmod(i // 4, 4)
        words[i, 4 * r + i % 4] = np.uint32(0x80 << (8 * k))
    assert L.fl5_check(np.ascontiguousarray(words.reshape(-1)), 80, 0) == 0
