"""CPU: the index arithmetic of the gathering network launch (csrc/lz_live_index.h, compiled for the host by
tests/live_gather_host_check.cpp) against a plain loop: row r of a launch is the r-th live game in ascending order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.live_patterns import PATTERNS, SIZES, live_pattern

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "live_gather_host_check.cpp")
LIB = os.path.join(HERE, "_build", "liblz_live_hostcheck.so")


@pytest.fixture(scope="module")
def hc():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    deps = [SRC, os.path.join(HERE, "..", "liuzhou_amd", "csrc", "lz_live_index.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    L = C.CDLL(LIB)
    L.lzlive_rows.restype = C.c_int
    L.lzlive_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.lzlive_select_all.restype = C.c_int
    L.lzlive_select_all.argtypes = [C.c_uint64, C.c_void_p]
    return L


def plain_rows(live):
    rows = []
    for g in range(len(live)):                         # the plain loop
        if live[g]:
            rows.append(g)
    return np.asarray(rows, dtype=np.int32)


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_row_to_game_equals_a_plain_loop(hc, B, pattern):
    live = live_pattern(pattern, B)
    flags = np.ascontiguousarray(live.astype(np.uint8))
    out = np.full(B, -7, dtype=np.int32)
    n = hc.lzlive_rows(flags.ctypes.data, B, out.ctypes.data)
    want = plain_rows(live)
    assert n == len(want)
    assert np.array_equal(out[:n], want)
    assert (out[n:] == -7).all()


def test_select_bit_on_single_words(hc):
    rng = np.random.default_rng(7)
    words = [0, 1, 1 << 63, (1 << 64) - 1, 0x8000000000000001, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0xFFFFFFFF00000000]
    words += [int(x) for x in rng.integers(0, 1 << 63, 64, dtype=np.uint64)]
    words += [int(x) | (1 << 63) for x in rng.integers(0, 1 << 63, 16, dtype=np.uint64)]
    for m in words:
        out = np.full(64, -1, dtype=np.int32)
        n = hc.lzlive_select_all(m, out.ctypes.data)
        want = [b for b in range(64) if (m >> b) & 1]
        assert n == len(want) and out[:n].tolist() == want
