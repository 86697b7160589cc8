"""CPU: the Gumbel variates of the per-game counter RNG.  `gumbel_draw` of liuzhou_amd/csrc/lz_rng.h, compiled for the
host, against a numpy restatement over oracle/rng_oracle.draw: the uniforms bit for bit, the variates at the rtol that
tests/test_rng_oracle.py grants the Gamma draws (two float logarithms of different libraries)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests.gumbel_tree import rng_gumbel

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gumbel_host_check.cpp")
LIB = os.path.join(HERE, "_build", "liblz_gumbel_hostcheck.so")


@pytest.fixture(scope="module")
def hc():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    deps = [SRC, os.path.join(HERE, "..", "liuzhou_amd", "csrc", "lz_rng.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB, SRC])
    return C.CDLL(LIB)


def _host(hc, seed, game, ply, count):
    B = game.shape[0]
    u, g = np.zeros((B, count), np.float32), np.zeros((B, count), np.float32)
    hc.hc_rng_gumbel(C.c_uint64(seed), C.c_void_p(game.ctypes.data), C.c_void_p(ply.ctypes.data), C.c_int64(B),
                     C.c_int64(count), C.c_void_p(u.ctypes.data), C.c_void_p(g.ctypes.data))
    return u, g


def test_header_gumbel_equals_the_restatement_and_is_slot_independent(hc):
    seed = 12345 + (7 << 32)
    game = np.array([0, 1, 2, 5, 1 << 33, 4095, 77, 77], np.int64)
    ply = np.array([0, 0, 3, 9, 1, 143, 20, 21], np.int64)
    u, g = _host(hc, seed, game, ply, 72)
    wu, wg = rng_gumbel(seed, game, ply, 72)
    assert np.array_equal(u.view(np.uint32), wu.view(np.uint32))
    assert (u > 0).all() and (u < 1).all() and np.isfinite(g).all()
    np.testing.assert_allclose(g, wg, rtol=2e-5, atol=0)
    perm = np.array([3, 0, 7, 1, 6, 2, 5, 4])
    _u2, g2 = _host(hc, seed, np.ascontiguousarray(game[perm]), np.ascontiguousarray(ply[perm]), 72)
    assert np.array_equal(g2, g[perm])
    assert not np.array_equal(g[6], g[7])          # same game, next ply: fresh variates


def test_the_stream_is_not_the_playout_caps():
    """Purpose 3, index 0 is the cap's uniform; the Gumbel variates start at index 1."""
    from oracle import rng_oracle as R
    game, ply = np.arange(16, dtype=np.int64), np.zeros(16, np.int64)
    cap = R.draw(5, game, ply, 3, 0, 0)[:, 0]
    first = R.draw(5, game, ply, 3, 1, 0)[:, 0]
    assert not np.array_equal(cap, first)
    u, _ = rng_gumbel(5, game, ply, 1)
    assert np.array_equal(u[:, 0], ((first >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23))


def test_mean_and_variance(hc):
    """1e5 draws: mean and variance within 4 standard errors of Euler's constant and pi^2 / 6 (a Gumbel's fourth central
    moment is 5.4 sigma^4, so the variance's standard error is sigma^2 sqrt(4.4 / N))."""
    game = np.arange(2000, dtype=np.int64)
    _u, g = _host(hc, 99, game, np.zeros(2000, np.int64), 50)
    x = g.astype(np.float64).reshape(-1)
    N, var = x.size, math.pi ** 2 / 6.0
    assert N == 100000
    assert abs(x.mean() - 0.5772156649) < 4.0 * math.sqrt(var / N), x.mean()
    assert abs(x.var() - var) < 4.0 * var * math.sqrt(4.4 / N), x.var()
