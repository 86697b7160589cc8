"""CPU: policy surprise weighting -- the properties of the numpy restatement (tests/policy_surprise.py), the host build of
csrc/lz_surprise.h (tests/surprise_host_check.cpp) against it, parameter validation, refusals and the counters."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import policy_surprise as PS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "surprise_host_check.cpp")
LIB = os.path.join(HERE, "_build", "liblz_surprise_hostcheck.so")
SEED = 20261019                                            # generator seed of the game grid: the oracle alone leaves out none
RUN_SEED = 0x5EED5EED12345                                 # key of the games' resampling offsets


@pytest.fixture(scope="module")
def grid():
    """(n, pattern, alpha, s, game, u) of every game of the grid."""
    return [(n, pat, a, s, game, PS.game_u(RUN_SEED, game)) for n, pat, a, s, game in PS.games(SEED)]


@pytest.fixture(scope="module")
def hc():
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    deps = [SRC] + [os.path.join(HERE, "..", "liuzhou_amd", "csrc", h) for h in ("lz_surprise.h", "lz_rng.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB, SRC])
    L = C.CDLL(LIB)
    L.lzsurprise_game_u.restype = C.c_float
    L.lzsurprise_game_u.argtypes = [C.c_uint64, C.c_int64]
    L.lzsurprise_plan.restype = C.c_int64
    L.lzsurprise_plan.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    L.lzsurprise_row.restype = C.c_double
    L.lzsurprise_row.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.lzsurprise_weight.restype = C.c_double
    L.lzsurprise_weight.argtypes = [C.c_double, C.c_int64, C.c_double, C.c_double]
    L.lzsurprise_count.restype = C.c_int64
    L.lzsurprise_count.argtypes = [C.c_double, C.c_double, C.c_double]
    return L


# ---- oracle properties ---------------------------------------------------------------------------------------------------
def test_grid_covers_the_issue_cases(grid):
    assert len(grid) == len(PS.LENGTHS) * len(PS.PATTERNS) * len(PS.ALPHAS) == 108
    assert all(0.0 <= float(u) < 1.0 for *_, u in grid)


def test_counts_sum_monotone_and_within_one_of_the_weight(grid):
    for n, pat, a, s, game, u in grid:
        w = PS.weights(s, a)
        c = PS.counts(s, a, u)
        src = PS.plan(s, a, u)
        assert abs(w.sum() - n) < 1e-9 * n, (n, pat, a)
        assert int(c.sum()) == n and (c >= 0).all(), (n, pat, a)
        assert len(src) == n and (np.diff(src) >= 0).all(), (n, pat, a)
        assert (np.abs(c - w) < 1.0).all(), (n, pat, a)
        # output slot k holds the j whose cumulative count first exceeds k
        cum = np.cumsum(c)
        assert all(int(src[k]) == int(np.searchsorted(cum, k, side="right")) for k in range(0, n, max(1, n // 17)))
        assert PS.rows_dropped(src) == int((c == 0).sum()) == int(np.maximum(c - 1, 0).sum())


def test_identity_without_surprise(grid):
    for n, pat, a, s, game, u in grid:
        if pat in ("zero", "uniform"):                     # S = 0, or every weight exactly 1
            assert np.array_equal(PS.plan(s, a, u), np.arange(n)), (n, pat, a)
    for n in (1, 7, 64):                                   # a sum below the flat threshold counts as none
        s = np.full(n, 1e-14, np.float32)
        assert np.array_equal(PS.weights(s, 1.0), np.ones(n))
    for n, pat, a, s, game, u in grid:                     # alpha = 0 is the identity whatever the surprises
        assert np.array_equal(PS.plan(s, 0.0, u), np.arange(n))


def test_two_pass_inplace_copy_equals_the_gather(grid):
    replaced = 0
    for n, pat, a, s, game, u in grid:
        src = PS.plan(s, a, u)
        rows = np.arange(1000, 1000 + n)
        assert np.array_equal(PS.two_pass_inplace(rows, src), rows[src]), (n, pat, a)
        replaced += PS.rows_dropped(src)
    assert replaced > 0                                    # the grid does move rows
    rng = np.random.default_rng(5)                         # and any monotone map with src[k] in range, not only planned ones
    for _ in range(200):
        n = int(rng.integers(1, 80))
        src = np.sort(rng.integers(0, n, n)).astype(np.int32)
        rows = rng.integers(0, 1 << 30, n)
        assert np.array_equal(PS.two_pass_inplace(rows, src), rows[src])


def test_mean_count_over_the_offset_grid_is_the_weight():
    """Over u = (k + 1/2) / 4096 the mean of floor(C_j + u) - floor(C_(j-1) + u) is within 2 / 4096 of w_j, on every game
    of the grid: the mean of floor(x + u) over that grid is within 1 / 4096 of x - 1/2 for every x, and a count is a
    difference of two."""
    us = (np.arange(4096) + 0.5) / 4096.0
    for n, pat, a, s, game in PS.games(SEED):
        b = np.floor(PS.cumulative(s, a)[None, :] + us[:, None])
        mean = (b[:, 1:] - b[:, :-1]).mean(axis=0)
        assert (np.abs(mean - PS.weights(s, a)) <= 2.0 / 4096).all(), (n, pat, a)


def test_surprise_of_a_row():
    rng = np.random.default_rng(3)
    legal = rng.random(220) < 0.3
    legal[5] = True
    pi = (rng.random(220) * legal).astype(np.float32)
    pi /= pi.sum()
    assert PS.surprise(legal, pi, pi) == 0.0               # KL(pi || pi)
    p = np.full(220, 1.0 / 220, np.float32)
    want = float(np.sum(pi[pi > 0].astype(np.float64) * np.log(pi[pi > 0].astype(np.float64) * 220.0)))
    assert abs(PS.surprise(legal, pi, p) - want) < 1e-6    # float32(1 / 220) is not exactly 1 / 220
    one = np.zeros(220, np.float32)
    one[5] = 1.0
    assert abs(PS.surprise(legal, one, np.zeros(220, np.float32)) - 30.0 * math.log(10.0)) < 1e-9     # the clamp
    assert PS.surprise(np.zeros(220, bool), one, p) == 0.0                                            # nothing legal


# ---- the host build of the header ----------------------------------------------------------------------------------------
def test_host_u_equals_the_oracle_bit_for_bit(hc):
    from oracle import rng_oracle
    for seed in (0, 1, RUN_SEED, (1 << 64) - 1):
        games = np.concatenate([np.arange(0, 200), np.asarray([1 << 31, (1 << 32) + 7, (1 << 40) + 1])]).astype(np.int64)
        want = rng_oracle.u01(rng_oracle.draw(seed, games, 0, 3, 1022, 0)[:, 0])
        got = np.asarray([hc.lzsurprise_game_u(seed, int(g)) for g in games], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert PS.game_u(seed, 5).view(np.uint32) == want[5].view(np.uint32)


def test_host_plan_equals_the_oracle(hc, grid):
    left_out = 0
    for n, pat, a, s, game, u in grid:
        if PS.near_integer(s, a, u):
            left_out += 1
            continue
        src = np.full(n + 2, -7, np.int32)
        total = C.c_double(-1.0)
        dropped = hc.lzsurprise_plan(np.ascontiguousarray(s).ctypes.data, n, a, float(u), src[1:].ctypes.data, C.byref(total))
        want = PS.plan(s, a, u)
        assert np.array_equal(src[1:n + 1], want), (n, pat, a)
        assert src[0] == -7 and src[n + 1] == -7
        assert dropped == PS.rows_dropped(want)
        assert abs(total.value - float(np.sum(s.astype(np.float64)))) <= 1e-12 * max(1.0, total.value)
    assert left_out == 0                                   # the generator seed was picked so


def test_host_scalars_equal_the_oracle(hc):
    rng = np.random.default_rng(11)
    for _ in range(50):
        legal = (rng.random(220) < 0.4).astype(np.uint8)
        pi = (rng.random(220) * (rng.random(220) < 0.7)).astype(np.float32)
        p = (rng.random(220) * (rng.random(220) < 0.8)).astype(np.float32)
        got = hc.lzsurprise_row(legal.ctypes.data, pi.ctypes.data, p.ctypes.data, 220)
        want = PS.surprise(legal, pi, p)
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
    assert hc.lzsurprise_weight(0.5, 10, 1.0, 0.0) == 1.0
    assert hc.lzsurprise_weight(0.5, 10, 1.0, 5e-12) == 1.0
    assert hc.lzsurprise_weight(0.5, 10, 1.0, 4.0) == 0.5 + 0.5 * 10 * 1.0 / 4.0
    assert hc.lzsurprise_count(1.75, 3.5, 0.5) == 2 and hc.lzsurprise_count(2.0, 2.4, 0.5) == 0


# ---- validation and refusals ---------------------------------------------------------------------------------------------
def test_weight_validation():
    from liuzhou_amd.policy_surprise import policy_surprise_on
    assert policy_surprise_on(0) is False and policy_surprise_on(0.0) is False
    assert policy_surprise_on(0.5) is True and policy_surprise_on(1) is True and policy_surprise_on(1e-9) is True
    for bad in (-0.1, 1.0001, math.nan, math.inf, -math.inf, "half", None, True):
        with pytest.raises(ValueError, match="policy_surprise_weight"):
            policy_surprise_on(bad)


def test_refusal_reasons():
    from liuzhou_amd.search_rules import SearchRules
    policy_surprise_refusal = SearchRules.parse(16, policy_surprise_weight=0.5).refusal
    assert policy_surprise_refusal() is None
    assert policy_surprise_refusal(batch_k=4) is None      # nothing in the legacy waves prevents it
    assert "device_tail" in policy_surprise_refusal(device_tail=False)
    assert "reseat" in policy_surprise_refusal(reseat=True)
    assert "PriorEvaluator" in policy_surprise_refusal(prior_evaluator=True)


def test_self_play_refuses_before_it_touches_a_device():
    from liuzhou_amd.tree_engine import PriorEvaluator, self_play_tree_gpu
    module = torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="device_tail"):
        self_play_tree_gpu(module, 2, 16, 1.0, 0.1, 10, 1.0, "cpu", evaluator="module", device_tail=False,
                           policy_surprise_weight=0.5)
    with pytest.raises(ValueError, match="PriorEvaluator"):
        self_play_tree_gpu(PriorEvaluator(lambda planes, packed: None), 2, 16, 1.0, 0.1, 10, 1.0, "cpu",
                           policy_surprise_weight=0.5)
    for bad in (math.nan, -0.5, 1.5):
        with pytest.raises(ValueError, match="policy_surprise_weight"):
            self_play_tree_gpu(module, 2, 16, 1.0, 0.1, 10, 1.0, "cpu", evaluator="module", policy_surprise_weight=bad)


def test_tail_refuses_the_in_kernel_reseat_before_it_touches_a_device():
    from liuzhou_amd.wave_tail import WaveTail
    with pytest.raises(ValueError, match="reseat"):
        WaveTail(None, 4, 16, "cpu", reseat=True, policy_surprise_weight=0.5)
    with pytest.raises(ValueError, match="policy_surprise_weight"):
        WaveTail(None, 4, 16, "cpu", policy_surprise_weight=2.0)
    with pytest.raises(RuntimeError, match="HIP device"):  # off: the tail it always was
        WaveTail(None, 4, 16, "cpu", reseat=True, policy_surprise_weight=0.0)


def test_root_backend_is_refused():
    from liuzhou_amd.search_rules import SearchRules
    refuse_backend = lambda on, backend: SearchRules.parse(16, policy_surprise_weight=0.5 if on else 0.0).refuse(
        search_backend=backend)
    refuse_backend(False, "cuda_root")
    refuse_backend(True, "tree")
    refuse_backend(True, "portable")
    with pytest.raises(ValueError, match="tree backend"):
        refuse_backend(True, "cuda_root")


# ---- counters ------------------------------------------------------------------------------------------------------------
def test_counters_derive_and_merge():
    from liuzhou_amd.policy_surprise import COUNTER_KEYS, DERIVED_KEYS, counters_from_block, surprise_meta
    from liuzhou_amd.self_play_worker import merge_self_play_stats
    from liuzhou_amd.self_play_types import SelfPlayV1Stats
    a = counters_from_block((4, 100, 20), 25.0)
    b = counters_from_block((1, 50, 0), 50.0)
    assert a == {"surprise_games": 4, "surprise_rows": 100, "surprise_rows_replaced": 20, "surprise_sum_micro": 25_000_000,
                 "surprise_mean": 250_000}
    assert set(a) == set(COUNTER_KEYS + DERIVED_KEYS)
    assert counters_from_block((0, 0, 0), 0.0)["surprise_mean"] == 0

    def st(c):
        keys = ("root_puct_ms",)
        return SelfPlayV1Stats(num_games=1, num_positions=1, black_wins=0, white_wins=0, draws=1, avg_game_length=1.0,
                               elapsed_sec=1.0, positions_per_sec=1.0, games_per_sec=1.0,
                               step_timing_ms={k: 1.0 for k in keys}, step_timing_ratio={k: 1.0 for k in keys},
                               step_timing_calls={k: 1 for k in keys}, mcts_counters=dict(c),
                               piece_delta_buckets={"0": 1}, device="cuda:0")
    m = merge_self_play_stats([st(a), st(b)], 1.0).mcts_counters
    assert m["surprise_rows"] == 150 and m["surprise_sum_micro"] == 75_000_000 and m["surprise_mean"] == 500_000
    assert surprise_meta(0.5, m) == {"weight": 0.5, "games": 5, "rows": 150, "rows_replaced": 20, "mean_surprise": 0.5}
    off = merge_self_play_stats([st({"leaf_eval_count": 3})], 1.0).mcts_counters
    assert not any(k in off for k in COUNTER_KEYS + DERIVED_KEYS)
