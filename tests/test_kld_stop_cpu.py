"""CPU: KLD-gain early stopping -- the checker's properties, parameter validation, the refusals that need no device and the
descriptor layout."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import kld_stop as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the checker -----------------------------------------------------------------------------------------------------------
def test_equal_distributions_gain_exactly_zero():
    rng = np.random.default_rng(1)
    for _ in range(200):
        ne = int(rng.integers(1, 73))
        o = rng.integers(0, 1 << 14, ne)
        if o.sum() == 0:
            o[0] = 1
        for mult in (2, 3, 7, 1000):
            per, stop, snap = K.check(o, o * mult, 8, 0, 1e-300)
            assert per == 0.0 and stop and np.array_equal(snap, o * mult)
    # the largest counts the 24-bit field holds: the products stay exact
    o = np.full(72, (1 << 23) - 1)
    assert K.check(o, o * 2, 8, 0, 1e-300)[0] == 0.0


def test_no_snapshot_mass_or_no_new_visits_decide_nothing():
    n = np.array([3, 0, 5])
    for snap in (np.zeros(3, dtype=np.int64), n, n + 1):          # O = 0, N = O, N < O
        per, stop, new = K.check(snap, n, 100, 0, 1e9)
        assert per is None and not stop and np.array_equal(new, n)


def test_children_without_old_visits_contribute_nothing():
    base = K.check([4, 4, 0, 0], [6, 6, 0, 0], 8, 0, 1.0)[0]
    assert base == 0.0
    # new mass on children the snapshot did not have: only the terms of the old children count
    per = K.check([4, 4, 0, 0], [6, 6, 5, 7], 8, 0, 1.0)[0]
    want = 2 * (0.5 * math.log((4 * 24) / (6 * 8))) / 16
    assert per == pytest.approx(want, rel=1e-15, abs=0.0)
    assert np.isfinite(per)


def test_gain_is_never_negative_and_min_simulations_gates_the_stop():
    rng = np.random.default_rng(2)
    for _ in range(500):
        ne = int(rng.integers(1, 73))
        o = rng.integers(0, 200, ne)
        n = o + rng.integers(0, 50, ne)
        per, stop, _ = K.check(o, n, 16, 32, 1e9)
        if per is not None:
            assert per >= -1e-15 and not stop                     # s < M: never a stop, whatever the gain
            assert K.check(o, n, 32, 32, per * 2 + 1e-12)[1]
            assert not K.check(o, n, 32, 32, per)[1]              # strictly below the threshold


def test_replay_follows_the_checks_in_order():
    flat = [np.array([0, 0]), np.array([4, 4]), np.array([8, 8]), np.array([12, 12]), np.array([16, 16])]
    # check 1 has O = 0; check 2 (s = 16) gains 0 -> stop at 17
    assert K.replay(flat, 40, 8, 0, 1e-9)[0] == 17
    assert K.replay(flat, 40, 8, 24, 1e-9)[0] == 25               # not before M
    assert K.replay(flat, 40, 8, 0, 0.0)[0] == 40                 # threshold 0 never stops (gain >= 0)
    assert K.replay(flat, 40, 8, 0, 1e-9, budget=10)[0] == 10     # a spent budget is never decided
    assert K.replay(flat, 18, 8, 0, 1e-9)[0] == 17                # s + 1 < sims: the check at 16 of 18 still runs ...
    assert K.replay(flat, 17, 8, 0, 1e-9) == (17, [])             # ... the one at 16 of 17 does not
    moving = [np.array([0, 0]), np.array([8, 0]), np.array([8, 8]), np.array([8, 16]), np.array([8, 24])]
    b, gains = K.replay(moving, 40, 8, 0, 1e-9)
    assert b == 40 and [s for s, _ in gains] == [16, 24, 32] and all(g > 1e-3 for _, g in gains)


# ---- 2. validation --------------------------------------------------------------------------------------------------------------
def test_parameters_are_validated():
    from liuzhou_amd.kld_stop import kld_stop_kwargs, parse_kld_stop
    off = parse_kld_stop()
    assert not off.on and off.kwargs() == {} and (off.interval, off.min_simulations) == (100, 100)
    on = parse_kld_stop(2e-5, 50)
    assert on.on and on.min_simulations == 50 and on.meta() == {"threshold": 2e-5, "interval": 50, "min_simulations": 50}
    assert parse_kld_stop(1e-4, 100, 0).min_simulations == 0
    assert kld_stop_kwargs(1e-4, 10, 30) == {"kld_stop_threshold": 1e-4, "kld_stop_interval": 10,
                                             "kld_stop_min_simulations": 30}
    assert kld_stop_kwargs(0.0, 10, 30) == {}
    for key, bads in (("kld_stop_threshold", (-1e-9, math.nan, math.inf, "x", True)),
                      ("kld_stop_interval", (0, -3, 2.5, math.nan, None)),
                      ("kld_stop_min_simulations", (-1, 1.5, math.inf))):
        for bad in bads:
            for thr in (0.0, 1e-4):                               # whether on or off
                with pytest.raises(ValueError, match=key):
                    parse_kld_stop(**{"kld_stop_threshold": thr, key: bad})


# ---- 3. refusals that need no device ----------------------------------------------------------------------------------------------
def test_configurations_are_refused_with_a_reason(monkeypatch):
    from liuzhou_amd.search_rules import SearchRules, persistent_default
    kld_stop_refusal = SearchRules.parse(800, kld_stop_threshold=1e-4).refusal
    monkeypatch.delenv("LZ_TREE_PERSISTENT", raising=False)
    assert kld_stop_refusal() is None
    assert "batch_k" in kld_stop_refusal(batch_k=2)
    assert "several networks" in kld_stop_refusal(several_networks=True)
    assert "external evaluator" in kld_stop_refusal(fused=False)
    assert "Gumbel" in SearchRules.parse(800, kld_stop_threshold=1e-4, gumbel_considered=8).refusal()
    assert "persistent" in kld_stop_refusal(persistent=True)
    monkeypatch.setenv("LZ_TREE_PERSISTENT", "1")
    assert "persistent" in kld_stop_refusal(persistent=persistent_default())


def test_engines_runner_worker_and_stage_refuse(monkeypatch):
    from liuzhou_amd.kld_stop import parse_kld_stop
    from liuzhou_amd.self_play_stage import run_self_play_stage
    from liuzhou_amd.self_play_worker import run_self_play_worker
    from liuzhou_amd.tree_engine import PortableTreeMCTS, PriorEvaluator, self_play_tree_gpu
    monkeypatch.delenv("LZ_TREE_PERSISTENT", raising=False)
    ks = parse_kld_stop(1e-4, 8)
    with pytest.raises(ValueError, match="batch_k"):
        PortableTreeMCTS(object(), 4, 32, "cuda:0", batch_k=2, kld_stop=ks)
    with pytest.raises(ValueError, match="external evaluator"):
        PortableTreeMCTS(PriorEvaluator(lambda p, s: None), 4, 32, "cuda:0", kld_stop=ks)
    with pytest.raises(ValueError, match="several networks"):
        PortableTreeMCTS([object(), object()], 32, 32, "cuda:0", segment_games=16, kld_stop=ks)
    common = dict(num_games=2, mcts_simulations=32, temperature_init=1.0, temperature_final=0.1, temperature_threshold=4,
                  exploration_weight=1.0, device="cuda:0")
    with pytest.raises(ValueError, match="external evaluator"):
        self_play_tree_gpu(PriorEvaluator(lambda p, s: None), kld_stop_threshold=1e-4, **common)
    with pytest.raises(ValueError, match="kld_stop_interval"):
        self_play_tree_gpu(PriorEvaluator(lambda p, s: None), kld_stop_threshold=1e-4, kld_stop_interval=0, **common)
    wk = dict(worker_idx=0, shard_device="cuda:0", shard_games=4, seed=1, model_state_path="none.pt", output_path="none",
              mcts_simulations=32, temperature_init=1.0, temperature_final=0.1, temperature_threshold=4,
              exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
              opening_random_moves=0, max_game_plies=8, concurrent_games_per_device=4)
    with pytest.raises(ValueError, match="tree backend"):
        run_self_play_worker(search_backend="cuda_root", kld_stop_threshold=1e-4, **wk)
    with pytest.raises(ValueError, match="Gumbel"):
        run_self_play_worker(search_backend="tree", gumbel_considered=8, kld_stop_threshold=1e-4, **wk)
    with pytest.raises(ValueError, match="kld_stop_threshold"):
        run_self_play_worker(search_backend="tree", kld_stop_threshold=-1.0, **wk)
    st = dict(model_state={}, num_games=4, output_path="none", devices=["cuda:0"], iteration_seed=1, mcts_simulations=32)
    with pytest.raises(ValueError, match="tree backend"):
        run_self_play_stage(search_backend="cuda_root", kld_stop_threshold=1e-4, **st)
    with pytest.raises(ValueError, match="Gumbel"):
        run_self_play_stage(search_backend="tree", gumbel_considered=8, kld_stop_threshold=1e-4, **st)


# ---- 4. the descriptor ----------------------------------------------------------------------------------------------------------
def test_the_ctypes_mirror_follows_the_header():
    """Field names in the order of include/liuzhou_hip.h, the rule's eight fields in one run between the solver's and the
    PUCT shape's (which stay the last five), and the size the library reports."""
    from liuzhou_amd import _lib as L
    from liuzhou_amd.tree_engine import LzTreeDesc
    text = open(os.path.join(ROOT, "include", "liuzhou_hip.h")).read()
    body = text[text.index("typedef struct LzTreeDesc {"):text.index("} LzTreeDesc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = body[body.index("{") + 1:]
    names = [re.findall(r"\w+", piece)[-1] for stmt in body.split(";") if stmt.strip() for piece in stmt.split(",")]
    mirror = [f[0] for f in LzTreeDesc._fields_]
    assert names == mirror
    new = ["kld_interval", "kld_min_sims", "kld_threshold", "kld_snapshot", "kld_budget", "kld_stops", "kld_saved",
           "kld_trace"]
    at = mirror.index("kld_interval")
    assert mirror[at:at + 8] == new and mirror[at - 1] == "solver_count" and mirror[at + 8] == "puct_shape"
    types = dict(LzTreeDesc._fields_)
    assert types["kld_interval"] is C.c_int32 and types["kld_min_sims"] is C.c_int32
    assert types["kld_threshold"] is C.c_double
    assert all(types[n] is C.c_void_p for n in new[3:])
    assert LzTreeDesc.kld_interval.offset == LzTreeDesc.solver_count.offset + 8
    assert LzTreeDesc.kld_trace.offset + 8 == LzTreeDesc.puct_shape.offset
    assert int(L.lib().lz_tree_desc_bytes()) == C.sizeof(LzTreeDesc)
    assert "lz_tree_kld_check" in L.SYMBOLS
