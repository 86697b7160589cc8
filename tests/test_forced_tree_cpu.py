"""CPU: the checker of the forced-playout tests (tests/forced_tree.py) and the plumbing of `forced_playouts_k`.

1. With k = 0 the Python tree equals oracle.OracleTree bit for bit (the checker is checked first).
2. With k = 2: the forced rule and the invariants of policy target pruning.
3. The inputs of the GPU parity test (tests/test_gpu_forced_playouts.py) are not vacuous.
4. Flag parsing, kwargs, refusals and manifest metadata through scripts/selfplay_stage.py and run_self_play_stage."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import lz_oracle as O
from tests import forced_tree as FT
from tests.stage_stub import stub_worker
from tests.tree_parity import hash_evaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the checker against the C oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("with_noise", [False, True])
def test_k0_equals_the_c_oracle_tree(with_noise):
    """40 positions of g1_rules.npz, 64 simulations, 3 moves with advance: the same pending state at every step, root
    child visits and priors bit-exact, value sums equal as doubles."""
    from oracle.selfplay_oracle import deterministic_pick
    B, sims, eps = 40, 64, 0.25
    states, _ = FT.parity_inputs(False, num_games=B, seed=5)
    rng = np.random.default_rng(17)
    cur = [O.state_from_batch(states, i) for i in range(B)]
    ref = [O.OracleTree(cur[i], 1.0) for i in range(B)]
    got = [FT.ForcedTree(cur[i], 1.0, 0.0) for i in range(B)]

    def step(is_root, noise):
        pa = [t.prepare_root() if is_root else t.select() for t in ref]
        pb = [t.prepare_root() if is_root else t.select() for t in got]
        assert pa == pb
        need = [i for i, p in enumerate(pa) if p]
        if need:
            sa = O.batch_from_states([ref[i].pending_state() for i in need])
            sb = O.batch_from_states([got[i].pending_state() for i in need])
            for f in sa:
                assert np.array_equal(np.asarray(sa[f]), np.asarray(sb[f])), f
            pri, val = hash_evaluator(sa)
            for j, i in enumerate(need):
                nz = noise[i] if (is_root and noise is not None) else None
                ref[i].complete(pri[j], float(val[j]), nz, eps)
                got[i].complete(pri[j], float(val[j]), nz, eps)
        if is_root and noise is not None:
            for i in range(B):
                if not pa[i] and not ref[i].root_terminal():
                    ref[i].root_noise(noise[i], eps)
                    got[i].root_noise(noise[i], eps)

    kept = 0
    for mv in range(3):
        noise = (rng.gamma(0.3, 1.0, size=(B, 80)).astype(np.float32) + np.float32(1e-6)) if with_noise else None
        step(True, noise)
        for _ in range(sims):
            step(False, None)
        for i in range(B):
            assert ref[i].root_terminal() == got[i].root_terminal()
            a, b = ref[i].root_children(), got[i].root_children()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4]), (mv, i)
            assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)), (mv, i, "value sums differ")
            assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)), (mv, i, "priors differ")
            assert ref[i].root_visits() == got[i].root_visits()
            assert ref[i].root_value_sum() == got[i].root_value_sum()
            assert ref[i].root_player() == got[i].root_player()
            assert np.array_equal(got[i].prune_targets(), b[1])              # k = 0: nothing is pruned
            assert got[i].forced_count == 0
            if ref[i].root_terminal():
                ref[i], got[i] = O.OracleTree(cur[i], 1.0), FT.ForcedTree(cur[i], 1.0, 0.0)
                continue
            pick = deterministic_pick(*a, ref[i].root_player())
            cur[i] = O.apply_index(cur[i], pick)
            ka, kb = ref[i].advance(pick), got[i].advance(pick)
            assert ka == kb
            kept += int(ka)
            if not ka:
                ref[i], got[i] = O.OracleTree(cur[i], 1.0), FT.ForcedTree(cur[i], 1.0, 0.0)
    assert kept > B                                                         # subtrees were carried over


# ---- 2. the rules with k = 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_noise", [False, True])
def test_forced_rule_and_pruning_invariants(with_noise):
    B, sims, k = 32, 64, 2.0
    states, noise = FT.parity_inputs(with_noise, num_games=B, seed=23)
    trees = [FT.ForcedTree(O.state_from_batch(states, i), 1.0, k) for i in range(B)]
    checked = [0]

    def on_select(i, t):
        # the due set was taken before the descent: the child visited is the lowest-index due one
        if t.last_due:
            assert t.last_root_child == min(t.last_due), i
            checked[0] += 1

    # the due test, restated on the tree's state right before every select
    def run():
        from tests.tree_parity import hash_evaluator as he
        pend = [t.prepare_root() for t in trees]
        need = [i for i, p in enumerate(pend) if p]
        pri, val = he(O.batch_from_states([trees[i].pending_state() for i in need]))
        for j, i in enumerate(need):
            trees[i].complete(pri[j], float(val[j]), None if noise is None else noise[i], 0.25)
        for _ in range(sims):
            pend = []
            for i, t in enumerate(trees):
                idx, vis, _vs, pr, _pl = t.root_children()
                n = t.root_visits()
                want_due = [j for j in range(len(idx))
                            if vis[j] > 0 and float(vis[j]) * float(vis[j]) < (k * float(pr[j])) * float(n)]
                before = vis.copy()
                pend.append(t.select())
                assert t.last_due == want_due, i
                on_select(i, t)
                if t.last_root_child >= 0 and not pend[-1]:                  # terminal leaf: backed up inside select
                    assert t.root_children()[1][t.last_root_child] == before[t.last_root_child] + 1
            need = [i for i, p in enumerate(pend) if p]
            if need:
                pri, val = he(O.batch_from_states([trees[i].pending_state() for i in need]))
                for j, i in enumerate(need):
                    trees[i].complete(pri[j], float(val[j]))
    run()
    assert checked[0] > 0
    live = 0
    for i, t in enumerate(trees):
        if t.root_terminal():
            continue
        live += 1
        idx, vis, _vs, pr, _pl = t.root_children()
        assert int(vis.sum()) == sims == t.root_visits(), i                  # every root still gains exactly `sims` visits
        tv = t.prune_targets()
        star = int(np.argmax(vis))                                           # first maximum = lowest index among equals
        assert np.all(tv >= 0) and np.all(tv <= vis), i
        assert tv[star] == vis[star], i
        assert not np.any((tv == 1) & (np.arange(len(tv)) != star)), i
        legal = np.zeros(220, bool)
        legal[O.legal_indices_py(O.state_from_batch(states, i))] = True
        for temp, beta in ((1.0, 0.0), (0.5, 0.0), (1.0, 0.5)):
            pol = FT.target_policy(t, temp, beta)
            assert abs(float(pol.sum(dtype=np.float64)) - 1.0) < 1e-5, i
            assert not pol[~legal].any(), i
    assert live >= B // 2


# ---- 3. the GPU parity test's inputs are not vacuous ------------------------------------------------------------------
def vacuity_shares(with_noise):
    """Over the positions, simulations and noise of the GPU injected-evaluator parity test: the share of non-terminal roots
    with at least one forced descent, and the share with at least one pruned visit (the Python tree alone decides)."""
    states, noise = FT.parity_inputs(with_noise)
    trees = [FT.ForcedTree(O.state_from_batch(states, i), 1.0, FT.PARITY_K) for i in range(FT.PARITY_GAMES)]
    forced = FT.search_alone(trees, FT.PARITY_SIMS, noise)
    live = [i for i, t in enumerate(trees) if not t.root_terminal()]
    pruned = [int((trees[i].root_children()[1] - trees[i].prune_targets()).sum()) for i in live]
    return (len(live), sum(forced[i] > 0 for i in live) / max(1, len(live)),
            sum(p > 0 for p in pruned) / max(1, len(live)))


@pytest.mark.parametrize("with_noise", [False, True])
def test_parity_inputs_are_not_vacuous(with_noise):
    """At least half of the non-terminal roots of the GPU parity test see a forced descent, and at least half lose visits
    to pruning.  Shares found (64 games x 64 simulations, k = 2, seed 11; all 64 roots are non-terminal), without and
    with noise alike: forced descents at 64 / 64 roots (1.000), pruned visits at 61 / 64 roots (0.953)."""
    live, forced_share, pruned_share = vacuity_shares(with_noise)
    print(f"noise={with_noise}: {live} live roots, forced share {forced_share:.3f}, pruned share {pruned_share:.3f}")
    assert live >= FT.PARITY_GAMES // 2
    assert forced_share >= 0.5
    assert pruned_share >= 0.5


# ---- 4. plumbing ------------------------------------------------------------------------------------------------------
def _cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import selfplay_stage as cli
    return cli


def test_flag_parses_in_the_reference_style():
    cli = _cli()
    a = cli.parse(["--search_backend", "tree", "--mcts_simulations", "64", "--forced_playouts_k", "2"])
    assert a.forced_playouts_k == 2.0 and a.ignored == []
    assert cli.parse([]).forced_playouts_k == 0.0


def test_validation():
    from liuzhou_amd.tree_engine import forced_playouts_on
    assert forced_playouts_on(0) is False and forced_playouts_on(0.0) is False
    assert forced_playouts_on(2) is True and forced_playouts_on(0.5) is True
    for k in (-1.0, -1e-9, math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError):
            forced_playouts_on(k)


def _stage(tmp_path, worker_fn, **kw):
    from liuzhou_amd.self_play_stage import run_self_play_stage
    return run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                               output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=32,
                               concurrent_games_per_device=4, worker_fn=worker_fn, in_process=True, **kw)


def test_kwarg_reaches_the_worker_only_when_on(tmp_path):
    seen = []

    def spy(**kw):
        seen.append(kw)
        return stub_worker(**kw)

    _stage(tmp_path / "off", spy, search_backend="tree")
    _stage(tmp_path / "zero", spy, search_backend="tree", forced_playouts_k=0.0)
    assert len(seen) == 4 and all("forced_playouts_k" not in k for k in seen)
    seen.clear()
    _stage(tmp_path / "on", spy, search_backend="tree", forced_playouts_k=2.0)
    assert len(seen) == 2 and all(k["forced_playouts_k"] == 2.0 for k in seen)


def test_stage_and_worker_refuse_bad_arguments(tmp_path):
    from liuzhou_amd.self_play_worker import run_self_play_worker
    with pytest.raises(ValueError):
        _stage(tmp_path, stub_worker, search_backend="cuda_root", forced_playouts_k=2.0)
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            _stage(tmp_path, stub_worker, search_backend="tree", forced_playouts_k=bad)
    common = dict(worker_idx=0, shard_device="cuda:0", shard_games=1, seed=1, model_state_path="x", output_path="y",
                  mcts_simulations=32, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                  exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
                  opening_random_moves=0, max_game_plies=64, concurrent_games_per_device=1)
    with pytest.raises(ValueError):
        run_self_play_worker(search_backend="cuda_root", forced_playouts_k=2.0, **common)
    with pytest.raises(ValueError):
        run_self_play_worker(search_backend="tree", forced_playouts_k=-0.5, **common)


def _forced_worker(**kw):
    """The stub worker as the real one reports forced playouts: k in its metadata, the counts in its counters."""
    from liuzhou_amd import self_play_worker as W
    on = "forced_playouts_k" in kw
    orig = W.write_worker_chunks

    def write(run_once, **a):
        if on:
            a["meta_common"] = {**a["meta_common"], "forced_playouts": {"k": kw["forced_playouts_k"]}}

        def run(n, **x):
            b, st = run_once(n, **x)
            if on:
                st.mcts_counters.update(forced_playouts=5 * st.num_positions, pruned_visits=2 * st.num_positions)
            return b, st
        return orig(run, **a)

    import tests.stage_stub as S
    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if k != "forced_playouts_k"})
    finally:
        S.write_worker_chunks = orig


def test_manifest_metadata_on_and_off(tmp_path):
    _, off = _stage(tmp_path / "off", _forced_worker, search_backend="tree")
    assert "forced_playouts" not in off["metadata"]
    _, on = _stage(tmp_path / "on", _forced_worker, search_backend="tree", forced_playouts_k=2.0)
    fp = on["metadata"]["forced_playouts"]
    assert fp == {"k": 2.0, "forced_playouts": 5 * on["num_samples"], "pruned_visits": 2 * on["num_samples"]}
    assert set(on) == set(off)                          # the manifest's own keys are unchanged
    assert set(on["metadata"]) - set(off["metadata"]) == {"forced_playouts"}
