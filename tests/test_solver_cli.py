"""CPU: `--mcts_solver` / `mcts_solver=` through scripts/selfplay_stage.py, run_self_play_stage and the worker: the flag
parses, the kwarg and metadata["mcts_solver"] travel only when the solver is on, and a backend without a tree refuses."""
import os
import sys

import pytest
import torch

from tests.stage_stub import stub_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import selfplay_stage as cli
    return cli


def _stage(tmp_path, worker_fn, **kw):
    from liuzhou_amd.self_play_stage import run_self_play_stage
    return run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                               output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=32,
                               concurrent_games_per_device=4, worker_fn=worker_fn, in_process=True, **kw)


def test_flag_parses_in_the_reference_style():
    cli = _cli()
    a = cli.parse(["--search_backend", "tree", "--mcts_simulations", "64", "--mcts_solver"])
    assert a.mcts_solver is True and a.ignored == []
    assert cli.parse([]).mcts_solver is False


def test_kwarg_reaches_the_worker_only_when_on(tmp_path):
    seen = []

    def spy(**kw):
        seen.append(kw)
        return stub_worker(**kw)

    _stage(tmp_path / "off", spy, search_backend="tree")
    _stage(tmp_path / "false", spy, search_backend="tree", mcts_solver=False)
    assert len(seen) == 4 and all("mcts_solver" not in k for k in seen)
    seen.clear()
    _stage(tmp_path / "on", spy, search_backend="tree", mcts_solver=True)
    assert len(seen) == 2 and all(k["mcts_solver"] is True for k in seen)


def test_stage_and_worker_refuse_a_backend_without_a_tree(tmp_path):
    from liuzhou_amd.self_play_worker import run_self_play_worker
    with pytest.raises(ValueError, match="tree backend"):
        _stage(tmp_path, stub_worker, search_backend="cuda_root", mcts_solver=True)
    common = dict(worker_idx=0, shard_device="cuda:0", shard_games=1, seed=1, model_state_path="x", output_path="y",
                  mcts_simulations=32, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                  exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
                  opening_random_moves=0, max_game_plies=64, concurrent_games_per_device=1)
    with pytest.raises(ValueError, match="tree backend"):
        run_self_play_worker(search_backend="cuda_root", mcts_solver=True, **common)


def _solver_worker(**kw):
    """The stub worker as the real one reports the solver: the flag in its metadata, the counts in its counters."""
    from liuzhou_amd import self_play_worker as W
    on = bool(kw.get("mcts_solver"))
    orig = W.write_worker_chunks

    def write(run_once, **a):
        if on:
            a["meta_common"] = {**a["meta_common"], "mcts_solver": True}

        def run(n, **x):
            b, st = run_once(n, **x)
            if on:
                st.mcts_counters.update(solver_proofs=3 * st.num_positions, solver_roots_decided=st.num_positions,
                                        solver_pick_overrides=st.num_games)
            return b, st
        return orig(run, **a)

    import tests.stage_stub as S
    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if k != "mcts_solver"})
    finally:
        S.write_worker_chunks = orig


def test_manifest_metadata_on_and_off(tmp_path):
    _, off = _stage(tmp_path / "off", _solver_worker, search_backend="tree")
    assert "mcts_solver" not in off["metadata"]
    assert not any(k.startswith("solver") for k in off["stats"]["mcts_counters"])
    _, on = _stage(tmp_path / "on", _solver_worker, search_backend="tree", mcts_solver=True)
    assert on["metadata"]["mcts_solver"] is True
    c = on["stats"]["mcts_counters"]
    assert c["solver_proofs"] == 3 * on["num_samples"] and c["solver_roots_decided"] == on["num_samples"]
    assert c["solver_pick_overrides"] == 10
    assert set(on) == set(off)
    assert set(on["metadata"]) - set(off["metadata"]) == {"mcts_solver"}
