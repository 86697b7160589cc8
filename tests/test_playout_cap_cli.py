"""CPU: the playout cap's parameters through scripts/selfplay_stage.py, run_self_play_stage and the manifests."""
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


def test_flags_parse_in_the_reference_style():
    cli = _cli()
    a = cli.parse(["--search_backend", "tree", "--mcts_simulations", "64", "--playout_cap_fast_simulations", "16",
                   "--playout_cap_full_prob", "0.25"])
    assert a.playout_cap_fast_simulations == 16 and a.playout_cap_full_prob == 0.25 and a.ignored == []
    d = cli.parse([])
    assert d.playout_cap_fast_simulations == 0 and d.playout_cap_full_prob == 1.0


def test_validation():
    from liuzhou_amd.tree_engine import playout_cap_on
    assert playout_cap_on(0, 1.0, 64) is False and playout_cap_on(0, 0.3, 64) is False
    assert playout_cap_on(16, 0.25, 64) is True and playout_cap_on(63, 1.0, 64) is True
    for f, p in ((64, 0.5), (65, 0.5), (-1, 0.5), (16, -0.1), (16, 1.5)):
        with pytest.raises(ValueError):
            playout_cap_on(f, p, 64)


def _stage(tmp_path, worker_fn, **kw):
    from liuzhou_amd.self_play_stage import run_self_play_stage
    return run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                               output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=32,
                               concurrent_games_per_device=4, worker_fn=worker_fn, in_process=True, **kw)


def test_kwargs_reach_the_worker_only_when_the_cap_is_on(tmp_path):
    seen = []

    def spy(**kw):
        seen.append(kw)
        return stub_worker(**kw)

    _stage(tmp_path / "off", spy, search_backend="tree")
    assert all("playout_cap_fast_simulations" not in k for k in seen)
    seen.clear()
    _stage(tmp_path / "on", spy, search_backend="tree", playout_cap_fast_simulations=8, playout_cap_full_prob=0.25)
    assert len(seen) == 2
    assert all(k["playout_cap_fast_simulations"] == 8 and k["playout_cap_full_prob"] == 0.25 for k in seen)


def test_stage_refuses_bad_arguments(tmp_path):
    with pytest.raises(ValueError):
        _stage(tmp_path, stub_worker, search_backend="cuda_root", playout_cap_fast_simulations=8,
               playout_cap_full_prob=0.25)
    with pytest.raises(ValueError):
        _stage(tmp_path, stub_worker, search_backend="tree", playout_cap_fast_simulations=32, playout_cap_full_prob=0.25)
    from liuzhou_amd.self_play_worker import run_self_play_worker
    with pytest.raises(ValueError):
        run_self_play_worker(worker_idx=0, shard_device="cuda:0", shard_games=1, seed=1, model_state_path="x",
                             output_path="y", mcts_simulations=32, temperature_init=1.0, temperature_final=0.1,
                             temperature_threshold=10, exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25,
                             soft_value_k=2.0, opening_random_moves=0, max_game_plies=64, concurrent_games_per_device=1,
                             search_backend="cuda_root", playout_cap_fast_simulations=8, playout_cap_full_prob=0.5)


def _cap_worker(**kw):
    """The stub worker as the real one reports the cap: settings in its metadata, searches in its counters."""
    from liuzhou_amd import self_play_worker as W
    cap = "playout_cap_fast_simulations" in kw
    orig = W.write_worker_chunks

    def write(run_once, **a):
        if cap:
            a["meta_common"] = {**a["meta_common"], "playout_cap": {"fast_simulations": kw["playout_cap_fast_simulations"],
                                                                    "full_prob": kw["playout_cap_full_prob"]}}

        def run(n, **x):
            b, st = run_once(n, **x)
            if cap:
                st.mcts_counters.update(full_searches=st.num_positions, fast_searches=3 * st.num_positions)
            return b, st
        return orig(run, **a)

    import tests.stage_stub as S
    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if not k.startswith("playout_cap")})
    finally:
        S.write_worker_chunks = orig


def test_manifest_metadata_with_the_cap_on_and_off(tmp_path):
    _, off = _stage(tmp_path / "off", _cap_worker, search_backend="tree")
    assert "playout_cap" not in off["metadata"]
    st, on = _stage(tmp_path / "on", _cap_worker, search_backend="tree", playout_cap_fast_simulations=8,
                    playout_cap_full_prob=0.25)
    pc = on["metadata"]["playout_cap"]
    assert pc["fast_simulations"] == 8 and pc["full_prob"] == 0.25
    assert pc["full_searches"] == on["num_samples"] == st.num_positions
    assert pc["fast_searches"] == 3 * on["num_samples"]
    assert set(on) == set(off)                          # the manifest's own keys are unchanged
