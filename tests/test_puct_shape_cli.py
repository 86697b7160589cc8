"""CPU: `--fpu_reduction` / `--fpu_root_reduction` / `--cpuct_log` / `--cpuct_base` through scripts/selfplay_stage.py,
run_self_play_stage and the worker: the flags parse, the kwargs and metadata["puct_shape"] travel only when one of the two
halves is on, bad values and a backend without a tree are refused; the arena script and its agents take the same four."""
import os
import sys

import pytest
import torch

from tests.stage_stub import stub_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("fpu_reduction", "fpu_root_reduction", "cpuct_log", "cpuct_base")


def _cli(name="selfplay_stage"):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    return __import__(name)


def _stage(tmp_path, worker_fn, **kw):
    from liuzhou_amd.self_play_stage import run_self_play_stage
    return run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                               output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=32,
                               concurrent_games_per_device=4, worker_fn=worker_fn, in_process=True, **kw)


def test_flags_parse_in_the_reference_style():
    cli = _cli()
    a = cli.parse(["--search_backend", "tree", "--fpu_reduction", "0.2", "--fpu_root_reduction", "0.1", "--cpuct_log",
                   "1.25", "--cpuct_base", "500"])
    assert (a.fpu_reduction, a.fpu_root_reduction, a.cpuct_log, a.cpuct_base) == (0.2, 0.1, 1.25, 500.0) and a.ignored == []
    d = cli.parse([])
    assert (d.fpu_reduction, d.fpu_root_reduction, d.cpuct_log, d.cpuct_base) == (None, None, 0.0, 19652.0)
    assert cli.parse(["--fpu_reduction", "0"]).fpu_reduction == 0.0       # a valid "on": the parent's value, no reduction


def test_flags_reach_the_stage_only_when_on(tmp_path, monkeypatch):
    """main() hands the stage exactly the halves that are on (and nothing when both are off)."""
    import liuzhou_amd.self_play_stage as S
    from liuzhou_amd.self_play_types import SelfPlayV1Stats
    cli = _cli()
    seen = []

    def fake(**kw):
        seen.append(kw)
        st = SelfPlayV1Stats(num_games=0, num_positions=0, black_wins=0, white_wins=0, draws=0, avg_game_length=0.0,
                             elapsed_sec=0.0, positions_per_sec=0.0, games_per_sec=0.0, step_timing_ms={}, step_timing_ratio={},
                             step_timing_calls={}, mcts_counters={}, piece_delta_buckets={})
        return st, {"num_shards": 0, "num_samples": 0, "metadata": {}}

    monkeypatch.setattr(S, "run_self_play_stage", fake)
    base = ["--model", "b6c64", "--self_play_output", str(tmp_path / "o.pt"), "--search_backend", "tree"]
    assert cli.main(base) == 0
    assert not any(k in seen[-1] for k in KEYS)
    assert cli.main(base + ["--cpuct_base", "100"]) == 0              # a base alone switches nothing on
    assert not any(k in seen[-1] for k in KEYS)
    assert cli.main(base + ["--fpu_reduction", "0.2"]) == 0
    assert seen[-1]["fpu_reduction"] == 0.2 and seen[-1]["fpu_root_reduction"] is None and "cpuct_log" not in seen[-1]
    assert cli.main(base + ["--cpuct_log", "1.0", "--cpuct_base", "8"]) == 0
    assert (seen[-1]["cpuct_log"], seen[-1]["cpuct_base"]) == (1.0, 8.0) and "fpu_reduction" not in seen[-1]
    assert cli.main(base + ["--fpu_root_reduction", "0.1"]) == 0      # reaches the stage, which refuses it (below)
    assert seen[-1]["fpu_reduction"] is None and seen[-1]["fpu_root_reduction"] == 0.1


def test_kwargs_reach_the_worker_only_when_on(tmp_path):
    seen = []

    def spy(**kw):
        seen.append(kw)
        return stub_worker(**kw)

    _stage(tmp_path / "off", spy, search_backend="tree")
    _stage(tmp_path / "none", spy, search_backend="tree", fpu_reduction=None, cpuct_log=0.0, cpuct_base=8.0)
    assert len(seen) == 4 and not any(k in kw for kw in seen for k in KEYS)
    seen.clear()
    _stage(tmp_path / "fpu", spy, search_backend="tree", fpu_reduction=0.0)
    assert len(seen) == 2 and all(kw["fpu_reduction"] == 0.0 and kw["fpu_root_reduction"] == 0.0 for kw in seen)
    assert not any("cpuct_log" in kw or "cpuct_base" in kw for kw in seen)
    seen.clear()
    _stage(tmp_path / "both", spy, search_backend="tree", fpu_reduction=0.2, fpu_root_reduction=0.1, cpuct_log=1.0,
           cpuct_base=8.0)
    assert all((kw["fpu_reduction"], kw["fpu_root_reduction"], kw["cpuct_log"], kw["cpuct_base"]) == (0.2, 0.1, 1.0, 8.0)
               for kw in seen)


def test_stage_and_worker_refuse(tmp_path):
    from liuzhou_amd.self_play_worker import run_self_play_worker
    with pytest.raises(ValueError, match="tree backend"):
        _stage(tmp_path, stub_worker, search_backend="cuda_root", fpu_reduction=0.2)
    with pytest.raises(ValueError, match="Gumbel"):
        _stage(tmp_path, stub_worker, search_backend="tree", gumbel_considered=8, cpuct_log=1.0)
    with pytest.raises(ValueError, match="fpu_root_reduction"):
        _stage(tmp_path, stub_worker, search_backend="tree", fpu_root_reduction=0.1)
    with pytest.raises(ValueError, match="cpuct_base"):
        _stage(tmp_path, stub_worker, search_backend="tree", cpuct_log=1.0, cpuct_base=0.0)
    with pytest.raises(ValueError, match="fpu_reduction"):
        _stage(tmp_path, stub_worker, search_backend="tree", fpu_reduction=float("nan"))
    common = dict(worker_idx=0, shard_device="cuda:0", shard_games=1, seed=1, model_state_path="x", output_path="y",
                  mcts_simulations=32, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                  exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
                  opening_random_moves=0, max_game_plies=64, concurrent_games_per_device=1)
    with pytest.raises(ValueError, match="tree backend"):
        run_self_play_worker(search_backend="cuda_root", cpuct_log=1.0, **common)
    with pytest.raises(ValueError, match="cpuct_log"):
        run_self_play_worker(search_backend="tree", cpuct_log=-1.0, **common)


def _shape_worker(**kw):
    """The stub worker as the real one reports the shape: the four values in its metadata when a half is on."""
    from liuzhou_amd import self_play_worker as W
    from liuzhou_amd.puct_shape import parse_puct_shape
    shape = parse_puct_shape(kw.get("fpu_reduction"), kw.get("fpu_root_reduction"), kw.get("cpuct_log", 0.0),
                             kw.get("cpuct_base", 19652.0))
    orig = W.write_worker_chunks

    def write(run_once, **a):
        if shape.on:
            a["meta_common"] = {**a["meta_common"], "puct_shape": shape.meta()}
        return orig(run_once, **a)

    import tests.stage_stub as S
    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if k not in KEYS})
    finally:
        S.write_worker_chunks = orig


def test_manifest_metadata_on_and_off(tmp_path):
    _, off = _stage(tmp_path / "off", _shape_worker, search_backend="tree")
    assert "puct_shape" not in off["metadata"]
    _, on = _stage(tmp_path / "on", _shape_worker, search_backend="tree", fpu_reduction=0.2, cpuct_log=1.0, cpuct_base=8.0)
    assert on["metadata"]["puct_shape"] == {"fpu_reduction": 0.2, "fpu_root_reduction": 0.2, "cpuct_log": 1.0,
                                            "cpuct_base": 8.0}
    assert set(on) == set(off)
    assert set(on["metadata"]) - set(off["metadata"]) == {"puct_shape"}
    _, tab = _stage(tmp_path / "tab", _shape_worker, search_backend="tree", cpuct_log=0.5)
    assert tab["metadata"]["puct_shape"] == {"fpu_reduction": None, "fpu_root_reduction": None, "cpuct_log": 0.5,
                                             "cpuct_base": 19652.0}


def test_arena_flags_and_agents():
    from liuzhou_amd.eval_arena import TreeSearchAgent, _joinable
    cli = _cli("eval_arena")
    a = cli.parse(["--challenger_checkpoint", "c.pt", "--backend", "portable", "--fpu_reduction", "0.2", "--cpuct_log", "1",
                   "--cpuct_base", "8"])
    assert (a.fpu_reduction, a.fpu_root_reduction, a.cpuct_log, a.cpuct_base) == (0.2, None, 1.0, 8.0)
    d = cli.parse(["--challenger_checkpoint", "c.pt"])
    assert (d.fpu_reduction, d.fpu_root_reduction, d.cpuct_log, d.cpuct_base) == (None, None, 0.0, 19652.0)

    def agent(**kw):                                              # the search settings alone: no network, no device
        x = TreeSearchAgent.__new__(TreeSearchAgent)
        from liuzhou_amd.puct_shape import parse_puct_shape
        x.sims, x.sample_moves, x.seed, x.device = 64, False, 0, torch.device("cpu")
        x.puct_shape = parse_puct_shape(**kw)
        return x

    assert _joinable([agent(), agent()])
    assert _joinable([agent(fpu_reduction=0.2), agent(fpu_reduction=0.2, fpu_root_reduction=0.2)])
    assert not _joinable([agent(fpu_reduction=0.2), agent()])
    assert not _joinable([agent(cpuct_log=1.0), agent(cpuct_log=1.0, cpuct_base=8.0)])
    assert _joinable([agent(cpuct_base=8.0), agent()])             # a base without the log is off on both sides
