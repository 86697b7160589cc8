"""CPU: `value_target_lambda` (TD(lambda) value targets) through scripts/selfplay_stage.py, run_self_play_stage, the worker
and the manifests."""
import math
import os
import sys

import pytest
import torch

from tests.stage_stub import stub_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "value_target_lambda"


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import selfplay_stage as cli
    return cli


def test_flag_parses_in_the_reference_style():
    cli = _cli()
    a = cli.parse(["--search_backend", "tree", "--mcts_simulations", "64", "--value_target_lambda", "0.8"])
    assert a.value_target_lambda == 0.8 and a.ignored == []
    assert cli.parse([]).value_target_lambda == 1.0


def _stage(tmp_path, worker_fn, **kw):
    from liuzhou_amd.self_play_stage import run_self_play_stage
    return run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                               output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=32,
                               concurrent_games_per_device=4, worker_fn=worker_fn, in_process=True, **kw)


def test_kwarg_reaches_the_worker_only_when_on(tmp_path):
    seen = []

    def spy(**kw):
        seen.append(kw)
        return stub_worker(**{k: v for k, v in kw.items() if k != KEY})

    _stage(tmp_path / "off", spy, search_backend="tree")
    _stage(tmp_path / "one", spy, search_backend="tree", value_target_lambda=1.0)
    _stage(tmp_path / "root", spy, search_backend="cuda_root", value_target_lambda=1.0)      # off: any backend
    assert len(seen) == 6 and all(KEY not in kw for kw in seen)
    seen.clear()
    _stage(tmp_path / "on", spy, search_backend="tree", value_target_lambda=0.8)
    _stage(tmp_path / "zero", spy, search_backend="tree", value_target_lambda=0)
    assert [kw[KEY] for kw in seen] == [0.8, 0.8, 0.0, 0.0]


WORKER_COMMON = dict(worker_idx=0, shard_device="cuda:0", shard_games=1, seed=1, model_state_path="x", output_path="y",
                     mcts_simulations=32, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                     exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
                     opening_random_moves=0, max_game_plies=64, concurrent_games_per_device=1)


def test_stage_and_worker_refuse_and_name_the_reason(tmp_path):
    from liuzhou_amd.self_play_worker import run_self_play_worker
    with pytest.raises(ValueError, match="tree backend"):
        _stage(tmp_path, stub_worker, search_backend="cuda_root", value_target_lambda=0.8)
    with pytest.raises(ValueError, match="tree backend"):
        run_self_play_worker(search_backend="cuda_root", value_target_lambda=0.8, **WORKER_COMMON)
    for bad in (math.nan, math.inf, -0.1, 1.5):
        for backend in ("tree", "cuda_root"):
            with pytest.raises(ValueError, match=KEY):
                _stage(tmp_path, stub_worker, search_backend=backend, value_target_lambda=bad)
            with pytest.raises(ValueError, match=KEY):
                run_self_play_worker(search_backend=backend, value_target_lambda=bad, **WORKER_COMMON)


def _td_worker(**kw):
    """The stub worker as the real one reports the mode: the setting in its metadata."""
    from liuzhou_amd import self_play_worker as W
    orig = W.write_worker_chunks

    def write(run_once, **a):
        if KEY in kw:
            a["meta_common"] = {**a["meta_common"], "value_target": {"td_lambda": kw[KEY]}}
        return orig(run_once, **a)

    import tests.stage_stub as S
    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if k != KEY})
    finally:
        S.write_worker_chunks = orig


def test_manifest_metadata_on_and_off(tmp_path):
    _, off = _stage(tmp_path / "off", _td_worker, search_backend="tree")
    assert "value_target" not in off["metadata"]
    _, one = _stage(tmp_path / "one", _td_worker, search_backend="tree", value_target_lambda=1.0)
    assert "value_target" not in one["metadata"]
    _, on = _stage(tmp_path / "on", _td_worker, search_backend="tree", value_target_lambda=0.8)
    assert on["metadata"]["value_target"] == {"td_lambda": 0.8}
    assert set(on) == set(off)                          # the manifest's own keys are unchanged
    assert set(on["metadata"]) - set(off["metadata"]) == {"value_target"}
    assert [os.path.basename(f) for f in on["shard_files"]] == [os.path.basename(f) for f in off["shard_files"]]
    keys = lambda man, base: set(torch.load(os.path.join(base, os.path.basename(man["shard_files"][0])), weights_only=False))
    assert keys(on, tmp_path / "on") == keys(off, tmp_path / "off")          # payload keys too
