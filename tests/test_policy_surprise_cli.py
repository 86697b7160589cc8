"""CPU: `policy_surprise_weight` through scripts/selfplay_stage.py, run_self_play_stage, the worker and the manifests."""
import math
import os
import sys

import pytest
import torch

from tests.stage_stub import stub_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "policy_surprise_weight"
BLOCK, SUM = (3, 21, 5), 10.5                              # what one run of a worker books (lz_wave_surprise_resample's order)


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import selfplay_stage as cli
    return cli


def test_flag_parses():
    cli = _cli()
    a = cli.parse(["--search_backend", "tree", "--policy_surprise_weight", "0.5"])
    assert a.policy_surprise_weight == 0.5 and a.ignored == []
    assert cli.parse([]).policy_surprise_weight == 0.0


def test_main_hands_the_flag_to_the_stage_only_when_set(monkeypatch, tmp_path):
    cli = _cli()
    import liuzhou_amd.self_play_stage as S
    seen = {}

    class _Stats:
        num_games = num_positions = black_wins = white_wins = draws = 0
        positions_per_sec = 0.0

    def stage(**kw):
        seen.update(kw)
        return _Stats(), {"num_shards": 0, "num_samples": 0, "metadata": {}}
    monkeypatch.setattr(S, "run_self_play_stage", stage)
    out = str(tmp_path / "sp.pt")
    assert cli.main(["--model", "b6c64", "--search_backend", "tree", "--self_play_output", out,
                     "--policy_surprise_weight", "0.5"]) == 0
    assert seen[KEY] == 0.5
    seen.clear()
    assert cli.main(["--model", "b6c64", "--search_backend", "tree", "--self_play_output", out]) == 0
    assert KEY not in seen


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
    _stage(tmp_path / "zero", spy, search_backend="tree", policy_surprise_weight=0.0)
    _stage(tmp_path / "root", spy, search_backend="cuda_root", policy_surprise_weight=0)       # off: any backend
    assert len(seen) == 6 and all(KEY not in kw for kw in seen)
    seen.clear()
    _stage(tmp_path / "on", spy, search_backend="tree", policy_surprise_weight=0.5)
    assert [kw[KEY] for kw in seen] == [0.5, 0.5]


WORKER_COMMON = dict(worker_idx=0, shard_device="cuda:0", shard_games=1, seed=1, model_state_path="x", output_path="y",
                     mcts_simulations=32, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                     exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
                     opening_random_moves=0, max_game_plies=64, concurrent_games_per_device=1)


def test_stage_and_worker_refuse_and_name_the_reason(tmp_path):
    from liuzhou_amd.self_play_worker import run_self_play_worker
    with pytest.raises(ValueError, match="tree backend"):
        _stage(tmp_path, stub_worker, search_backend="cuda_root", policy_surprise_weight=0.5)
    with pytest.raises(ValueError, match="tree backend"):
        run_self_play_worker(search_backend="cuda_root", policy_surprise_weight=0.5, **WORKER_COMMON)
    for backend in ("tree", "cuda_root"):
        for bad in (math.nan, -0.1, 1.5, math.inf):
            with pytest.raises(ValueError, match=KEY):
                _stage(tmp_path, stub_worker, search_backend=backend, policy_surprise_weight=bad)
            with pytest.raises(ValueError, match=KEY):
                run_self_play_worker(search_backend=backend, policy_surprise_weight=bad, **WORKER_COMMON)


def _surprise_worker(**kw):
    """The stub worker as the real one reports the feature: the weight in its metadata, the counters in its stats."""
    from liuzhou_amd import self_play_worker as W
    from liuzhou_amd.policy_surprise import counters_from_block
    import tests.stage_stub as S
    orig = W.write_worker_chunks
    on = KEY in kw

    def write(run_once, **a):
        if on:
            a["meta_common"] = {**a["meta_common"], "policy_surprise": {"weight": float(kw[KEY])}}

        def counted(n):
            batch, st = run_once(n)
            if on:
                st.mcts_counters.update(counters_from_block(BLOCK, SUM))
            return batch, st
        return orig(counted, **a)

    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if k != KEY})
    finally:
        S.write_worker_chunks = orig


def test_manifest_metadata_on_and_off(tmp_path):
    from liuzhou_amd.policy_surprise import COUNTER_KEYS, DERIVED_KEYS
    st_off, off = _stage(tmp_path / "off", _surprise_worker, search_backend="tree")
    assert "policy_surprise" not in off["metadata"]
    _, zero = _stage(tmp_path / "zero", _surprise_worker, search_backend="tree", policy_surprise_weight=0.0)
    assert "policy_surprise" not in zero["metadata"]
    st_on, on = _stage(tmp_path / "on", _surprise_worker, search_backend="tree", policy_surprise_weight=0.5)
    # 10 games over 2 devices, 4 per chunk: 2 chunks per worker, 4 runs in all; the sums add up, the mean does not
    assert on["metadata"]["policy_surprise"] == {"weight": 0.5, "games": 12, "rows": 84, "rows_replaced": 20,
                                                 "mean_surprise": 0.5}
    assert st_on.mcts_counters["surprise_mean"] == 500_000 and st_on.mcts_counters["surprise_sum_micro"] == 42_000_000
    assert not any(k in st_off.mcts_counters for k in COUNTER_KEYS + DERIVED_KEYS)
    assert set(on) == set(off)                              # the manifest's own keys are unchanged
    assert set(on["metadata"]) - set(off["metadata"]) == {"policy_surprise"}
    assert [os.path.basename(f) for f in on["shard_files"]] == [os.path.basename(f) for f in off["shard_files"]]
    keys = lambda man, base: set(torch.load(os.path.join(base, os.path.basename(man["shard_files"][0])), weights_only=False))
    assert keys(on, tmp_path / "on") == keys(off, tmp_path / "off")          # payload keys too
    # the worker's own manifest carries its share: two runs of this worker
    ws = tmp_path / "ws"
    _stage(tmp_path / "kept", _surprise_worker, search_backend="tree", policy_surprise_weight=0.5, shard_dir=str(ws))
    wm = torch.load(str(ws / "worker_manifest_000002_00.pt"), weights_only=False)
    assert wm["metadata"]["policy_surprise"] == {"weight": 0.5, "games": 6, "rows": 42, "rows_replaced": 10,
                                                 "mean_surprise": 0.5}
