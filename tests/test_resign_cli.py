"""CPU: the resignation parameters through scripts/selfplay_stage.py, run_self_play_stage, the worker and the manifests."""
import math
import os
import sys

import pytest
import torch

from tests.stage_stub import stub_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("resign_threshold", "resign_min_moves", "resign_consecutive", "resign_playthrough_fraction", "resign_streak")
ON = dict(resign_threshold=-0.9, resign_min_moves=20, resign_consecutive=2, resign_playthrough_fraction=0.25,
          resign_streak="ply")
META = {"threshold": -0.9, "min_moves": 20, "consecutive": 2, "playthrough_fraction": 0.25, "streak": "ply"}
BLOCK = (4, 3, 1, 2, 2, 1, 100, 30)                        # what a worker's run books (lz_wave_resign_book's order)


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import selfplay_stage as cli
    return cli


def test_flags_parse_in_the_reference_style():
    cli = _cli()
    a = cli.parse(["--search_backend", "tree", "--self_play_resign_threshold", "-0.9", "--self_play_resign_min_moves", "20",
                   "--self_play_resign_consecutive", "2", "--self_play_resign_playthrough_fraction", "0.25",
                   "--self_play_resign_streak", "ply"])
    assert (a.self_play_resign_threshold, a.self_play_resign_min_moves, a.self_play_resign_consecutive,
            a.self_play_resign_playthrough_fraction, a.self_play_resign_streak) == (-0.9, 20, 2, 0.25, "ply")
    assert a.ignored == []
    d = cli.parse([])
    assert (d.self_play_resign_threshold, d.self_play_resign_min_moves, d.self_play_resign_consecutive,
            d.self_play_resign_playthrough_fraction, d.self_play_resign_streak) == (0.0, 10, 3, 0.1, "side")
    with pytest.raises(SystemExit):
        cli.parse(["--self_play_resign_streak", "game"])


def test_main_hands_the_flags_to_the_stage(monkeypatch, tmp_path):
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
                     "--self_play_resign_threshold", "-0.9", "--self_play_resign_min_moves", "20",
                     "--self_play_resign_consecutive", "2", "--self_play_resign_playthrough_fraction", "0.25",
                     "--self_play_resign_streak", "ply"]) == 0
    assert {k: seen[k] for k in KEYS} == ON
    seen.clear()
    assert cli.main(["--model", "b6c64", "--search_backend", "tree", "--self_play_output", out]) == 0
    assert {k: seen[k] for k in KEYS} == dict(resign_threshold=0.0, resign_min_moves=10, resign_consecutive=3,
                                              resign_playthrough_fraction=0.1, resign_streak="side")


def _stage(tmp_path, worker_fn, **kw):
    from liuzhou_amd.self_play_stage import run_self_play_stage
    return run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                               output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=32,
                               concurrent_games_per_device=4, worker_fn=worker_fn, in_process=True, **kw)


def test_kwargs_reach_the_worker_only_when_on(tmp_path):
    seen = []

    def spy(**kw):
        seen.append(kw)
        return stub_worker(**{k: v for k, v in kw.items() if k not in KEYS})

    _stage(tmp_path / "off", spy, search_backend="tree")
    _stage(tmp_path / "zero", spy, search_backend="tree", resign_threshold=0.0, resign_min_moves=3, resign_streak="ply")
    _stage(tmp_path / "root", spy, search_backend="cuda_root", resign_threshold=0.0)          # off: any backend
    assert len(seen) == 6 and all(k not in kw for kw in seen for k in KEYS)
    seen.clear()
    _stage(tmp_path / "on", spy, search_backend="tree", **ON)
    _stage(tmp_path / "dflt", spy, search_backend="tree", resign_threshold=-1)
    assert [{k: kw[k] for k in KEYS} for kw in seen] == [ON, ON] + 2 * [dict(
        resign_threshold=-1.0, resign_min_moves=10, resign_consecutive=3, resign_playthrough_fraction=0.1,
        resign_streak="side")]


WORKER_COMMON = dict(worker_idx=0, shard_device="cuda:0", shard_games=1, seed=1, model_state_path="x", output_path="y",
                     mcts_simulations=32, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                     exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
                     opening_random_moves=0, max_game_plies=64, concurrent_games_per_device=1)


def test_stage_and_worker_refuse_and_name_the_reason(tmp_path):
    from liuzhou_amd.self_play_worker import run_self_play_worker
    with pytest.raises(ValueError, match="tree backend"):
        _stage(tmp_path, stub_worker, search_backend="cuda_root", resign_threshold=-0.9)
    with pytest.raises(ValueError, match="tree backend"):
        run_self_play_worker(search_backend="cuda_root", resign_threshold=-0.9, **WORKER_COMMON)
    for backend in ("tree", "cuda_root"):
        for key, bads in (("resign_threshold", (math.nan, math.inf, 0.5, -1.5)), ("resign_min_moves", (-1, 2.5)),
                          ("resign_consecutive", (0, math.nan)), ("resign_playthrough_fraction", (-0.1, 1.5, math.nan)),
                          ("resign_streak", ("game",))):
            for bad in bads:
                kw = {"resign_threshold": -0.9, key: bad}
                with pytest.raises(ValueError, match=key):
                    _stage(tmp_path, stub_worker, search_backend=backend, **kw)
                with pytest.raises(ValueError, match=key):
                    run_self_play_worker(search_backend=backend, **kw, **WORKER_COMMON)


def _resign_worker(**kw):
    """The stub worker as the real one reports the feature: the settings in its metadata, the counters in its stats."""
    from liuzhou_amd import self_play_worker as W
    from liuzhou_amd.resign import counters_from_block, resign_meta
    import tests.stage_stub as S
    orig = W.write_worker_chunks
    on = "resign_threshold" in kw

    def write(run_once, **a):
        if on:
            a["meta_common"] = {**a["meta_common"], "resign": resign_meta(kw)}

        def counted(n):
            batch, st = run_once(n)
            if on:
                st.mcts_counters.update(counters_from_block(BLOCK))
            return batch, st
        return orig(counted, **a)

    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if k not in KEYS})
    finally:
        S.write_worker_chunks = orig


def test_manifest_metadata_on_and_off(tmp_path):
    from liuzhou_amd.resign import COUNTER_KEYS, DERIVED_KEYS
    st_off, off = _stage(tmp_path / "off", _resign_worker, search_backend="tree")
    assert "resign" not in off["metadata"]
    _, zero = _stage(tmp_path / "zero", _resign_worker, search_backend="tree", resign_threshold=0.0)
    assert "resign" not in zero["metadata"]
    st_on, on = _stage(tmp_path / "on", _resign_worker, search_backend="tree", **ON)
    # 10 games over 2 devices, 4 per chunk: 2 chunks per worker, 4 runs in all; the sums add up, the averages do not
    want = {**META, **{k: 4 * v for k, v in zip(COUNTER_KEYS, BLOCK)}, "resign_avg_ply": 25,
            "resign_plies_saved_estimate": 240}
    assert on["metadata"]["resign"] == want
    assert all(st_on.mcts_counters[k] == want[k] for k in COUNTER_KEYS + DERIVED_KEYS)
    assert not any(k in st_off.mcts_counters for k in COUNTER_KEYS + DERIVED_KEYS)
    assert set(on) == set(off)                              # the manifest's own keys are unchanged
    assert set(on["metadata"]) - set(off["metadata"]) == {"resign"}
    assert [os.path.basename(f) for f in on["shard_files"]] == [os.path.basename(f) for f in off["shard_files"]]
    keys = lambda man, base: set(torch.load(os.path.join(base, os.path.basename(man["shard_files"][0])), weights_only=False))
    assert keys(on, tmp_path / "on") == keys(off, tmp_path / "off")          # payload keys too
