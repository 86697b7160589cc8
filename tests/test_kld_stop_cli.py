"""CPU: the KLD-gain early stopping parameters through scripts/selfplay_stage.py, run_self_play_stage, the worker and the
manifests."""
import math
import os
import sys

import pytest
import torch

from tests.stage_stub import stub_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("kld_stop_threshold", "kld_stop_interval", "kld_stop_min_simulations")
ON = dict(kld_stop_threshold=2e-5, kld_stop_interval=50, kld_stop_min_simulations=150)
META = {"threshold": 2e-5, "interval": 50, "min_simulations": 150}
COUNTS = {"kld_stopped_searches": 11, "kld_simulations_saved": 2300}       # what one run of a worker books


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import selfplay_stage as cli
    return cli


def test_flags_parse():
    cli = _cli()
    a = cli.parse(["--search_backend", "tree", "--kld_stop_threshold", "2e-5", "--kld_stop_interval", "50",
                   "--kld_stop_min_simulations", "150"])
    assert (a.kld_stop_threshold, a.kld_stop_interval, a.kld_stop_min_simulations) == (2e-5, 50, 150)
    assert a.ignored == []
    d = cli.parse([])
    assert (d.kld_stop_threshold, d.kld_stop_interval, d.kld_stop_min_simulations) == (0.0, 100, None)


def test_main_hands_the_flags_to_the_stage_only_when_on(monkeypatch, tmp_path):
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
    assert cli.main(["--model", "b6c64", "--search_backend", "tree", "--self_play_output", out, "--kld_stop_threshold", "2e-5",
                     "--kld_stop_interval", "50", "--kld_stop_min_simulations", "150"]) == 0
    assert {k: seen[k] for k in KEYS} == ON
    seen.clear()
    assert cli.main(["--model", "b6c64", "--search_backend", "tree", "--self_play_output", out, "--kld_stop_threshold", "1e-4"]) == 0
    assert {k: seen[k] for k in KEYS} == dict(kld_stop_threshold=1e-4, kld_stop_interval=100, kld_stop_min_simulations=None)
    seen.clear()
    assert cli.main(["--model", "b6c64", "--search_backend", "tree", "--self_play_output", out, "--kld_stop_interval", "7"]) == 0
    assert not any(k in seen for k in KEYS)


def _stage(tmp_path, worker_fn, **kw):
    from liuzhou_amd.self_play_stage import run_self_play_stage
    return run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                               output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=800,
                               concurrent_games_per_device=4, worker_fn=worker_fn, in_process=True, **kw)


def test_kwargs_reach_the_worker_only_when_on(tmp_path):
    seen = []

    def spy(**kw):
        seen.append(kw)
        return stub_worker(**{k: v for k, v in kw.items() if k not in KEYS})

    _stage(tmp_path / "off", spy, search_backend="tree")
    _stage(tmp_path / "zero", spy, search_backend="tree", kld_stop_threshold=0.0, kld_stop_interval=7)
    _stage(tmp_path / "root", spy, search_backend="cuda_root", kld_stop_threshold=0.0)        # off: any backend
    assert len(seen) == 6 and all(k not in kw for kw in seen for k in KEYS)
    seen.clear()
    _stage(tmp_path / "on", spy, search_backend="tree", **ON)
    _stage(tmp_path / "dflt", spy, search_backend="tree", kld_stop_threshold=1e-4)
    assert [{k: kw[k] for k in KEYS} for kw in seen] == [ON, ON] + 2 * [dict(
        kld_stop_threshold=1e-4, kld_stop_interval=100, kld_stop_min_simulations=100)]


WORKER_COMMON = dict(worker_idx=0, shard_device="cuda:0", shard_games=1, seed=1, model_state_path="x", output_path="y",
                     mcts_simulations=800, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                     exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
                     opening_random_moves=0, max_game_plies=64, concurrent_games_per_device=1)


def test_stage_and_worker_refuse_and_name_the_reason(tmp_path):
    from liuzhou_amd.self_play_worker import run_self_play_worker
    with pytest.raises(ValueError, match="tree backend"):
        _stage(tmp_path, stub_worker, search_backend="cuda_root", kld_stop_threshold=1e-4)
    with pytest.raises(ValueError, match="tree backend"):
        run_self_play_worker(search_backend="cuda_root", kld_stop_threshold=1e-4, **WORKER_COMMON)
    with pytest.raises(ValueError, match="Gumbel"):
        _stage(tmp_path, stub_worker, search_backend="tree", kld_stop_threshold=1e-4, gumbel_considered=16)
    with pytest.raises(ValueError, match="Gumbel"):
        run_self_play_worker(search_backend="tree", kld_stop_threshold=1e-4, gumbel_considered=16, **WORKER_COMMON)
    for backend in ("tree", "cuda_root"):
        for key, bads in (("kld_stop_threshold", (math.nan, math.inf, -0.5)), ("kld_stop_interval", (0, 2.5)),
                          ("kld_stop_min_simulations", (-1, math.nan))):
            for bad in bads:
                kw = {"kld_stop_threshold": 1e-4, key: bad}
                with pytest.raises(ValueError, match=key):
                    _stage(tmp_path, stub_worker, search_backend=backend, **kw)
                with pytest.raises(ValueError, match=key):
                    run_self_play_worker(search_backend=backend, **kw, **WORKER_COMMON)


def _kld_worker(**kw):
    """The stub worker as the real one reports the rule: the settings in its metadata, the counters in its stats."""
    from liuzhou_amd import self_play_worker as W
    from liuzhou_amd.kld_stop import kld_stop_meta
    import tests.stage_stub as S
    orig = W.write_worker_chunks
    on = "kld_stop_threshold" in kw

    def write(run_once, **a):
        if on:
            a["meta_common"] = {**a["meta_common"], "kld_stop": kld_stop_meta(kw)}

        def counted(n):
            batch, st = run_once(n)
            if on:
                st.mcts_counters.update(COUNTS)
            return batch, st
        return orig(counted, **a)

    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if k not in KEYS})
    finally:
        S.write_worker_chunks = orig


def test_manifest_metadata_on_and_off(tmp_path):
    st_off, off = _stage(tmp_path / "off", _kld_worker, search_backend="tree")
    assert "kld_stop" not in off["metadata"]
    _, zero = _stage(tmp_path / "zero", _kld_worker, search_backend="tree", kld_stop_threshold=0.0)
    assert "kld_stop" not in zero["metadata"]
    st_on, on = _stage(tmp_path / "on", _kld_worker, search_backend="tree", **ON)
    # 10 games over 2 devices, 4 per chunk: 2 chunks per worker, 4 runs in all; the counters add up
    want = {**META, **{k: 4 * v for k, v in COUNTS.items()}}
    assert on["metadata"]["kld_stop"] == want
    assert all(st_on.mcts_counters[k] == want[k] for k in COUNTS)
    assert not any(k in st_off.mcts_counters for k in COUNTS)
    assert set(on) == set(off)                              # the manifest's own keys are unchanged
    assert set(on["metadata"]) - set(off["metadata"]) == {"kld_stop"}
    assert [os.path.basename(f) for f in on["shard_files"]] == [os.path.basename(f) for f in off["shard_files"]]
    keys = lambda man, base: set(torch.load(os.path.join(base, os.path.basename(man["shard_files"][0])), weights_only=False))
    assert keys(on, tmp_path / "on") == keys(off, tmp_path / "off")          # payload keys too
