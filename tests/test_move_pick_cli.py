"""CPU: the move-selection parameters (move_visit_offset, move_value_cutoff, temperature_halflife) through
scripts/selfplay_stage.py, run_self_play_stage, the worker and the manifests."""
import math
import os
import sys

import pytest
import torch

from tests.stage_stub import stub_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICK_KEYS = ("move_visit_offset", "move_value_cutoff")
KEYS = PICK_KEYS + ("temperature_halflife",)
ON = dict(move_visit_offset=3.0, move_value_cutoff=0.25, temperature_halflife=6.0)
META = {"visit_offset": 3.0, "value_cutoff": 0.25, "temperature_halflife": 6.0}
COUNTS = {"move_pick_applied": 40, "move_pick_cut_visits": 31, "move_pick_cut_value": 7, "move_pick_changed": 5}


def _cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import selfplay_stage as cli
    return cli


def test_flags_parse():
    cli = _cli()
    a = cli.parse(["--search_backend", "tree", "--move_visit_offset", "3", "--move_value_cutoff", "0.25",
                   "--temperature_halflife", "6"])
    assert (a.move_visit_offset, a.move_value_cutoff, a.temperature_halflife) == (3.0, 0.25, 6.0)
    assert a.ignored == []
    d = cli.parse([])
    assert (d.move_visit_offset, d.move_value_cutoff, d.temperature_halflife) == (0.0, 0.0, 0.0)


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
    base = ["--model", "b6c64", "--search_backend", "tree", "--self_play_output", str(tmp_path / "sp.pt")]
    assert cli.main(base + ["--move_visit_offset", "3", "--move_value_cutoff", "0.25", "--temperature_halflife", "6"]) == 0
    assert {k: seen[k] for k in KEYS} == ON
    seen.clear()
    assert cli.main(base + ["--move_value_cutoff", "0.5"]) == 0
    assert {k: seen[k] for k in PICK_KEYS} == dict(move_visit_offset=0.0, move_value_cutoff=0.5)
    assert "temperature_halflife" not in seen
    seen.clear()
    assert cli.main(base + ["--temperature_halflife", "4"]) == 0
    assert seen["temperature_halflife"] == 4.0 and not any(k in seen for k in PICK_KEYS)
    seen.clear()
    assert cli.main(base) == 0
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
    _stage(tmp_path / "zero", spy, search_backend="tree", move_visit_offset=0.0, move_value_cutoff=0, temperature_halflife=0.0)
    _stage(tmp_path / "root", spy, search_backend="cuda_root", move_visit_offset=0.0)          # off: any backend
    assert len(seen) == 6 and all(k not in kw for kw in seen for k in KEYS)
    seen.clear()
    _stage(tmp_path / "on", spy, search_backend="tree", **ON)
    _stage(tmp_path / "cut", spy, search_backend="tree", move_value_cutoff=0.5)
    _stage(tmp_path / "half", spy, search_backend="tree", temperature_halflife=4)
    got = [{k: kw[k] for k in KEYS if k in kw} for kw in seen]
    assert got == [ON, ON] + 2 * [dict(move_visit_offset=0.0, move_value_cutoff=0.5)] + 2 * [dict(temperature_halflife=4.0)]


WORKER_COMMON = dict(worker_idx=0, shard_device="cuda:0", shard_games=1, seed=1, model_state_path="x", output_path="y",
                     mcts_simulations=800, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                     exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
                     opening_random_moves=0, max_game_plies=64, concurrent_games_per_device=1)


def test_stage_and_worker_refuse_and_name_the_reason(tmp_path):
    from liuzhou_amd.self_play_worker import run_self_play_worker
    for on in (dict(move_visit_offset=1.0), dict(move_value_cutoff=0.5), dict(temperature_halflife=4.0)):
        with pytest.raises(ValueError, match="tree backend"):
            _stage(tmp_path, stub_worker, search_backend="cuda_root", **on)
        with pytest.raises(ValueError, match="tree backend"):
            run_self_play_worker(search_backend="cuda_root", **on, **WORKER_COMMON)
    for on in (dict(move_visit_offset=1.0), dict(move_value_cutoff=0.5)):
        with pytest.raises(ValueError, match="Gumbel"):
            _stage(tmp_path, stub_worker, search_backend="tree", gumbel_considered=16, **on)
        with pytest.raises(ValueError, match="Gumbel"):
            run_self_play_worker(search_backend="tree", gumbel_considered=16, **on, **WORKER_COMMON)
        with pytest.raises(ValueError, match="sample_moves"):
            _stage(tmp_path, stub_worker, search_backend="tree", sample_moves=False, **on)
        with pytest.raises(ValueError, match="sample_moves"):
            run_self_play_worker(search_backend="tree", sample_moves=False, **on, **WORKER_COMMON)
    for backend in ("tree", "cuda_root"):
        for key, bads in (("move_visit_offset", (True, math.nan, math.inf, -0.5)),
                          ("move_value_cutoff", (math.nan, -0.125, 2.5)),
                          ("temperature_halflife", (math.nan, math.inf, -1.0))):
            for bad in bads:
                with pytest.raises(ValueError, match=key):
                    _stage(tmp_path, stub_worker, search_backend=backend, **{key: bad})
                with pytest.raises(ValueError, match=key):
                    run_self_play_worker(search_backend=backend, **{key: bad}, **WORKER_COMMON)


def _pick_worker(**kw):
    """The stub worker as the real one reports the rule: the settings in its metadata, the counters in its stats."""
    from liuzhou_amd import self_play_worker as W
    from liuzhou_amd.move_pick import move_pick_meta
    import tests.stage_stub as S
    orig = W.write_worker_chunks
    on = any(k in kw for k in KEYS)
    repick = "move_visit_offset" in kw

    def write(run_once, **a):
        if on:
            a["meta_common"] = {**a["meta_common"], "move_pick": move_pick_meta(kw)}

        def counted(n):
            batch, st = run_once(n)
            if repick:
                st.mcts_counters.update(COUNTS)
            return batch, st
        return orig(counted, **a)

    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if k not in KEYS})
    finally:
        S.write_worker_chunks = orig


def test_manifest_metadata_on_and_off(tmp_path):
    st_off, off = _stage(tmp_path / "off", _pick_worker, search_backend="tree")
    assert "move_pick" not in off["metadata"]
    _, zero = _stage(tmp_path / "zero", _pick_worker, search_backend="tree", move_visit_offset=0.0, temperature_halflife=0.0)
    assert "move_pick" not in zero["metadata"]
    st_on, on = _stage(tmp_path / "on", _pick_worker, search_backend="tree", **ON)
    # 10 games over 2 devices, 4 per chunk: 2 chunks per worker, 4 runs in all; the counters add up
    want = {**META, **{k: 4 * v for k, v in COUNTS.items()}}
    assert on["metadata"]["move_pick"] == want
    assert all(st_on.mcts_counters[k] == want[k] for k in COUNTS)
    assert not any(k in st_off.mcts_counters for k in COUNTS)
    st_half, half = _stage(tmp_path / "half", _pick_worker, search_backend="tree", temperature_halflife=4.0)
    assert half["metadata"]["move_pick"] == {"visit_offset": 0.0, "value_cutoff": 0.0, "temperature_halflife": 4.0}
    assert not any(k in st_half.mcts_counters for k in COUNTS)               # the half-life alone books no counter
    assert set(on) == set(off)                              # the manifest's own keys are unchanged
    assert set(on["metadata"]) - set(off["metadata"]) == {"move_pick"}
    assert [os.path.basename(f) for f in on["shard_files"]] == [os.path.basename(f) for f in off["shard_files"]]
    keys = lambda man, base: set(torch.load(os.path.join(base, os.path.basename(man["shard_files"][0])), weights_only=False))
    assert keys(on, tmp_path / "on") == keys(off, tmp_path / "off")          # payload keys too
