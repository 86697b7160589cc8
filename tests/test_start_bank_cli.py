"""CPU: the start bank's options through scripts/selfplay_stage.py and scripts/staged_loop.py, run_self_play_stage, the
worker and the manifests."""
import os
import sys

import pytest
import torch

from tests.stage_stub import stub_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("start_fork_prob", "start_capture_prob", "start_bank_capacity", "start_min_move", "start_max_move")
ON = dict(start_fork_prob=0.5, start_capture_prob=0.25, start_bank_capacity=4096, start_min_move=4, start_max_move=90)
DEFAULTS = dict(start_fork_prob=0.0, start_capture_prob=0.0, start_bank_capacity=65536, start_min_move=1, start_max_move=143)
META = {"fork_prob": 0.5, "capture_prob": 0.25, "capacity": 4096, "min_move": 4, "max_move": 90}
COUNTERS = {"start_forked_games": 6, "start_fork_move_sum": 150, "start_captured": 40}       # what one run of a worker books
FLAGS = ["--start_fork_prob", "0.5", "--start_capture_prob", "0.25", "--start_bank_capacity", "4096", "--start_min_move", "4",
         "--start_max_move", "90"]


def _script(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    return __import__(name)


def test_flags_parse_with_the_documented_defaults():
    cli = _script("selfplay_stage")
    a = cli.parse(["--search_backend", "tree", *FLAGS])
    assert {k: getattr(a, k) for k in KEYS} == ON and a.ignored == []
    assert {k: getattr(cli.parse([]), k) for k in KEYS} == DEFAULTS
    loop = _script("staged_loop")
    b = loop.parse_args([f.replace("_", "-") for f in FLAGS])
    assert {k: getattr(b, k) for k in KEYS} == ON and loop.start_options(b) == ON
    assert {k: getattr(loop.parse_args([]), k) for k in KEYS} == DEFAULTS and loop.start_options(loop.parse_args([])) == {}
    for bad in (["--start-fork-prob", "1.5"], ["--start-capture-prob", "0.5", "--start-bank-capacity", "0"],
                ["--start-fork-prob", "0.5", "--search", "root"], ["--start-min-move", "9", "--start-max-move", "3"]):
        with pytest.raises(SystemExit):
            loop.parse_args(bad)


def test_main_hands_the_flags_to_the_stage(monkeypatch, tmp_path):
    cli = _script("selfplay_stage")
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
    assert cli.main(["--model", "b6c64", "--search_backend", "tree", "--self_play_output", out, *FLAGS]) == 0
    assert {k: seen[k] for k in KEYS} == ON
    seen.clear()
    assert cli.main(["--model", "b6c64", "--search_backend", "tree", "--self_play_output", out]) == 0
    assert not any(k in seen for k in KEYS)                  # off: the stage is called as before


def _stage(tmp_path, worker_fn, **kw):
    from liuzhou_amd.self_play_stage import run_self_play_stage
    return run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                               output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=32,
                               concurrent_games_per_device=4, worker_fn=worker_fn, in_process=True, **kw)


def test_kwargs_reach_the_stub_worker_only_when_on(tmp_path):
    seen = []

    def spy(**kw):
        seen.append(kw)
        return stub_worker(**{k: v for k, v in kw.items() if k not in KEYS})

    _stage(tmp_path / "off", spy, search_backend="tree")
    _stage(tmp_path / "zero", spy, search_backend="tree", start_bank_capacity=7, start_min_move=3)
    _stage(tmp_path / "root", spy, search_backend="cuda_root", start_fork_prob=0.0)           # off: any backend
    assert len(seen) == 6 and all(k not in kw for kw in seen for k in KEYS)
    seen.clear()
    _stage(tmp_path / "on", spy, search_backend="tree", **ON)
    _stage(tmp_path / "capture", spy, search_backend="tree", start_capture_prob=1)
    assert [{k: kw[k] for k in KEYS} for kw in seen] == [ON, ON] + 2 * [{**DEFAULTS, "start_capture_prob": 1.0}]
    assert all(type(kw[k]) is type(DEFAULTS[k]) for kw in seen for k in KEYS)


def _bank_worker(**kw):
    """The stub worker as the real one reports the rule: the settings in its metadata, the counters in its stats."""
    from liuzhou_amd import self_play_worker as W
    from liuzhou_amd.search_rules import SearchRules
    import tests.stage_stub as S
    orig = W.write_worker_chunks
    meta = SearchRules.parse(32, **{k: kw[k] for k in KEYS if k in kw}).meta()

    def write(run_once, **a):
        a["meta_common"] = {**a["meta_common"], **meta}

        def counted(n):
            batch, st = run_once(n)
            if meta:
                st.mcts_counters.update(COUNTERS)
            return batch, st
        return orig(counted, **a)

    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if k not in KEYS})
    finally:
        S.write_worker_chunks = orig


def test_the_merged_manifest_entry_sums_the_counters(tmp_path):
    st_off, off = _stage(tmp_path / "off", _bank_worker, search_backend="tree")
    assert "start_bank" not in off["metadata"] and not any(k in st_off.mcts_counters for k in COUNTERS)
    st_on, on = _stage(tmp_path / "on", _bank_worker, search_backend="tree", **ON)
    # 10 games over 2 devices, 4 per chunk: 2 chunks per worker, 4 runs in all
    want = {**META, "start_captured": 160, "start_forked_games": 24, "start_fork_move_sum": 600, "fork_avg_move": 25.0}
    assert on["metadata"]["start_bank"] == want
    assert all(st_on.mcts_counters[k] == 4 * v for k, v in COUNTERS.items())
    assert set(on) == set(off) and set(on["metadata"]) - set(off["metadata"]) == {"start_bank"}


def test_a_worker_manifest_carries_its_shards_counters():
    from liuzhou_amd.search_rules import start_meta
    assert start_meta(META, {**COUNTERS, "leaf_eval_count": 9}) == {
        **META, "start_captured": 40, "start_forked_games": 6, "start_fork_move_sum": 150, "fork_avg_move": 25.0}
    assert start_meta(META, {})["fork_avg_move"] == 0.0      # no fork: no average
