"""CPU: the Gumbel root search's parameters through scripts/selfplay_stage.py, run_self_play_stage, the worker, the engines'
constructors and the manifests."""
import math
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
    a = cli.parse(["--search_backend", "tree", "--mcts_simulations", "64", "--gumbel_considered", "16",
                   "--gumbel_c_visit", "25", "--gumbel_c_scale", "0.5"])
    assert a.gumbel_considered == 16 and a.gumbel_c_visit == 25.0 and a.gumbel_c_scale == 0.5 and a.ignored == []
    d = cli.parse([])
    assert d.gumbel_considered == 0 and d.gumbel_c_visit == 50.0 and d.gumbel_c_scale == 1.0


def test_validation():
    from liuzhou_amd.gumbel import gumbel_on
    assert gumbel_on(0) is False and gumbel_on(16) is True and gumbel_on(72, 0.0, 0.0) is True
    for m in (-1, 73):
        with pytest.raises(ValueError):
            gumbel_on(m)
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            gumbel_on(16, bad, 1.0)
        with pytest.raises(ValueError):
            gumbel_on(16, 50.0, bad)


def _stage(tmp_path, worker_fn, **kw):
    from liuzhou_amd.self_play_stage import run_self_play_stage
    return run_self_play_stage(model_state={"w": torch.zeros(2)}, num_games=10, devices=["cuda:0", "cuda:1"],
                               output_path=str(tmp_path / "sp.pt"), iteration_seed=2, mcts_simulations=32,
                               concurrent_games_per_device=4, worker_fn=worker_fn, in_process=True, **kw)


GUMBEL_KEYS = ("gumbel_considered", "gumbel_c_visit", "gumbel_c_scale")


def test_kwargs_reach_the_worker_only_when_on(tmp_path):
    seen = []

    def spy(**kw):
        seen.append(kw)
        return stub_worker(**{k: v for k, v in kw.items() if k not in GUMBEL_KEYS})

    _stage(tmp_path / "off", spy, search_backend="tree")
    _stage(tmp_path / "zero", spy, search_backend="tree", gumbel_considered=0, gumbel_c_visit=10.0, gumbel_c_scale=2.0)
    assert len(seen) == 4 and all(not any(k in kw for k in GUMBEL_KEYS) for kw in seen)
    seen.clear()
    _stage(tmp_path / "on", spy, search_backend="tree", gumbel_considered=16, gumbel_c_visit=25.0)
    assert len(seen) == 2
    assert all(kw["gumbel_considered"] == 16 and kw["gumbel_c_visit"] == 25.0 and kw["gumbel_c_scale"] == 1.0
               for kw in seen)


WORKER_COMMON = dict(worker_idx=0, shard_device="cuda:0", shard_games=1, seed=1, model_state_path="x", output_path="y",
                     mcts_simulations=32, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                     exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25, soft_value_k=2.0,
                     opening_random_moves=0, max_game_plies=64, concurrent_games_per_device=1)


def test_stage_and_worker_refuse(tmp_path, monkeypatch):
    from liuzhou_amd.self_play_worker import run_self_play_worker
    refusals = (dict(search_backend="cuda_root"),
                dict(search_backend="tree", forced_playouts_k=2.0),
                dict(search_backend="tree", policy_target_temperature=0.5),
                dict(search_backend="tree", policy_target_prior_pseudocount=0.5))
    for kw in refusals:
        with pytest.raises(ValueError):
            _stage(tmp_path, stub_worker, gumbel_considered=16, **kw)
        with pytest.raises(ValueError):
            run_self_play_worker(gumbel_considered=16, **kw, **WORKER_COMMON)
    for bad in (dict(gumbel_considered=-1), dict(gumbel_considered=73), dict(gumbel_considered=16, gumbel_c_visit=-1.0),
                dict(gumbel_considered=16, gumbel_c_scale=math.nan), dict(gumbel_considered=16, gumbel_c_visit=math.inf)):
        with pytest.raises(ValueError):
            _stage(tmp_path, stub_worker, search_backend="tree", **bad)
        with pytest.raises(ValueError):
            run_self_play_worker(search_backend="tree", **bad, **WORKER_COMMON)
    monkeypatch.setenv("LZ_TREE_PERSISTENT", "1")
    with pytest.raises(ValueError, match="persistent"):
        _stage(tmp_path, stub_worker, search_backend="tree", gumbel_considered=16)
    with pytest.raises(ValueError, match="persistent"):
        run_self_play_worker(search_backend="tree", gumbel_considered=16, **WORKER_COMMON)


def test_every_refusal_names_its_reason(monkeypatch):
    from liuzhou_amd.search_rules import SearchRules, persistent_default
    gumbel_refusal = SearchRules.parse(32, gumbel_considered=16).refusal
    assert gumbel_refusal() is None
    for kw, word in ((dict(batch_k=2), "batch_k"), (dict(several_networks=True), "several networks"),
                     (dict(fused=False), "external evaluator"),
                     (dict(policy_target_temperature=1.0), "policy_target_temperature"),
                     (dict(policy_target_prior_pseudocount=0.25), "policy_target_prior_pseudocount")):
        assert word in gumbel_refusal(**kw), kw
    assert "forced playouts" in SearchRules.parse(32, gumbel_considered=16, forced_playouts_k=2.0).refusal()
    monkeypatch.setenv("LZ_TREE_PERSISTENT", "1")
    assert "persistent" in gumbel_refusal(persistent=persistent_default())


def test_engines_refuse_before_they_touch_a_device(monkeypatch):
    """The constructors check the configuration first, so the refusals are visible without a GPU."""
    from liuzhou_amd.tree_engine import PortableTreeMCTS, self_play_tree_gpu
    module = torch.nn.Linear(1, 1)
    for kw, word in ((dict(batch_k=2), "batch_k"), (dict(), "external evaluator"),
                     (dict(segment_games=16), "several networks")):
        with pytest.raises(ValueError, match=word):
            PortableTreeMCTS(module, 32, 16, "cpu", gumbel_considered=8, **kw)
    with pytest.raises(ValueError):
        PortableTreeMCTS(module, 32, 16, "cpu", gumbel_considered=80)
    with pytest.raises(ValueError, match="external evaluator"):
        self_play_tree_gpu(module, 2, 16, 1.0, 0.1, 10, 1.0, "cpu", evaluator="module", gumbel_considered=8)
    with pytest.raises(ValueError):
        self_play_tree_gpu(module, 2, 16, 1.0, 0.1, 10, 1.0, "cpu", evaluator="module", gumbel_considered=8,
                           gumbel_c_scale=-1.0)


def _gumbel_worker(**kw):
    """The stub worker as the real one reports the mode: settings in its metadata, the searches in its counters."""
    from liuzhou_amd import self_play_worker as W
    on = "gumbel_considered" in kw
    orig = W.write_worker_chunks

    def write(run_once, **a):
        if on:
            a["meta_common"] = {**a["meta_common"], "gumbel": {"considered": kw["gumbel_considered"],
                                                               "c_visit": kw["gumbel_c_visit"],
                                                               "c_scale": kw["gumbel_c_scale"]}}

        def run(n, **x):
            b, st = run_once(n, **x)
            if on:
                st.mcts_counters.update(gumbel_searches=st.num_positions)
            return b, st
        return orig(run, **a)

    import tests.stage_stub as S
    S.write_worker_chunks = write
    try:
        return S.stub_worker(**{k: v for k, v in kw.items() if k not in GUMBEL_KEYS})
    finally:
        S.write_worker_chunks = orig


def test_manifest_metadata_on_and_off(tmp_path):
    _, off = _stage(tmp_path / "off", _gumbel_worker, search_backend="tree")
    assert "gumbel" not in off["metadata"]
    _, on = _stage(tmp_path / "on", _gumbel_worker, search_backend="tree", gumbel_considered=16, gumbel_c_scale=0.5)
    assert on["metadata"]["gumbel"] == {"considered": 16, "c_visit": 50.0, "c_scale": 0.5,
                                        "gumbel_searches": on["num_samples"]}
    assert set(on) == set(off)                          # the manifest's own keys are unchanged
    assert set(on["metadata"]) - set(off["metadata"]) == {"gumbel"}
