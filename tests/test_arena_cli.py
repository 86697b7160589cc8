"""CPU: argument handling of scripts/eval_arena.py (`--backend portable` selects the tree backend, the v1 defaults stay)
and the payload keys of the arena's results."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec = importlib.util.spec_from_file_location("eval_arena_cli", os.path.join(ROOT, "scripts", "eval_arena.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_backend_selection_and_accepted_flags():
    cli = _cli()
    a = cli.parse(["--challenger_checkpoint", "c.pt"])
    assert a.backend == "v1" and cli.backend_of(a) == "v1" and a.mcts_simulations == 256 and a.temperature == 0.05
    assert a.ignored == []
    p = cli.parse(["--challenger_checkpoint", "c.pt", "--backend", "portable", "--portable_mcts_backend", "python",
                   "--portable_cpp_threads", "8", "--train_devices", "cuda:0"])
    assert cli.backend_of(p) == "portable"
    assert p.ignored == ["--train_devices", "cuda:0"]                 # other backends' flags: accepted and ignored
    for other in ("v1", "legacy", "v0"):
        assert cli.backend_of(cli.parse(["--challenger_checkpoint", "c.pt", "--backend", other])) == "v1"


def test_payload_keys():
    from liuzhou_amd.eval_arena import EvaluationStats, RoundRobinResult, SEARCH_BACKENDS, make_agent
    st = EvaluationStats(wins=3, losses=1, draws=0, total_games=4,
                         color_breakdown={"black": {"wins": 2, "losses": 0, "draws": 0, "games": 2}})
    p = st.to_payload("vs_previous")
    assert set(p) == {"name", "wins", "losses", "draws", "total_games", "win_rate", "loss_rate", "draw_rate",
                      "color_breakdown"}
    assert p["win_rate"] == 0.75
    wdl = torch.zeros((2, 2, 3), dtype=torch.int64)
    wdl[0, 1] = torch.tensor([3, 0, 1]); wdl[1, 0] = torch.tensor([1, 0, 3])
    rr = RoundRobinResult(wdl=wdl, points=[9, 3], pairs=[(0, 1)], pair_stats={(0, 1): st})
    q = rr.to_payload(["a", "b"])
    assert q["models"] == ["a", "b"] and q["points"] == [9, 3] and q["wdl"][1][0] == [1, 0, 3]
    assert q["pairs"][0]["a"] == "a" and q["pairs"][0]["wins"] == 3
    assert SEARCH_BACKENDS == ("v1", "portable")
    with pytest.raises(ValueError):
        make_agent(None, "tree", "cpu", 8, 0.1, False)
