"""GPU: the arena's tree backend (TreeSearchAgent, `--backend portable`) -- one joint search per ply over both sides'
games must play exactly what one search per agent plays; checkpoint evaluation, the CLI and the round robin on top."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(seed, config="b6c64"):
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    m = ChessNet(**MODEL_CONFIGS[config])
    stable_resnet_init(m, seed)
    return m.eval()


def _trim(log):
    keep = (log >= 0).any(dim=0).nonzero().view(-1)
    return log[:, : int(keep.max()) + 1] if keep.numel() else log[:, :0]


def _same(a, b):
    assert (a.wins, a.losses, a.draws, a.color_breakdown) == (b.wins, b.losses, b.draws, b.color_breakdown)
    assert torch.equal(_trim(a.move_log), _trim(b.move_log))


@pytest.mark.parametrize("sample", [False, True])
def test_joint_search_plays_what_per_agent_searches_play(sample):
    _need_gpu()
    from liuzhou_amd.eval_arena import TreeSearchAgent, play_matches
    mk = lambda s: TreeSearchAgent(_model(s), DEV, 12, temperature=1.0 if sample else 0.1, sample_moves=sample, seed=4)
    a, b = mk(20260314), mk(7)
    kw = dict(max_game_plies=90, record_moves=True, seed=5, opening_random_moves=2)
    joint = play_matches(a, b, 26, DEV, joint=True, **kw)
    alone = play_matches(a, b, 26, DEV, joint=False, **kw)
    _same(joint, alone)
    assert joint.total_games == 26 and joint.wins + joint.losses + joint.draws == 26
    assert joint.move_log.shape[0] == 26 and int((joint.move_log >= 0).sum()) > 26 * 4


def test_tree_agent_against_random():
    _need_gpu()
    from liuzhou_amd.eval_arena import RandomAgent, TreeSearchAgent, play_matches
    a = TreeSearchAgent(_model(3), DEV, 8)
    r1 = play_matches(a, RandomAgent(), 20, DEV, max_game_plies=80, seed=2, record_moves=True)
    r2 = play_matches(a, RandomAgent(), 20, DEV, max_game_plies=80, seed=2, record_moves=True, joint=False)
    _same(r1, r2)
    assert r1.total_games == 20


def _checkpoints(tmp_path, seeds):
    paths = []
    for seed in seeds:
        p = tmp_path / f"model_{seed}.pt"
        torch.save({"model_state_dict": _model(seed).state_dict()}, p)
        paths.append(str(p))
    return paths


def test_evaluate_checkpoint_portable(tmp_path):
    _need_gpu()
    from liuzhou_amd.eval_arena import evaluate_checkpoint
    paths = _checkpoints(tmp_path, (20260314, 7))
    keys = {"name", "wins", "losses", "draws", "total_games", "win_rate", "loss_rate", "draw_rate", "color_breakdown",
            "seed"}
    r = evaluate_checkpoint(paths[0], None, num_games=17, device=DEV, mcts_simulations=8, opening_random_moves=4,
                            max_game_plies=100, seed=1, search_backend="portable")
    v1 = evaluate_checkpoint(paths[0], None, num_games=17, device=DEV, mcts_simulations=8, opening_random_moves=4,
                             max_game_plies=100, seed=1)
    assert set(r) == set(v1) == keys
    assert r["name"] == "vs_random" and r["total_games"] == 16 and r["wins"] + r["losses"] + r["draws"] == 16
    r2 = evaluate_checkpoint(paths[0], paths[1], num_games=16, device=DEV, mcts_simulations=8, max_game_plies=100, seed=2,
                             search_backend="portable")
    assert set(r2) == keys and r2["name"] == "vs_previous" and r2["wins"] + r2["losses"] + r2["draws"] == 16
    with pytest.raises(ValueError):
        evaluate_checkpoint(paths[0], None, num_games=2, device=DEV, search_backend="tree")


def test_cli_reports_the_backend_that_ran(tmp_path):
    _need_gpu()
    paths = _checkpoints(tmp_path, (11, 12))
    out = tmp_path / "eval.json"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "eval_arena.py"), "--challenger_checkpoint", paths[0],
           "--previous_checkpoint", paths[1], "--backend", "portable", "--portable_mcts_backend", "python",
           "--portable_cpp_threads", "4", "--eval_games_vs_previous", "8", "--mcts_simulations", "6",
           "--output_json", str(out)]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=600)
    res = json.loads(out.read_text())
    assert res["backend"] == "portable" and res["vs_previous"]["total_games"] == 8


def test_round_robin_equals_the_pairwise_matches():
    _need_gpu()
    from liuzhou_amd.eval_arena import TreeSearchAgent, play_matches, play_round_robin
    agents = [TreeSearchAgent(_model(s), DEV, 10) for s in (1, 2, 3)]
    rr = play_round_robin(agents, 6, DEV, max_game_plies=80, record_moves=True)
    assert rr.pairs == [(0, 1), (0, 2), (1, 2)]
    for (i, j) in rr.pairs:
        ref = play_matches(agents[i], agents[j], 6, DEV, max_game_plies=80, record_moves=True)
        _same(rr.pair_stats[(i, j)], ref)
        assert rr.wdl[i, j, 0] == rr.wdl[j, i, 2] and rr.wdl[i, j, 1] == rr.wdl[j, i, 1]
    for i in range(3):
        assert rr.points[i] == int(3 * rr.wdl[i, :, 0].sum() + rr.wdl[i, :, 1].sum())
        assert int(rr.wdl[i].sum()) == 12
    per = play_round_robin(agents, 6, DEV, max_game_plies=80, record_moves=True, joint=False)
    assert torch.equal(per.wdl, rr.wdl)


def test_tree_arena_reproduces_the_reference_portable_worker():
    """g19 (scripts/gen_golden_tree_arena.py): the reference's own arena worker on its tree backend
    (`_eval_worker_v1(search_backend="portable", portable_mcts_backend="python")`, two tiny checkpoints, deterministic
    picks, no random openings) recorded on CPU -- outcome tuple, every game's moves, every evaluation of both agents.  The
    tree backend, both networks replaced by tables of those evaluations (searched jointly, through the split-phase path),
    must play the same moves, count the same results, and evaluate no position the reference did not."""
    _need_gpu()
    import numpy as np
    from liuzhou_amd.eval_arena import TreeSearchAgent, play_matches
    from tests.golden_utils import load
    z = load("g19_tree_arena.npz")
    G, sims = (int(x) for x in z["config"])

    def fnv64(rows):
        h = np.full(rows.shape[0], 0xCBF29CE484222325, np.uint64)
        for j in range(rows.shape[1]):
            h = (h ^ rows[:, j].astype(np.uint64)) * np.uint64(0x100000001B3)
        return h

    class TableNet(torch.nn.Module):
        """forward(planes) -> (log_p1, log_p2, log_pmc, value[N,1]) looked up by the packed planes."""
        def __init__(self, tag):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1))
            self.rows = {int(k): i for i, k in enumerate(z[f"{tag}_keys"])}
            self.heads, self.vals = z[f"{tag}_heads"], z[f"{tag}_values"]
            self.misses = 0

        def forward(self, x):
            keys = fnv64(np.packbits(x.detach().float().cpu().numpy().astype(bool).reshape(x.shape[0], -1), axis=1))
            heads = np.zeros((x.shape[0], 108), np.float32); val = np.zeros((x.shape[0], 1), np.float32)
            for i, k in enumerate(keys.tolist()):
                r = self.rows.get(k)
                if r is None:
                    self.misses += 1
                    continue
                heads[i], val[i, 0] = self.heads[r], self.vals[r]
            t = lambda a: torch.from_numpy(a).to(x.device)
            return t(heads[:, 0:36].copy()), t(heads[:, 36:72].copy()), t(heads[:, 72:108].copy()), t(val)

    nets = {tag: TableNet(tag) for tag in ("chall", "opp")}
    agents = {tag: TreeSearchAgent(nets[tag], DEV, sims, temperature=0.1, sample_moves=False) for tag in nets}
    stats = play_matches(agents["chall"], agents["opp"], G, DEV, record_moves=True)
    cb = stats.color_breakdown
    got = [stats.wins, stats.losses, stats.draws, cb["black"]["wins"], cb["black"]["losses"], cb["black"]["draws"],
           cb["white"]["wins"], cb["white"]["losses"], cb["white"]["draws"]]
    moves = stats.move_log.cpu().numpy()
    ref = z["moves"]
    L = ref.shape[1]
    assert moves.shape[1] >= L
    assert np.array_equal(moves[:, :L], ref), "the games diverge from the reference worker's move sequences"
    assert (moves[:, L:] == -1).all()
    assert got == [int(v) for v in z["result"]], got
    assert nets["chall"].misses == 0 and nets["opp"].misses == 0, "a position the reference never evaluated was searched"


def test_a_kept_challenger_meets_each_new_opponent():
    """The joint engine kept between matches must follow the opponent: one challenger against two opponents created one
    after the other (the first one dropped) plays what a fresh challenger plays against the second."""
    _need_gpu()
    import gc
    from liuzhou_amd.eval_arena import TreeSearchAgent, play_matches
    kw = dict(max_game_plies=70, record_moves=True, seed=3)
    chall = TreeSearchAgent(_model(20260314), DEV, 8)
    opp = TreeSearchAgent(_model(7), DEV, 8)
    first = play_matches(chall, opp, 18, DEV, **kw)
    del opp
    gc.collect()
    second = play_matches(chall, TreeSearchAgent(_model(8), DEV, 8), 18, DEV, **kw)
    fresh = play_matches(TreeSearchAgent(_model(20260314), DEV, 8), TreeSearchAgent(_model(8), DEV, 8), 18, DEV, **kw)
    _same(second, fresh)
    assert sum(1 for k in chall._engines if isinstance(k, tuple)) == 1          # one joint engine kept per agent
    assert first.total_games == second.total_games == 18
