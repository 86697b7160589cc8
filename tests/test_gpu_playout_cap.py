"""Playout cap randomization of the tree search (LzTreeDesc.sim_budget / root_noise, PortableTreeMCTS(fast_simulations,
full_prob), self_play_tree_gpu(playout_cap_*)): a game's fast search is bit for bit a search of `fast` simulations without
root noise, its full search one of `sims` simulations with noise; only full searches record rows."""
import numpy as np
import pytest
import torch

from tests.golden_utils import load, states, FIELDS
from tests.tree_parity import to_gpu_batch, EDGE_LOGICAL

DEV = torch.device("cuda:0")
SEED = 7


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _net():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    torch.manual_seed(20260314)
    return FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))


def _positions(idx):
    st_all = states(load("g1_rules.npz"), "s")
    return to_gpu_batch({f: np.ascontiguousarray(np.asarray(st_all[f])[idx]) for f in FIELDS}, DEV)


def _game_tree(e, g):
    nodes = e.game_nodes(g)
    runs = [tuple(e.edge_run(int(n["edge_begin"]), max(0, int(n["nedges"])))[f].tobytes() for f in EDGE_LOGICAL)
            for n in nodes]
    return tuple(nodes[f].tobytes() for f in ("w0", "w1", "w2", "w3", "nedges", "parent")), runs


def _play(m, ids, games, moves, full=None):
    """`moves` searches of the positions `ids` (global game ids `ids`) with kept subtrees; per move the outputs, then the
    trees.  `full`: the injected full / fast mask (the same for every move)."""
    from liuzhou_amd import v0_core
    batch = _positions(np.asarray(ids) % 997)
    n = len(ids)
    gid = torch.as_tensor(np.asarray(ids), dtype=torch.int64, device=DEV)
    if full is not None:
        m.injected_full_search = full
    outs = []
    for t in range(moves):
        plies = torch.full((n,), t, dtype=torch.int64, device=DEV)
        out = m.search_batch(batch, temperatures=torch.ones(n, device=DEV), rng_game_ids=gid, rng_plies=plies)
        outs.append((out.chosen_action_indices.clone(), out.policy_dense.clone(), out.root_value.clone()))
        done = torch.zeros(n, dtype=torch.bool, device=DEV)
        v0_core.self_play_step_inplace(*batch.tensors(), plies.clone(), done, torch.arange(n, device=DEV),
                                       out.chosen_action_codes.clone(), out.terminal_mask.clone(),
                                       out.chosen_valid_mask.clone(), 512, 2.0)
    torch.cuda.synchronize()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("graph", [True, False])
def test_fast_and_full_searches_equal_uniform_searches_of_their_budget(monkeypatch, split, graph):
    """Injected mask over 40 games, 3 moves with kept subtrees: every game's picks, policies, root values and tree records
    equal those of an engine that searches only the full games (sims = S, noise, dense launches) or only the fast ones
    (sims = F, no noise).  One-wave step (LZ_TREE_SPLIT=0) and two-wave split step; graph and direct launches."""
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    monkeypatch.setenv("LZ_TREE_SPLIT", split)
    net = _net()
    B, S, F, moves = 40, 24, 6, 3
    full = torch.from_numpy(np.random.default_rng(3).random(B) < 0.5).to(DEV)
    kw = dict(sample_moves=True, reuse_tree=True, reuse_factor=4.0, seed=SEED, use_graph=graph)
    capped = PortableTreeMCTS(net, B, S, DEV, add_dirichlet_noise=True, fast_simulations=F, full_prob=0.5, **kw)
    ids = list(range(100, 100 + B))
    got = _play(capped, ids, B, moves, full=full)
    assert torch.equal(capped.last_full_search, full)
    fi = [g for g in range(B) if bool(full[g])]
    si = [g for g in range(B) if not bool(full[g])]
    ref_full = PortableTreeMCTS(net, len(fi), S, DEV, add_dirichlet_noise=True, compact_evals=False, **kw)
    ref_fast = PortableTreeMCTS(net, len(si), F, DEV, add_dirichlet_noise=False, compact_evals=False, **kw)
    for ref, sub in ((ref_full, fi), (ref_fast, si)):
        want = _play(ref, [ids[g] for g in sub], len(sub), moves)
        sel = torch.as_tensor(sub, device=DEV)
        for (ca, pa, va), (cb, pb, vb) in zip(got, want):
            assert torch.equal(ca.index_select(0, sel), cb)
            assert torch.equal(pa.index_select(0, sel), pb)
            assert torch.equal(va.index_select(0, sel), vb)
        for j, g in enumerate(sub):
            assert _game_tree(capped.engine, g) == _game_tree(ref.engine, j)
            assert int(capped.engine.buf["root_visits"][g]) == int(ref.engine.buf["root_visits"][j])
    assert int(capped.engine.reuse_dropped.sum()) == 0
    # full searches launch S + 1 evaluations at most, fast ones F + 1: the lists shrink with the budgets
    assert capped.leaf_evals <= moves * (len(fi) * (S + 1) + len(si) * (F + 1))


@pytest.mark.gpu
def test_dual_stream_halves_search_like_one_engine():
    """DualStreamTreeMCTS with the cap: both halves draw their games' masks from the global game ids and search exactly
    like one PortableTreeMCTS over all games."""
    _need_gpu()
    from liuzhou_amd.tree_engine import DualStreamTreeMCTS, PortableTreeMCTS
    net = _net()
    B, S, F = 48, 16, 4
    kw = dict(add_dirichlet_noise=True, sample_moves=True, reuse_tree=True, reuse_factor=4.0, seed=SEED,
              fast_simulations=F, full_prob=0.4)
    ids = list(range(B))
    dual = DualStreamTreeMCTS(net, B, S, DEV, **kw)
    one = PortableTreeMCTS(net, B, S, DEV, **kw)
    a = _play(dual, ids, B, 3)
    b = _play(one, ids, B, 3)
    assert torch.equal(dual.last_full_search, one.last_full_search)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert torch.equal(u, v)
    assert torch.equal(dual.cap_counts, one.cap_counts)


@pytest.mark.gpu
def test_device_draws_equal_the_oracle():
    """full_search of a move = oracle.rng_oracle.uniform(seed, game, ply, 3) < p for every (game id, ply)."""
    _need_gpu()
    from oracle import rng_oracle
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    B, S, F, p = 64, 8, 2, 0.3
    m = PortableTreeMCTS(_net(), B, S, DEV, fast_simulations=F, full_prob=p, seed=SEED, use_graph=False)
    batch = _positions(np.arange(B))
    for ply in (0, 5, 17):
        gid = torch.arange(1000, 1000 + B, dtype=torch.int64, device=DEV)
        plies = torch.full((B,), ply, dtype=torch.int64, device=DEV)
        m.search_batch(batch, temperatures=torch.ones(B, device=DEV), rng_game_ids=gid, rng_plies=plies)
        want = rng_oracle.uniform(SEED, np.arange(1000, 1000 + B), ply, 3) < p
        assert np.array_equal(m.last_full_search.cpu().numpy(), want)
        budget = m.sim_budget.cpu().numpy()
        assert np.array_equal(budget, np.where(want, S, F))


def _selfplay(net, **kw):
    from liuzhou_amd.tree_engine import self_play_tree_gpu, clear_engine_cache
    args = dict(num_games=24, mcts_simulations=16, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                exploration_weight=1.0, device=str(DEV), concurrent_games=12, max_game_plies=40, seed=SEED)
    args.update(kw)
    out = self_play_tree_gpu(net, **args)
    clear_engine_cache()
    return out


def _batch_equal(a, b):
    for f in ("state_tensors", "legal_masks", "policy_targets", "value_targets", "soft_value_targets"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x,
                                                  y.view(torch.uint8) if y.dtype == torch.bool else y), f


def _stats_key(st):
    return (st.num_games, st.num_positions, st.black_wins, st.white_wins, st.draws, st.avg_game_length,
            dict(st.piece_delta_buckets))


@pytest.mark.gpu
@pytest.mark.parametrize("device_tail", [True, False])
def test_full_prob_one_equals_the_cap_off(device_tail):
    _need_gpu()
    net = _net()
    ba, sa = _selfplay(net, device_tail=device_tail)
    bb, sb = _selfplay(net, device_tail=device_tail, playout_cap_fast_simulations=4, playout_cap_full_prob=1.0)
    _batch_equal(ba, bb)
    assert _stats_key(sa) == _stats_key(sb)
    assert sb.mcts_counters["fast_searches"] == 0
    assert sb.mcts_counters["full_searches"] == sb.num_positions == sb.mcts_counters["recorded_positions"]


@pytest.mark.gpu
@pytest.mark.parametrize("device_tail", [True, False])
def test_rows_are_the_full_searches_and_every_game_is_booked(device_tail):
    _need_gpu()
    net = _net()
    b, st = _selfplay(net, device_tail=device_tail, playout_cap_fast_simulations=4, playout_cap_full_prob=0.3)
    c = st.mcts_counters
    assert b.num_samples == st.num_positions == c["full_searches"] == c["recorded_positions"]
    assert c["fast_searches"] > 0 and c["full_searches"] > 0
    assert st.black_wins + st.white_wins + st.draws == st.num_games
    # plies, not rows: every search of a live game is one ply of some game
    assert abs(st.avg_game_length * st.num_games - (c["full_searches"] + c["fast_searches"])) < 1e-3 * st.num_games
    assert torch.isfinite(b.value_targets).all() and set(b.value_targets.unique().tolist()) <= {-1.0, 0.0, 1.0}
    pol = b.policy_targets
    assert torch.allclose(pol.sum(1), torch.ones(pol.shape[0], device=pol.device), atol=1e-4)
    assert not (pol * (~b.legal_masks).to(pol.dtype)).any()
    # every game's searches fast: no row at all, yet every game counts
    b0, s0 = _selfplay(net, device_tail=device_tail, playout_cap_fast_simulations=4, playout_cap_full_prob=0.0)
    assert b0.num_samples == 0 and s0.num_positions == 0 and s0.mcts_counters["full_searches"] == 0
    assert s0.black_wins + s0.white_wins + s0.draws == s0.num_games
    if device_tail:                                     # (the host loop keeps no piece-difference histogram)
        assert sum(s0.piece_delta_buckets.values()) == s0.num_games


@pytest.mark.gpu
def test_rows_through_the_finished_row_log():
    """The streaming worker's path (row_log): the same rows and outcomes as the chunk path with the cap on."""
    _need_gpu()
    from liuzhou_amd.finished_log import FinishedRowLog
    net = _net()
    kw = dict(playout_cap_fast_simulations=4, playout_cap_full_prob=0.3)
    b, st = _selfplay(net, **kw)
    log = FinishedRowLog(DEV, segment_games=8, num_slots=12, max_steps=40)
    _, sl = _selfplay(net, row_log=log, **kw)
    assert _stats_key(sl)[:5] == _stats_key(st)[:5] and sl.avg_game_length == st.avg_game_length
    assert sl.mcts_counters["full_searches"] == st.mcts_counters["full_searches"]


@pytest.mark.gpu
def test_same_seed_same_games_whatever_the_wave_size():
    _need_gpu()
    net = _net()
    kw = dict(playout_cap_fast_simulations=4, playout_cap_full_prob=0.3)
    b1, s1 = _selfplay(net, **kw)
    b2, s2 = _selfplay(net, **kw)
    _batch_equal(b1, b2)
    assert _stats_key(s1) == _stats_key(s2)
    b3, s3 = _selfplay(net, concurrent_games=8, **kw)
    assert _stats_key(s3) == _stats_key(s1)
    rows = lambda b: sorted(b.state_tensors[i].cpu().numpy().tobytes() + b.policy_targets[i].cpu().numpy().tobytes() +
                            b.value_targets[i:i + 1].cpu().numpy().tobytes() for i in range(b.num_samples))
    assert rows(b1) == rows(b3)


@pytest.mark.gpu
def test_refusals(monkeypatch):
    _need_gpu()
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.tree_engine import PortableTreeMCTS, PriorEvaluator
    net = _net()
    cap = dict(fast_simulations=4, full_prob=0.5)
    with pytest.raises(ValueError):
        PortableTreeMCTS(net, 16, 16, DEV, batch_k=2, **cap)
    with pytest.raises(ValueError):
        PortableTreeMCTS([net, net], 32, 16, DEV, segment_games=16, **cap)
    with pytest.raises(ValueError):
        PortableTreeMCTS(PriorEvaluator(lambda p, s: None), 16, 16, DEV, **cap)
    with pytest.raises(ValueError):
        PortableTreeMCTS(net, 16, 16, DEV, fast_simulations=16, full_prob=0.5)
    with pytest.raises(ValueError):
        PortableTreeMCTS(net, 16, 16, DEV, fast_simulations=4, full_prob=1.5)
    with pytest.raises(ValueError):
        _selfplay(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV), evaluator="module", playout_cap_fast_simulations=4,
                  playout_cap_full_prob=0.5)
    with pytest.raises(ValueError):
        _selfplay(net, batch_k=2, playout_cap_fast_simulations=4, playout_cap_full_prob=0.5)
    monkeypatch.setenv("LZ_TREE_PERSISTENT", "1")
    with pytest.raises(ValueError):
        PortableTreeMCTS(net, 16, 16, DEV, **cap)
