"""MCTS-Solver of the tree search (LzTreeDesc.solver / root_proven / solver_count, lz_tree_solver_pick,
PortableTreeMCTS(solver), self_play_tree_gpu(mcts_solver)) against the pure-Python tree of tests/solver_tree.py on the
generated positions of solver_tree.solver_positions(): the same leaves at every simulation, bit-identical root statistics
and info bytes, equal root results, counters and picks."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lz_oracle as O
from tests import solver_tree as ST
from tests.golden_utils import FIELDS
from tests.tree_parity import (EDGE_LOGICAL, game_tree, hash_evaluator, replay_part_in_oracle, root_edges, to_gpu_batch,
                               unpack_packed)

DEV = torch.device("cuda:0")
SEED = 7


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_NET = []


def _net():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    if not _NET:
        torch.manual_seed(20260314)
        _NET.append(FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV)))
    return _NET[0]


def _all_positions():
    pos = ST.solver_positions()
    return pos["win"] + pos["decided"] + pos["open"]


def _deterministic_pick(t):
    from oracle.selfplay_oracle import deterministic_pick
    idx, vis, vs, pr, pl = t.root_children()
    return deterministic_pick(idx, vis, vs, pr, pl, t.root_player())


def _compare_roots(eng, trees, tag):
    """Root edges of every game against the checker: visits, f64 value sums, priors and info bytes bit for bit; the root
    result and the counter."""
    edges = root_edges(eng)
    rp = eng.root_proven.cpu().numpy()
    sc = eng.solver_count.cpu().numpy()
    for i, t in enumerate(trees):
        assert int(rp[i]) == t.root_proven, (tag, i, "root_proven differs", int(rp[i]), t.root_proven)
        assert int(sc[i]) == t.solver_count, (tag, i, "solver_count differs", int(sc[i]), t.solver_count)
        if t.root_terminal():
            continue
        idx, vis, vs, pr, _pl = t.root_children()
        E = edges[i]
        assert np.array_equal(E["act"].astype(np.int64), idx.astype(np.int64)), (tag, i)
        assert np.array_equal((E["n_info"] & 0xFFFFFF).astype(np.int64), vis.astype(np.int64)), (tag, i, "visits differ")
        assert np.array_equal(E["W"].view(np.uint64), vs.astype(np.float64).view(np.uint64)), (tag, i, "W sums differ")
        assert np.array_equal(E["P"].view(np.uint32), pr.astype(np.float32).view(np.uint32)), (tag, i, "priors differ")
        assert np.array_equal((E["n_info"] >> 24).astype(np.uint8), t.root_infos()), (tag, i, "info bytes differ")


def _compare_trees(eng, trees, tag, on_cut=None):
    """Every edge of every game's device tree against the checker, walked in parallel from the root: visits, f64 value
    sums, priors and info bytes bit for bit, and a node on the device wherever the checker has expanded one.  `on_cut(i,
    node, edge record)` is called for an edge that has no node on the device where the checker has one (an advance that
    pruned); without it such an edge is an error.  Returns the number of edges compared below the root level."""
    deep = 0
    for i, t in enumerate(trees):
        nodes, runs = game_tree(eng, i)
        if t.root_terminal() or int(nodes[0]["nedges"]) <= 0:
            continue
        stack = [(0, t.root)]
        while stack:
            dn, cn = stack.pop()
            E, n = runs[dn], t.nodes[cn]
            assert len(E) == n.n_children, (tag, i, dn, "edge counts differ")
            for k in range(n.n_children):
                c = n.first_child + k
                ch = t.nodes[c]
                assert int(E["act"][k]) == ch.action_index and int(E["n_info"][k] & 0xFFFFFF) == ch.visit_count, (tag, i, dn, k)
                assert E["W"][k:k + 1].view(np.uint64)[0] == np.array([ch.value_sum], np.float64).view(np.uint64)[0], (tag, i, dn, k)
                assert E["P"][k:k + 1].view(np.uint32)[0] == np.array([ch.prior], np.float32).view(np.uint32)[0], (tag, i, dn, k)
                assert int(E["n_info"][k] >> 24) == t.info_byte(c), (tag, i, dn, k, "info bytes differ")
                deep += int(dn != 0)
                has = ch.expanded and ch.n_children > 0
                if int(E["child"][k]) >= 0:
                    assert has, (tag, i, dn, k, "a node on the device that the checker has not expanded")
                    stack.append((int(E["child"][k]), c))
                elif has:
                    assert on_cut is not None, (tag, i, dn, k, "the checker has a node here, the device has none")
                    on_cut(i, c, E[k])
    return deep


def _injected_step(eng, trees, is_root, tag):
    """One step of the step-by-step protocol under hash_evaluator on both sides: the same games need an evaluation, of the
    same leaf state; the root results agree afterwards."""
    kind = eng.buf["leaf_kind"].cpu().numpy()
    leaf = unpack_packed(eng.buf["leaf_state"].cpu().numpy())
    pend = [t.prepare_root() if is_root else t.select() for t in trees]
    assert np.array_equal(kind == 1, np.array(pend)), (tag, "GPU and checker disagree on which games need an evaluation")
    need = np.nonzero(pend)[0]
    if need.size:
        want = O.batch_from_states([trees[i].pending_state() for i in need])
        for f in FIELDS:
            a = np.asarray(leaf[f])[need].reshape(need.size, -1).astype(np.int64)
            b = np.asarray(want[f]).reshape(need.size, -1).astype(np.int64)
            assert np.array_equal(a, b), f"{tag}: leaf state field {f} differs"
    pri, val = hash_evaluator(leaf)
    for i in need:
        trees[i].complete(pri[i], float(val[i]))
    eng.expand(is_root=is_root, values=torch.from_numpy(val).to(DEV), priors220=torch.from_numpy(pri).to(DEV))
    assert eng.root_proven.cpu().tolist() == [t.root_proven for t in trees], (tag, "root_proven differs")


# ---- 1. step by step against the checker -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_step_by_step_against_the_checker():
    """lz_tree_select / lz_tree_expand with injected priors and values on the 24 generated positions (12 forced wins, 6 proven
    draws or losses, 6 open), 100 simulations, then a second move with kept subtrees: the same leaf at every simulation, the
    root result equal after every step, bit-identical root edges, equal counters, and the pick of lz_tree_solver_pick equal
    to the checker's.  Found by the checker alone (tests/test_solver_tree_cpu.py): at least 8 roots proven won."""
    _need_gpu()
    from liuzhou_amd.tree_engine import TreeEngine
    cur = _all_positions()
    B, sims = len(cur), 100
    eng = TreeEngine(B, sims, DEV, 1.0, reuse_factor=4.0)
    eng.set_solver(True)
    trees = [ST.SolverTree(cs, 1.0) for cs in cur]
    won = overrides = deep = 0
    for mv in range(2):
        eng.set_roots(to_gpu_batch(O.batch_from_states(cur), DEV))
        if mv == 0:
            eng.begin()
        else:
            eng.advance()
        _injected_step(eng, trees, True, mv)
        for _ in range(sims):
            eng.select()
            _injected_step(eng, trees, False, mv)
        _compare_roots(eng, trees, mv)
        deep += _compare_trees(eng, trees, mv)                    # the climb's marks below the root level too
        eng.finish(torch.full((B,), 0.1, dtype=torch.float32, device=DEV), None)
        before = eng.chosen_index.cpu().numpy().copy()
        eng.solver_pick()
        chosen = eng.chosen_index.cpu().numpy()
        code = eng.chosen_code.cpu().numpy()
        for i, t in enumerate(trees):
            if t.root_terminal():
                assert chosen[i] == -1
                continue
            assert int(before[i]) == _deterministic_pick(t), (mv, i)
            assert int(chosen[i]) == t.solver_pick(int(before[i])), (mv, i, "solver pick differs")
            overrides += int(chosen[i] != before[i])
            won += int(t.root_proven == 3)
            nxt = O.apply_index(cur[i], int(chosen[i]))
            # chosen_code is the code of chosen_index
            idx = O.legal_indices_py(cur[i])
            assert int(chosen[i]) in idx and code[i, 0] >= 0
            cur[i] = nxt
            sc = t.solver_count
            if not t.advance(int(chosen[i])):
                trees[i] = ST.SolverTree(cur[i], 1.0)
            trees[i].solver_count = sc                          # the engine's counter runs over the moves
        assert int(eng.solver_overrides.sum()) == overrides
    assert won >= 8 and deep > 100
    assert eng.reuse_dropped.tolist() == [0, 0]


@pytest.mark.gpu
def test_a_proven_edge_that_lost_its_subtree_stays_decided():
    """A node arena with room for 20 kept nodes: after 400 simulations every game plays the child with the largest subtree,
    and lz_tree_advance has to prune (reuse_dropped[1] > 0).  The checker mirrors the cut on the edges the device reports
    as cut (drop_subtree).  Some of them are proven edges: bit 4 set, child < 0.  The next search (100 simulations, step by
    step) asks for the same leaf at every simulation -- descents that reach such an edge end there with the value of bits
    2..3 -- and afterwards those edges have more visits, still no node, and every edge of every tree agrees with the checker.
    (By the checker alone: game 16 keeps 11 of 21 nodes and loses the subtrees of 10 proven edges.)"""
    _need_gpu()
    from liuzhou_amd.tree_engine import TreeEngine
    cur = _all_positions()
    B, sims, room = len(cur), 400, 20
    eng = TreeEngine(B, sims, DEV, 1.0, reuse_factor=(room - 0.5) / sims)
    assert eng.node_cap - (sims + 1) == room
    eng.set_solver(True)
    trees = [ST.SolverTree(cs, 1.0) for cs in cur]
    eng.set_roots(to_gpu_batch(O.batch_from_states(cur), DEV))
    eng.begin()
    _injected_step(eng, trees, True, 0)
    for _ in range(sims):
        eng.select()
        _injected_step(eng, trees, False, 0)
    _compare_trees(eng, trees, 0)

    def size(t, n):
        nd = t.nodes[n]
        return 1 + sum(size(t, c) for c in range(nd.first_child, nd.first_child + nd.n_children)
                       if t.nodes[c].expanded and t.nodes[c].n_children > 0)

    played = []
    for t, cs in zip(trees, cur):                                 # the child with the largest subtree (lowest index first)
        r = t.nodes[t.root]
        kids = [c for c in range(r.first_child, r.first_child + r.n_children)
                if t.nodes[c].expanded and t.nodes[c].n_children > 0 and not t.nodes[c].terminal]
        best = max(kids, key=lambda c: (size(t, c), -c)) if kids else (r.first_child if r.n_children > 0 else -1)
        played.append(t.nodes[best].action_index if best >= 0 else -1)
    cur = [O.apply_index(cs, a) if a >= 0 else cs for cs, a in zip(cur, played)]
    eng.set_roots(to_gpu_batch(O.batch_from_states(cur), DEV))
    eng.advance(played_action=torch.tensor(played, dtype=torch.int32, device=DEV))
    assert int(eng.reuse_dropped[1]) > 0, "no kept subtree was pruned"
    fresh = eng.buf["nodes"].view(B, eng.node_cap, 6)[:, 0].contiguous().cpu().numpy().view(
        np.dtype(eng._NODE_DT)).reshape(B)["nedges"] < 0
    for i, t in enumerate(trees):                                  # a root the device starts afresh (nothing kept, or dropped)
        sc = t.solver_count
        if played[i] < 0 or bool(fresh[i]) or not t.advance(played[i]):
            trees[i] = ST.SolverTree(cur[i], 1.0)
        trees[i].solver_count = sc
    lost = []                                                      # (game, checker node, visits) of proven edges without a node

    def on_cut(i, c, edge):
        if int(edge["n_info"] >> 24) & ST.INFO_PROVEN:
            lost.append((i, c, int(edge["n_info"] & 0xFFFFFF)))
        trees[i].drop_subtree(c)

    _compare_trees(eng, trees, "cut", on_cut)
    assert lost, "no proven edge lost its subtree"
    _injected_step(eng, trees, True, 1)
    for _ in range(100):
        eng.select()
        _injected_step(eng, trees, False, 1)
    _compare_roots(eng, trees, 1)
    _compare_trees(eng, trees, 1)                                  # (no on_cut: neither side has hung a node on those edges)
    for i, c, _v in lost:
        assert not trees[i].nodes[c].expanded
    assert sum(trees[i].nodes[c].visit_count - v for i, c, v in lost) > 0     # visits are still counted there


# ---- 2. the production path -------------------------------------------------------------------------------------------
def _production(dual, graph=True, compact=False, sims=64, solver=True, positions=None, **extra):
    from liuzhou_amd.tree_engine import DualStreamTreeMCTS, PortableTreeMCTS
    cur = list(_all_positions() if positions is None else positions)
    B = len(cur)
    kw = dict(exploration_weight=1.0, add_dirichlet_noise=True, dirichlet_epsilon=0.25, sample_moves=True, use_graph=graph,
              reuse_tree=True, reuse_factor=4.0, trace=True, seed=777, compact_evals=compact, solver=solver, **extra)
    m = (DualStreamTreeMCTS if dual else PortableTreeMCTS)(_net(), B, sims, DEV, **kw)
    return m, cur


@pytest.mark.gpu
@pytest.mark.parametrize("dual", [False, True])
def test_production_search_replayed_in_the_checker(dual):
    """PortableTreeMCTS / DualStreamTreeMCTS(solver, noise, kept subtrees, fused network, hipGraph, expand trace) over 3
    consecutive moves of the 24 positions, replayed step by step in the checker (tree_parity.replay_part_in_oracle):
    bit-identical root visits, value sums, priors and info bytes, equal root results and counters, and a played move that
    obeys the pick rule."""
    _need_gpu()
    m, cur = _production(dual)
    B = len(cur)
    parts = list(zip(m.bounds, m.parts)) if dual else [((0, B), m)]
    trees = [ST.SolverTree(cs, 1.0) for cs in cur]
    proofs = 0
    for mv in range(3):
        out = m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV),
                             temperatures=torch.ones(B, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize(DEV)
        chosen = out.chosen_action_indices.cpu().numpy()
        rp = out.root_proven.cpu().numpy()
        for (a, b), part in parts:
            replay_part_in_oracle(part, trees[a:b], mv, 0.25)
            _compare_roots(part.engine, trees[a:b], (mv, a))
            assert part.engine.reuse_dropped.tolist() == [0, 0]
        for i, t in enumerate(trees):
            assert int(rp[i]) == t.root_proven
            sc = t.solver_count
            if t.root_terminal():
                assert chosen[i] == -1
                trees[i] = ST.SolverTree(cur[i], 1.0)
            else:
                assert t.solver_pick(int(chosen[i])) == int(chosen[i]), (mv, i, "the played move breaks the pick rule")
                cur[i] = O.apply_index(cur[i], int(chosen[i]))
                if not t.advance(int(chosen[i])):
                    trees[i] = ST.SolverTree(cur[i], 1.0)
            trees[i].solver_count = sc
        proofs = sum(t.solver_count for t in trees)
    assert proofs > 0 and int(m.solver_counts[0]) == proofs


@pytest.mark.gpu
def test_dense_list_and_gathering_launches_build_the_same_trees(monkeypatch):
    _need_gpu()
    results = []
    for compact, gather in ((False, "0"), (True, "0"), (True, "1")):
        monkeypatch.setenv("LZ_TREE_GATHER", gather)
        m, cur = _production(False, compact=compact)
        B = len(cur)
        out = m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV),
                             temperatures=torch.ones(B, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize(DEV)
        e = m.engine
        results.append(([tuple(E[f].tobytes() for f in EDGE_LOGICAL) for E in root_edges(e)], out.root_proven.cpu().tolist(),
                        e.solver_count.cpu().tolist(), out.chosen_action_indices.cpu().tolist(), out.policy_dense.cpu().numpy()))
    for r in results[1:]:
        assert r[0] == results[0][0] and r[1] == results[0][1] and r[2] == results[0][2] and r[3] == results[0][3]
        assert np.array_equal(r[4], results[0][4])
    assert sum(results[0][2]) > 0


# ---- 3. playing ---------------------------------------------------------------------------------------------------------
def _is_winning_move(cs, a):
    c = O.apply_index(cs, a)
    for depth in (2, 4):
        v = ST.brute_value(c, depth)
        if v is not None:
            return (v if int(c.player) == int(cs.player) else -v) == 1
    return False


def _play_wins(solver, copies=4, sims=200):
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    wins = ST.solver_positions()["win"]
    cur = [cs for cs in wins for _ in range(copies)]
    B = len(cur)
    m = PortableTreeMCTS(_net(), B, sims, DEV, exploration_weight=1.0, add_dirichlet_noise=True, sample_moves=True,
                         seed=SEED, solver=solver)
    out = m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV),
                         temperatures=torch.ones(B, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize(DEV)
    return m, cur, out


@pytest.mark.gpu
def test_a_forced_win_is_played_at_temperature_one():
    """The 12 forced-win positions, 4 copies each with their own random streams, 200 simulations of the random-init 6x64
    net, sample_moves at temperature 1: with the solver every root is proven won and every played move wins; without it,
    on the same seed, some played moves do not."""
    _need_gpu()
    m, cur, out = _play_wins(True)
    chosen = out.chosen_action_indices.cpu().tolist()
    rp = out.root_proven.cpu().tolist()
    print("solver on: roots proven won", sum(p == 3 for p in rp), "of", len(cur), "overrides", int(m.solver_counts[2]))
    assert all(p == 3 for p in rp)
    assert all(_is_winning_move(cs, a) for cs, a in zip(cur, chosen))
    m0, _, out0 = _play_wins(False)
    assert out0.root_proven is None
    chosen0 = out0.chosen_action_indices.cpu().tolist()
    lost = sum(not _is_winning_move(cs, a) for cs, a in zip(cur, chosen0))
    print("solver off: played moves that do not win", lost, "of", len(cur))
    assert lost >= 1


# ---- 4. off is byte-identical, on differs only where something was proven ----------------------------------------------
def _selfplay(net, **kw):
    from liuzhou_amd.tree_engine import self_play_tree_gpu, clear_engine_cache
    args = dict(num_games=12, mcts_simulations=24, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                exploration_weight=1.0, device=str(DEV), concurrent_games=12, max_game_plies=24, seed=SEED)
    args.update(kw)
    out = self_play_tree_gpu(net, **args)
    clear_engine_cache()
    return out


def _batch_equal(a, b):
    for f in ("state_tensors", "legal_masks", "policy_targets", "value_targets", "soft_value_targets"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x,
                                                  y.view(torch.uint8) if y.dtype == torch.bool else y), f


@pytest.mark.gpu
def test_off_is_the_call_without_the_kwarg():
    _need_gpu()
    net = _net()
    ba, sa = _selfplay(net)
    bb, sb = _selfplay(net, mcts_solver=False)
    _batch_equal(ba, bb)
    assert sa.mcts_counters.keys() == sb.mcts_counters.keys()
    assert not any(k.startswith("solver") for k in sb.mcts_counters)


@pytest.mark.gpu
def test_on_differs_from_off_only_where_something_was_proven():
    """One search of the 24 positions and of 24 positions of g1_rules.npz (mostly far from any end of the game), same seed,
    on against off: a game whose counters report no proof (solver_count == 0, root_proven == 0) has the same tree, target and
    pick; some game with a proof differs.  (Of the 24 generated positions every one reports a proof within 64 simulations.)"""
    _need_gpu()
    from tests.golden_utils import load, states as gstates
    st_all = gstates(load("g1_rules.npz"), "s")
    pick = np.random.default_rng(3).integers(0, st_all["board"].shape[0], 24)
    positions = _all_positions() + [O.state_from_batch(st_all, int(i)) for i in pick]
    res = []
    for solver in (True, False):
        m, cur = _production(False, solver=solver, positions=positions)
        B = len(cur)
        out = m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV),
                             temperatures=torch.ones(B, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize(DEV)
        res.append((m, [tuple(E[f].tobytes() for f in EDGE_LOGICAL) for E in root_edges(m.engine)],
                    out.chosen_action_indices.cpu().tolist(), out.policy_dense.cpu().numpy()))
    on, off = res
    sc = on[0].engine.solver_count.cpu().tolist()
    rp = on[0].engine.root_proven.cpu().tolist()
    quiet = [i for i in range(len(sc)) if sc[i] == 0 and rp[i] == 0]
    loud = [i for i in range(len(sc)) if i not in quiet]
    assert quiet and loud
    for i in quiet:
        assert on[1][i] == off[1][i] and on[2][i] == off[2][i] and np.array_equal(on[3][i], off[3][i]), i
    assert any(on[1][i] != off[1][i] for i in loud)


# ---- 5. composition -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("extra", [dict(fast_simulations=16, full_prob=0.5), dict(forced_playouts_k=2.0),
                                   dict(gumbel_considered=8)], ids=["cap", "forced", "gumbel"])
def test_composes_with_the_other_search_options(extra):
    """The forced-win positions (4 copies each) with the playout cap, forced playouts or the Gumbel root search next to the
    solver: no refusal, proofs counted, every root that is proven won plays a winning move."""
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    wins = ST.solver_positions()["win"]
    cur = [cs for cs in wins for _ in range(4)]
    B = len(cur)
    m = PortableTreeMCTS(_net(), B, 64, DEV, exploration_weight=1.0, sample_moves=True, seed=SEED, solver=True, **extra)
    out = m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV),
                         temperatures=torch.ones(B, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize(DEV)
    rp = out.root_proven.cpu().tolist()
    chosen = out.chosen_action_indices.cpu().tolist()
    counts = m.solver_counts.tolist()
    print(extra, "proofs / roots decided / overrides", counts, "roots proven won", sum(p == 3 for p in rp))
    assert counts[0] > 0 and counts[1] == sum(p != 0 for p in rp) > 0
    for cs, a, p in zip(cur, chosen, rp):
        if p == 3:
            assert _is_winning_move(cs, a)
    assert counts[2] > 0                                          # some pick was changed to a proven win


@pytest.mark.gpu
def test_self_play_with_the_cap_and_td_lambda():
    _need_gpu()
    b, s = _selfplay(_net(), mcts_solver=True, playout_cap_fast_simulations=8, playout_cap_full_prob=0.5,
                     value_target_lambda=0.8)
    c = s.mcts_counters
    assert {"solver_proofs", "solver_roots_decided", "solver_pick_overrides"} <= set(c)
    assert b.num_samples == s.num_positions > 0
    b2, s2 = _selfplay(_net(), mcts_solver=True, playout_cap_fast_simulations=8, playout_cap_full_prob=0.5,
                       value_target_lambda=0.8)
    _batch_equal(b, b2)
    assert all(c[k] == s2.mcts_counters[k] for k in ("solver_proofs", "solver_roots_decided", "solver_pick_overrides"))
    # the counters against what they count: a decided root is a proof, a changed pick needs a decided root, there is at most
    # one of either per search (full_searches + fast_searches: every search of a live game)
    searches = c["full_searches"] + c["fast_searches"]
    assert 0 <= c["solver_pick_overrides"] <= c["solver_roots_decided"] <= min(c["solver_proofs"], searches)
    # ... and against the run without the solver: games from the opening position, cut at 24 plies, stay in the placement
    # phase, where nothing ends the game -- a run whose counters report no proof is the off run byte for byte
    b0, s0 = _selfplay(_net(), playout_cap_fast_simulations=8, playout_cap_full_prob=0.5, value_target_lambda=0.8)
    print("cap + TD(lambda) self-play: solver counters", {k: v for k, v in c.items() if k.startswith("solver")})
    if c["solver_proofs"] == 0:
        _batch_equal(b, b0)
        assert (s.black_wins, s.white_wins, s.draws, s.num_positions) == (s0.black_wins, s0.white_wins, s0.draws, s0.num_positions)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unsupported_entry_points_refuse_the_descriptor():
    """lz_tree_wave_select / _expand / lz_tree_search_waves, lz_tree_search_multi* and lz_tree_search_persistent return
    LZ_ERR_UNSUPPORTED (-2) for a descriptor with solver != 0 and accept it again with solver = 0; the step entry points want
    root_proven (LZ_ERR_ARG)."""
    _need_gpu()
    from liuzhou_amd import _lib as L
    from liuzhou_amd.tree_engine import LzTreeDesc, TreeEngine
    net = _net()
    eng = TreeEngine(16, 8, DEV, 1.0, batch_k=2)
    eng.set_roots(to_gpu_batch(O.initial_states(16), DEV))
    eng.begin()
    proven = torch.zeros((16,), dtype=torch.int32, device=DEV)
    d = LzTreeDesc()
    C.memmove(C.byref(d), C.byref(eng.desc), C.sizeof(LzTreeDesc))
    d.solver, d.root_proven = 1, proven.data_ptr()
    lib, stream = L.lib(), L.stream_ptr(DEV)
    p = L.ptr
    with torch.cuda.device(DEV):
        assert lib.lz_tree_wave_select(C.byref(d), C.byref(eng.wdesc), L.i64(8), C.c_int(1), stream) == -2
        assert lib.lz_tree_wave_expand(C.byref(d), C.byref(eng.wdesc), p(eng.lp1), p(eng.lp2), p(eng.lpm), None,
                                       p(eng.values), C.c_int(0), stream) == -2
        assert lib.lz_tree_search_waves(C.byref(d), C.byref(eng.wdesc), C.byref(net.desc), L.i64(8), L.i64(4), p(eng.lp1),
                                        p(eng.lp2), p(eng.lpm), p(eng.values), None, L.i64(0), C.c_float(0.25),
                                        C.c_int(0), C.c_int(0), stream) == -2
        for fn in (lib.lz_tree_search_multi, lib.lz_tree_search_multi_continue):
            assert fn(C.byref(d), None, C.c_int32(1), L.i64(8), p(eng.lp1), p(eng.lp2), p(eng.lpm), p(eng.values), None,
                      L.i64(0), C.c_float(0.25), stream) == -2
        slots = torch.zeros((4096,), dtype=torch.int32, device=DEV)
        assert lib.lz_tree_search_persistent(C.byref(d), C.byref(net.desc), L.i64(8), p(eng.lp1), p(eng.lp2), p(eng.lpm),
                                             p(eng.values), None, L.i64(0), C.c_float(0.25), C.c_int(0), p(slots),
                                             L.i64(0), None, stream) == -2
        d.root_proven = None
        assert lib.lz_tree_select(C.byref(d), stream) == -1
        d.solver = 0
        assert lib.lz_tree_wave_select(C.byref(d), C.byref(eng.wdesc), L.i64(8), C.c_int(1), stream) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eng.set_solver(True)                                       # batch_k > 1


# ---- 7. worker ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_worker_run_reports_the_mode(tmp_path):
    _need_gpu()
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.self_play_worker import run_self_play_worker
    from liuzhou_amd.tree_engine import clear_engine_cache
    mod = ChessNet(**MODEL_CONFIGS["b6c64"])
    stable_resnet_init(mod, 20260314)
    ck = tmp_path / "model_state_cpu.pt"
    torch.save(mod.state_dict(), ck)
    out = tmp_path / "w.pt"
    run_self_play_worker(worker_idx=0, shard_device="cuda:0", shard_games=16, seed=5, model_state_path=str(ck),
                         output_path=str(out), mcts_simulations=16, temperature_init=1.0, temperature_final=0.1,
                         temperature_threshold=10, exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25,
                         soft_value_k=2.0, opening_random_moves=2, max_game_plies=12, concurrent_games_per_device=8,
                         chunk_output_dir=str(tmp_path), chunk_file_prefix="w", search_backend="tree", mcts_solver=True)
    clear_engine_cache()
    man = torch.load(out, weights_only=False)
    assert man["metadata"]["mcts_solver"] is True
    assert man["num_samples"] == 16 * 12
    c = man["stats"]["mcts_counters"]
    assert all(k in c for k in ("solver_proofs", "solver_roots_decided", "solver_pick_overrides"))


# ---- 8. guards ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_guard_words_around_the_solver_arrays():
    """root_proven and solver_count inside larger buffers filled with a guard value: a search with many proofs, a pick and an
    advance write nothing outside [0, B)."""
    _need_gpu()
    from liuzhou_amd.tree_engine import TreeEngine
    cur = _all_positions()
    B, sims, G, PAD = len(cur), 100, 0x5A5A5A5A, 64
    eng = TreeEngine(B, sims, DEV, 1.0, reuse_factor=4.0)
    eng.set_solver(True)
    bufs = [torch.full((B + 2 * PAD,), G, dtype=torch.int32, device=DEV) for _ in range(3)]
    for b in bufs:
        b[PAD:PAD + B] = 0
    eng.root_proven, eng.solver_count, eng.solver_overrides = (b[PAD:PAD + B] for b in bufs)
    eng.desc.root_proven, eng.desc.solver_count = eng.root_proven.data_ptr(), eng.solver_count.data_ptr()
    eng.set_roots(to_gpu_batch(O.batch_from_states(cur), DEV))
    eng.search(_net(), sims)
    eng.finish(torch.ones(B, dtype=torch.float32, device=DEV), None)
    eng.solver_pick()
    nxt = [O.apply_index(cs, int(a)) if a >= 0 else cs for cs, a in zip(cur, eng.chosen_index.cpu().tolist())]
    eng.set_roots(to_gpu_batch(O.batch_from_states(nxt), DEV))
    eng.advance()
    eng.search(_net(), sims, continue_trees=True)
    torch.cuda.synchronize(DEV)
    assert int(eng.solver_count.sum()) > 0
    for b in bufs:
        assert bool((b[:PAD] == G).all()) and bool((b[PAD + B:] == G).all())
