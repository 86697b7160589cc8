"""First-play urgency and the visit-scaled exploration constant of the tree search (LzTreeDesc.puct_shape / fpu_* /
cpuct_table*, TreeEngine.set_puct_shape, PortableTreeMCTS / self_play_tree_gpu(fpu_reduction, fpu_root_reduction, cpuct_log,
cpuct_base)) against the pure-Python tree of tests/shape_tree.py: the same leaves at every simulation, bit-identical root
statistics.  Every search here is at most 64 games x 64 simulations on the 6x64 net."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lz_oracle as O
from tests import forced_tree as FT
from tests import shape_tree as SH
from tests import solver_tree as ST
from tests.golden_utils import FIELDS, load, states as gstates
from tests.tree_parity import (EDGE_LOGICAL, hash_evaluator, replay_part_in_oracle, root_edges, to_gpu_batch, unpack_packed)

DEV = torch.device("cuda:0")
SEED = 7
BOTH = SH.SETTINGS["both"]
CASES = {"fpu": SH.SETTINGS["fpu"], "table": SH.SETTINGS["table"], "clamps": SH.CLAMPS}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_NETS = {}


def _net(seed=20260314):
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    if seed not in _NETS:
        torch.manual_seed(seed)
        _NETS[seed] = FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))
    return _NETS[seed]


def _tree_kw(setting):
    """ShapedTree's keyword arguments of a setting (the engine calls the table length `table_len` too)."""
    return dict(setting)


def _mcts_kw(setting):
    """PortableTreeMCTS's keyword arguments of a setting."""
    kw = dict(setting)
    if "table_len" in kw:
        kw["cpuct_table_len"] = kw.pop("table_len")
    return kw


def _compare_roots(eng, trees, tag):
    """Root edges of every game against the checker: actions, visits, f64 value sums and priors bit for bit, and the root's
    own visits and value sum (what V of the root is made of)."""
    edges = root_edges(eng)
    rv = eng.buf["root_visits"].cpu().numpy()
    rw = eng.buf["root_w"].cpu().numpy()
    live = 0
    for i, t in enumerate(trees):
        if t.root_terminal():
            continue
        live += 1
        idx, vis, vs, pr, _pl = t.root_children()
        E = edges[i]
        assert np.array_equal(E["act"].astype(np.int64), idx.astype(np.int64)), (tag, i)
        assert np.array_equal((E["n_info"] & 0xFFFFFF).astype(np.int64), vis.astype(np.int64)), (tag, i, "visits differ")
        assert np.array_equal(E["W"].view(np.uint64), vs.astype(np.float64).view(np.uint64)), (tag, i, "W sums differ")
        assert np.array_equal(E["P"].view(np.uint32), pr.astype(np.float32).view(np.uint32)), (tag, i, "priors differ")
        assert int(rv[i]) == t.root_visits(), (tag, i, "root visits differ")
        assert rw[i:i + 1].view(np.uint64)[0] == np.array([t.root_value_sum()], np.float64).view(np.uint64)[0], (tag, i)
    return live


def _injected_step(eng, trees, is_root, noise, eps, tag):
    """One step of the step-by-step protocol under hash_evaluator on both sides: the same games need an evaluation, of the
    same leaf state."""
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
        trees[i].complete(pri[i], float(val[i]), noise[i] if (is_root and noise is not None) else None, eps)
    if is_root and noise is not None:
        for i, t in enumerate(trees):
            if not pend[i] and not t.root_terminal():
                t.root_noise(noise[i], eps)                         # a kept root: the fresh mix on its priors
    nz = None if (noise is None or not is_root) else torch.from_numpy(noise.astype(np.float32)).to(DEV)
    eng.expand(is_root=is_root, values=torch.from_numpy(val).to(DEV), priors220=torch.from_numpy(pri).to(DEV), noise=nz,
               epsilon=eps)
    return pend


def _injected_search(eng, trees, sims, noise, eps, tag):
    kept = _injected_step(eng, trees, True, noise, eps, tag)
    for s in range(sims):
        eng.select()
        _injected_step(eng, trees, False, noise, eps, (tag, s))
    return kept


# ---- 1. step by step against the checker -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_step_by_step_against_the_checker(case, with_noise):
    """lz_tree_select / lz_tree_expand with injected priors and values on the 64 x 64 inputs tests/test_shape_tree_cpu.py
    shows to be non-vacuous: first-play urgency alone (0.2 / 0.1), the table alone (log 1.0, base 8), and both with a
    reduction of 1.5 and a 16-entry table, so that both clamps fire.  The same leaf at every simulation; afterwards root child
    visits, priors and value sums bit for bit."""
    _need_gpu()
    from liuzhou_amd.tree_engine import TreeEngine
    B, sims, eps = FT.PARITY_GAMES, FT.PARITY_SIMS, FT.PARITY_EPS
    st, noise = FT.parity_inputs(with_noise)
    eng = TreeEngine(B, sims, DEV, 1.0)
    eng.set_puct_shape(**CASES[case])
    assert int(eng.desc.puct_shape) == SH.ShapedTree(O.state_from_batch(st, 0), **_tree_kw(CASES[case])).shape.flags
    eng.set_roots(to_gpu_batch(st, DEV))
    eng.begin()
    trees = SH.make_trees(st, _tree_kw(CASES[case]))
    _injected_search(eng, trees, sims, noise, eps, case)
    live = _compare_roots(eng, trees, case)
    assert 2 * live >= B and all(t.root_visits() == sims for t in trees if not t.root_terminal())
    if case == "clamps":
        assert sum(t.fpu_clamped for t in trees) > 0 and sum(t.table_clamped for t in trees) > 0
        assert int(eng.desc.cpuct_table_len) == 16 and eng.cpuct_table.numel() == 16
    assert int(eng.buf["pool_stats"][0]) == 0


@pytest.mark.gpu
def test_three_games_in_a_partly_filled_workgroup():
    _need_gpu()
    from liuzhou_amd.tree_engine import TreeEngine
    st, noise = FT.parity_inputs(True, num_games=3)
    eng = TreeEngine(3, 64, DEV, 1.0)
    eng.set_puct_shape(**BOTH)
    eng.set_roots(to_gpu_batch(st, DEV))
    eng.begin()
    trees = SH.make_trees(st, BOTH)
    _injected_search(eng, trees, 64, noise, 0.25, "three")
    assert _compare_roots(eng, trees, "three") >= 1


# ---- 2. kept subtrees: the root's V from root_W / root_visits ------------------------------------------------------------
@pytest.mark.gpu
def test_two_moves_with_kept_subtrees():
    """Two consecutive searches, the deterministic pick played in between and its subtree kept by lz_tree_advance: the kept
    root's own mean is root_W / root_visits (a fresh root's first level used root_init_value), its visit count indexes the
    table from the first simulation on."""
    _need_gpu()
    from liuzhou_amd.tree_engine import TreeEngine, OUT_CAP
    from oracle.selfplay_oracle import deterministic_pick
    B, sims, eps = 48, 48, 0.25
    st, _ = FT.parity_inputs(False, num_games=B, seed=5)
    rng = np.random.default_rng(9)
    eng = TreeEngine(B, sims, DEV, 1.0, reuse_factor=4.0)
    eng.set_puct_shape(**BOTH)
    cur = [O.state_from_batch(st, i) for i in range(B)]
    trees = [SH.ShapedTree(cs, 1.0, **BOTH) for cs in cur]
    kept_roots = 0
    for mv in range(2):
        eng.set_roots(to_gpu_batch(O.batch_from_states(cur), DEV))
        if mv == 0:
            eng.begin()
        else:
            eng.advance()
        noise = rng.gamma(0.3, 1.0, size=(B, OUT_CAP)).astype(np.float32) + np.float32(1e-6)
        pend = _injected_search(eng, trees, sims, noise, eps, mv)
        if mv == 1:
            kept = [(not p) and not t.root_terminal() for p, t in zip(pend, trees)]
            kept_roots = sum(kept)
            # those roots began the search with visits of their own: V = root_W / root_visits, c = table[visits]
            assert all(t.root_visits() > sims for t, k in zip(trees, kept) if k)
        _compare_roots(eng, trees, mv)
        eng.finish(torch.full((B,), 0.1, dtype=torch.float32, device=DEV), None)
        chosen = eng.chosen_index.cpu().numpy()
        for i, t in enumerate(trees):
            if t.root_terminal():
                assert chosen[i] == -1
                continue
            idx, vis, vs, pr, pl = t.root_children()
            pick = deterministic_pick(idx, vis, vs, pr, pl, t.root_player())
            assert int(chosen[i]) == pick, (mv, i)
            cur[i] = O.apply_index(cur[i], pick)
            if not t.advance(pick):
                trees[i] = SH.ShapedTree(cur[i], 1.0, **BOTH)
    assert kept_roots * 2 >= B and eng.reuse_dropped.tolist() == [0, 0]


# ---- 3. the production path ------------------------------------------------------------------------------------------------
def _inputs(B, seed=0):
    st_all = gstates(load("g1_rules.npz"), "s")
    idx0 = np.random.default_rng(seed).integers(0, st_all["board"].shape[0], B)
    return {f: np.ascontiguousarray(np.asarray(st_all[f])[idx0]) for f in FIELDS}


def _production(dual=False, B=48, sims=48, graph=True, compact=False, setting=BOTH, positions=None, **extra):
    from liuzhou_amd.tree_engine import DualStreamTreeMCTS, PortableTreeMCTS
    if positions is None:
        st = _inputs(B)
        positions = [O.state_from_batch(st, i) for i in range(B)]
    kw = dict(exploration_weight=1.0, add_dirichlet_noise=True, dirichlet_epsilon=0.25, sample_moves=True, use_graph=graph,
              reuse_tree=True, reuse_factor=4.0, trace=True, seed=777, compact_evals=compact, **_mcts_kw(setting), **extra)
    m = (DualStreamTreeMCTS if dual else PortableTreeMCTS)(_net(), len(positions), sims, DEV, **kw)
    return m, list(positions)


def _new_tree(cs, setting=BOTH, **kw):
    return SH.ShapedTree(cs, 1.0, **_tree_kw(setting), **kw)


def _play_and_replay(m, cur, trees, moves, dual=False, after=None, make=_new_tree, eps=0.25):
    """`moves` searched moves of a production engine, each replayed in the checker trees (tree_parity.replay_part_in_oracle),
    the played child kept on both sides.  `after(mv, out, parts)` sees every move before the trees advance."""
    B = len(cur)
    parts = list(zip(m.bounds, m.parts)) if dual else [((0, B), m)]
    kept = 0
    for mv in range(moves):
        out = m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV),
                             temperatures=torch.ones(B, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize(DEV)
        chosen = out.chosen_action_indices.cpu().numpy()
        for (a, b), part in parts:
            stats = replay_part_in_oracle(part, trees[a:b], mv, eps)
            kept += stats["kept"]
            _compare_roots(part.engine, trees[a:b], (mv, a))
            assert part.engine.reuse_dropped.tolist() == [0, 0]
        if after is not None:
            after(mv, out, parts)
        for i, t in enumerate(trees):
            if t.root_terminal():
                assert chosen[i] == -1
                trees[i] = make(cur[i])
                continue
            assert int(chosen[i]) in t.root_children()[0]
            cur[i] = O.apply_index(cur[i], int(chosen[i]))
            if not t.advance(int(chosen[i])):
                trees[i] = make(cur[i])
    return kept


@pytest.mark.gpu
@pytest.mark.parametrize("dual", [False, True])
def test_production_search_replayed_in_the_checker(dual):
    """PortableTreeMCTS / DualStreamTreeMCTS(first-play urgency 0.2 / 0.1, table log 1.0 base 8; noise, kept subtrees, fused
    network, hipGraph, expand trace) over 3 consecutive moves, replayed step by step in the checker: the same leaf at every
    step, bit-identical root visits, value sums and priors."""
    _need_gpu()
    m, cur = _production(dual)
    assert m.puct_shape.on and m.puct_shape.flags == 3
    trees = [_new_tree(cs) for cs in cur]
    kept = _play_and_replay(m, cur, trees, 3, dual)
    assert kept > 0


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
        results.append(([tuple(E[f].tobytes() for f in EDGE_LOGICAL) for E in root_edges(m.engine)],
                        out.chosen_action_indices.cpu().tolist(), out.policy_dense.cpu().numpy()))
    for r in results[1:]:
        assert r[0] == results[0][0] and r[1] == results[0][1] and np.array_equal(r[2], results[0][2])


@pytest.mark.gpu
def test_the_shape_changes_the_production_search():
    """The same engine with and without the shape, same seed, one search each, each replayed in its own checker (shaped /
    plain): the device's root visits equal the checker's on both sides, so the roots the shape changes on the device are
    exactly the roots it changes in the checker -- and there are some (nothing here is a no-op).  How many is printed, not
    bounded: the floor of tests/test_shape_tree_cpu.py (at least half) is stated for the hash-evaluator inputs, and nothing
    derives one for the near-flat priors of a random-init network under Dirichlet noise."""
    _need_gpu()
    vis, want = [], []
    for setting in (BOTH, {}):
        m, cur = _production(False, setting=setting)
        m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV), temperatures=torch.ones(len(cur), device=DEV))
        torch.cuda.synchronize(DEV)
        trees = [_new_tree(cs, setting) for cs in cur]
        replay_part_in_oracle(m, trees, 0, 0.25)
        _compare_roots(m.engine, trees, ("shaped" if setting else "plain"))
        vis.append([tuple((E["n_info"] & 0xFFFFFF).tolist()) for E in root_edges(m.engine)])
        want.append([tuple(int(v) for v in t.root_children()[1]) if not t.root_terminal() else () for t in trees])
    live = [i for i, v in enumerate(want[1]) if len(v) > 0]
    changed = [i for i in live if vis[0][i] != vis[1][i]]
    print(f"production search, shaped against plain: {len(changed)} of {len(live)} live roots changed")
    assert changed == [i for i in live if want[0][i] != want[1][i]]
    assert len(changed) > 0


# ---- 4. composition ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_with_forced_playouts_the_target_is_pruned_under_c_of_the_root_visits():
    _need_gpu()
    from tests.test_gpu_forced_playouts import _target_visits
    K = 2.0
    m, cur = _production(False, forced_playouts_k=K)
    make = lambda cs: _new_tree(cs, forced_k=K)
    trees = [make(cs) for cs in cur]
    seen = dict(pruned=0, moved=0)

    def after(mv, out, parts):
        e = parts[0][1].engine
        got_t = _target_visits(e)
        pv = e.pruned_visits.cpu().numpy()
        pol = out.policy_dense.cpu().numpy()
        for i, t in enumerate(trees):
            if t.root_terminal():
                continue
            idx, vis, _vs, _pr, _pl = t.root_children()
            tv = t.prune_targets()
            wt = np.zeros(220, np.int32); wt[idx] = tv
            assert np.array_equal(got_t[i], wt), (mv, i, "child_target_visits differ")
            assert int(pv[i]) == int((vis - tv).sum()), (mv, i)
            np.testing.assert_allclose(pol[i], FT.target_policy(t, 1.0), atol=1e-6, rtol=0)
            seen["pruned"] += int((vis - tv).sum())
            table, t.table = t.table, None                          # the same rule under the constant c_puct
            seen["moved"] += int(not np.array_equal(t.prune_targets(), tv))
            t.table = table
        assert int(e.forced_count.sum()) == sum(t.forced_count for t in trees), mv

    # (the engine's forced counter runs over the moves: carry the checker's along when a tree is replaced)
    B = len(cur)
    for mv in range(2):
        out = m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV), temperatures=torch.ones(B, device=DEV))
        torch.cuda.synchronize(DEV)
        replay_part_in_oracle(m, trees, mv, 0.25)
        _compare_roots(m.engine, trees, mv)
        after(mv, out, [((0, B), m)])
        chosen = out.chosen_action_indices.cpu().numpy()
        for i, t in enumerate(trees):
            fc = t.forced_count
            if t.root_terminal():
                trees[i] = make(cur[i])
            else:
                cur[i] = O.apply_index(cur[i], int(chosen[i]))
                if not t.advance(int(chosen[i])):
                    trees[i] = make(cur[i])
            trees[i].forced_count = fc
    assert seen["pruned"] > 0 and seen["moved"] > 0 and int(m.engine.forced_count.sum()) > 0


class _Capped:
    """A checker tree inside a playout-cap search: `budget` simulations, root noise only when `noisy`."""

    def __init__(self, tree, budget, noisy):
        self.t, self.budget, self.noisy, self.done = tree, int(budget), bool(noisy), 0

    def __getattr__(self, name):
        return getattr(self.t, name)

    def prepare_root(self):
        self.done = 0
        return self.t.prepare_root()

    def select(self):
        if self.done >= self.budget:
            return False
        self.done += 1
        return self.t.select()

    def complete(self, pri, val, noise=None, eps=0.25):
        return self.t.complete(pri, val, noise if self.noisy else None, eps)

    def root_noise(self, noise, eps):
        if self.noisy:
            self.t.root_noise(noise, eps)


@pytest.mark.gpu
def test_with_the_playout_cap():
    """An injected full / fast mask over 48 games, 2 moves: a fast game runs 12 simulations without root noise, a full one all
    48 with it, shaped alike; every game replayed in the checker."""
    _need_gpu()
    S, F = 48, 12
    m, cur = _production(False, sims=S, fast_simulations=F, full_prob=0.5)
    B = len(cur)
    trees = [_new_tree(cs) for cs in cur]
    rng = np.random.default_rng(3)
    for mv in range(2):
        full = rng.random(B) < 0.5
        m.injected_full_search = torch.from_numpy(full).to(DEV)
        out = m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV), temperatures=torch.ones(B, device=DEV))
        torch.cuda.synchronize(DEV)
        fresh = [t.root_visits() == 0 for t in trees]
        capped = [_Capped(t, S if full[i] else F, full[i]) for i, t in enumerate(trees)]
        replay_part_in_oracle(m, capped, mv, 0.25)
        _compare_roots(m.engine, trees, mv)
        chosen = out.chosen_action_indices.cpu().numpy()
        for i, t in enumerate(trees):
            if t.root_terminal():
                trees[i] = _new_tree(cur[i])
                continue
            if fresh[i]:
                assert t.root_visits() == (S if full[i] else F), (mv, i)
            cur[i] = O.apply_index(cur[i], int(chosen[i]))
            if not t.advance(int(chosen[i])):
                trees[i] = _new_tree(cur[i])
        assert full.any() and not full.all()


@pytest.mark.gpu
def test_with_the_solver_on_the_generated_positions():
    """The 24 positions of solver_tree.solver_positions() with the solver and the shape, 64 simulations, 2 moves: root edges,
    info bytes, root results and the proof counter equal the checker's."""
    _need_gpu()
    pos = ST.solver_positions()
    positions = pos["win"] + pos["decided"] + pos["open"]
    m, cur = _production(False, sims=64, positions=positions, solver=True)
    make = lambda cs: _new_tree(cs, solver=True)
    trees = [make(cs) for cs in cur]
    B = len(cur)
    for mv in range(2):
        out = m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV), temperatures=torch.ones(B, device=DEV))
        torch.cuda.synchronize(DEV)
        replay_part_in_oracle(m, trees, mv, 0.25)
        _compare_roots(m.engine, trees, mv)
        edges = root_edges(m.engine)
        rp = out.root_proven.cpu().numpy()
        sc = m.engine.solver_count.cpu().numpy()
        chosen = out.chosen_action_indices.cpu().numpy()
        for i, t in enumerate(trees):
            assert int(rp[i]) == t.root_proven and int(sc[i]) == t.solver_count, (mv, i)
            count = t.solver_count
            if t.root_terminal():
                trees[i] = make(cur[i])
            else:
                assert np.array_equal((edges[i]["n_info"] >> 24).astype(np.uint8), t.root_infos()), (mv, i)
                assert t.solver_pick(int(chosen[i])) == int(chosen[i]), (mv, i, "the played move breaks the pick rule")
                cur[i] = O.apply_index(cur[i], int(chosen[i]))
                if not t.advance(int(chosen[i])):
                    trees[i] = make(cur[i])
            trees[i].solver_count = count
    assert sum(t.solver_count for t in trees) > 0


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
def test_with_td_lambda_targets(monkeypatch):
    """Shaped self-play with TD(lambda) value targets against the same run without them: only the value column differs, and it
    is the checker's blend (value_target.td_lambda_targets) of the logged root values of the shaped searches."""
    _need_gpu()
    from tests.test_gpu_td_targets import TOL, _expected_values, _logged_selfplay
    shape = dict(fpu_reduction=0.2, fpu_root_reduction=0.1, cpuct_log=1.0, cpuct_base=8.0)
    kw = dict(num_games=8, mcts_simulations=16, concurrent_games=8, max_game_plies=48, **shape)
    b0, _s0, log0 = _logged_selfplay(_net(), monkeypatch, False, **kw)
    b1, _s1, log1 = _logged_selfplay(_net(), monkeypatch, False, value_target_lambda=0.8, **kw)
    for f in ("state_tensors", "legal_masks", "policy_targets", "soft_value_targets"):
        assert torch.equal(getattr(b0, f).view(torch.uint8) if getattr(b0, f).dtype == torch.bool else getattr(b0, f),
                           getattr(b1, f).view(torch.uint8) if getattr(b1, f).dtype == torch.bool else getattr(b1, f)), f
    assert len(log0) == len(log1) and all(np.array_equal(a, b) for x, y in zip(log0, log1) for a, b in zip(x, y))
    want, games = _expected_values(log1, b0, 0.8)
    got = b1.value_targets.cpu().numpy()
    assert games == 8 and float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) <= TOL
    assert (got != b0.value_targets.cpu().numpy()).any()
    # ... and the shaped games are not the plain ones
    bp, _sp = _selfplay(_net(), num_games=8, mcts_simulations=16, concurrent_games=8, max_game_plies=48)
    assert bp.state_tensors.shape != b0.state_tensors.shape or not torch.equal(bp.policy_targets, b0.policy_targets)


# ---- 5. several networks in one search ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_networks_search_like_two_single_network_searches():
    """lz_tree_search_multi with the shape: two networks x 16-slot segments build the trees of two shaped single-network
    searches of the same positions."""
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    nets = [_net(), _net(7)]
    G, S = 16, 48
    st = _inputs(2 * G, seed=2)
    kw = dict(exploration_weight=1.0, add_dirichlet_noise=False, sample_moves=False, reuse_tree=False, compact_evals=True,
              seed=4, **_mcts_kw(BOTH))
    joint = PortableTreeMCTS(nets, 2 * G, S, DEV, segment_games=G, **kw)
    assert joint.fused_multi and joint.puct_shape.on
    temps = torch.full((2 * G,), 0.1, dtype=torch.float32, device=DEV)
    out = joint.search_batch(to_gpu_batch(st, DEV), temperatures=temps)
    torch.cuda.synchronize(DEV)
    got = [tuple(E[f].tobytes() for f in EDGE_LOGICAL) for E in root_edges(joint.engine)]
    plain = []
    for k, net in enumerate(nets):
        half = {f: np.ascontiguousarray(np.asarray(st[f])[k * G:(k + 1) * G]) for f in FIELDS}
        one = PortableTreeMCTS(net, G, S, DEV, **kw)
        o1 = one.search_batch(to_gpu_batch(half, DEV), temperatures=temps[:G])
        torch.cuda.synchronize(DEV)
        want = [tuple(E[f].tobytes() for f in EDGE_LOGICAL) for E in root_edges(one.engine)]
        assert got[k * G:(k + 1) * G] == want, k
        assert torch.equal(out.chosen_action_indices[k * G:(k + 1) * G], o1.chosen_action_indices)
        off = PortableTreeMCTS(net, G, S, DEV, **{k2: v for k2, v in kw.items() if k2 not in _mcts_kw(BOTH)})
        off.search_batch(to_gpu_batch(half, DEV), temperatures=temps[:G])
        torch.cuda.synchronize(DEV)
        plain += [tuple(E[f].tobytes() for f in EDGE_LOGICAL) for E in root_edges(off.engine)]
    assert sum(a != b for a, b in zip(got, plain)) > 0              # and they are not the unshaped trees


# ---- 6. off is off -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_off_is_the_call_without_the_kwargs():
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    net = _net()
    ba, sa = _selfplay(net)
    bb, sb = _selfplay(net, fpu_reduction=None, fpu_root_reduction=None, cpuct_log=0.0, cpuct_base=19652.0)
    _batch_equal(ba, bb)
    assert sa.mcts_counters.keys() == sb.mcts_counters.keys()
    assert (sa.black_wins, sa.white_wins, sa.draws, sa.num_positions) == (sb.black_wins, sb.white_wins, sb.draws, sb.num_positions)
    m = PortableTreeMCTS(net, 16, 8, DEV, fpu_reduction=None, cpuct_log=0.0, cpuct_base=8.0)
    d = m.engine.desc
    assert not m.puct_shape.on and m.engine.cpuct_table is None
    assert (int(d.puct_shape), int(d.cpuct_table_len), d.cpuct_table, d.fpu_reduction, d.fpu_root_reduction) == (0, 0, None, 0.0, 0.0)
    bc, _ = _selfplay(net, fpu_reduction=0.2, cpuct_log=1.0, cpuct_base=8.0)            # and on is not off
    assert bc.state_tensors.shape != ba.state_tensors.shape or not torch.equal(bc.policy_targets, ba.policy_targets)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals():
    """A shaped descriptor: lz_tree_select / lz_tree_search with Gumbel on, the wave entry points (batch_k = 2) and the
    persistent search return LZ_ERR_UNSUPPORTED (-2) and leave the trees as they were; a table bit without a table, a table
    of one entry and negative or non-finite reductions return LZ_ERR_ARG (-1); the Python layers raise ValueError."""
    _need_gpu()
    from liuzhou_amd import _lib as L
    from liuzhou_amd.tree_engine import LzTreeDesc, PortableTreeMCTS, TreeEngine
    net = _net()
    lib, stream, p = L.lib(), L.stream_ptr(DEV), L.ptr
    table = torch.tensor(SH.shared_table(1.0, 1.0, 8.0, 16), dtype=torch.float64, device=DEV)

    def shaped(eng, **fields):
        d = LzTreeDesc()
        C.memmove(C.byref(d), C.byref(eng.desc), C.sizeof(LzTreeDesc))
        d.puct_shape, d.cpuct_table_len, d.cpuct_table = 3, 16, table.data_ptr()
        d.fpu_reduction, d.fpu_root_reduction = 0.2, 0.1
        for k, v in fields.items():
            setattr(d, k, v)
        return d

    def snapshot(eng):
        torch.cuda.synchronize(DEV)
        return [eng.buf[k].clone() for k in ("n_nodes", "root_visits", "leaf_kind", "path_len", "leaf_edge")]

    # Gumbel
    eng = TreeEngine(16, 8, DEV, 1.0)
    eng.set_gumbel(8, sims=8)
    eng.set_roots(to_gpu_batch(O.initial_states(16), DEV))
    eng.begin()
    before = snapshot(eng)
    d = shaped(eng)
    with torch.cuda.device(DEV):
        assert lib.lz_tree_select(C.byref(d), stream) == -2
        assert lib.lz_tree_search(C.byref(d), C.byref(net.desc), L.i64(8), p(eng.planes), p(eng.lp1), p(eng.lp2), p(eng.lpm),
                                  p(eng.values), None, L.i64(0), C.c_float(0.25), stream) == -2
    assert all(torch.equal(a, b) for a, b in zip(before, snapshot(eng)))
    with pytest.raises(ValueError, match="Gumbel"):
        eng.set_puct_shape(fpu_reduction=0.2)
    # batch_k = 2: the legacy waves
    eng2 = TreeEngine(16, 8, DEV, 1.0, batch_k=2)
    eng2.set_roots(to_gpu_batch(O.initial_states(16), DEV))
    eng2.begin()
    before = snapshot(eng2)
    d = shaped(eng2)
    with torch.cuda.device(DEV):
        assert lib.lz_tree_wave_select(C.byref(d), C.byref(eng2.wdesc), L.i64(8), C.c_int(1), stream) == -2
        assert lib.lz_tree_search_waves(C.byref(d), C.byref(eng2.wdesc), C.byref(net.desc), L.i64(8), L.i64(4), p(eng2.lp1),
                                        p(eng2.lp2), p(eng2.lpm), p(eng2.values), None, L.i64(0), C.c_float(0.25),
                                        C.c_int(0), C.c_int(0), stream) == -2
        # the persistent search
        slots = torch.zeros((4096,), dtype=torch.int32, device=DEV)
        assert lib.lz_tree_search_persistent(C.byref(d), C.byref(net.desc), L.i64(8), p(eng2.lp1), p(eng2.lp2), p(eng2.lpm),
                                             p(eng2.values), None, L.i64(0), C.c_float(0.25), C.c_int(0), p(slots),
                                             L.i64(0), None, stream) == -2
    assert all(torch.equal(a, b) for a, b in zip(before, snapshot(eng2)))
    with pytest.raises(ValueError, match="batch_k"):
        eng2.set_puct_shape(cpuct_log=1.0)
    # bad descriptors
    eng3 = TreeEngine(16, 8, DEV, 1.0)
    eng3.set_roots(to_gpu_batch(O.initial_states(16), DEV))
    eng3.begin()
    before = snapshot(eng3)
    bad = [dict(cpuct_table=None), dict(cpuct_table_len=1), dict(cpuct_table_len=0), dict(fpu_reduction=-0.5),
           dict(fpu_root_reduction=-1e-9), dict(fpu_reduction=float("nan")), dict(fpu_root_reduction=float("inf"))]
    with torch.cuda.device(DEV):
        for fields in bad:
            d = shaped(eng3, **fields)
            assert lib.lz_tree_select(C.byref(d), stream) == -1, fields
            assert lib.lz_tree_search(C.byref(d), C.byref(net.desc), L.i64(8), p(eng3.planes), p(eng3.lp1), p(eng3.lp2),
                                      p(eng3.lpm), p(eng3.values), None, L.i64(0), C.c_float(0.25), stream) == -1, fields
        # a half that is off is not looked at: first-play urgency alone needs no table, the table alone no reductions
        assert lib.lz_tree_select(C.byref(shaped(eng3, puct_shape=1, cpuct_table=None, cpuct_table_len=0)), stream) == 0
    torch.cuda.synchronize(DEV)
    eng3.begin()
    with torch.cuda.device(DEV):
        assert lib.lz_tree_select(C.byref(shaped(eng3, puct_shape=2, fpu_reduction=-1.0)), stream) == 0
    torch.cuda.synchronize(DEV)
    assert all(torch.equal(a, b) for a, b in zip(before[:2], snapshot(eng3)[:2]))
    # the Python layers
    with pytest.raises(ValueError, match="Gumbel"):
        PortableTreeMCTS(net, 16, 8, DEV, gumbel_considered=4, fpu_reduction=0.2)
    with pytest.raises(ValueError, match="batch_k"):
        PortableTreeMCTS(net, 16, 8, DEV, batch_k=2, cpuct_log=1.0)
    with pytest.raises(ValueError, match="Gumbel"):
        _selfplay(net, gumbel_considered=4, cpuct_log=1.0)
    with pytest.raises(ValueError):
        _selfplay(net, fpu_reduction=-0.1)


# ---- 8. worker -----------------------------------------------------------------------------------------------------------------
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
                         chunk_output_dir=str(tmp_path), chunk_file_prefix="w", search_backend="tree", fpu_reduction=0.2,
                         cpuct_log=1.25)
    clear_engine_cache()
    man = torch.load(out, weights_only=False)
    assert man["metadata"]["puct_shape"] == {"fpu_reduction": 0.2, "fpu_root_reduction": 0.2, "cpuct_log": 1.25,
                                             "cpuct_base": 19652.0}
    assert man["num_samples"] == 16 * 12
