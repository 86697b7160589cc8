"""CPU: the checker of the MCTS-Solver tests (tests/solver_tree.py), the test positions, and the refusals that need no
device.

1. With the solver off the Python tree equals oracle.OracleTree bit for bit on the searches of g5_tree.npz.
2. The node rule R and the climb against a brute-force minimax over the oracle's rules.
3. The generated positions meet the condition the GPU tests rely on, by the checker alone.
4. Selection and pick of the checker on those positions: sound results, proven wins played.
5. Validation and refusals."""
import numpy as np
import pytest

from oracle import lz_oracle as O
from tests import solver_tree as ST
from tests.golden_utils import FIELDS, load, states
from tests.tree_parity import hash_evaluator


# ---- 1. the checker against the C oracle ------------------------------------------------------------------------------
def test_solver_off_equals_the_c_oracle_tree_on_g5():
    z0 = load("g5_tree.npz")
    root_states = states(z0, "r")
    z = {k: z0[k] for k in ("case_root", "case_sims", "case_eval_start", "case_eval_count", "case_noise", "case_noise_flag",
                            "eval_priors", "eval_value")}          # (an .npz re-reads an array at every access)
    for ci in range(z["case_root"].shape[0]):
        ri, sims, k = int(z["case_root"][ci]), int(z["case_sims"][ci]), int(z["case_eval_start"][ci])
        noise = z["case_noise"][ci] if bool(z["case_noise_flag"][ci]) else None
        cs = O.state_from_batch(root_states, ri)
        ref, got = O.OracleTree(cs, 1.0), ST.SolverTree(cs, 1.0, solver=False)

        def same_pending():
            a, b = O.batch_from_states([ref.pending_state()]), O.batch_from_states([got.pending_state()])
            for f in FIELDS:
                assert np.array_equal(np.asarray(a[f]), np.asarray(b[f])), (ci, f)

        pa, pb = ref.prepare_root(), got.prepare_root()
        assert pa == pb
        if pa:
            same_pending()
            for t in (ref, got):
                t.complete(z["eval_priors"][k], float(z["eval_value"][k]), noise, 0.25)
            k += 1
        for _ in range(sims):
            pa, pb = ref.select(), got.select()
            assert pa == pb, ci
            if pa:
                same_pending()
                for t in (ref, got):
                    t.complete(z["eval_priors"][k], float(z["eval_value"][k]))
                k += 1
        assert k == int(z["case_eval_start"][ci]) + int(z["case_eval_count"][ci])
        a, b = ref.root_children(), got.root_children()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4]), ci
        assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)), (ci, "value sums differ")
        assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)), (ci, "priors differ")
        assert ref.root_visits() == got.root_visits() and ref.root_value_sum() == got.root_value_sum()
        assert got.root_proven == 0 and got.solver_count == 0 and not got.proven


# ---- 2. the rule and the climb against brute force ----------------------------------------------------------------------
def _expand_all(tree, levels):
    """Expand every undecided node down to `levels` levels below the root, breadth first, through complete() -- so that the
    marks are made by the same code a search runs (a search never expands below a decided node either)."""
    tree.prepare_root()
    tree.complete(np.full(220, 1.0 / 220, np.float32), 0.0)
    frontier = [[tree.root]]
    for _ in range(levels):
        nxt = []
        for path in frontier:
            n = tree.nodes[path[-1]]
            for c in range(n.first_child, n.first_child + n.n_children):
                if tree.decided(c):
                    continue
                tree.path, tree.pending, tree.pending_is_root = path + [c], c, False
                tree.complete(np.full(220, 1.0 / 220, np.float32), 0.0)
                nxt.append(path + [c])
        frontier = nxt


def test_rule_and_climb_equal_brute_force_minimax():
    pos = ST.solver_positions()
    checked = 0
    for kind in ("win", "decided", "open"):
        for cs in pos[kind][:4]:
            tree = ST.SolverTree(cs, 1.0)
            _expand_all(tree, 2)                            # edges three deep are known
            want = ST.brute_value(cs, 3)
            assert tree.root_proven == (0 if want is None else want + 2), kind
            r = tree.nodes[tree.root]
            for c in range(r.first_child, r.first_child + r.n_children):
                if tree.nodes[c].terminal:
                    continue
                v = ST.brute_value(tree.nodes[c].state, 2)
                assert tree.proven.get(c) == v, (kind, c)
                checked += 1
    assert checked > 50


# ---- 3. the positions ---------------------------------------------------------------------------------------------------
def test_positions_meet_the_condition():
    """At least 8 roots with a forced win within 3 edges and a child that does not win, at least 4 proven draws or losses,
    at least 4 where nothing is provable within the budget (seed 20261018, 400 playouts at most: 12 / 6 / 6 found)."""
    pos = ST.solver_positions()
    assert len(pos["win"]) >= 8 and len(pos["decided"]) >= 4 and len(pos["open"]) >= 4
    for cs in pos["win"]:
        legal = O.legal_indices_py(cs)
        wins = ST.winning_children(cs, 2)
        assert ST.brute_value(cs, 3) == 1 and 0 < len(wins) < len(legal)
    for cs in pos["decided"]:
        assert ST.brute_value(cs, 3) in (0, -1)
    for cs in pos["open"]:
        assert ST.brute_value(cs, 3) is None


def test_the_fixture_holds_the_generated_forced_wins():
    """tests/golden/g20_solver.npz (what scripts/bench_solver.py --effect reads): the 12 forced-win positions as generated
    here, and per position the moves the brute force proves winning (2 edges below the child, 4 where 2 decide nothing)."""
    z = load("g20_solver.npz")
    wins = ST.solver_positions()["win"]
    want = O.batch_from_states(wins)
    for f in FIELDS:
        assert np.array_equal(np.asarray(z["s_" + f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)), f
    mask = z["winning_moves"]
    assert mask.shape == (len(wins), 220) and mask.dtype == np.bool_
    for i, cs in enumerate(wins):
        assert set(ST.winning_children(cs, 2)) <= set(np.nonzero(mask[i])[0].tolist()) <= set(O.legal_indices_py(cs))


# ---- 4. the checker's search on them -----------------------------------------------------------------------------------
def _search(trees, sims):
    def complete(pend):
        need = [i for i, p in enumerate(pend) if p]
        if need:
            pri, val = hash_evaluator(O.batch_from_states([trees[i].pending_state() for i in need]))
            for j, i in enumerate(need):
                trees[i].complete(pri[j], float(val[j]))
    complete([t.prepare_root() for t in trees])
    for _ in range(sims):
        complete([t.select() for t in trees])


def test_search_results_are_sound_and_proven_wins_are_played():
    pos = ST.solver_positions()
    css = pos["win"] + pos["decided"]
    on = [ST.SolverTree(cs, 1.0) for cs in css]
    off = [ST.SolverTree(cs, 1.0, solver=False) for cs in css]
    _search(on, 200)
    _search(off, 200)
    proven_wins = 0
    for cs, t, t0 in zip(css, on, off):
        want = ST.brute_value(cs, 3)
        assert t.root_proven in (0, want + 2)                    # what is proven is true
        assert t.root_visits() == t0.root_visits() == 200        # every simulation is backed up, solver or not
        assert t0.root_proven == 0 and t0.solver_count == 0
        idx, vis, _vs, _pr, _pl = t.root_children()
        finish_pick = int(idx[int(np.argmax(vis))])
        played = t.solver_pick(finish_pick)
        if t.root_proven == 3:
            proven_wins += 1
            child = O.apply_index(cs, played)                     # brute force does not contradict the proof
            v = ST.brute_value(child, 2)
            assert want == 1 and (v is None or (v if int(child.player) == int(cs.player) else -v) == 1)
        if want == 1 and t.root_proven == 3:
            # the pick is the most visited winning child
            infos = t.root_infos()
            xs = [t.x(t.root, t.nodes[t.root].first_child + j) if infos[j] & 18 else None for j in range(len(idx))]
            wins = [j for j, v in enumerate(xs) if v == 1]
            assert played == int(idx[max(wins, key=lambda j: (vis[j], -j))])
    assert proven_wins >= 8                                       # 200 simulations prove the three-edge wins


def test_a_pruned_subtree_keeps_its_proof():
    cs = ST.solver_positions()["win"][0]
    t = ST.SolverTree(cs, 1.0)
    _search([t], 200)
    r = t.nodes[t.root]
    marked = [c for c in range(r.first_child, r.first_child + r.n_children) if c in t.proven and t.nodes[c].expanded]
    assert marked
    t.drop_subtree(marked[0])
    assert t.decided(marked[0]) and t.info_byte(marked[0]) & ST.INFO_PROVEN
    before = t.root_visits()
    _search([t], 20)                                              # the next search still ends descents at that edge
    assert not t.nodes[marked[0]].expanded and t.root_visits() == before + 20


# ---- 5. validation and refusals ----------------------------------------------------------------------------------------
def test_refusal_reasons():
    from liuzhou_amd.search_rules import SearchRules
    solver_refusal = SearchRules.parse(8, mcts_solver=True).refusal
    assert solver_refusal() is None
    assert "batch_k" in solver_refusal(batch_k=2)
    assert "several networks" in solver_refusal(several_networks=True)
    assert "external evaluator" in solver_refusal(fused=False)


def test_engines_and_runner_refuse_with_a_reason():
    from liuzhou_amd.tree_engine import PortableTreeMCTS, PriorEvaluator, self_play_tree_gpu
    with pytest.raises(ValueError, match="batch_k"):
        PortableTreeMCTS(object(), 4, 8, "cuda:0", batch_k=2, solver=True)
    with pytest.raises(ValueError, match="external evaluator"):
        PortableTreeMCTS(PriorEvaluator(lambda p, s: None), 4, 8, "cuda:0", solver=True)
    with pytest.raises(ValueError, match="several networks"):
        PortableTreeMCTS([object(), object()], 32, 8, "cuda:0", segment_games=16, solver=True)
    common = dict(num_games=2, mcts_simulations=8, temperature_init=1.0, temperature_final=0.1, temperature_threshold=4,
                  exploration_weight=1.0, device="cuda:0")
    with pytest.raises(ValueError, match="external evaluator"):
        self_play_tree_gpu(PriorEvaluator(lambda p, s: None), mcts_solver=True, **common)
    with pytest.raises(ValueError, match="batch_k"):
        self_play_tree_gpu(PriorEvaluator(lambda p, s: None), mcts_solver=True, batch_k=4, **common)


def test_persistent_kernel_is_refused(monkeypatch):
    from liuzhou_amd.search_rules import SearchRules, persistent_default
    monkeypatch.setenv("LZ_TREE_PERSISTENT", "1")
    assert "persistent" in SearchRules.parse(8, mcts_solver=True).refusal(persistent=persistent_default())
