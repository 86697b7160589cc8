"""CPU: the restatements of the tree read-out stage (tests/readout_ref.py), the hand-built roots harness's host half
(tests/hand_roots.py) and the cases of tests/test_gpu_readout.py (tests/readout_cases.py), DESIGN.md section 25.

1. Every class of rows the GPU tests rely on is there at least three times, and no row holds an input the contract leaves
   undefined or sits on a tolerance boundary.
2. Every index a read-out kernel derives from the records lies inside the buffers the harness allocates.
3. The restatements agree with the float32 oracle, with the reference's own functions (g22_finish_edges.npz), with the
   reference's hand-written vectors and with the checker classes on their shared parity inputs.
4. The legal-move bound: 60, pinned with the host encoder."""
import collections

import numpy as np
import pytest

from oracle import lz_oracle as O
from tests import hand_roots as H
from tests import readout_cases as K
from tests import readout_ref as R
from tests.golden_utils import load

F32 = np.float32
ORACLE_BOUND = 2e-6          # the float32 oracle against the float64 restatement, in probabilities (the existing tests' cap)


def _counts():
    cnt = collections.Counter()
    for _L, _g, r in K.all_rows():
        cnt.update(r["tags"])
    return cnt


def test_every_class_is_there_three_times():
    cnt = _counts()
    for name, req in (("finish", K.REQUIRED), ("pruning", K.PRUNE_REQUIRED), ("solver", K.SOLVER_REQUIRED),
                      ("gumbel", K.GUMBEL_REQUIRED)):
        print(name, {k: cnt[k] for k in req})
        assert not [k for k in req if cnt[k] < 3], [(k, cnt[k]) for k in req if cnt[k] < 3]


def _target_temperature(L, g):
    return L["temps"][g] if L["target_temps"] is None else L["target_temps"][g]


def test_no_case_holds_an_excluded_input_or_sits_on_a_boundary():
    """Excluded (the reference raises): NaN / inf priors or W; a live root whose scores sum to 0 where a softmax is taken
    of them.  Boundaries: Q / P differences among tied candidates are 0 or 4 x the tolerance; a sampled pick's uniform is
    0, the float32 below 1 with a last live child wider than 1e-3, or further than 4e-4 from both ends of its interval;
    a one-hot target over float32 scores has an exactly tied maximum or one that leads by 1e-5 of itself (80 float32
    ulps; the kernel's score differs from the restatement's by the roundings of one sum, one division, one product)."""
    for L, g, r in K.all_rows():
        if not K.live(r):
            continue
        N, P = np.asarray(r["N"]), np.asarray(r["P"], F32)
        assert np.isfinite(P).all() and np.isfinite(np.asarray(r["W"])).all() and (P >= 0).all(), (L["name"], g)
        T, Tt = L["temps"][g], _target_temperature(L, g)
        sampled = L["sample_moves"] and not (L["force"] is not None and L["force"][g])
        plain = L["target_temps"] is None and not L["beta"] > 0
        if sampled or plain:
            assert N.sum() > 0 or T <= R.T_EDGE, (L["name"], g, "selection policy without mass")
        tv = N
        if "forced_k" in L and K.prune_on(L, g):
            white = (np.asarray(r["info"]) & 1) != 0
            tv = R.prune_targets(N, P, R.child_q(r["W"], N, white, r["player"]), r["root_visits"], L["forced_k"], K.prune_c(L, g))
        scores = R.target_scores(tv, P, L["beta"])
        assert scores.sum() > 0 or Tt <= R.T_EDGE, (L["name"], g, "target without mass")
        if Tt <= R.T_EDGE and L["beta"] > 0:
            top = np.sort(np.unique(scores.astype(F32)))[::-1]
            assert len(top) == 1 or top[0] - top[1] > 1e-5 * top[0], (L["name"], g)
        if L["mode"] == "det":
            white = (np.asarray(r["info"]) & 1) != 0
            q = R.child_q(r["W"], N, white, r["player"]).astype(F32)
            c = np.nonzero(N == N.max())[0]
            d = np.abs(q[c] - q[c].max())
            assert ((d == 0) | (d >= F32(4e-6))).all(), (L["name"], g)
            c = c[d == 0]
            d = np.abs(P[c] - P[c].max())
            assert ((d == 0) | (d >= F32(4e-8))).all(), (L["name"], g)
        elif sampled:
            pol = R.policy(N, T)
            cum = np.concatenate([[0.0], np.cumsum(pol)])
            u, k = L["uniforms"][g], R.sampled_pick(pol, L["uniforms"][g])
            assert pol[k] > 1e-3 or F32(T) <= R.T_EDGE, (L["name"], g)
            if u == K.U_TOP:
                assert k == np.nonzero(pol > 0)[0][-1]
            elif u != 0:
                assert cum[k] + 4e-4 < u < cum[k + 1] - 4e-4, (L["name"], g)


def _options(L):
    o = {}
    if "forced_k" in L:
        o.update(forced_k=L["forced_k"], root_noise=L["root_noise"])
        if L["table"] is not None:
            o["cpuct_table"] = L["table"]
    if "gl" in L:
        o.update(gumbel_m=L["m"], gumbel_gl=L["gl"], gumbel_base=L["base"], gumbel_root_value=L["v0"], root_noise=L["root_noise"],
                 gumbel_root_base=np.array([r["root_visits"] for r in L["roots"]], np.int32))
    if "overrides" in L:
        o["root_proven"] = np.zeros(L["B"], np.int32)
    return o


def test_every_derived_index_is_inside_its_buffer():
    n = 0
    for fn in (K.finish_launches, K.prune_launches, K.solver_launches, K.gumbel_launches, lambda: [K.wide_launch(61)]):
        for L in fn():
            lay = H.layout(L["roots"], options=_options(L))          # asserts (check_bounds)
            assert lay["pool_chunks"] * lay["edge_chunk"] >= int((lay["edge_begin"] + np.maximum(lay["nedges"], 1)).max())
            assert L["out_cap"] in (36, 72) and all(len(a) == L["B"] for a in (L["temps"],))
            n += L["B"]
    bad = [H.root_from_state(K.fixture(), 0, ne=73, act=np.arange(73), P=np.zeros(73, F32), N=np.zeros(73, int), W=np.zeros(73),
                             info=np.zeros(73, int), root_visits=0, root_w=0.0, root_init_value=0.0, root_terminal=0)]
    with pytest.raises(AssertionError):
        H.layout(bad)
    print("roots checked:", n)


def test_restatement_equals_the_float32_oracle():
    worst = K.oracle_distance(K.finish_launches())
    print("float32 oracle against ref_finish, per 1 / T:", {k: f"{v:.3e}" for k, v in sorted(worst.items())})
    assert max(worst.values()) <= ORACLE_BOUND and worst[0.0] == 0.0, worst


def test_restatement_equals_the_reference_fixture():
    """g22_finish_edges.npz: the reference's policy_from_visits_and_priors and deterministic_action_from_search on the finish
    rows; a row the reference refuses carries the reason (1: no policy mass, 2: a negative temperature)."""
    z = load("g22_finish_edges.npz")
    launches = K.finish_launches()
    rows = list(K.g22_rows())
    assert [(int(a), int(b)) for a, b in zip(z["launch"], z["game"])] == rows
    worst, refused = 0.0, collections.Counter()
    for k, (i, g) in enumerate(rows):
        N, P, q, Tt, beta = K.g22_inputs(launches[i], g)
        n = len(N)
        assert np.array_equal(z["visits"][k, :n], N) and F32(Tt) == z["temperature"][k] and F32(beta) == z["beta"][k]
        assert int(z["action"][k]) == R.deterministic_pick(N, q, P), (i, g)
        scores = R.target_scores(N, P, beta)
        why = 1 if scores.sum() <= 0 else 2 if Tt < 0 else 0
        assert int(z["refused"][k]) == why, (i, g)
        refused[why] += 1
        if why == 0:
            worst = max(worst, float(np.abs(z["policy"][k, :n].astype(np.float64) - R.policy(scores, Tt)).max()))
            assert not z["policy"][k, n:].any()
    print(f"g22: {len(rows)} rows, refused {dict(refused)}, worst policy distance {worst:.3e}")
    assert worst <= ORACLE_BOUND and refused[1] >= 3 and refused[2] >= 3


def test_restatement_gives_the_reference_hand_written_vectors():
    """The vectors of tests/test_gpu_reference_cases.py (test_portable_mcts.py:320-402)."""
    fin = lambda root, **kw: R.ref_finish(root, **{"temperature": 1.0, **kw})
    a = fin(H.one_root([0, 1, 2, 3], [4, 4, 4, 4], [0.1, 0.3, 0.3, 0.3], [0.9, 0.2, 0.4, 0.4]))
    assert a["chosen_index"] == 2 and a["chosen_code"] == [1, 2, -1, -1]
    assert fin(H.one_root([5, 9, 12], [3, 7, 7], [0.9, -0.5, -0.5], [0.8, 0.1, 0.1]))["chosen_index"] == 9
    root = H.one_root([0, 1, 2, 3], [8, 0, 0, 0], [0.0] * 4, [0.4, 0.3, 0.2, 0.1])
    assert fin(root)["policy"][:4].tolist() == [1.0, 0.0, 0.0, 0.0]
    b = fin(root, target_temperature=1.0, beta=1.0)
    want = np.array([8.4, 0.3, 0.2, 0.1]) / 9.0
    assert np.abs(b["policy"][:4] - want).max() <= 1e-7 and b["chosen_index"] == 0 and not b["policy"][4:].any()
    root = H.one_root([3, 4, 7], [10, 30, 20], [0.0, 0.1, 0.2], [0.3, 0.3, 0.4])
    for tt in (None, 0.25, 4.0):
        c = fin(root, target_temperature=tt)
        w = np.array([10.0, 30.0, 20.0]) ** (1.0 / (tt or 1.0))
        assert c["chosen_index"] == 4 and np.abs(c["policy"][[3, 4, 7]] - w / w.sum()).max() <= 1e-12


def test_terminal_roots_and_root_value():
    base = K._terminal_states()
    for r in base:
        for ne in (-1, 0):
            out = R.ref_finish(dict(r, ne=ne, root_terminal=0, root_visits=3, root_w=1.0, root_init_value=0.5), temperature=1.0)
            want = 0.0 if r["status"] == 2 else (1.0 if r["status"] == r["player"] else -1.0)
            assert out["terminal"] and not out["chosen_valid"] and out["root_value"] == F32(want) and out["child_count"] == 0
    stuck = H.root_from_state(K.fixture(), 0, ne=0, root_terminal=0, root_visits=0, root_w=0.0, root_init_value=0.5)
    assert stuck["status"] == 0 and R.ref_finish(stuck, temperature=1.0)["root_value"] == F32(-1)
    live = K.finish_launches()[0]["roots"][5]
    assert R.ref_finish(dict(live, root_visits=3, root_w=1.0), temperature=1.0)["root_value"] == F32(np.float64(1.0) / 3.0)
    assert R.ref_finish(dict(live, root_visits=0, root_init_value=F32(0.375)), temperature=1.0)["root_value"] == F32(0.375)


def test_checker_classes_agree_on_their_parity_inputs():
    """The tree classes call the array-level rules; fed from root_children() the rules give what the trees report."""
    from tests import forced_tree as FT
    from tests import gumbel_tree as GT
    from tests import shape_tree as ST
    states, noise = FT.parity_inputs(True, num_games=16)
    trees = [FT.ForcedTree(O.state_from_batch(states, i), 1.0, FT.PARITY_K) for i in range(16)]
    FT.search_alone(trees, 48, noise)
    shaped = ST.make_trees(states, dict(cpuct_log=2.0, cpuct_base=8.0, table_len=32), forced_k=FT.PARITY_K)
    FT.search_alone(shaped, 48, noise)
    pruned = 0
    for t in trees + shaped:
        if t.root_terminal():
            continue
        idx, vis, vs, pr, pl = t.root_children()
        q = R.child_q(vs, vis, pl < 0, t.root_player())
        c = t.c_of(t.root_visits()) if isinstance(t, ST.ShapedTree) else t.c
        want = R.prune_targets(vis, pr, q, t.root_visits(), t.k, c)
        assert np.array_equal(t.prune_targets(), want)
        pruned += int((want != vis).any())
    assert pruned >= 8
    from tests import solver_tree as SV
    solved = [SV.SolverTree(O.state_from_batch(states, i), 1.0, solver=True) for i in range(16)]
    FT.search_alone(solved, 48, noise)
    for t in solved:
        if t.root_terminal():
            continue
        idx, vis, _vs, _pr, _pl = t.root_children()
        xs = [R.solver_x(b, t.root_player()) if b & (R.INFO_TERMINAL | R.INFO_PROVEN) else None for b in t.root_infos()]
        for a in idx:
            assert t.solver_pick(int(a)) == R.solver_pick(idx, vis, xs, int(a))
    states, g = GT.parity_inputs(num_games=12)
    gt = [GT.GumbelTree(O.state_from_batch(states, i), 1.0, considered=8, sims=32) for i in range(12)]
    GT.search_alone(gt, 32, g)
    for t in gt:
        if t.root_terminal() or not t.active():
            continue
        idx, vis, vs, pr, pl = t.root_children()
        q = R.child_q(vs, vis, pl < 0, t.root_player())
        pick, probs, score, vmix = R.gumbel_finish(vis, pr, q, t.gl, t.base, t.v0, t.c_visit, t.c_scale)
        p2, target, s2, v2 = t.gumbel_finish()
        assert pick == p2 and vmix == v2 and np.array_equal(score, s2) and np.array_equal(target[idx], probs)


def test_solver_rule_on_info_bytes():
    acts, N = [10, 20, 30, 40], [5, 9, 9, 1]
    x = lambda *info: [R.solver_x(b, 1) if b & 18 else None for b in info]
    assert R.solver_pick(acts, N, x(0, 2 | 8, 16 | 8, 0), 10) == 20            # two wins, tied visits: the lowest index
    assert R.solver_pick(acts, N, x(1 | 2 | 0, 0, 0, 0), 10) == 10             # white child lost for itself = won for black
    assert R.solver_pick(acts, N, x(2 | 0, 0, 0, 0), 10) == 20                 # the picked child is lost: the most visited other
    assert R.solver_pick(acts, N, x(2, 2, 2, 2), 10) == 10                     # every child lost: kept
    assert R.solver_pick(acts, N, x(0, 2, 0, 0), 10) == 10                     # a lost child that was not picked: kept
    assert R.solver_pick(acts, N, x(2 | 4, 0, 0, 0), 10) == 10                 # a drawn pick: kept


def test_at_most_sixty_legal_moves():
    """Legal movement actions are (own piece, adjacent empty cell) pairs; the 6 x 6 grid has 60 adjacencies, all between the
    two cell colours, so a mover who owns one colour class next to an empty other one has all 60 -- and nobody has more.
    Placement and the selections offer at most 36.  The fixtures stay below that."""
    import torch
    from liuzhou_amd.mcts_gpu import encode_actions_fast
    from tests.golden_utils import states
    from tests.tree_parity import to_gpu_batch
    st = {f: np.asarray(v[:2]).copy() for f, v in O.initial_states(2).items()}
    checker = np.fromfunction(lambda r, c: (r + c) % 2 == 0, (6, 6))
    st["board"][0] = np.where(checker, 1, 0)
    st["board"][1] = np.where(checker, 0, -1)
    st["phase"][:] = 4
    st["current_player"][:] = [1, -1]
    mask, _ = encode_actions_fast(to_gpu_batch(st, "cpu"))
    assert mask.sum(1).tolist() == [60, 60] and not mask[:, :36].any() and not mask[:, 180:].any()
    most = 0
    for name in ("g1_rules.npz",):
        m, _ = encode_actions_fast(to_gpu_batch(states(load(name), "s"), "cpu"))
        most = max(most, int(m.sum(1).max()))
    print("most legal moves in the fixture positions:", most)
    assert most <= 60 and most == 36


def test_a_search_without_a_simulation_is_refused():
    """The no-mass root: a root expanded and never searched.  The reference raises; the host refuses
    the configuration where its parameters are validated, before anything touches a device."""
    from liuzhou_amd import tree_engine as TE
    assert TE.search_simulations(1) == 1 and TE.search_simulations(800) == 800
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="num_simulations"):
            TE.search_simulations(bad)
    with pytest.raises(ValueError, match="num_simulations"):
        TE.PortableTreeMCTS(None, 16, 0, "cpu")
    with pytest.raises(ValueError, match="num_simulations"):
        TE.DualStreamTreeMCTS(None, 16, 0, "cpu")
