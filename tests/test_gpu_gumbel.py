"""Gumbel root search with Sequential Halving of the tree search (LzTreeDesc.gumbel_*, lz_rng_gumbel, lz_tree_finish_gumbel,
PortableTreeMCTS(gumbel_considered), self_play_tree_gpu(gumbel_considered)) against the pure-Python tree of
tests/gumbel_tree.py: the same leaves at every simulation, bit-identical root statistics, picks, scores and vmix."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lz_oracle as O
from tests import gumbel_tree as GT
from tests.golden_utils import FIELDS, load, states
from tests.tree_parity import (EDGE_LOGICAL, engine_visits, hash_evaluator, replay_part_in_oracle, to_gpu_batch,
                               unpack_packed)

DEV = torch.device("cuda:0")
SEED = 7
M = 16


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _net():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    torch.manual_seed(20260314)
    return FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))


# ---- 6. the variates --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rng_gumbel_equals_the_host_restatement_and_is_slot_independent():
    _need_gpu()
    from liuzhou_amd.game_rng import GameRng
    seed = 12345 + (7 << 32)
    game = np.array([0, 1, 2, 5, 1 << 33, 4095, 77, 77, 9, 10], np.int64)
    ply = np.array([0, 0, 3, 9, 1, 143, 20, 21, 0, 2], np.int64)
    B, K = game.shape[0], 72
    rng = GameRng(B, DEV, seed=seed)

    def draw(gm, pl, uniforms):
        rng.game.copy_(torch.from_numpy(gm).to(DEV)); rng.ply.copy_(torch.from_numpy(pl).to(DEV))
        out = torch.full((B, 80), -7.0, dtype=torch.float32, device=DEV)
        rng.gumbel_into(out, K, uniforms=uniforms)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    wu, wg = GT.rng_gumbel(seed, game, ply, K)
    u, g = draw(game, ply, True), draw(game, ply, False)
    assert np.array_equal(u[:, :K].view(np.uint32), wu.view(np.uint32)), "uniform bits differ"
    assert (u[:, K:] == -7.0).all() and (g[:, K:] == -7.0).all()              # nothing beyond `count`
    assert np.isfinite(g[:, :K]).all()
    np.testing.assert_allclose(g[:, :K], wg, rtol=2e-5, atol=0)
    perm = np.random.default_rng(1).permutation(B)
    g2 = draw(np.ascontiguousarray(game[perm]), np.ascontiguousarray(ply[perm]), False)
    assert np.array_equal(g2, g[perm])
    assert not np.array_equal(g[6], g[7])


# ---- 7. injected-evaluator parity of the step protocol ----------------------------------------------------------------
def _injected_search(eng, trees, sims):
    """The step-by-step protocol under hash_evaluator on both sides: the same leaf state requested at every simulation.
    After the root step the checker takes gl and v0 from the device's buffers."""
    def complete(is_root):
        kind = eng.buf["leaf_kind"].cpu().numpy()
        leaf = unpack_packed(eng.buf["leaf_state"].cpu().numpy())
        pend = [t.prepare_root() if is_root else t.select() for t in trees]
        want_kind = np.array([1 if p else 0 for p in pend])
        assert np.array_equal((kind == 1).astype(int), want_kind), "GPU and checker disagree on which games need an evaluation"
        need = np.nonzero(want_kind)[0]
        if need.size:
            o_states = O.batch_from_states([trees[i].pending_state() for i in need])
            for f in FIELDS:
                a = np.asarray(leaf[f])[need].reshape(need.size, -1).astype(np.int64)
                b = np.asarray(o_states[f]).reshape(need.size, -1).astype(np.int64)
                assert np.array_equal(a, b), f"leaf state field {f} differs"
        pri, val = hash_evaluator(leaf)
        for i in need:
            trees[i].complete(pri[i], float(val[i]))
        eng.expand(is_root=is_root, values=torch.from_numpy(val).to(DEV), priors220=torch.from_numpy(pri).to(DEV))
        return pend, val

    pend, val = complete(True)
    gl = eng.gumbel["gl"].cpu().numpy()
    v0 = eng.gumbel["root_value"].cpu().numpy()
    for i, t in enumerate(trees):
        t.root_step(pend[i], gl=gl[i], v0=float(v0[i]))
    for _ in range(sims):
        eng.select()
        complete(False)
    return pend, val, gl, v0


def _check_finish(eng, trees, what=""):
    """Engine outputs of a Gumbel finish against the checker: picks, scores and vmix bit for bit, the target within 1e-6.
    Returns (live roots, roots whose pick differs from the visit-count pick or the top prior, roots with more than m
    children)."""
    from oracle.selfplay_oracle import deterministic_pick
    got_v, got_p = engine_visits(eng)
    chosen = eng.chosen_index.cpu().numpy()
    pol = eng.policy_dense.cpu().numpy()
    rv = eng.root_value.cpu().numpy()
    term = eng.terminal_mask.cpu().numpy()
    score = eng.gumbel["score"].cpu().numpy()
    vmix = eng.gumbel["vmix"].cpu().numpy()
    live = differs = wide = 0
    for i, t in enumerate(trees):
        if t.root_terminal():
            assert term[i] and chosen[i] == -1, (what, i)
            continue
        live += 1
        idx, vis, vs, pr, pl = t.root_children()
        want = np.zeros(220, np.int32); want[idx] = vis
        assert np.array_equal(got_v[i], want), (what, i, "visits differ", np.abs(got_v[i] - want).sum())
        wp = np.zeros(220, np.float32); wp[idx] = pr
        assert np.array_equal(got_p[i], wp), (what, i, "priors differ")
        assert abs(float(rv[i]) - t.root_value_sum() / max(1, t.root_visits())) < 1e-6
        if not t.active():
            continue
        pick, target, wscore, wvmix = t.gumbel_finish()
        ne = len(idx)
        assert int(chosen[i]) == int(idx[pick]), (what, i, "pick differs")
        assert np.array_equal(score[i, :ne].view(np.uint64), wscore.view(np.uint64)), (what, i, "gumbel_score differs")
        assert not score[i, ne:].any()
        assert np.float64(vmix[i]).view(np.uint64) == np.float64(wvmix).view(np.uint64), (what, i, "gumbel_vmix differs")
        np.testing.assert_allclose(pol[i], target, atol=1e-6, rtol=0)
        differs += int(int(idx[pick]) != deterministic_pick(idx, vis, vs, pr, pl, t.root_player())
                       or pick != int(np.argmax(pr)))
        wide += int(ne > t.m)
    return live, differs, wide


@pytest.mark.gpu
@pytest.mark.parametrize("m", [16, 4])
def test_injected_evaluator_parity(m):
    """TreeEngine with the Gumbel rule against the Python tree, 64 games x 64 simulations: leaves, root child visits and
    priors, picks, gumbel_score and gumbel_vmix bit for bit, policy_dense within 1e-6 (the bound the project uses for a
    probability formed from identical inputs).  Not vacuous: the Gumbel pick differs from the most-visited-then-Q pick or
    from the top prior in at least one game, and at least one root has more than m children."""
    _need_gpu()
    from liuzhou_amd.tree_engine import TreeEngine
    B, sims = GT.PARITY_GAMES, GT.PARITY_SIMS
    st, g = GT.parity_inputs()
    eng = TreeEngine(B, sims, DEV, 1.0)
    eng.set_gumbel(m, 50.0, 1.0, sims)
    eng.gumbel["g"].copy_(torch.from_numpy(g).to(DEV))
    eng.set_roots(to_gpu_batch(st, DEV))
    eng.begin()
    trees = [GT.GumbelTree(O.state_from_batch(st, i), 1.0, considered=m, sims=sims) for i in range(B)]
    pend, val, gl, v0 = _injected_search(eng, trees, sims)
    # the snapshot itself: gl = g + log P to float rounding of the device's logf, v0 = the root's network value, N0 = 0
    base = eng.gumbel["base"].cpu().numpy()
    for i, t in enumerate(trees):
        if not t.active():
            continue
        ne = len(t.base)
        pr = t.root_children()[3]
        np.testing.assert_allclose(gl[i, :ne], g[i, :ne] + np.log(pr), rtol=2e-5, atol=2e-6)
        assert np.float32(v0[i]) == np.float32(val[i]) and not base[i, :ne].any()
        assert t.root_order[: min(m, ne)] == sorted(range(ne), key=lambda k: (-float(gl[i, k]), k))[: min(m, ne)]
        assert t.no_candidate == 0
    eng.finish(torch.full((B,), 1.0, dtype=torch.float32, device=DEV), None)
    live, differs, wide = _check_finish(eng, trees)
    assert int(eng.gumbel["count"].sum()) == sum(t.searches for t in trees) == live
    assert live >= B // 2 and differs >= 1 and wide >= 1


@pytest.mark.gpu
def test_finish_gumbel_for_other_games_writes_what_finish_writes():
    """A PUCT search finished through lz_tree_finish_gumbel with every game's root-noise switch off: byte for byte the
    outputs of lz_tree_finish, whatever the pick mode; scores and vmix zero."""
    _need_gpu()
    from liuzhou_amd.tree_engine import TreeEngine
    from tests import forced_tree as FT
    B, sims = 48, 24
    st, _ = GT.parity_inputs(num_games=B, seed=3)
    eng = TreeEngine(B, sims, DEV, 1.0)
    eng.set_roots(to_gpu_batch(st, DEV))
    eng.begin()
    trees = [FT.ForcedTree(O.state_from_batch(st, i), 1.0, 0.0) for i in range(B)]
    from tests.test_gpu_forced_playouts import _injected_search as forced_search
    forced_search(eng, trees, sims, None, 0.25)
    names = ("policy_dense", "chosen_index", "chosen_code", "chosen_valid", "terminal_mask", "root_value", "child_count",
             "child_action", "child_visits", "child_prior")
    u = torch.rand((B,), device=DEV)
    force = (torch.arange(B, device=DEV) % 5 == 0).to(torch.uint8)
    off = torch.zeros((B,), dtype=torch.uint8, device=DEV)
    for kw in (dict(uniforms=None), dict(uniforms=u), dict(uniforms=u, force_uniform=force)):
        temps = torch.full((B,), 0.8, dtype=torch.float32, device=DEV)
        outs = []
        for gumbel in (False, True):
            for n in names:
                getattr(eng, n).view(torch.uint8).fill_(0xA5)
            if gumbel:
                eng.set_gumbel(8, 50.0, 1.0, sims)
                eng.desc.root_noise = off.data_ptr()
                eng.gumbel["score"].fill_(-7.0); eng.gumbel["vmix"].fill_(-7.0)
            eng.finish(temps, kw.get("uniforms"), None, 0.0, kw.get("force_uniform"))
            torch.cuda.synchronize()
            outs.append({n: getattr(eng, n).view(torch.uint8).clone() for n in names})
            if gumbel:
                assert not eng.gumbel["score"].any() and not eng.gumbel["vmix"].any()
                eng.desc.root_noise = None
                eng.set_gumbel(0)
        for n in names:
            assert torch.equal(outs[0][n], outs[1][n]), n


# ---- 8. the production launch path ------------------------------------------------------------------------------------
def _production_inputs(B, seed=0):
    st_all = states(load("g1_rules.npz"), "s")
    idx0 = np.random.default_rng(seed).integers(0, st_all["board"].shape[0], B)
    return {f: np.ascontiguousarray(np.asarray(st_all[f])[idx0]) for f in FIELDS}


def _feed(part, trees):
    gl = part.engine.gumbel["gl"].cpu().numpy()
    v0 = part.engine.gumbel["root_value"].cpu().numpy()
    for i, t in enumerate(trees):
        t.feed(gl=gl[i], v0=float(v0[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("split,graph,lists", [("0", True, False), ("1", True, True), ("0", False, True),
                                               ("1", False, False)])
def test_production_search_replayed_in_the_python_tree(monkeypatch, split, graph, lists):
    """PortableTreeMCTS(gumbel_considered=16, kept subtrees, fused network, expand trace) over 3 consecutive moves,
    replayed step by step in the Python tree (tree_parity.replay_part_in_oracle) with gl and v0 from the device's
    buffers: bit-identical root visits, value sums and priors, identical picks, scores and vmix, the target within 1e-6.
    One-wave and split step, graph and direct launches, dense and list launches.  `add_dirichlet_noise` is on and must
    not matter."""
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    monkeypatch.setenv("LZ_TREE_SPLIT", split)
    B, S, moves = 48, 48, 3
    st = _production_inputs(B)
    m = PortableTreeMCTS(_net(), B, S, DEV, exploration_weight=1.0, add_dirichlet_noise=True, dirichlet_epsilon=0.25,
                         sample_moves=True, use_graph=graph, reuse_tree=True, reuse_factor=4.0, trace=True, seed=777,
                         compact_evals=lists, gumbel_considered=M)
    cur = [O.state_from_batch(st, i) for i in range(B)]
    make = lambda cs: GT.GumbelTree(cs, 1.0, considered=M, sims=S)
    trees = [make(cur[i]) for i in range(B)]
    kept = differs = wide = carried = 0
    for mv in range(moves):
        batch = to_gpu_batch(O.batch_from_states(cur), DEV)
        out = m.search_batch(batch, temperatures=torch.full((B,), 1.0, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize(DEV)
        assert m.last_search_lists == lists
        _feed(m, trees)
        stats = replay_part_in_oracle(m, trees, mv, None)
        kept += stats["kept"]
        assert m.engine.reuse_dropped.tolist() == [0, 0]
        base = m.engine.gumbel["base"].cpu().numpy()
        rb = m.engine.gumbel["root_base"].cpu().numpy()
        for i, t in enumerate(trees):
            if t.active():
                assert base[i, :len(t.base)].tolist() == t.base and int(rb[i]) == t.root_base, (mv, i)
                carried += int(sum(t.base) > 0)
        _live, d, w = _check_finish(m.engine, trees, what=f"move {mv}")
        differs += d; wide += w
        assert int(m.gumbel_searches.item()) == sum(t.searches for t in trees), mv
        chosen = out.chosen_action_indices.cpu().numpy()
        for i in range(B):
            n_searches = trees[i].searches                   # the engine's counter runs over the moves
            if trees[i].root_terminal():
                trees[i] = make(cur[i]); trees[i].searches = n_searches
                continue
            cur[i] = O.apply_index(cur[i], int(chosen[i]))
            if not trees[i].advance(int(chosen[i])):
                trees[i] = make(cur[i]); trees[i].searches = n_searches
    assert kept > 0 and carried > 0 and differs > 0 and wide > 0


def _positions(idx):
    st_all = states(load("g1_rules.npz"), "s")
    return to_gpu_batch({f: np.ascontiguousarray(np.asarray(st_all[f])[idx]) for f in FIELDS}, DEV)


def _game_tree(e, g):
    nodes = e.game_nodes(g)
    runs = [tuple(e.edge_run(int(n["edge_begin"]), max(0, int(n["nedges"])))[f].tobytes() for f in EDGE_LOGICAL)
            for n in nodes]
    return tuple(nodes[f].tobytes() for f in ("w0", "w1", "w2", "w3", "nedges", "parent")), runs


def _play(m, ids, moves, full=None):
    """`moves` searches of the positions `ids` (global game ids `ids`) with kept subtrees; per move the outputs and the
    engines' per-child arrays (scores / vmix: zeros for an engine without the rule)."""
    from liuzhou_amd import v0_core
    from liuzhou_amd.tree_engine import OUT_CAP
    batch = _positions(np.asarray(ids) % 997)
    n = len(ids)
    gid = torch.as_tensor(np.asarray(ids), dtype=torch.int64, device=DEV)
    if full is not None:
        m.injected_full_search = full
    outs = []
    for t in range(moves):
        plies = torch.full((n,), t, dtype=torch.int64, device=DEV)
        out = m.search_batch(batch, temperatures=torch.ones(n, device=DEV), rng_game_ids=gid, rng_plies=plies)
        engines = [p.engine for p in getattr(m, "parts", [])] or [m.engine]
        sc = [e.gumbel["score"] if e.gumbel else torch.zeros((e.B, OUT_CAP), dtype=torch.float64, device=DEV) for e in engines]
        vm = [e.gumbel["vmix"] if e.gumbel else torch.zeros((e.B,), dtype=torch.float64, device=DEV) for e in engines]
        outs.append((out.chosen_action_indices.clone(), out.policy_dense.clone(), out.root_value.clone(),
                     torch.cat([e.child_visits for e in engines]).clone(),
                     torch.cat([e.child_count for e in engines]).clone(), torch.cat(sc).clone(), torch.cat(vm).clone()))
        done = torch.zeros(n, dtype=torch.bool, device=DEV)
        v0_core.self_play_step_inplace(*batch.tensors(), plies.clone(), done, torch.arange(n, device=DEV),
                                       out.chosen_action_codes.clone(), out.terminal_mask.clone(),
                                       out.chosen_valid_mask.clone(), 512, 2.0)
    torch.cuda.synchronize()
    return outs


@pytest.mark.gpu
def test_dual_stream_halves_search_like_one_engine():
    _need_gpu()
    from liuzhou_amd.tree_engine import DualStreamTreeMCTS, PortableTreeMCTS
    net = _net()
    B, S = 48, 24
    kw = dict(add_dirichlet_noise=True, sample_moves=True, reuse_tree=True, reuse_factor=4.0, seed=SEED,
              gumbel_considered=8)
    ids = list(range(B))
    dual = DualStreamTreeMCTS(net, B, S, DEV, **kw)
    one = PortableTreeMCTS(net, B, S, DEV, **kw)
    a = _play(dual, ids, 3)
    b = _play(one, ids, 3)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert torch.equal(u, v)
    assert torch.equal(dual.gumbel_searches, one.gumbel_searches) and int(one.gumbel_searches.item()) > 0
    assert bool(b[-1][5].any()) and bool(b[-1][6].any())


# ---- 9. with the cap; m = 0 --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("split,graph", [("0", True), ("1", False)])
def test_with_the_cap_full_games_are_gumbel_and_fast_games_are_puct(monkeypatch, split, graph):
    """Injected full / fast mask over 40 games, 3 moves with kept subtrees: the full games equal a Gumbel engine that
    searches only them (the engine the replay test above pins to the Python tree); the fast games equal a PUCT search of
    their budget without noise, visit-count pick, no scores."""
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    monkeypatch.setenv("LZ_TREE_SPLIT", split)
    net = _net()
    B, S, F, moves = 40, 24, 6, 3
    full = torch.from_numpy(np.random.default_rng(3).random(B) < 0.5).to(DEV)
    kw = dict(sample_moves=True, reuse_tree=True, reuse_factor=4.0, seed=SEED, use_graph=graph)
    capped = PortableTreeMCTS(net, B, S, DEV, add_dirichlet_noise=True, fast_simulations=F, full_prob=0.5,
                              gumbel_considered=8, **kw)
    ids = list(range(100, 100 + B))
    got = _play(capped, ids, moves, full=full)
    fi = [g for g in range(B) if bool(full[g])]
    si = [g for g in range(B) if not bool(full[g])]
    ref_full = PortableTreeMCTS(net, len(fi), S, DEV, add_dirichlet_noise=True, compact_evals=False, gumbel_considered=8, **kw)
    ref_fast = PortableTreeMCTS(net, len(si), F, DEV, add_dirichlet_noise=False, compact_evals=False, **kw)
    for ref, sub in ((ref_full, fi), (ref_fast, si)):
        want = _play(ref, [ids[g] for g in sub], moves)
        sel = torch.as_tensor(sub, device=DEV)
        for a, b in zip(got, want):
            for j in range(7):              # picks, targets, root values, child_visits, child_count, scores, vmix
                assert torch.equal(a[j].index_select(0, sel), b[j]), j
        for j, g in enumerate(sub):
            assert _game_tree(capped.engine, g) == _game_tree(ref.engine, j)
    cnt = capped.engine.gumbel["count"].cpu().numpy()
    assert cnt[fi].sum() > 0 and cnt[si].sum() == 0
    assert torch.equal(capped.gumbel_searches, ref_full.gumbel_searches)
    assert bool(got[-1][5].index_select(0, torch.as_tensor(fi, device=DEV)).any())


@pytest.mark.gpu
def test_m0_engine_is_the_engine_without_the_kwargs():
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    net = _net()
    B, S = 32, 24
    kw = dict(add_dirichlet_noise=True, sample_moves=True, reuse_tree=True, reuse_factor=4.0, seed=SEED)
    a = PortableTreeMCTS(net, B, S, DEV, **kw)
    b = PortableTreeMCTS(net, B, S, DEV, gumbel_considered=0, gumbel_c_visit=10.0, gumbel_c_scale=3.0, **kw)
    assert not b.gumbel and not b.engine.gumbel and b.engine.desc.gumbel_m == 0
    ids = list(range(B))
    for x, y in zip(_play(a, ids, 3), _play(b, ids, 3)):
        for u, v in zip(x, y):
            assert torch.equal(u, v)
    for g in range(B):
        assert _game_tree(a.engine, g) == _game_tree(b.engine, g)


# ---- 10. self-play and the worker -------------------------------------------------------------------------------------
def _selfplay(net, **kw):
    from liuzhou_amd.tree_engine import self_play_tree_gpu, clear_engine_cache
    args = dict(num_games=24, mcts_simulations=32, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
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
def test_m0_is_the_call_without_the_kwargs(device_tail):
    _need_gpu()
    net = _net()
    ba, sa = _selfplay(net, device_tail=device_tail)
    bb, sb = _selfplay(net, device_tail=device_tail, gumbel_considered=0, gumbel_c_visit=20.0, gumbel_c_scale=2.0)
    _batch_equal(ba, bb)
    assert _stats_key(sa) == _stats_key(sb)
    assert "gumbel_searches" not in sb.mcts_counters and set(sa.mcts_counters) == set(sb.mcts_counters)


@pytest.mark.gpu
def test_self_play_with_the_gumbel_search():
    """Same seed -> identical batches; finite rows that sum to 1 on legal actions only and are dense (a visit-count target
    of 32 simulations has at most 32 non-zero entries; this one covers the legal set); games finish; the counter counts
    the searches; with the cap only the full searches run the rule and record rows."""
    _need_gpu()
    net = _net()
    kw = dict(gumbel_considered=M)
    b1, s1 = _selfplay(net, **kw)
    b2, s2 = _selfplay(net, **kw)
    _batch_equal(b1, b2)
    assert _stats_key(s1) == _stats_key(s2)
    assert s1.num_games == 24 and s1.black_wins + s1.white_wins + s1.draws == 24
    pol = b1.policy_targets
    assert b1.num_samples == s1.num_positions > 0 and bool(torch.isfinite(pol).all())
    assert torch.allclose(pol.sum(1), torch.ones(pol.shape[0], device=pol.device), atol=1e-5)
    assert not (pol * (~b1.legal_masks).to(pol.dtype)).any()
    dense = lambda p, legal: float(((p > 0).sum(1) == legal.sum(1)).float().mean())
    assert dense(pol, b1.legal_masks) > 0.9                  # (an fp32 underflow of a hopeless child is not an error)
    n1 = s1.mcts_counters["gumbel_searches"]
    assert s1.num_positions <= n1 <= s1.num_positions + s1.num_games and n1 == s2.mcts_counters["gumbel_searches"]
    b0, _ = _selfplay(net)
    assert b0.num_samples != b1.num_samples or not torch.equal(b0.policy_targets, b1.policy_targets)
    b3, s3 = _selfplay(net, playout_cap_fast_simulations=8, playout_cap_full_prob=0.5, **kw)
    c = s3.mcts_counters
    assert 0 < b3.num_samples == c["recorded_positions"] <= c["gumbel_searches"] <= c["full_searches"]
    assert c["fast_searches"] > 0
    p3 = b3.policy_targets
    assert torch.allclose(p3.sum(1), torch.ones(p3.shape[0], device=p3.device), atol=1e-5)
    assert dense(p3, b3.legal_masks) > 0.9 and not (p3 * (~b3.legal_masks).to(p3.dtype)).any()
    b4, s4 = _selfplay(net, device_tail=False, **kw)
    assert s4.mcts_counters["gumbel_searches"] >= s4.num_positions == b4.num_samples > 0
    assert torch.allclose(b4.policy_targets.sum(1), torch.ones(b4.num_samples, device=pol.device), atol=1e-5)


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
                         chunk_output_dir=str(tmp_path), chunk_file_prefix="w", search_backend="tree",
                         gumbel_considered=8, gumbel_c_visit=40.0)
    clear_engine_cache()
    man = torch.load(out, weights_only=False)
    assert man["metadata"]["gumbel"] == {"considered": 8, "c_visit": 40.0, "c_scale": 1.0}
    assert man["num_samples"] == 16 * 12
    assert man["stats"]["mcts_counters"]["gumbel_searches"] >= man["num_samples"]
    chunks = [torch.load(tmp_path / f, weights_only=False) for f in man["shard_files"]]
    pol = torch.cat([c["policy_targets"] for c in chunks]).float()
    legal = torch.cat([c["legal_masks"] for c in chunks]).bool()
    assert bool(torch.isfinite(pol).all()) and torch.allclose(pol.sum(1), torch.ones(pol.shape[0]), atol=1e-4)
    assert bool((pol[~legal] == 0).all())


# ---- refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(monkeypatch):
    _need_gpu()
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.tree_engine import DualStreamTreeMCTS, PortableTreeMCTS, PriorEvaluator, TreeEngine
    net = _net()
    for bad in (dict(gumbel_considered=-1), dict(gumbel_considered=73), dict(gumbel_considered=8, gumbel_c_visit=-1.0),
                dict(gumbel_considered=8, gumbel_c_scale=float("nan"))):
        with pytest.raises(ValueError):
            PortableTreeMCTS(net, 16, 16, DEV, **bad)
        with pytest.raises(ValueError):
            _selfplay(net, **bad)
        with pytest.raises(ValueError):
            TreeEngine(16, 16, DEV, 1.0).set_gumbel(bad["gumbel_considered"], bad.get("gumbel_c_visit", 50.0),
                                                    bad.get("gumbel_c_scale", 1.0))
    g = dict(gumbel_considered=8)
    with pytest.raises(ValueError, match="batch_k"):
        PortableTreeMCTS(net, 16, 16, DEV, batch_k=2, **g)
    with pytest.raises(ValueError, match="several networks"):
        PortableTreeMCTS([net, net], 32, 16, DEV, segment_games=16, **g)
    with pytest.raises(ValueError, match="external evaluator"):
        PortableTreeMCTS(PriorEvaluator(lambda p, s: None), 16, 16, DEV, **g)
    with pytest.raises(ValueError, match="external evaluator"):
        PortableTreeMCTS(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV), 16, 16, DEV, **g)
    with pytest.raises(ValueError, match="forced playouts"):
        PortableTreeMCTS(net, 16, 16, DEV, forced_playouts_k=2.0, **g)
    with pytest.raises(ValueError, match="policy_target_temperature"):
        PortableTreeMCTS(net, 16, 16, DEV, policy_target_temperature=0.5, **g)
    with pytest.raises(ValueError, match="policy_target_prior_pseudocount"):
        PortableTreeMCTS(net, 16, 16, DEV, policy_target_prior_pseudocount=0.5, **g)
    with pytest.raises(ValueError):
        DualStreamTreeMCTS(net, 16, 16, DEV, batch_k=2, **g)
    with pytest.raises(ValueError):
        _selfplay(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV), evaluator="module", **g)
    for kw in (dict(batch_k=2), dict(forced_playouts_k=2.0), dict(policy_target_temperature=0.5),
               dict(policy_target_prior_pseudocount=0.5)):
        with pytest.raises(ValueError):
            _selfplay(net, **kw, **g)
    eng = TreeEngine(16, 16, DEV, 1.0)
    eng.set_forced_playouts(2.0)
    with pytest.raises(ValueError):
        eng.set_gumbel(8)
    monkeypatch.setenv("LZ_TREE_PERSISTENT", "1")
    with pytest.raises(ValueError, match="persistent"):
        PortableTreeMCTS(net, 16, 16, DEV, **g)
    with pytest.raises(ValueError, match="persistent"):
        _selfplay(net, **g)


@pytest.mark.gpu
def test_unsupported_entry_points_refuse_the_descriptor():
    """lz_tree_wave_select / lz_tree_search_waves, lz_tree_search_multi* and lz_tree_search_persistent return
    LZ_ERR_UNSUPPORTED (-2) for a descriptor that sets the Gumbel rule, and so do the entry points that implement it when
    forced playouts are set as well; with gumbel_m = 0 the descriptor is accepted again."""
    _need_gpu()
    from liuzhou_amd import _lib as L
    from liuzhou_amd.tree_engine import LzTreeDesc, TreeEngine
    net = _net()
    eng = TreeEngine(16, 8, DEV, 1.0, batch_k=2)
    eng.set_roots(_positions(np.arange(16)))
    eng.begin()
    donor = TreeEngine(16, 8, DEV, 1.0)
    donor.set_gumbel(4, 50.0, 1.0, 8)
    d = LzTreeDesc()
    C.memmove(C.byref(d), C.byref(eng.desc), C.sizeof(LzTreeDesc))
    for name in ("gumbel_m", "gumbel_sims", "gumbel_c_visit", "gumbel_c_scale", "gumbel_g", "gumbel_table", "gumbel_gl",
                 "gumbel_base", "gumbel_root_base", "gumbel_root_value", "gumbel_count", "gumbel_stride"):
        setattr(d, name, getattr(donor.desc, name))
    lib, stream = L.lib(), L.stream_ptr(DEV)
    p = L.ptr
    with torch.cuda.device(DEV):
        assert lib.lz_tree_wave_select(C.byref(d), C.byref(eng.wdesc), L.i64(8), C.c_int(1), stream) == -2
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
        d.forced_k = 2.0                                     # two rules for the same level
        assert lib.lz_tree_select(C.byref(d), stream) == -2
        assert lib.lz_tree_search(C.byref(d), C.byref(net.desc), L.i64(8), None, p(eng.lp1), p(eng.lp2), p(eng.lpm),
                                  p(eng.values), None, L.i64(0), C.c_float(0.25), stream) == -2
        d.forced_k = 0.0
        d.gumbel_sims = 0                                    # a malformed descriptor is an argument error
        assert lib.lz_tree_select(C.byref(d), stream) == -1
        d.gumbel_m = 0
        assert lib.lz_tree_wave_select(C.byref(d), C.byref(eng.wdesc), L.i64(8), C.c_int(1), stream) == 0
    torch.cuda.synchronize()
