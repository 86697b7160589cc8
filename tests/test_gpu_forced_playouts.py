"""Forced playouts and policy target pruning of the tree search (LzTreeDesc.forced_k / forced_count, lz_tree_finish_pruned,
PortableTreeMCTS(forced_playouts_k), self_play_tree_gpu(forced_playouts_k)) against the pure-Python tree of
tests/forced_tree.py: the same leaves at every simulation, bit-identical root statistics and pruned visits N'."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lz_oracle as O
from tests import forced_tree as FT
from tests.golden_utils import FIELDS, load, states
from tests.tree_parity import (EDGE_LOGICAL, engine_visits, hash_evaluator, replay_part_in_oracle, to_gpu_batch,
                               unpack_packed)

DEV = torch.device("cuda:0")
SEED = 7
K = 2.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _net():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    torch.manual_seed(20260314)
    return FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))


def _target_visits(engine):
    """child_target_visits as a dense [B, 220] array (like tree_parity.engine_visits)."""
    cnt = engine.child_count.cpu().numpy()
    act = engine.child_action.cpu().numpy()
    tv = engine.child_target_visits.cpu().numpy()
    out = np.zeros((engine.B, 220), np.int32)
    for g in range(engine.B):
        out[g, act[g, :int(cnt[g])]] = tv[g, :int(cnt[g])]
    return out


def _injected_search(eng, trees, sims, noise, eps):
    """The step-by-step protocol under hash_evaluator on both sides (after tree_parity.run_injected_parity): the same leaf
    state requested at every simulation."""
    nz_dev = None if noise is None else torch.from_numpy(noise.astype(np.float32)).to(DEV)

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
            trees[i].complete(pri[i], float(val[i]), noise[i] if (is_root and noise is not None) else None, eps)
        eng.expand(is_root=is_root, values=torch.from_numpy(val).to(DEV), priors220=torch.from_numpy(pri).to(DEV),
                   noise=nz_dev if is_root else None, epsilon=eps)

    complete(True)
    for _ in range(sims):
        eng.select()
        complete(False)


# ---- 5. injected-evaluator parity -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_noise", [False, True])
def test_injected_evaluator_parity(with_noise):
    """TreeEngine with k = 2 against the Python tree, 64 games x 64 simulations (the inputs tests/test_forced_tree_cpu.py
    shows to be non-vacuous: forced descents at 64 / 64 roots, pruned visits at 61 / 64): root child visits, priors and
    child_target_visits bit-exact, forced_count and pruned_visits equal, policy_dense within 1e-6 of the target formed
    from the checker's N', picks by the raw-visit rule."""
    _need_gpu()
    from liuzhou_amd.tree_engine import TreeEngine
    from oracle.selfplay_oracle import deterministic_pick
    B, sims, eps, temperature = FT.PARITY_GAMES, FT.PARITY_SIMS, FT.PARITY_EPS, 1.0
    st, noise = FT.parity_inputs(with_noise)
    eng = TreeEngine(B, sims, DEV, 1.0)
    eng.set_forced_playouts(FT.PARITY_K)
    eng.set_roots(to_gpu_batch(st, DEV))
    eng.begin()
    trees = [FT.ForcedTree(O.state_from_batch(st, i), 1.0, FT.PARITY_K) for i in range(B)]
    _injected_search(eng, trees, sims, noise, eps)
    eng.finish(torch.full((B,), temperature, dtype=torch.float32, device=DEV), None)
    got_v, got_p = engine_visits(eng)
    got_t = _target_visits(eng)
    chosen = eng.chosen_index.cpu().numpy()
    pol = eng.policy_dense.cpu().numpy()
    rv = eng.root_value.cpu().numpy()
    term = eng.terminal_mask.cpu().numpy()
    fc = eng.forced_count.cpu().numpy()
    pv = eng.pruned_visits.cpu().numpy()
    live = forced_roots = pruned_roots = 0
    for i, t in enumerate(trees):
        assert int(fc[i]) == t.forced_count, (i, "forced_count differs")
        if t.root_terminal():
            assert term[i] and int(pv[i]) == 0, i
            continue
        live += 1
        idx, vis, vs, pr, pl = t.root_children()
        want = np.zeros(220, np.int32); want[idx] = vis
        assert np.array_equal(got_v[i], want), (i, "visits differ", np.abs(got_v[i] - want).sum())
        wp = np.zeros(220, np.float32); wp[idx] = pr
        assert np.array_equal(got_p[i], wp), (i, "priors differ")
        assert int(vis.sum()) == sims
        tv = t.prune_targets()
        wt = np.zeros(220, np.int32); wt[idx] = tv
        assert np.array_equal(got_t[i], wt), (i, "child_target_visits differ", got_t[i][idx], tv, vis)
        assert int(pv[i]) == int((vis - tv).sum()), (i, "pruned_visits differs")
        np.testing.assert_allclose(pol[i], FT.target_policy(t, temperature), atol=1e-6, rtol=0)
        assert abs(float(rv[i]) - t.root_value_sum() / max(1, t.root_visits())) < 1e-6
        assert int(chosen[i]) == deterministic_pick(idx, vis, vs, pr, pl, t.root_player()), (i, "pick is not by raw visits")
        forced_roots += int(t.forced_count > 0)
        pruned_roots += int((vis - tv).sum() > 0)
    # not vacuous (the floors of tests/test_forced_tree_cpu.py, on the very same inputs)
    assert live >= B // 2 and forced_roots * 2 >= live and pruned_roots * 2 >= live


# ---- 8b. lz_tree_finish_pruned with forced_k = 0 ----------------------------------------------------------------------
@pytest.mark.gpu
def test_finish_pruned_with_k0_writes_what_finish_writes():
    _need_gpu()
    from liuzhou_amd.tree_engine import TreeEngine
    B, sims = 48, 24
    st, noise = FT.parity_inputs(True, num_games=B, seed=3)
    eng = TreeEngine(B, sims, DEV, 1.0)
    eng.set_roots(to_gpu_batch(st, DEV))
    eng.begin()
    trees = [FT.ForcedTree(O.state_from_batch(st, i), 1.0, 0.0) for i in range(B)]
    _injected_search(eng, trees, sims, noise, 0.25)
    names = ("policy_dense", "chosen_index", "chosen_code", "chosen_valid", "terminal_mask", "root_value", "child_count",
             "child_action", "child_visits", "child_prior")
    u = torch.rand((B,), device=DEV)
    force = (torch.arange(B, device=DEV) % 5 == 0).to(torch.uint8)
    cases = [dict(uniforms=None), dict(uniforms=u), dict(uniforms=u, force_uniform=force),
             dict(uniforms=None, target_temperatures=torch.full((B,), 0.5, device=DEV), prior_pseudocount=0.25)]
    for kw in cases:
        temps = torch.full((B,), 0.8, dtype=torch.float32, device=DEV)
        outs = []
        for pruned in (False, True):
            for n in names:
                getattr(eng, n).view(torch.uint8).fill_(0xA5)
            eng.child_target_visits.fill_(-7); eng.pruned_visits.fill_(-7)
            eng.finish(temps, kw.get("uniforms"), kw.get("target_temperatures"), kw.get("prior_pseudocount", 0.0),
                       kw.get("force_uniform"), pruned=pruned)
            torch.cuda.synchronize()
            outs.append({n: getattr(eng, n).view(torch.uint8).clone() for n in names})
        for n in names:
            assert torch.equal(outs[0][n], outs[1][n]), n
        cnt = eng.child_count.cpu().numpy()
        tv, cv = eng.child_target_visits.cpu().numpy(), eng.child_visits.cpu().numpy()
        for g in range(B):
            assert np.array_equal(tv[g, :cnt[g]], cv[g, :cnt[g]]), g
        assert not eng.pruned_visits.any()


# ---- 6. the production launch path ------------------------------------------------------------------------------------
def _production_inputs(B, seed=0):
    st_all = states(load("g1_rules.npz"), "s")
    idx0 = np.random.default_rng(seed).integers(0, st_all["board"].shape[0], B)
    return {f: np.ascontiguousarray(np.asarray(st_all[f])[idx0]) for f in FIELDS}


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("graph", [True, False])
def test_production_search_replayed_in_the_python_tree(monkeypatch, split, graph):
    """PortableTreeMCTS(forced_playouts_k=2, noise, kept subtrees, fused network, expand trace) over 3 consecutive moves,
    replayed step by step in the Python tree (tree_parity.replay_part_in_oracle): bit-identical root visits, value sums
    and priors, identical child_target_visits, forced_count and pruned_visits, the target within 1e-6 of the one formed
    from N', the sampled pick from the raw-visit policy.  One-wave and split step, graph and direct launches."""
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    monkeypatch.setenv("LZ_TREE_SPLIT", split)
    B, S, moves, temperature = 48, 48, 3, 1.0
    st = _production_inputs(B)
    m = PortableTreeMCTS(_net(), B, S, DEV, exploration_weight=1.0, add_dirichlet_noise=True, dirichlet_epsilon=0.25,
                         sample_moves=True, use_graph=graph, reuse_tree=True, reuse_factor=4.0, trace=True, seed=777,
                         forced_playouts_k=K)
    cur = [O.state_from_batch(st, i) for i in range(B)]
    trees = [FT.ForcedTree(cur[i], 1.0, K) for i in range(B)]
    forced_total = pruned_total = kept = 0
    for mv in range(moves):
        batch = to_gpu_batch(O.batch_from_states(cur), DEV)
        out = m.search_batch(batch, temperatures=torch.full((B,), temperature, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize(DEV)
        chosen = out.chosen_action_indices.cpu().numpy()
        pol = out.policy_dense.cpu().numpy()
        before = [t.forced_count for t in trees]
        stats = replay_part_in_oracle(m, trees, mv, 0.25)
        kept += stats["kept"]
        assert m.engine.reuse_dropped.tolist() == [0, 0]
        got_v, _ = engine_visits(m.engine)
        got_t = _target_visits(m.engine)
        pv = m.engine.pruned_visits.cpu().numpy()
        u = m._uniforms.cpu().numpy()
        for i, t in enumerate(trees):
            if t.root_terminal():
                assert chosen[i] == -1 and int(pv[i]) == 0
                continue
            idx, vis, _vs, _pr, _pl = t.root_children()
            tv = t.prune_targets()
            wt = np.zeros(220, np.int32); wt[idx] = tv
            assert np.array_equal(got_t[i], wt), (mv, i, "child_target_visits differ")
            assert int(pv[i]) == int((vis - tv).sum()), (mv, i)
            pruned_total += int((vis - tv).sum())
            np.testing.assert_allclose(pol[i], FT.target_policy(t, temperature), atol=1e-6, rtol=0)
            # sampled pick: inverse CDF of the selection policy (raw visits) over the children in ascending action order
            sel = O.policy_from_visits(vis, temperature)
            k = int(np.nonzero(idx == chosen[i])[0][0])
            cum = np.cumsum(sel.astype(np.float64))
            assert sel[k] > 0 and cum[k] > u[i] - 1e-6 and (k == 0 or cum[k - 1] <= u[i] + 1e-6), (mv, i)
        forced_total += sum(t.forced_count - b for t, b in zip(trees, before))
        assert int(m.engine.forced_count.sum()) == sum(t.forced_count for t in trees), mv
        for i in range(B):
            fc = trees[i].forced_count                       # the engine's counter runs over the moves
            if trees[i].root_terminal():
                trees[i] = FT.ForcedTree(cur[i], 1.0, K)
                trees[i].forced_count = fc
                continue
            cur[i] = O.apply_index(cur[i], int(chosen[i]))
            if not trees[i].advance(int(chosen[i])):
                trees[i] = FT.ForcedTree(cur[i], 1.0, K)
                trees[i].forced_count = fc
    assert kept > 0 and forced_total > 0 and pruned_total > 0
    assert m.forced_counts.tolist()[1] == pruned_total


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
    engines' per-child visit arrays."""
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
        engines = [p.engine for p in getattr(m, "parts", [])] or [m.engine]
        outs.append((out.chosen_action_indices.clone(), out.policy_dense.clone(), out.root_value.clone(),
                     torch.cat([e.child_visits for e in engines]).clone(),
                     torch.cat([e.child_target_visits for e in engines]).clone(),
                     torch.cat([e.child_count for e in engines]).clone(),
                     torch.cat([e.pruned_visits for e in engines]).clone()))
        done = torch.zeros(n, dtype=torch.bool, device=DEV)
        v0_core.self_play_step_inplace(*batch.tensors(), plies.clone(), done, torch.arange(n, device=DEV),
                                       out.chosen_action_codes.clone(), out.terminal_mask.clone(),
                                       out.chosen_valid_mask.clone(), 512, 2.0)
    torch.cuda.synchronize()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("graph", [True, False])
def test_with_the_cap_full_games_are_forced_and_fast_games_are_not(monkeypatch, split, graph):
    """Injected full / fast mask over 40 games, 3 moves with kept subtrees: the full games equal an engine with k = 2 that
    searches only them (the engine the replay test above pins to the Python tree), forced and pruned; the fast games
    equal a k = 0 search of their budget without noise, with child_target_visits == child_visits and nothing pruned."""
    _need_gpu()
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    monkeypatch.setenv("LZ_TREE_SPLIT", split)
    net = _net()
    B, S, F, moves = 40, 24, 6, 3
    full = torch.from_numpy(np.random.default_rng(3).random(B) < 0.5).to(DEV)
    kw = dict(sample_moves=True, reuse_tree=True, reuse_factor=4.0, seed=SEED, use_graph=graph)
    capped = PortableTreeMCTS(net, B, S, DEV, add_dirichlet_noise=True, fast_simulations=F, full_prob=0.5,
                              forced_playouts_k=K, **kw)
    ids = list(range(100, 100 + B))
    got = _play(capped, ids, moves, full=full)
    fi = [g for g in range(B) if bool(full[g])]
    si = [g for g in range(B) if not bool(full[g])]
    ref_full = PortableTreeMCTS(net, len(fi), S, DEV, add_dirichlet_noise=True, compact_evals=False, forced_playouts_k=K, **kw)
    ref_fast = PortableTreeMCTS(net, len(si), F, DEV, add_dirichlet_noise=False, compact_evals=False, **kw)
    for ref, sub in ((ref_full, fi), (ref_fast, si)):
        want = _play(ref, [ids[g] for g in sub], moves)
        sel = torch.as_tensor(sub, device=DEV)
        for a, b in zip(got, want):
            for j in (0, 1, 2, 3, 5):                        # picks, targets, root values, child_visits, child_count
                assert torch.equal(a[j].index_select(0, sel), b[j]), j
            if ref is ref_full:                              # N' and the cut of the forced engine
                assert torch.equal(a[4].index_select(0, sel), b[4]) and torch.equal(a[6].index_select(0, sel), b[6])
            else:                                            # fast games: never pruned
                cnt = a[5].index_select(0, sel).cpu().numpy()
                tv, cv = a[4].index_select(0, sel).cpu().numpy(), a[3].index_select(0, sel).cpu().numpy()
                for r in range(len(sub)):
                    assert np.array_equal(tv[r, :cnt[r]], cv[r, :cnt[r]]), r
                assert not a[6].index_select(0, sel).any()
        for j, g in enumerate(sub):
            assert _game_tree(capped.engine, g) == _game_tree(ref.engine, j)
    fc = capped.engine.forced_count.cpu().numpy()
    assert fc[fi].sum() > 0 and fc[si].sum() == 0
    assert torch.equal(capped.engine.forced_count[torch.as_tensor(fi, device=DEV)], ref_full.engine.forced_count)
    assert sum(int(x[6].sum()) for x in got) > 0 and capped.forced_counts.tolist() == ref_full.forced_counts.tolist()


# ---- 7. two streams ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dual_stream_halves_search_like_one_engine():
    _need_gpu()
    from liuzhou_amd.tree_engine import DualStreamTreeMCTS, PortableTreeMCTS
    net = _net()
    B, S = 48, 24
    kw = dict(add_dirichlet_noise=True, sample_moves=True, reuse_tree=True, reuse_factor=4.0, seed=SEED,
              forced_playouts_k=K)
    ids = list(range(B))
    dual = DualStreamTreeMCTS(net, B, S, DEV, **kw)
    one = PortableTreeMCTS(net, B, S, DEV, **kw)
    a = _play(dual, ids, 3)
    b = _play(one, ids, 3)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert torch.equal(u, v)
    assert torch.equal(dual.forced_counts, one.forced_counts) and int(one.forced_counts.min()) > 0
    assert torch.equal(torch.cat([p.engine.forced_count for p in dual.parts]), one.engine.forced_count)


# ---- 8 / 9. self-play --------------------------------------------------------------------------------------------------
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
def test_k0_is_the_call_without_the_kwarg(device_tail):
    _need_gpu()
    net = _net()
    ba, sa = _selfplay(net, device_tail=device_tail)
    bb, sb = _selfplay(net, device_tail=device_tail, forced_playouts_k=0.0)
    _batch_equal(ba, bb)
    assert _stats_key(sa) == _stats_key(sb)
    assert "forced_playouts" not in sb.mcts_counters and "pruned_visits" not in sb.mcts_counters


@pytest.mark.gpu
def test_self_play_with_forced_playouts():
    """Same seed -> identical batches; rows sum to 1 on legal actions only; forced descents and pruned visits happen; the
    same games whatever the wave size (multiset of rows); the same outcomes through the finished-row log."""
    _need_gpu()
    from liuzhou_amd.finished_log import FinishedRowLog
    net = _net()
    kw = dict(forced_playouts_k=K)
    b1, s1 = _selfplay(net, **kw)
    b2, s2 = _selfplay(net, **kw)
    _batch_equal(b1, b2)
    assert _stats_key(s1) == _stats_key(s2)
    c = s1.mcts_counters
    assert c["forced_playouts"] > 0 and c["pruned_visits"] > 0
    assert c["forced_playouts"] == s2.mcts_counters["forced_playouts"] and c["pruned_visits"] == s2.mcts_counters["pruned_visits"]
    pol = b1.policy_targets
    assert torch.allclose(pol.sum(1), torch.ones(pol.shape[0], device=pol.device), atol=1e-4)
    assert not (pol * (~b1.legal_masks).to(pol.dtype)).any()
    b0, _ = _selfplay(net)
    assert b0.num_samples != b1.num_samples or not torch.equal(b0.policy_targets, b1.policy_targets)   # k changes the targets
    b3, s3 = _selfplay(net, concurrent_games=8, **kw)
    assert _stats_key(s3) == _stats_key(s1)
    rows = lambda b: sorted(b.state_tensors[i].cpu().numpy().tobytes() + b.policy_targets[i].cpu().numpy().tobytes() +
                            b.value_targets[i:i + 1].cpu().numpy().tobytes() for i in range(b.num_samples))
    assert rows(b1) == rows(b3)
    assert (s3.mcts_counters["forced_playouts"], s3.mcts_counters["pruned_visits"]) == (c["forced_playouts"], c["pruned_visits"])
    log = FinishedRowLog(DEV, segment_games=8, num_slots=12, max_steps=40)
    _, sl = _selfplay(net, row_log=log, **kw)
    assert _stats_key(sl)[:5] == _stats_key(s1)[:5] and sl.avg_game_length == s1.avg_game_length
    assert sl.mcts_counters["forced_playouts"] == c["forced_playouts"]
    # the host loop (device_tail=False) forces and prunes too
    b4, s4 = _selfplay(net, device_tail=False, **kw)
    assert s4.mcts_counters["forced_playouts"] > 0 and s4.mcts_counters["pruned_visits"] > 0
    assert b4.num_samples == s4.num_positions > 0
    assert torch.allclose(b4.policy_targets.sum(1), torch.ones(b4.num_samples, device=pol.device), atol=1e-4)
    assert not (b4.policy_targets * (~b4.legal_masks).to(pol.dtype)).any()


# ---- 10. refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(monkeypatch):
    _need_gpu()
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.tree_engine import DualStreamTreeMCTS, PortableTreeMCTS, PriorEvaluator, TreeEngine
    net = _net()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            PortableTreeMCTS(net, 16, 16, DEV, forced_playouts_k=bad)
        with pytest.raises(ValueError):
            _selfplay(net, forced_playouts_k=bad)
    with pytest.raises(ValueError):
        TreeEngine(16, 16, DEV, 1.0).set_forced_playouts(-2.0)
    with pytest.raises(ValueError):
        PortableTreeMCTS(net, 16, 16, DEV, batch_k=2, forced_playouts_k=K)
    with pytest.raises(ValueError):
        PortableTreeMCTS([net, net], 32, 16, DEV, segment_games=16, forced_playouts_k=K)
    with pytest.raises(ValueError):
        PortableTreeMCTS(PriorEvaluator(lambda p, s: None), 16, 16, DEV, forced_playouts_k=K)
    with pytest.raises(ValueError):
        PortableTreeMCTS(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV), 16, 16, DEV, forced_playouts_k=K)
    with pytest.raises(ValueError):
        DualStreamTreeMCTS(net, 16, 16, DEV, batch_k=2, forced_playouts_k=K)
    with pytest.raises(ValueError):
        _selfplay(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV), evaluator="module", forced_playouts_k=K)
    with pytest.raises(ValueError):
        _selfplay(net, batch_k=2, forced_playouts_k=K)
    monkeypatch.setenv("LZ_TREE_PERSISTENT", "1")
    with pytest.raises(ValueError):
        PortableTreeMCTS(net, 16, 16, DEV, forced_playouts_k=K)
    with pytest.raises(ValueError):
        _selfplay(net, forced_playouts_k=K)


@pytest.mark.gpu
def test_unsupported_entry_points_refuse_the_descriptor():
    """lz_tree_wave_select / lz_tree_search_waves, lz_tree_search_multi* and lz_tree_search_persistent return
    LZ_ERR_UNSUPPORTED (-2) for a descriptor with forced_k > 0, and accept it again with forced_k = 0."""
    _need_gpu()
    from liuzhou_amd import _lib as L
    from liuzhou_amd.tree_engine import LzTreeDesc, TreeEngine
    net = _net()
    eng = TreeEngine(16, 8, DEV, 1.0, batch_k=2)
    eng.set_roots(_positions(np.arange(16)))
    eng.begin()
    d = LzTreeDesc()
    C.memmove(C.byref(d), C.byref(eng.desc), C.sizeof(LzTreeDesc))
    d.forced_k = 2.0
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
        d.forced_k = 0.0
        assert lib.lz_tree_wave_select(C.byref(d), C.byref(eng.wdesc), L.i64(8), C.c_int(1), stream) == 0
    torch.cuda.synchronize()
