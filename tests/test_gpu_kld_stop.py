"""KLD-gain early stopping of the tree search (LzTreeDesc.kld_*, PortableTreeMCTS(kld_stop=), self_play_tree_gpu
(kld_stop_*)): one check of tree_kld_check_kernel against the float64 checker (tests/kld_stop.py), and a stopped search is
bit for bit a search of its budget."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import kld_stop as K
from tests.golden_utils import load, states, FIELDS
from tests.tree_parity import to_gpu_batch, EDGE_LOGICAL

DEV = torch.device("cuda:0")
SEED = 7
MAXC = 72


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _net():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    torch.manual_seed(20260314)
    return FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))


_CACHE = {}


def _fixture():
    """The positions of g1_rules.npz and their legal action counts (host build of the encoder)."""
    if "st" not in _CACHE:
        from liuzhou_amd.mcts_gpu import encode_actions_fast
        st = states(load("g1_rules.npz"), "s")
        mask, _ = encode_actions_fast(to_gpu_batch(st, "cpu"))
        _CACHE["st"], _CACHE["legal"] = st, mask.sum(1).numpy()
    return _CACHE["st"], _CACHE["legal"]


def _positions(idx):
    st_all, _ = _fixture()
    return to_gpu_batch({f: np.ascontiguousarray(np.asarray(st_all[f])[idx]) for f in FIELDS}, DEV)


def _pick(counts):
    """Position indices by legal action count: `counts` = [(lo, hi, how many)], the first positions of every band."""
    _, legal = _fixture()
    out = []
    for lo, hi, n in counts:
        band = np.nonzero((legal >= lo) & (legal <= hi))[0]
        assert len(band) >= n
        out += band[:n].tolist()
    return np.asarray(out)


def _game_tree(e, g):
    nodes = e.game_nodes(g)
    runs = [tuple(e.edge_run(int(n["edge_begin"]), max(0, int(n["nedges"])))[f].tobytes() for f in EDGE_LOGICAL)
            for n in nodes]
    return tuple(nodes[f].tobytes() for f in ("w0", "w1", "w2", "w3", "nedges", "parent")), runs


def _root_visits(e, g):
    return np.asarray([r["visit_count"] for r in e.root_edge_records(g)], dtype=np.int64)


def _play(m, pos, gids, moves, budgets=None):
    """`moves` searches from the positions `pos` (global game ids `gids`) with kept subtrees.  Per move the outputs and the
    budgets the search left; `budgets`: per move the budgets to inject."""
    from liuzhou_amd import v0_core
    batch = _positions(np.asarray(pos))
    n = len(pos)
    gid = torch.as_tensor(np.asarray(gids), dtype=torch.int64, device=DEV)
    outs, left = [], []
    for t in range(moves):
        if budgets is not None:
            m.injected_sim_budget = budgets[t]
        plies = torch.full((n,), t, dtype=torch.int64, device=DEV)
        out = m.search_batch(batch, temperatures=torch.ones(n, device=DEV), rng_game_ids=gid, rng_plies=plies)
        outs.append((out.chosen_action_indices.clone(), out.policy_dense.clone(), out.root_value.clone()))
        left.append(None if m.last_sim_budget is None else m.last_sim_budget.clone())
        done = torch.zeros(n, dtype=torch.bool, device=DEV)
        v0_core.self_play_step_inplace(*batch.tensors(), plies.clone(), done, torch.arange(n, device=DEV),
                                       out.chosen_action_codes.clone(), out.terminal_mask.clone(),
                                       out.chosen_valid_mask.clone(), 512, 2.0)
    torch.cuda.synchronize()
    return outs, left


# ---- 1. one check through the C ABI ----------------------------------------------------------------------------------------------
GUARD = 16
PAT = {torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.float64: -12345.0}


def _guarded(n, dtype):
    whole = torch.full((n + 2 * GUARD,), PAT[dtype], dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, dtype):
    w = whole.cpu()
    return bool((w[:GUARD] == PAT[dtype]).all()) and bool((w[-GUARD:] == PAT[dtype]).all())


@pytest.mark.gpu
def test_one_check_equals_the_checker():
    """64 games after a plain 24-simulation search; crafted snapshot rows; lz_tree_kld_check at s = 16 with M = 24 (never
    a stop) and with M = 8.  Gains within 1e-11 of the float64 checker; decisions, budgets, counters and the new snapshot
    exact; an inactive slot, spent budgets and an edgeless root untouched; guard words intact."""
    _need_gpu()
    from liuzhou_amd import _lib as L
    from liuzhou_amd.tree_engine import LzTreeDesc, PortableTreeMCTS
    B, S, s = 64, 24, 16
    pos = _pick([(1, 1, 10), (2, 2, 8), (36, 36, 13), (3, 6, 11), (7, 20, 14), (21, 35, 8)])
    m = PortableTreeMCTS(_net(), B, S, DEV, add_dirichlet_noise=True, seed=SEED, use_graph=False)
    m.search_batch(_positions(pos), temperatures=torch.ones(B, device=DEV))
    torch.cuda.synchronize()
    e = m.engine
    vis = [_root_visits(e, g) for g in range(B)]
    ne = np.asarray([len(v) for v in vis])
    assert (ne == 1).sum() >= 8 and (ne == 2).sum() >= 1 and (ne == 36).sum() >= 1 and ne.max() <= 36
    assert all(int(v.sum()) == S for v in vis if len(v))
    # crafted rows, by kind; columns from ne on hold garbage the kernel must not read into its sums
    rng = np.random.default_rng(11)
    snap = rng.integers(1, 50, (B, MAXC)).astype(np.int32)
    kind = np.arange(B) % 6
    kind[:10] = [2, 2, 2, 2, 0, 1, 3, 4, 5, 2]                        # the one-child roots: five rows of exactly half
    for g in range(B):
        n = vis[g]
        k = len(n)
        if kind[g] == 0:
            row = np.zeros(k, np.int64)                               # O = 0: nothing decided
        elif kind[g] == 1:
            row = n.copy()                                            # N = O: nothing decided
        elif kind[g] == 2:
            row = n // 2                                              # exactly half where integral: gain exactly 0
        elif kind[g] == 3:
            row = np.zeros(k, np.int64)
            if k:
                row[int(np.argmax(n))] = int(n.max())                 # all the old mass on one visited child
        elif kind[g] == 4:
            row = n.copy()
            row[1::2] = 0                                             # o_k = 0 < n_k on every other child
        else:
            row = rng.integers(0, n + 1) if k else np.zeros(0, np.int64)
        snap[g, :k] = row
    halves = [g for g in range(B) if kind[g] == 2 and len(vis[g]) and not (vis[g] % 2).any()]
    assert len(halves) >= 3
    inactive, spent_eq, spent_lt = halves[0], halves[1], [g for g in range(B) if kind[g] == 5][0]
    budget0 = np.full(B, S, np.int32)
    budget0[spent_eq], budget0[spent_lt] = s + 1, 5
    active = np.ones(B, np.uint8)
    active[inactive] = 0

    def want(M, theta):
        rows = []
        for g in range(B):
            k = len(vis[g])
            if k == 0 or not active[g] or budget0[g] <= s + 1:
                rows.append((None, False, snap[g].astype(np.int64)))
                continue
            per, stop, new = K.check(snap[g, :k], vis[g], s, M, theta)
            rows.append((per, stop, np.concatenate([new, np.zeros(MAXC - k, np.int64)])))
        return rows

    gains = sorted(r[0] for r in want(8, 1.0) if r[0] is not None and r[0] > 0.0)
    assert len(gains) >= 16
    # theta in the widest gap (as a ratio) of the middle half of the positive gains: rows on both sides of it, every
    # decision far from double rounding
    lo, hi = len(gains) // 4, (3 * len(gains)) // 4
    ratios = [gains[i + 1] / gains[i] for i in range(lo, hi)]
    at = lo + int(np.argmax(ratios))
    assert gains[at + 1] / gains[at] >= 1.0 + 1e-6
    theta = float(np.sqrt(gains[at] * gains[at + 1]))
    decided = [r for r in want(8, theta) if r[0] is not None]
    zero_rows = sum(1 for r in decided if r[0] == 0.0)
    assert zero_rows >= 3 and sum(r[1] for r in decided) >= zero_rows + lo and sum(not r[1] for r in decided) >= 4

    w_snap, d_snap = _guarded(B * MAXC, torch.int32)
    w_bud, d_bud = _guarded(B, torch.int32)
    w_stops, d_stops = _guarded(B, torch.int64)
    w_saved, d_saved = _guarded(B, torch.int64)
    w_trace, d_trace = _guarded(B, torch.float64)
    e.buf["active"].copy_(torch.from_numpy(active).to(DEV))
    d = LzTreeDesc()
    C.memmove(C.byref(d), C.byref(e.desc), C.sizeof(LzTreeDesc))
    d.sim_budget = d.kld_budget = d_bud.data_ptr()
    d.kld_snapshot, d.kld_stops, d.kld_saved, d.kld_trace = (t.data_ptr() for t in (d_snap, d_stops, d_saved, d_trace))
    d.kld_threshold, d.kld_interval = theta, 8
    lib, st = L.lib(), L.stream_ptr(DEV)
    for M in (24, 8):                                                 # s < M first: gains, no decision
        d.kld_min_sims = M
        d_snap.copy_(torch.from_numpy(snap.reshape(-1)).to(DEV))
        d_bud.copy_(torch.from_numpy(budget0).to(DEV))
        d_stops.fill_(5); d_saved.fill_(100); d_trace.fill_(-1.0)
        assert lib.lz_tree_kld_check(C.byref(d), 16, st) == 0
        torch.cuda.synchronize()
        rows = want(M, theta)
        got_snap = d_snap.cpu().numpy().reshape(B, MAXC)
        got_bud, got_trace = d_bud.cpu().numpy(), d_trace.cpu().numpy()
        got_stops, got_saved = d_stops.cpu().numpy(), d_saved.cpu().numpy()
        assert not np.isnan(got_trace).any()
        stops = 0
        for g, (per, stop, new) in enumerate(rows):
            assert np.array_equal(got_snap[g], new), (M, g)
            if per is None:
                assert got_trace[g] == -1.0, (M, g)                   # untouched when no gain was formed
            else:
                N, O = int(vis[g].sum()), int(snap[g, :len(vis[g])].sum())
                assert abs(got_trace[g] - per) <= 1e-11 and abs(got_trace[g] * (N - O) - per * (N - O)) <= 1e-11, (M, g)
                if kind[g] == 2 and g in halves:
                    assert got_trace[g] == 0.0
            assert got_bud[g] == (s + 1 if stop else budget0[g]), (M, g)
            assert got_stops[g] == 5 + int(stop) and got_saved[g] == 100 + (int(budget0[g]) - (s + 1) if stop else 0), (M, g)
            stops += int(stop)
        assert stops == (0 if M == 24 else sum(r[1] for r in decided))
        assert got_bud[inactive] == S and got_bud[spent_eq] == s + 1 and got_bud[spent_lt] == 5
        for whole, dt in ((w_snap, torch.int32), (w_bud, torch.int32), (w_stops, torch.int64), (w_saved, torch.int64),
                          (w_trace, torch.float64)):
            assert _guards_intact(whole, dt)
    # step 0 stores the snapshot only
    d_snap.copy_(torch.from_numpy(snap.reshape(-1)).to(DEV)); d_bud.copy_(torch.from_numpy(budget0).to(DEV))
    d_stops.fill_(5); d_trace.fill_(-1.0)
    assert lib.lz_tree_kld_check(C.byref(d), 0, st) == 0
    torch.cuda.synchronize()
    got_snap = d_snap.cpu().numpy().reshape(B, MAXC)
    for g in range(B):
        k = len(vis[g])
        new = np.concatenate([vis[g], np.zeros(MAXC - k, np.int64)]) if (k and active[g] and budget0[g] > 1) else snap[g]
        assert np.array_equal(got_snap[g], new)
    assert bool((d_stops == 5).all()) and bool((d_trace == -1.0).all()) and np.array_equal(d_bud.cpu().numpy(), budget0)
    # the budget must be the array the searches read; the step-by-step entry points refuse the rule
    d.kld_budget = d_snap.data_ptr()
    assert lib.lz_tree_kld_check(C.byref(d), 16, st) == -1
    d.kld_budget = d_bud.data_ptr()
    d.kld_interval = 0
    assert lib.lz_tree_kld_check(C.byref(d), 16, st) == -1
    d.kld_interval = 8
    assert lib.lz_tree_select(C.byref(d), st) == -2
    d.sim_budget = None                                               # the rule set, the budget array missing
    assert lib.lz_tree_select(C.byref(d), st) == -2
    assert lib.lz_tree_kld_check(C.byref(d), 16, st) == -1
    d.kld_threshold = 0.0                                             # off: nothing is launched
    d_snap.fill_(7)
    assert lib.lz_tree_kld_check(C.byref(d), 16, st) == 0
    torch.cuda.synchronize()
    assert bool((d_snap == 7).all())


# ---- 2. a stopped search is a search of its budget -----------------------------------------------------------------------------
B2, S2, I2, M2 = 40, 48, 8, 16
KW2 = dict(sample_moves=True, reuse_tree=True, reuse_factor=4.0, seed=SEED, add_dirichlet_noise=True)


def _pos2():
    return _pick([(1, 1, 10), (2, 4, 18), (30, 36, 12)])


def _threshold(net, split):
    """Every game's root visits at every check of the first move (engines with the rule off and sims = 8k, direct
    launches), and theta: the geometric midpoint of the widest gap (as a ratio) in the middle half of the pooled positive
    per-simulation gains.  (A gain of exactly 0 -- a root with one child -- is below every theta > 0 and is not pooled.)"""
    key = ("theta", split)
    if key not in _CACHE:
        from liuzhou_amd.tree_engine import PortableTreeMCTS
        pos, gids = _pos2(), list(range(300, 300 + B2))
        at = [[np.zeros(0, np.int64)] * B2]
        for k in range(1, (S2 - 2) // I2 + 1):
            m = PortableTreeMCTS(net, B2, I2 * k, DEV, use_graph=False, **KW2)
            _play(m, pos, gids, 1)
            at.append([_root_visits(m.engine, g) for g in range(B2)])
        at[0] = [np.zeros_like(v) for v in at[1]]                    # fresh roots: the snapshot behind launch 0
        traj = [[at[j][g] for j in range(len(at))] for g in range(B2)]
        pooled = sorted(p for g in range(B2) for _, p in K.replay(traj[g], S2, I2, M2, 0.0)[1] if p > 0.0)
        lo, hi = len(pooled) // 4, (3 * len(pooled)) // 4
        ratios = [pooled[i + 1] / pooled[i] for i in range(lo, hi)]
        i = lo + int(np.argmax(ratios))
        print(f"[kld] split={split} pooled gains {len(pooled)}: min {pooled[0]:.3e} q1 {pooled[lo]:.3e} "
              f"median {pooled[len(pooled) // 2]:.3e} q3 {pooled[hi]:.3e} max {pooled[-1]:.3e}; gap {pooled[i]:.6e} .. "
              f"{pooled[i + 1]:.6e} (ratio {pooled[i + 1] / pooled[i]:.6f})")
        _CACHE[key] = (traj, float(np.sqrt(pooled[i] * pooled[i + 1])), pooled[i + 1] / pooled[i])
    return _CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["0", "1"])
@pytest.mark.parametrize("graph", [True, False])
def test_a_stopped_search_is_a_search_of_its_budget(monkeypatch, split, graph):
    """40 games, S = 48, I = 8, M = 16, root noise, 3 moves with kept subtrees.  theta comes from the checker; the budgets
    of the first move equal the checker's replay; picks, policies, root values, every game's node and edge records and
    root_visits equal, byte for byte, those of a playout-cap engine (fast_simulations = 1, full_prob = 1: every search full)
    that is handed the rule's per-move budgets -- it launches no new kernel."""
    _need_gpu()
    from liuzhou_amd.kld_stop import parse_kld_stop
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    monkeypatch.setenv("LZ_TREE_SPLIT", split)
    net = _net()
    traj, theta, ratio = _threshold(net, split)
    assert ratio >= 1.0 + 1e-6
    pos, gids, moves = _pos2(), list(range(300, 300 + B2)), 3
    rule = PortableTreeMCTS(net, B2, S2, DEV, use_graph=graph, kld_stop=parse_kld_stop(theta, I2, M2), **KW2)
    got, budgets = _play(rule, pos, gids, moves)
    first = budgets[0].cpu().numpy()
    replay = np.asarray([K.replay(traj[g], S2, I2, M2, theta)[0] for g in range(B2)])
    early, full = int((first < S2).sum()), int((first == S2).sum())
    print(f"[kld] split={split} graph={graph} theta {theta:.6e}: {early} games stop early, {full} run to S; budgets "
          f"{sorted(set(first.tolist()))}")
    assert np.array_equal(first, replay)
    assert early >= B2 // 4 and full >= B2 // 4
    assert all(bool((b <= S2).all()) and bool((b >= 1).all()) for b in budgets)
    stopped = sum(int((b < S2).sum()) for b in budgets)
    saved = sum(int((S2 - b).sum()) for b in budgets)
    assert rule.kld_counts.tolist() == [stopped, saved]
    ref = PortableTreeMCTS(net, B2, S2, DEV, use_graph=graph, fast_simulations=1, full_prob=1.0, **KW2)
    want, handed = _play(ref, pos, gids, moves, budgets=budgets)
    for (ca, pa, va), (cb, pb, vb) in zip(got, want):
        assert torch.equal(ca, cb) and torch.equal(pa, pb) and torch.equal(va, vb)
    for a, b in zip(budgets, handed):
        assert torch.equal(a, b)
    for g in range(B2):
        assert _game_tree(rule.engine, g) == _game_tree(ref.engine, g)
    assert torch.equal(rule.engine.buf["root_visits"], ref.engine.buf["root_visits"])
    assert int(rule.engine.reuse_dropped.sum()) == 0
    assert rule.leaf_evals <= sum(int((b + 1).sum()) for b in budgets)
    assert rule.leaf_evals == ref.leaf_evals


# ---- 3. two streams -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dual_stream_halves_search_like_one_engine():
    _need_gpu()
    from liuzhou_amd.kld_stop import parse_kld_stop
    from liuzhou_amd.tree_engine import DualStreamTreeMCTS, PortableTreeMCTS
    net = _net()
    B, S = 48, 32
    kw = dict(KW2, kld_stop=parse_kld_stop(5e-3, 8, 8))
    pos, gids = _pick([(1, 1, 12), (2, 6, 18), (20, 36, 18)]), list(range(B))
    order = np.random.default_rng(5).permutation(B)                   # both halves get every kind of root
    pos = pos[order]
    dual = DualStreamTreeMCTS(net, B, S, DEV, **kw)
    one = PortableTreeMCTS(net, B, S, DEV, **kw)
    a, ba = _play(dual, pos, gids, 3)
    b, bb = _play(one, pos, gids, 3)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert torch.equal(u, v)
    for u, v in zip(ba, bb):
        assert torch.equal(u, v)
    assert any(bool((u < S).any()) for u in ba) and any(bool((u == S).any()) for u in ba)
    assert torch.equal(dual.kld_counts, one.kld_counts) and int(one.kld_counts[0]) > 0


# ---- 4. with the playout cap -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_rule_only_lowers_the_caps_budgets():
    """Cap F = 6 < M = 8 with a threshold above every gain: a full search stops at its first eligible check (s = 8),
    a fast one is never stopped."""
    _need_gpu()
    from liuzhou_amd.kld_stop import parse_kld_stop
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    B, S, F = 40, 32, 6
    full = torch.from_numpy(np.random.default_rng(3).random(B) < 0.5).to(DEV)
    m = PortableTreeMCTS(_net(), B, S, DEV, fast_simulations=F, full_prob=0.5, kld_stop=parse_kld_stop(1e9, 4, 8), **KW2)
    m.injected_full_search = full
    _, budgets = _play(m, _pick([(1, 1, 6), (2, 36, 34)]), list(range(B)), 2)
    stopped = 0
    for b in budgets:
        draw = torch.where(full, S, F).to(torch.int32)
        assert bool((b <= draw).all())
        assert torch.equal(b[~full], draw[~full])                     # F < M: never stopped
        assert bool((b[full] == 9).all())                             # snapshot 0, O = 0 at s = 4, stop at s = 8
        stopped += int(full.sum())
    assert m.kld_counts.tolist() == [stopped, stopped * (S - 9)]
    assert m.cap_counts.tolist() == [2 * int(full.sum()), 2 * int((~full).sum())]


# ---- 5. self-play -------------------------------------------------------------------------------------------------------------------
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
def test_self_play_off_is_unchanged_and_on_stops_searches(device_tail):
    _need_gpu()
    net = _net()
    ba, sa = _selfplay(net, device_tail=device_tail)
    bb, sb = _selfplay(net, device_tail=device_tail, kld_stop_threshold=0.0, kld_stop_interval=4, kld_stop_min_simulations=4)
    _batch_equal(ba, bb)
    assert _stats_key(sa) == _stats_key(sb)
    drop = ("setup_ms", "build_ms", "final_sync_ms", "loop_ms", "host_wait_ms", "engine_cache_hit")
    assert {k: v for k, v in sa.mcts_counters.items() if k not in drop} == \
           {k: v for k, v in sb.mcts_counters.items() if k not in drop}
    assert not any(k.startswith("kld_") for k in sb.mcts_counters)
    # a threshold above every gain: every eligible check stops.  Fresh roots (no kept subtrees): the snapshot is zeros, the
    # check at s = 4 has O = 0 and the one at s = 8 stops, so every stopped search saves 16 - 9 simulations
    on = dict(kld_stop_threshold=1e9, kld_stop_interval=4, kld_stop_min_simulations=4)
    bf, sf = _selfplay(net, device_tail=device_tail, reuse_tree=False, **on)
    c = sf.mcts_counters
    assert c["kld_stopped_searches"] > 0 and c["kld_simulations_saved"] == 7 * c["kld_stopped_searches"]
    assert c["leaf_eval_count"] <= sa.mcts_counters["leaf_eval_count"]
    # kept subtrees: a carried root has O > 0 at s = 4 already (saves 11), a fresh one stops at s = 8 (saves 7)
    bk, sk = _selfplay(net, device_tail=device_tail, **on)
    k = sk.mcts_counters
    assert k["kld_stopped_searches"] > 0
    assert 7 * k["kld_stopped_searches"] <= k["kld_simulations_saved"] <= 11 * k["kld_stopped_searches"]
    for b, st in ((bf, sf), (bk, sk)):
        assert b.num_samples == st.num_positions > 0 and st.black_wins + st.white_wins + st.draws == st.num_games
        pol = b.policy_targets
        assert torch.allclose(pol.sum(1), torch.ones(pol.shape[0], device=pol.device), atol=1e-4)
        assert not (pol * (~b.legal_masks).to(pol.dtype)).any()
        assert torch.isfinite(b.value_targets).all()


@pytest.mark.gpu
def test_worker_run_reports_the_rule(tmp_path):
    _need_gpu()
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.self_play_stage import load_self_play_payload, merge_worker_manifests
    from liuzhou_amd.self_play_worker import run_self_play_worker
    from liuzhou_amd.tree_engine import clear_engine_cache
    torch.manual_seed(20260314)
    mod = ChessNet(**MODEL_CONFIGS["b6c64"])
    ck = tmp_path / "model_state_cpu.pt"
    torch.save(mod.state_dict(), ck)
    out = tmp_path / "w.pt"
    run_self_play_worker(worker_idx=0, shard_device="cuda:0", shard_games=16, seed=5, model_state_path=str(ck),
                         output_path=str(out), mcts_simulations=16, temperature_init=1.0, temperature_final=0.1,
                         temperature_threshold=10, exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25,
                         soft_value_k=2.0, opening_random_moves=2, max_game_plies=40, concurrent_games_per_device=8,
                         chunk_output_dir=str(tmp_path), chunk_file_prefix="w", search_backend="tree",
                         kld_stop_threshold=1e9, kld_stop_interval=4, kld_stop_min_simulations=4)
    clear_engine_cache()
    man = torch.load(out, weights_only=False)
    settings = {"threshold": 1e9, "interval": 4, "min_simulations": 4}
    assert man["metadata"]["kld_stop"] == settings
    c = man["stats"]["mcts_counters"]
    assert c["kld_stopped_searches"] > 0 and c["kld_simulations_saved"] >= 7 * c["kld_stopped_searches"]
    merged = merge_worker_manifests([str(out)], output_path=str(tmp_path / "sp.pt"))
    assert merged["metadata"]["kld_stop"] == {**settings, "kld_stopped_searches": int(c["kld_stopped_searches"]),
                                              "kld_simulations_saved": int(c["kld_simulations_saved"])}
    samples, _, meta = load_self_play_payload(str(tmp_path / "sp.pt"))
    assert meta["kld_stop"] == merged["metadata"]["kld_stop"]
    assert samples.value_targets.shape[0] == man["num_samples"] > 0


# ---- 6. refusals on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(monkeypatch):
    _need_gpu()
    from liuzhou_amd.kld_stop import parse_kld_stop
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    net = _net()
    ks = parse_kld_stop(1e-3, 4, 4)
    on = dict(kld_stop_threshold=1e-3, kld_stop_interval=4)
    with pytest.raises(ValueError, match="Gumbel"):
        PortableTreeMCTS(net, 16, 16, DEV, gumbel_considered=8, kld_stop=ks)
    with pytest.raises(ValueError, match="Gumbel"):
        _selfplay(net, gumbel_considered=8, **on)
    with pytest.raises(ValueError, match="batch_k"):
        PortableTreeMCTS(net, 16, 16, DEV, batch_k=4, kld_stop=ks)
    with pytest.raises(ValueError, match="batch_k"):
        _selfplay(net, batch_k=4, **on)
    with pytest.raises(ValueError, match="external evaluator"):
        _selfplay(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV), evaluator="module", **on)
    monkeypatch.setenv("LZ_TREE_PERSISTENT", "1")
    with pytest.raises(ValueError, match="persistent"):
        PortableTreeMCTS(net, 16, 16, DEV, kld_stop=ks)
    with pytest.raises(ValueError, match="persistent"):
        _selfplay(net, **on)
