"""Visit-offset / value-cutoff move selection of the tree backend (lz_tree_move_pick, PortableTreeMCTS(move_visit_offset=,
move_value_cutoff=), self_play_tree_gpu(move_visit_offset=, move_value_cutoff=, temperature_halflife=)): the kernel against
the float64 checker (tests/move_pick.py) on real roots with crafted statistics, the production path, self-play, worker."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import move_pick as chk
from tests.golden_utils import load, states, FIELDS
from tests.hand_roots import _code
from tests.tree_parity import to_gpu_batch, root_edges, EDGE_DT, NODE_DT

DEV = torch.device("cuda:0")
SEED = 7
OFFSETS = (0.0, 0.5, 1.0, 3.0, 1e6)
CUTOFFS = (0.0, 0.125, 1.0, 2.0)
TEMPS = (1.0, 0.5, 2.0, 1e-7)
INFO_WHITE = 1


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


_CACHE = {}


def _fixture():
    """The positions of g1_rules.npz and their legal action counts (host build of the encoder)."""
    if "st" not in _CACHE:
        from liuzhou_amd.mcts_gpu import encode_actions_fast
        st = states(load("g1_rules.npz"), "s")
        mask, _ = encode_actions_fast(to_gpu_batch(st, "cpu"))
        _CACHE["st"], _CACHE["legal"] = st, mask.sum(1).numpy()
    return _CACHE["st"], _CACHE["legal"]


def _by_count(counts):
    """Position indices by legal action count: `counts` = [(lo, hi, how many)], from every band its first positions with
    the phases taking turns (the fixture is ordered by phase)."""
    st, legal = _fixture()
    phase = np.asarray(st["phase"])
    out = []
    for lo, hi, n in counts:
        band = np.nonzero((legal >= lo) & (legal <= hi))[0]
        assert len(band) >= n
        rank = np.zeros(len(band), dtype=np.int64)               # the i-th position of its phase inside the band
        for p in np.unique(phase[band]):
            rank[phase[band] == p] = np.arange(int((phase[band] == p).sum()))
        out += band[np.lexsort((phase[band], rank))][:n].tolist()
    return np.asarray(out)


def _positions(idx, terminal=()):
    """The fixture positions `idx` on the device; the slots in `terminal` get the no-capture limit (a drawn, terminal root)."""
    st_all, _ = _fixture()
    st = {f: np.ascontiguousarray(np.asarray(st_all[f])[idx]).copy() for f in FIELDS}
    for g in terminal:
        st["moves_since_capture"][g] = 36
    return to_gpu_batch(st, DEV), st


GUARD = 16
PAT = {torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}


def _guarded(n, dtype):
    whole = torch.full((n + 2 * GUARD,), PAT[dtype], dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, dtype):
    w = whole.cpu()
    return bool((w[:GUARD] == PAT[dtype]).all()) and bool((w[-GUARD:] == PAT[dtype]).all())


def _write_run(e, e0, recs):
    e.buf["edges"][e0:e0 + len(recs)].copy_(torch.from_numpy(recs.view(np.int64).reshape(len(recs), 4)).to(DEV))


def _craft(rng, kind, ne, o, c, white, root_player):
    """Visits N and eighths j (q_k = j_k / 8 in the root mover's frame; W = N * j / 8 in the child's, exact in double) of one
    root by kind.  Returns N, W."""
    N = rng.integers(0, 41, ne).astype(np.int64)
    j = rng.integers(-8, 9, ne).astype(np.float64)
    ks = int(rng.integers(0, ne))
    if kind == 1:                                             # ties for k*
        N[:] = np.minimum(N, 30)
        N[rng.integers(0, ne, 3)] = 30
    elif kind == 2:                                           # n' exactly 0 next to n' just above it
        N[ks] = 40
        for k in range(ne):
            if k != ks and k % 2 == 0:
                N[k] = int(o) if o == int(o) and o <= 30 else 1
            elif k != ks and k % 4 == 1:
                N[k] = int(o) + 1 if o <= 30 else 2
    elif kind == 3:                                           # q exactly at q* - c, and one double ulp below it
        N[:] = np.minimum(N, 31)
        N[ks] = 32
        j[ks] = 8
        for k in range(ne):
            if k != ks and k % 3 != 2:
                N[k] = 16                                     # a power of two: W / N is exact for any W
                j[k] = 8.0 * (j[ks] / 8.0 - c)
                if k % 3 == 1:
                    j[k] = 8.0 * np.nextafter(j[ks] / 8.0 - c, -np.inf)
    elif kind == 4:                                           # everything but k* cut: by the offset, or by the value test
        N[:] = 0 if rng.random() < 0.5 else np.minimum(N, 1)
        N[ks] = 35
        j[:] = -8
        j[ks] = 8
    elif kind == 5:                                           # nothing visited at all
        N[:] = 0
    q = j / 8.0
    q[N == 0] = 0.0
    sign = np.where(np.where(white, -1, 1) == root_player, 1.0, -1.0)
    W = sign * (N.astype(np.float64) * q)
    got = chk.child_q(W, N, white, root_player)
    assert np.array_equal(got, q + 0.0)                        # exact in double, as the test needs it
    return N, W


# ---- 1. the kernel against the checker -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_kernel_equals_the_checker():
    """64 real roots (ne from 1 to 36, three terminal ones, one slot that is not searched, one root edited to 65 and one to
    128 edges inside their own chunks) after a 32-simulation search; the roots' edge records are overwritten with crafted
    N and W; every (o, c) of the issue's grid in one call each, temperatures and force masks varied per game.  Picks,
    codes and counters equal the checker exactly; every other finish output and the guard words stay as they were."""
    _need_gpu()
    from liuzhou_amd import _lib as L
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    B, S = 64, 32
    idx = _by_count([(1, 1, 6), (2, 2, 4), (36, 36, 8), (3, 6, 12), (7, 20, 22), (21, 35, 12)])
    terminal = [20, 37, 58]                                      # three of the mid-sized roots
    batch, st = _positions(idx, terminal)
    idle = [g for g in range(B) if g not in terminal][5]
    active = torch.ones(B, dtype=torch.bool, device=DEV)
    active[idle] = False
    m = PortableTreeMCTS(_net(), B, S, DEV, add_dirichlet_noise=True, seed=SEED, use_graph=False)
    m.search_batch(batch, temperatures=torch.ones(B, device=DEV), active=active)
    torch.cuda.synchronize()
    e = m.engine
    term = e.terminal_mask.cpu().numpy().astype(bool)
    assert all(term[g] for g in terminal) and term[idle] and term.sum() >= 4
    nodes = e.buf["nodes"].view(B, e.node_cap, 6)[:, 0].contiguous().cpu().numpy().view(NODE_DT).reshape(B)
    real = root_edges(e)
    ne = np.asarray([len(r) for r in real])
    live = [g for g in range(B) if not term[g]]
    assert ne[live].min() == 1 and ne.max() == 36 and (ne[live] == 1).sum() >= 4
    # two roots get more edges than any position has: the node record says 65 / 128, the run is rewritten whole.  Both runs
    # start their chunk (the root expands first), so they stay inside it.
    roomy = [g for g in live if ne[g] == 36 and g % 4 != 3 and g % 11 != 3]      # (games the calls below re-pick)
    wide = {roomy[0]: 65, roomy[1]: 128}
    assert e.edge_chunk >= 128
    for g, n in wide.items():
        e0 = int(nodes[g]["edge_begin"])
        assert e0 % e.edge_chunk == 0
        rec = nodes[g:g + 1].copy()
        rec["nedges"] = n
        e.buf["nodes"].view(B, e.node_cap, 6)[g, 0].copy_(torch.from_numpy(rec.view(np.int64).reshape(6)).to(DEV))
        ne[g] = n
    root_player = np.where(np.asarray(st["current_player"]) == 1, 1, -1)
    phase = np.asarray(st["phase"])
    e0s = [int(nodes[g]["edge_begin"]) for g in range(B)]
    lib, stream = L.lib(), L.stream_ptr(DEV)
    rng = np.random.default_rng(20260119)
    temps_np = np.asarray([TEMPS[g % 4] for g in range(B)], dtype=np.float32)
    force_np = np.zeros(B, dtype=np.uint8)
    force_np[[g for g in live if g % 11 == 3]] = 1
    temps, force = torch.from_numpy(temps_np).to(DEV), torch.from_numpy(force_np).to(DEV)
    w_idx, d_idx = _guarded(B, torch.int32)
    w_code, d_code = _guarded(4 * B, torch.int32)
    w_cnt, d_cnt = _guarded(4, torch.int64)
    seen = dict(applied=0, changed=0, cut_visits=0, cut_value=0, star_cut=0, only_star=0, ties=0, upper=0, zero_np=0,
                edge_q=0, ulp_q=0)
    for case, (o, c) in enumerate([(o, c) for o in OFFSETS for c in CUTOFFS]):
        recs = {}
        for g in live:
            n = int(ne[g])
            r = np.zeros(n, EDGE_DT)
            k0 = len(real[g])
            r[:k0] = real[g]
            if n > k0:                                          # the widened roots: fresh records behind the real ones
                r["act"][k0:] = [a for a in range(220) if a not in set(real[g]["act"].tolist())][:n - k0]
                r["P"][k0:] = 1.0 / n
                r["n_info"][k0:] = rng.integers(0, 2, n - k0).astype(np.uint32) << 24
                r["child"][k0:] = -1
            white = ((r["n_info"] >> 24) & INFO_WHITE).astype(bool)
            N, W = _craft(rng, (g + case) % 6, n, o, c, white, int(root_player[g]))
            r["n_info"] = (r["n_info"] & np.uint32(0xFF000000)) | N.astype(np.uint32)
            r["W"] = W
            _write_run(e, e0s[g], r)
            recs[g] = (N, chk.child_q(W, N, white, int(root_player[g])), r["act"].astype(np.int64))
        # uniforms: fixed seed, redrawn (deterministically) until u * S is clear of every C_k in the checker
        u_np = np.zeros(B, dtype=np.float32)
        results = {}
        for g in range(B):
            on = g in recs and chk.applies(terminal=False, sample_moves=True, temperature=temps_np[g],
                                           force_uniform=bool(force_np[g]), offset=o, cutoff=c)
            for _ in range(64):
                u_np[g] = np.float32(rng.uniform(0.001, 0.999))
                if not on:
                    break
                results[g] = chk.pick(*recs[g][:2], temps_np[g], u_np[g], o, c)
                if chk.margin_ok(results[g]):
                    break
            assert not on or chk.margin_ok(results[g]), (case, g)
        uniforms = torch.from_numpy(u_np).to(DEV)
        e.finish(temps, uniforms, None, 0.0, force, True)
        torch.cuda.synchronize()
        others = [t.clone() for t in (e.policy_dense, e.child_visits, e.child_prior, e.root_value, e.terminal_mask,
                                      e.chosen_valid, e.child_count, e.child_action)]
        fin_idx = e.chosen_index.cpu().numpy().astype(np.int64)
        fin_code = e.chosen_code.cpu().numpy().reshape(B, 4).astype(np.int64)
        d_idx.copy_(e.chosen_index); d_code.copy_(e.chosen_code.reshape(-1)); d_cnt.fill_(1000)
        rc = lib.lz_tree_move_pick(C.byref(e.desc), L.ptr(temps), L.ptr(force), L.ptr(uniforms), 1, C.c_double(o),
                                   C.c_double(c), L.ptr(d_idx), L.ptr(d_code), L.ptr(d_cnt), stream)
        torch.cuda.synchronize()
        assert rc == 0
        want_idx, want_code, cnt = fin_idx.copy(), fin_code.copy(), np.zeros(4, np.int64)
        for g, r in results.items():
            a = int(recs[g][2][r["pick"]])
            cnt += [1, r["cut_visits"], r["cut_value"], int(a != fin_idx[g])]
            if a != fin_idx[g]:
                want_idx[g], want_code[g] = a, _code(phase[g], a)
            N = recs[g][0]
            seen["star_cut"] += int(r["target"] is None)
            seen["only_star"] += int(r["target"] is not None and r["eligible"].sum() == 1 and len(N) > 1)
            seen["ties"] += int((N == N.max()).sum() > 1)
            seen["upper"] += int(r["pick"] >= 64)
            seen["zero_np"] += int(o > 0 and np.any(N.astype(np.float64) - o == 0.0))
            q, ks = recs[g][1], r["kstar"]
            seen["edge_q"] += int(c > 0 and np.any((q == q[ks] - c) & r["eligible"] & (np.arange(len(N)) != ks)))
            seen["ulp_q"] += int(c > 0 and np.any((q == np.nextafter(q[ks] - c, -np.inf)) & ~r["eligible"] & (N - o > 0)))
        got_idx, got_code = d_idx.cpu().numpy().astype(np.int64), d_code.cpu().numpy().reshape(B, 4).astype(np.int64)
        got_cnt = d_cnt.cpu().numpy() - 1000
        print(f"move_pick case o={o} c={c}: applied {cnt[0]} cut_visits {cnt[1]} cut_value {cnt[2]} changed {cnt[3]}; "
              f"device {got_cnt.tolist()}; picks differing {int((got_idx != want_idx).sum())}")
        if o == 0.0 and c == 0.0:
            assert not results and cnt.sum() == 0              # off: nothing launched
        assert np.array_equal(got_idx, want_idx), (o, c, np.nonzero(got_idx != want_idx)[0])
        assert np.array_equal(got_code, want_code), (o, c)
        assert np.array_equal(got_cnt, cnt), (o, c, got_cnt, cnt)
        assert _guards_intact(w_idx, torch.int32) and _guards_intact(w_code, torch.int32) and _guards_intact(w_cnt, torch.int64)
        for t, was in zip((e.policy_dense, e.child_visits, e.child_prior, e.root_value, e.terminal_mask, e.chosen_valid,
                           e.child_count, e.child_action), others):
            assert torch.equal(t.view(torch.uint8), was.view(torch.uint8))
        # untouched games: terminal roots, the idle slot, force_uniform games, T = 1e-7
        for g in range(B):
            if g not in results:
                assert got_idx[g] == fin_idx[g] and np.array_equal(got_code[g], fin_code[g])
        for k, v in zip(("applied", "cut_visits", "cut_value", "changed"), cnt):
            seen[k] += int(v)
        # without sample_moves nothing is launched either
        d_idx.copy_(e.chosen_index); d_cnt.fill_(1000)
        assert lib.lz_tree_move_pick(C.byref(e.desc), L.ptr(temps), L.ptr(force), L.ptr(uniforms), 0, C.c_double(o),
                                     C.c_double(c), L.ptr(d_idx), L.ptr(d_code), L.ptr(d_cnt), stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(d_idx, e.chosen_index) and d_cnt.cpu().tolist() == [1000] * 4
    print("move_pick coverage:", seen)
    assert all(v > 0 for v in seen.values()), seen
    # arguments the entry refuses
    for o, c in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (0.0, -0.5), (0.0, 2.5), (0.0, float("nan"))):
        assert lib.lz_tree_move_pick(C.byref(e.desc), L.ptr(temps), L.ptr(force), L.ptr(uniforms), 1, C.c_double(o),
                                     C.c_double(c), L.ptr(d_idx), L.ptr(d_code), L.ptr(d_cnt), stream) == -1
    assert lib.lz_tree_move_pick(C.byref(e.desc), L.ptr(temps), L.ptr(force), None, 1, C.c_double(1.0), C.c_double(0.0),
                                 L.ptr(d_idx), L.ptr(d_code), L.ptr(d_cnt), stream) == -1
    # counters are optional
    assert lib.lz_tree_move_pick(C.byref(e.desc), L.ptr(temps), L.ptr(force), L.ptr(uniforms), 1, C.c_double(1.0),
                                 C.c_double(0.5), L.ptr(d_idx), L.ptr(d_code), None, stream) == 0
    torch.cuda.synchronize()


# ---- 2. the production path -------------------------------------------------------------------------------------------------------
def _replay(engines, bounds, u_np, temps_np, o, c, chosen):
    """The checker over the logged root statistics of every part: the played move of every game, and the first three
    counters the device must report (the fourth needs the finish's own pick, which the re-pick has overwritten)."""
    cnt = np.zeros(3, np.int64)
    for e, (a, b) in zip(engines, bounds):
        term = e.terminal_mask.cpu().numpy().astype(bool)
        edges = root_edges(e)
        nodes = e.buf["nodes"].view(e.B, e.node_cap, 6)[:, 0].contiguous().cpu().numpy().view(NODE_DT).reshape(e.B)
        for i in range(e.B):
            g = a + i
            if term[i]:
                assert chosen[g] == -1
                continue
            E = edges[i]
            N = (E["n_info"] & 0xFFFFFF).astype(np.int64)
            white = ((E["n_info"] >> 24) & INFO_WHITE).astype(bool)
            player = -1 if (int(nodes[i]["state"][0]) >> 53) & 1 else 1
            r = chk.pick(N, chk.child_q(E["W"], N, white, player), temps_np[g], u_np[g], o, c)
            assert chk.margin_ok(r), g
            assert chosen[g] == int(E["act"][r["pick"]]), (g, chosen[g], int(E["act"][r["pick"]]))
            cnt += [1, r["cut_visits"], r["cut_value"]]
    return cnt


@pytest.mark.gpu
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_production_path_picks_equal_the_checker(dual, graph):
    _need_gpu()
    from liuzhou_amd.tree_engine import DualStreamTreeMCTS, PortableTreeMCTS
    B, S, o, c = 64, 64, 2.0, 0.25
    idx = _by_count([(1, 1, 4), (2, 6, 12), (7, 20, 24), (21, 36, 24)])
    idx = idx[np.random.default_rng(5).permutation(B)]
    batch, _ = _positions(idx)
    cls = DualStreamTreeMCTS if dual else PortableTreeMCTS
    m = cls(_net(), B, S, DEV, add_dirichlet_noise=True, seed=SEED, use_graph=graph, move_visit_offset=o, move_value_cutoff=c)
    parts = m.parts if dual else [m]
    bounds = m.bounds if dual else [(0, B)]
    u_np = np.random.default_rng(77).uniform(0.001, 0.999, B).astype(np.float32)
    temps_np = np.asarray([(1.0, 0.5, 2.0)[g % 3] for g in range(B)], dtype=np.float32)
    for p, (a, b) in zip(parts, bounds):
        p.injected_uniforms = torch.from_numpy(u_np[a:b]).to(DEV)
    out = m.search_batch(batch, temperatures=torch.from_numpy(temps_np).to(DEV))
    torch.cuda.synchronize()
    chosen = out.chosen_action_indices.cpu().numpy()
    cnt = _replay([p.engine for p in parts], bounds, u_np, temps_np, o, c, chosen)
    got = m.move_pick_counts.cpu().numpy()
    print(f"production dual={dual} graph={graph}: checker {cnt.tolist()} device {got.tolist()}")
    assert np.array_equal(got[:3], cnt) and 0 <= got[3] <= got[0] and cnt[0] > 0 and cnt[1] > 0


@pytest.mark.gpu
def test_the_solver_keeps_the_last_word():
    """The forced-win positions of the solver tests, 4 copies each, solver on and re-pick on: wherever the root has a child
    proven won for the mover, the played move is such a child."""
    _need_gpu()
    from oracle import lz_oracle as O
    from tests import solver_tree as ST
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    cur = [cs for cs in ST.solver_positions()["win"] for _ in range(4)]
    B = len(cur)
    m = PortableTreeMCTS(_net(), B, 200, DEV, add_dirichlet_noise=True, seed=777, use_graph=False, solver=True,
                         move_visit_offset=1.0, move_value_cutoff=0.5)
    out = m.search_batch(to_gpu_batch(O.batch_from_states(cur), DEV), temperatures=torch.ones(B, device=DEV))
    torch.cuda.synchronize()
    e = m.engine
    chosen = out.chosen_action_indices.cpu().numpy()
    term = e.terminal_mask.cpu().numpy().astype(bool)
    nodes = e.buf["nodes"].view(B, e.node_cap, 6)[:, 0].contiguous().cpu().numpy().view(NODE_DT).reshape(B)
    wins = 0
    for g, E in enumerate(root_edges(e)):
        if term[g] or not len(E):
            continue
        info = (E["n_info"] >> 24).astype(np.int64)
        player = -1 if (int(nodes[g]["state"][0]) >> 53) & 1 else 1
        d = ((info >> 2) & 3) - 1
        x = np.where(np.where(info & 1, -1, 1) == player, d, -d)
        won = ((info & (2 | 16)) != 0) & (x > 0)
        if won.any():
            wins += 1
            assert chosen[g] in set(E["act"][won].tolist()), g
    print("solver + re-pick: roots with a proven win", wins, "of", B, "re-pick counters", m.move_pick_counts.tolist())
    assert wins >= B // 2 and int(m.move_pick_counts[0]) == B


# ---- 3. self-play -------------------------------------------------------------------------------------------------------------------
G = 16


def _selfplay(net, **kw):
    from liuzhou_amd.tree_engine import self_play_tree_gpu, clear_engine_cache
    args = dict(num_games=G, mcts_simulations=64, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                exploration_weight=1.0, device=str(DEV), concurrent_games=G, max_game_plies=32, seed=SEED)
    args.update(kw)
    out = self_play_tree_gpu(net, **args)
    clear_engine_cache()
    return out


FIELDS_B = ("state_tensors", "legal_masks", "policy_targets", "value_targets", "soft_value_targets")


def _raw(t):
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _batch_equal(a, b):
    for f in FIELDS_B:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and torch.equal(_raw(x), _raw(y)), f


def _ply0_equal(a, b):
    """The rows of ply 0 (the first G rows: every game is live and records its row) -- value targets apart, which are
    written when the game ends and follow its path."""
    for f in ("state_tensors", "legal_masks", "policy_targets"):
        assert torch.equal(_raw(getattr(a, f)[:G]), _raw(getattr(b, f)[:G])), f


DROP = ("setup_ms", "build_ms", "final_sync_ms", "loop_ms", "host_wait_ms", "engine_cache_hit")


@pytest.mark.gpu
@pytest.mark.parametrize("device_tail", [True, False])
def test_self_play_off_is_unchanged_and_on_changes_only_the_paths(device_tail):
    _need_gpu()
    net = _net()
    ba, sa = _selfplay(net, device_tail=device_tail)
    bb, sb = _selfplay(net, device_tail=device_tail, move_visit_offset=0.0, move_value_cutoff=0.0, temperature_halflife=0.0)
    _batch_equal(ba, bb)
    assert {k: v for k, v in sa.mcts_counters.items() if k not in DROP} == \
           {k: v for k, v in sb.mcts_counters.items() if k not in DROP}
    assert not any(k.startswith("move_pick") for k in sb.mcts_counters)
    # o = 10^6: the most visited child on every sampled ply.  Ply 0 searches the same trees as the off run and as a run
    # that plays the argmax (sample_moves=False); wherever a ply-0 root has one most visited child, the positions of ply 1
    # equal the argmax run's.
    bo, so = _selfplay(net, device_tail=device_tail, move_visit_offset=1e6)
    bm, _ = _selfplay(net, device_tail=device_tail, sample_moves=False)
    _ply0_equal(bo, ba)
    _ply0_equal(bm, ba)
    pol = ba.policy_targets[:G]
    unique = (pol == pol.max(1, keepdim=True).values).sum(1) == 1
    assert int(unique.sum()) >= 4
    assert torch.equal(bo.state_tensors[G:2 * G][unique], bm.state_tensors[G:2 * G][unique])
    assert not torch.equal(bo.state_tensors[G:2 * G], ba.state_tensors[G:2 * G])      # the off run samples at T = 1
    c = so.mcts_counters
    assert c["move_pick_applied"] > 0 and c["move_pick_cut_value"] == 0 and c["move_pick_cut_visits"] > 0
    assert 0 < c["move_pick_changed"] <= c["move_pick_applied"]
    # a moderate setting: ply-0 rows as in the off run, later paths differ
    bc, sc = _selfplay(net, device_tail=device_tail, move_visit_offset=2.0, move_value_cutoff=0.25)
    _ply0_equal(bc, ba)
    assert bc.num_samples == sc.num_positions > 0 and sc.black_wins + sc.white_wins + sc.draws == sc.num_games
    assert sc.mcts_counters["move_pick_changed"] > 0
    assert any(not torch.equal(_raw(getattr(bc, f)[:min(bc.num_samples, ba.num_samples)]),
                               _raw(getattr(ba, f)[:min(bc.num_samples, ba.num_samples)])) for f in FIELDS_B) \
        or bc.num_samples != ba.num_samples


@pytest.mark.gpu
@pytest.mark.parametrize("device_tail", [True, False])
def test_self_play_composes_with_cap_forced_playouts_and_td(device_tail):
    _need_gpu()
    net = _net()
    kw = dict(device_tail=device_tail, playout_cap_fast_simulations=8, playout_cap_full_prob=0.5, forced_playouts_k=2.0,
              **({"value_target_lambda": 0.8} if device_tail else {}))
    boff, soff = _selfplay(net, **kw)
    bon, son = _selfplay(net, move_visit_offset=2.0, move_value_cutoff=0.25, **kw)
    for f in ("state_tensors", "legal_masks", "policy_targets"):
        # the full / fast draw is keyed by game and ply: the first recorded row is the same ply-0 search in both runs
        assert torch.equal(_raw(getattr(boff, f)[:1]), _raw(getattr(bon, f)[:1])), f
    c = son.mcts_counters
    assert c["move_pick_applied"] > 0 and c["move_pick_changed"] > 0 and c["forced_playouts"] > 0 and c["fast_searches"] > 0
    assert not any(k.startswith("move_pick") for k in soff.mcts_counters)
    pol = bon.policy_targets
    assert bon.num_samples == son.num_positions > 0
    assert torch.allclose(pol.sum(1), torch.ones(pol.shape[0], device=pol.device), atol=1e-4)
    assert not (pol * (~bon.legal_masks).to(pol.dtype)).any()
    assert torch.isfinite(bon.value_targets).all()


@pytest.mark.gpu
@pytest.mark.parametrize("device_tail", [True, False])
def test_half_life_temperatures_equal_the_table(device_tail, monkeypatch):
    _need_gpu()
    from liuzhou_amd import tree_engine as TE
    from liuzhou_amd.move_pick import temperature_table
    seen = []
    orig = TE.PortableTreeMCTS.search_batch

    def spy(self, state, *, temperatures, rng_plies=None, **kw):
        seen.append((temperatures.clone(), rng_plies.clone()))
        return orig(self, state, temperatures=temperatures, rng_plies=rng_plies, **kw)
    monkeypatch.setattr(TE.PortableTreeMCTS, "search_batch", spy)
    _selfplay(_net(), device_tail=device_tail, temperature_halflife=3.0, temperature_threshold=8, max_game_plies=20)
    table = torch.from_numpy(temperature_table(1.0, 0.1, 8, 3.0, 20)).to(DEV)
    assert len(seen) >= 8
    plies_seen = set()
    for temps, plies in seen:
        assert temps.dtype == torch.float32
        assert torch.equal(temps, table[plies.clamp(0, 20)])
        plies_seen |= set(plies.cpu().tolist())
    assert {0, 3, 7, 8}.issubset(plies_seen)
    seen.clear()
    _selfplay(_net(), device_tail=device_tail, temperature_threshold=8, max_game_plies=20)
    for temps, plies in seen:
        assert torch.equal(temps, torch.where(plies < 8, 1.0, 0.1).to(torch.float32))


# ---- 4. worker and refusals ---------------------------------------------------------------------------------------------------------
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
                         move_visit_offset=2.0, move_value_cutoff=0.25, temperature_halflife=4.0)
    clear_engine_cache()
    man = torch.load(out, weights_only=False)
    settings = {"visit_offset": 2.0, "value_cutoff": 0.25, "temperature_halflife": 4.0}
    assert man["metadata"]["move_pick"] == settings
    c = man["stats"]["mcts_counters"]
    assert c["move_pick_applied"] > 0 and c["move_pick_cut_visits"] > 0 and 0 < c["move_pick_changed"] <= c["move_pick_applied"]
    merged = merge_worker_manifests([str(out)], output_path=str(tmp_path / "sp.pt"))
    assert merged["metadata"]["move_pick"] == {**settings, **{k: int(c[k]) for k in (
        "move_pick_applied", "move_pick_cut_visits", "move_pick_cut_value", "move_pick_changed")}}
    samples, _, meta = load_self_play_payload(str(tmp_path / "sp.pt"))
    assert meta["move_pick"] == merged["metadata"]["move_pick"]
    assert samples.value_targets.shape[0] == man["num_samples"] > 0


@pytest.mark.gpu
def test_refusals():
    _need_gpu()
    from liuzhou_amd.tree_engine import DualStreamTreeMCTS, PortableTreeMCTS
    net = _net()
    for on in (dict(move_visit_offset=1.0), dict(move_value_cutoff=0.5)):
        with pytest.raises(ValueError, match="Gumbel"):
            PortableTreeMCTS(net, 16, 16, DEV, gumbel_considered=8, **on)
        with pytest.raises(ValueError, match="Gumbel"):
            _selfplay(net, gumbel_considered=8, **on)
        with pytest.raises(ValueError, match="sample_moves"):
            PortableTreeMCTS(net, 16, 16, DEV, sample_moves=False, **on)
        with pytest.raises(ValueError, match="sample_moves"):
            DualStreamTreeMCTS(net, 16, 16, DEV, sample_moves=False, **on)
        with pytest.raises(ValueError, match="sample_moves"):
            _selfplay(net, sample_moves=False, **on)
    for bad in (dict(move_visit_offset=-1.0), dict(move_value_cutoff=2.5), dict(move_visit_offset=float("nan")),
                dict(move_visit_offset=True)):
        with pytest.raises(ValueError, match="move_v"):
            PortableTreeMCTS(net, 16, 16, DEV, **bad)
        with pytest.raises(ValueError, match="move_v"):
            _selfplay(net, **bad)
    with pytest.raises(ValueError, match="temperature_halflife"):
        _selfplay(net, temperature_halflife=-1.0)
