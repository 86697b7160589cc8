"""Resignation with play-through calibration in the tree backend's self-play (lz_wave_resign, lz_wave_resign_book,
WaveTail(resign_threshold), self_play_tree_gpu(resign_threshold)) against the sequential rule of tests/resign_rule.py.

Every comparison is on integers and bytes.  The one exception is the TD(lambda = 0.5) case: the target kernel evaluates its
recurrence as a chunked scan in double and rounds once to float32, so it is compared with the tolerance its own tests use
and document (tests/test_gpu_td_targets.py: 1e-6)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.resign_rule import resign_rule
from tests.resign_wave import CONFIGS, GAME_BASE, KSEED, MIN_MOVES, THR, ScriptedWave, plays_through

DEV = torch.device("cuda:0")
F = np.float32
FIELDS = ("state_tensors", "legal_masks", "policy_targets", "value_targets", "soft_value_targets")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ---- (a) the two kernels on hand-built slots, through the C ABI --------------------------------------------------------
def _guard(n, dtype, fill, cols=None):
    full = torch.full((n + 2,) if cols is None else (n + 2, cols), fill, dtype=dtype, device=DEV)
    return full, full[1:n + 1]


FILL = {"streak": 7, "would": 1, "would_ply": 99, "term_out": 9, "was_live": 9, "resigned": 9}     # garbage: ply 0 clears it


@pytest.mark.gpu
@pytest.mark.parametrize("consecutive,streak,fraction", CONFIGS)
def test_kernels_on_hand_built_slots(consecutive, streak, fraction):
    """tests/resign_wave.py plays ~70 scripted slots for 12 plies on the host (rule: tests/resign_rule.py, play-through set:
    host Philox); the kernels get each ply's inputs and must leave exactly the expected state, outputs and counters."""
    _need_gpu()
    from liuzhou_amd import _lib as L
    from liuzhou_amd.mcts_gpu import GpuStateBatch
    lib, st = L.lib(), L.stream_ptr(DEV)
    wave = ScriptedWave(consecutive, streak, fraction)
    G = wave.G
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    full, view = {}, {}
    for k, dt in (("streak", torch.int32), ("would", torch.int32), ("would_ply", torch.int32), ("term_out", torch.uint8),
                  ("was_live", torch.uint8), ("resigned", torch.uint8)):
        full[k], view[k] = _guard(G, dt, FILL[k], cols=2 if k == "streak" else None)
    c_full, counters = _guard(8, torch.int64, -5)
    counters.zero_()
    states = GpuStateBatch.initial(DEV, G)
    prev = {k: v.cpu().numpy().copy() for k, v in full.items()}
    for t, ply in enumerate(wave.plies()):
        done, plies, slot_game = d(ply["done"]), d(ply["plies"]), d(ply["slot_game"])
        states.phase.copy_(d(ply["phase"]))
        states.current_player.copy_(d(ply["player"]))
        rv, term = d(ply["root_value"]), d(ply["terminal"])
        L.check(lib.lz_wave_resign(
            L.ptr(done), L.i64(G), L.ptr(plies), L.ptr(states.phase), L.ptr(states.current_player), L.ptr(rv), L.ptr(term),
            L.ptr(slot_game), L.i64(GAME_BASE), C.c_uint64(KSEED), C.c_float(THR), L.i64(MIN_MOVES), C.c_int32(consecutive),
            C.c_float(fraction), C.c_int(1 if streak == "ply" else 0), L.ptr(view["streak"]), L.ptr(view["would"]),
            L.ptr(view["would_ply"]), L.ptr(view["term_out"]), L.ptr(view["was_live"]), L.ptr(view["resigned"]), st),
            "wave_resign")
        got = {k: v.cpu().numpy().copy() for k, v in full.items()}
        for k in got:                                                   # guards
            assert (got[k][0] == FILL[k]).all() and (got[k][-1] == FILL[k]).all(), (t, k)
        for g, want in enumerate(ply["expected"]):
            i = g + 1
            if want is None:                                            # finished: was_live = 0, everything else untouched
                assert got["was_live"][i] == 0, (t, g)
                for k in ("streak", "would", "would_ply", "term_out", "resigned"):
                    assert (got[k][i] == prev[k][i]).all(), (t, g, k)
                continue
            resigned, term_out, wd, wp = want
            assert got["was_live"][i] == 1, (t, g)
            assert (got["resigned"][i], got["term_out"][i]) == (resigned, term_out), (t, g)
            assert (got["would"][i], got["would_ply"][i]) == (wd, wp), (t, g)
        prev = got
        states.board.copy_(d(ply["board_after"]))
        states.phase.copy_(d(ply["phase_after"]))
        done_after, plies_after, cvalid = d(ply["done_after"]), d(ply["plies_after"]), d(ply["cvalid"])
        L.check(lib.lz_wave_resign_book(
            C.byref(L.soa(states.tensors())), L.i64(G), L.ptr(done_after), L.ptr(view["was_live"]),
            L.ptr(plies_after), L.ptr(view["term_out"]), L.ptr(cvalid), L.ptr(view["resigned"]),
            L.ptr(view["would"]), L.ptr(view["would_ply"]), L.ptr(slot_game), L.i64(GAME_BASE), C.c_uint64(KSEED),
            C.c_float(fraction), L.ptr(counters), st), "wave_resign_book")
        assert c_full.cpu().tolist() == [-5] + ply["tally"] + [-5], t
        for k, v in full.items():                                       # the book kernel writes the counters only
            assert np.array_equal(v.cpu().numpy(), got[k]), (t, k)
    wave.check_coverage()


@pytest.mark.gpu
def test_entry_points_refuse_bad_arguments():
    _need_gpu()
    from liuzhou_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr(DEV)
    n = 4
    z = lambda dt: torch.zeros((n,), dtype=dt, device=DEV)
    done, plies, phase, player, rv, term = z(torch.uint8), z(torch.int64), z(torch.int64), z(torch.int64), z(torch.float32), z(torch.uint8)
    streak, would, wp = torch.zeros((n, 2), dtype=torch.int32, device=DEV), z(torch.int32), z(torch.int32)
    to, wl, rs = z(torch.uint8), z(torch.uint8), z(torch.uint8)

    def call(thr=-0.5, mm=0, cons=1, frac=0.5, streak_p=streak):
        return lib.lz_wave_resign(L.ptr(done), L.i64(n), L.ptr(plies), L.ptr(phase), L.ptr(player), L.ptr(rv), L.ptr(term),
                                  None, L.i64(0), C.c_uint64(1), C.c_float(thr), L.i64(mm), C.c_int32(cons), C.c_float(frac),
                                  C.c_int(0), L.ptr(streak_p), L.ptr(would), L.ptr(wp), L.ptr(to), L.ptr(wl), L.ptr(rs), st)
    assert call() == 0
    for kw in (dict(thr=0.0), dict(thr=0.5), dict(thr=-1.5), dict(thr=float("nan")), dict(mm=-1), dict(cons=0),
               dict(frac=-0.1), dict(frac=1.5), dict(frac=float("nan")), dict(streak_p=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()


# ---- (b), (c) self-play -------------------------------------------------------------------------------------------------
SEED = 7
# The threshold: the root values of the untrained 6x64 net lie within +-0.005 (measured over 64 games x 144 plies x 16
# simulations: min -0.0041, and 3 to 13 of 64 movers at or below -0.001 on a movement ply), so -0.01 never resigns and the
# threshold is raised toward 0 until the net does resign; the play-through share stays 0.25.
RESIGN = dict(resign_threshold=-0.001, resign_min_moves=0, resign_consecutive=1, resign_playthrough_fraction=0.25)
COUNTERS = ("resigned_games", "resigned_black", "resigned_white", "playthrough_games", "playthrough_would_resign",
            "playthrough_false_positive", "resign_avg_ply", "resign_plies_saved_estimate")


def _net():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    torch.manual_seed(20260314)
    return FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))


def _selfplay(net, **kw):
    from liuzhou_amd.tree_engine import self_play_tree_gpu, clear_engine_cache
    args = dict(num_games=64, mcts_simulations=16, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                exploration_weight=1.0, device=str(DEV), concurrent_games=64, max_game_plies=72, seed=SEED)
    args.update(kw)
    out = self_play_tree_gpu(net, **args)
    clear_engine_cache()
    return out


def _bytes_equal(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def _stats_key(st):
    return (st.num_games, st.num_positions, st.black_wins, st.white_wins, st.draws, st.avg_game_length,
            dict(st.piece_delta_buckets))


def _logged_selfplay(net, monkeypatch, cap=False, **kw):
    """Self-play with every search of the runner logged: per slot (root value, mover, live, game id, ply, phase, terminal
    root, records a row)."""
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    log = []
    orig = PortableTreeMCTS.search_batch

    def wrapped(self, states, *a, **k):
        if "rng_game_ids" not in k:                                     # not a ply of the runner
            return orig(self, states, *a, **k)
        player, phase, live = states.current_player.clone(), states.phase.clone(), k["active"].clone()
        game, ply = k["rng_game_ids"].clone(), k["rng_plies"].clone()
        out = orig(self, states, *a, **k)
        rec = self.full_search.clone().bool() if cap else torch.ones_like(live)
        log.append((out.root_value.clone(), player, live, game, ply, phase, out.terminal_mask.clone(), rec))
        return out
    with monkeypatch.context() as m:
        m.setattr(PortableTreeMCTS, "search_batch", wrapped)
        batch, stats = _selfplay(net, **kw)
    return batch, stats, [tuple(x.cpu().numpy() for x in e) for e in log]


def _games_of(log):
    """game id -> its searched plies in order [(mover, phase, value, terminal)], and game id -> [(ply, arena row)] of the
    rows it recorded (arena order: ply after ply, ascending slots -- lz_wave_record)."""
    plies, rows = {}, {}
    r = 0
    for rv, player, live, game, ply, phase, term, rec in log:
        for s in np.nonzero(live)[0]:
            g = plies.setdefault(int(game[s]), [])
            assert int(ply[s]) == len(g)                                # every search of the game, from ply 0
            g.append((int(player[s]), int(phase[s]), F(rv[s]), bool(term[s])))
            if rec[s]:
                rows.setdefault(int(game[s]), []).append((int(ply[s]), r))
                r += 1
    return plies, rows, r


def _predict(plies, kw, seed=SEED):
    """What the rule says about every game of a run: (resign ply or None, would, would_ply, plays through)."""
    ids = sorted(plies)
    pt = plays_through(seed, ids, kw["resign_playthrough_fraction"])
    return {g: (*resign_rule(plies[g], kw["resign_threshold"], kw["resign_min_moves"], kw["resign_consecutive"],
                             kw.get("resign_streak", "side"), playthrough=bool(p)), bool(p)) for g, p in zip(ids, pt)}


def _check_counters(stats, plies, pred):
    """mcts_counters against the prediction over the games as they were played (`plies`: the on run's log)."""
    c = stats.mcts_counters
    res = {g: p for g, p in pred.items() if p[0] is not None}
    for g, (r, _, _, _) in res.items():                                 # the predicted ply is the ply the game ended at
        assert len(plies[g]) == r + 1, g
    assert c["resigned_games"] == len(res)
    assert c["resigned_black"] == sum(1 for g, p in res.items() if plies[g][p[0]][0] >= 0)
    assert c["resigned_white"] == len(res) - c["resigned_black"]
    assert c["playthrough_games"] == sum(1 for p in pred.values() if p[3])
    assert c["playthrough_would_resign"] == sum(1 for p in pred.values() if p[3] and p[1] != 0)
    assert c["resign_ply_sum"] == sum(p[0] for p in res.values())
    assert 0 <= c["playthrough_false_positive"] <= c["playthrough_would_resign"]
    assert all(k in c for k in COUNTERS)
    return res


@pytest.mark.gpu
def test_off_is_the_call_without_the_kwargs(monkeypatch):
    _need_gpu()
    from liuzhou_amd import wave_tail
    tails = []
    init = wave_tail.WaveTail.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        tails.append(self)
    monkeypatch.setattr(wave_tail.WaveTail, "__init__", spy)
    net = _net()
    kw = dict(num_games=16, concurrent_games=8, max_game_plies=48)
    ba, sa = _selfplay(net, **kw)
    bb, sb = _selfplay(net, resign_threshold=0.0, resign_min_moves=0, resign_consecutive=1, resign_playthrough_fraction=0.25,
                       resign_streak="ply", **kw)
    for f in FIELDS:
        assert _bytes_equal(getattr(ba, f), getattr(bb, f)), f
    assert _stats_key(sa) == _stats_key(sb) and set(sa.mcts_counters) == set(sb.mcts_counters)
    assert not any(k.startswith(("resign", "playthrough")) for k in sa.mcts_counters)
    assert len(tails) == 2
    for t in tails:
        assert t.resign is None and t.was_live is None
        assert all(getattr(t, k) is None for k in ("streak", "would", "would_ply", "terminal_out", "resigned", "resign_counters"))


@pytest.mark.gpu
def test_on_cuts_games_where_the_rule_says(monkeypatch):
    """64 games of the 6x64 net, one wave: a resigning run is the run without resignation with games cut short."""
    _need_gpu()
    net = _net()
    b0, s0, log0 = _logged_selfplay(net, monkeypatch)
    b1, s1, log1 = _logged_selfplay(net, monkeypatch, **RESIGN)
    plies0, rows0, n0 = _games_of(log0)
    plies1, rows1, n1 = _games_of(log1)
    assert n0 == b0.num_samples and n1 == b1.num_samples and sorted(plies0) == sorted(plies1) == list(range(64))
    pred = _predict(plies0, RESIGN)                                     # from the run that never resigns
    res = _check_counters(s1, plies1, _predict(plies1, RESIGN))
    off = [getattr(b0, f).cpu().numpy() for f in FIELDS]
    on = [getattr(b1, f).cpu().numpy() for f in FIELDS]
    for g in range(64):
        r, wd, wp, pt = pred[g]
        assert len(plies1[g]) == (r + 1 if r is not None else len(plies0[g])), (g, r)
        assert all(a[:2] == b[:2] and a[3] == b[3] and a[2].tobytes() == b[2].tobytes()      # the same searches, bit for bit
                   for a, b in zip(plies1[g], plies0[g])), g
        assert [p for p, _ in rows1[g]] == [p for p, _ in rows0[g]][:len(rows1[g])] and len(rows1[g]) == len(plies1[g])
        for (_, a), (_, b) in zip(rows1[g], rows0[g]):                  # every row is the off run's row
            for k in range(3):                                          # state, mask, policy
                assert on[k][a].tobytes() == off[k][b].tobytes(), (g, FIELDS[k])
        vals = on[3][[a for _, a in rows1[g]]]
        if r is not None:                                               # the resigner lost: sign x (-mover)
            loser = 1 if plies1[g][r][0] >= 0 else -1
            signs = np.array([1.0 if plies1[g][p][0] >= 0 else -1.0 for p, _ in rows1[g]], np.float32)
            assert np.array_equal(vals, signs * F(-loser)), g
            assert vals[-1] == F(-1)                                    # the last row is the resigner's own
        else:
            assert np.array_equal(vals.view(np.uint32), off[3][[b for _, b in rows0[g]]].view(np.uint32)), g
    assert set(res) == {g for g, p in pred.items() if p[0] is not None}
    normal = [g for g in range(64) if not pred[g][3]]
    share = len(res) / len(normal)
    print(f"resign: {len(res)} of {len(normal)} games that may resign did ({share:.2f}); play-through "
          f"{64 - len(normal)}, would resign {s1.mcts_counters['playthrough_would_resign']}, false positives "
          f"{s1.mcts_counters['playthrough_false_positive']}; rows {n1} of {n0}")
    assert 0 < len(normal) < 64
    assert share >= 0.25                                                # not vacuous: the random net does resign
    assert s1.num_positions == n1 < n0
    assert s1.black_wins + s1.white_wins + s1.draws == 64


@pytest.mark.gpu
def test_re_seated_slots(monkeypatch):
    _need_gpu()
    kw = dict(RESIGN, resign_streak="side")
    b, st, log = _logged_selfplay(_net(), monkeypatch, num_games=24, concurrent_games=8, **kw)
    plies, rows, n = _games_of(log)
    assert sorted(plies) == list(range(24)) and n == b.num_samples
    res = _check_counters(st, plies, _predict(plies, kw))
    assert any(g >= 8 for g in res) and len(res) >= 4                   # games seated later resign too


@pytest.mark.gpu
def test_ply_streak_mode(monkeypatch):
    _need_gpu()
    kw = dict(RESIGN, resign_threshold=-0.0002, resign_consecutive=2, resign_streak="ply", resign_playthrough_fraction=0.0)
    b, st, log = _logged_selfplay(_net(), monkeypatch, num_games=16, concurrent_games=16, **kw)
    plies, rows, n = _games_of(log)
    res = _check_counters(st, plies, _predict(plies, kw))
    print(f"resign, ply streak of 2: {len(res)} of 16 games resigned")
    assert st.mcts_counters["playthrough_games"] == 0


@pytest.mark.gpu
def test_playout_cap_and_td_targets(monkeypatch):
    """The cap (a game's resignation ply may record no row) with TD(0.5): the targets are the checker's over the shortened
    games, z = the resignation's result."""
    _need_gpu()
    from tests.td_targets import td_lambda_targets
    net = _net()
    kw = dict(RESIGN, num_games=16, concurrent_games=16, playout_cap_fast_simulations=4, playout_cap_full_prob=0.5)
    ba, sa, loga = _logged_selfplay(net, monkeypatch, cap=True, **kw)
    bb, sb, logb = _logged_selfplay(net, monkeypatch, cap=True, value_target_lambda=0.5, **kw)
    plies, rows, n = _games_of(logb)
    assert _games_of(loga)[1] == rows and n == bb.num_samples == ba.num_samples
    for f in ("state_tensors", "legal_masks", "policy_targets", "soft_value_targets"):
        assert _bytes_equal(getattr(ba, f), getattr(bb, f)), f
    res = _check_counters(sb, plies, _predict(plies, kw))
    assert {k: sa.mcts_counters[k] for k in COUNTERS} == {k: sb.mcts_counters[k] for k in COUNTERS}
    assert len(res) >= 4 and sb.mcts_counters["fast_searches"] > 0
    za, got = ba.value_targets.cpu().numpy(), bb.value_targets.cpu().numpy()
    worst = 0.0
    for g, rws in rows.items():
        sign = lambda p: 1.0 if plies[g][p][0] >= 0 else -1.0
        z = sign(rws[0][0]) * float(za[rws[0][1]])
        if g in res:
            assert z == (-1.0 if plies[g][res[g][0]][0] >= 0 else 1.0)
        q = [float(F(sign(p)) * plies[g][p][2]) for p in range(len(plies[g]))]
        y = td_lambda_targets(q, z, 0.5).astype(np.float32)
        for p, row in rws:
            worst = max(worst, abs(float(got[row]) - float(F(sign(p)) * y[p])))
    print(f"resign + cap + TD(0.5): worst |value - checker| = {worst:.3e}")
    assert worst <= 1e-6
    assert sb.avg_game_length == pytest.approx(np.mean([len(plies[g]) for g in range(16)]))


@pytest.mark.gpu
def test_streamed_rows_are_the_runners_rows():
    _need_gpu()
    from liuzhou_amd.finished_log import FinishedRowLog
    net = _net()
    kw = dict(RESIGN, num_games=24, concurrent_games=8)
    b, st = _selfplay(net, **kw)
    got = {f: [] for f in FIELDS}

    def take(seg):
        seg.ready.synchronize()
        n = int(seg.arena.counters[0].item())
        a = seg.arena
        for f, t in zip(FIELDS, (a.state, a.legal, a.policy, a.value, a.soft)):
            got[f].append(t[:n].clone())
        seg.release()
    log = FinishedRowLog(DEV, segment_games=2, num_slots=8, max_steps=72, on_segment=take)
    _, sl = _selfplay(net, row_log=log, **kw)
    assert log.segments_cut >= 2
    assert _stats_key(sl)[:5] == _stats_key(st)[:5]
    assert {k: sl.mcts_counters[k] for k in COUNTERS} == {k: st.mcts_counters[k] for k in COUNTERS}
    assert st.mcts_counters["resigned_games"] >= 4
    cat = {f: torch.cat(v) for f, v in got.items()}
    assert cat["value_targets"].shape[0] == b.num_samples

    def rows(dct):
        a = [dct[f].contiguous().cpu().numpy() for f in FIELDS]
        return sorted(b"".join(x[i].tobytes() for x in a) for i in range(a[0].shape[0]))
    assert rows(cat) == rows({f: getattr(b, f) for f in FIELDS})


@pytest.mark.gpu
def test_two_streams_give_the_games_of_one_engine():
    _need_gpu()
    net = _net()
    b1, s1 = _selfplay(net, dual_stream=False, **RESIGN)
    b2, s2 = _selfplay(net, dual_stream=True, **RESIGN)
    assert s2.mcts_counters["search_parts"] == 2 and s1.mcts_counters["search_parts"] == 1
    for f in FIELDS:
        assert _bytes_equal(getattr(b1, f), getattr(b2, f)), f
    assert _stats_key(s1) == _stats_key(s2)
    assert {k: s1.mcts_counters[k] for k in COUNTERS} == {k: s2.mcts_counters[k] for k in COUNTERS}
    assert s1.mcts_counters["resigned_games"] >= 12


@pytest.mark.gpu
def test_worker_run_reports_the_feature(tmp_path):
    _need_gpu()
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.resign import COUNTER_KEYS, DERIVED_KEYS
    from liuzhou_amd.self_play_stage import load_self_play_payload, merge_worker_manifests
    from liuzhou_amd.self_play_worker import run_self_play_worker
    from liuzhou_amd.tree_engine import clear_engine_cache
    torch.manual_seed(20260314)                                         # the net of the other tests: it does resign
    mod = ChessNet(**MODEL_CONFIGS["b6c64"])
    ck = tmp_path / "model_state_cpu.pt"
    torch.save(mod.state_dict(), ck)
    out = tmp_path / "w.pt"
    run_self_play_worker(worker_idx=0, shard_device="cuda:0", shard_games=16, seed=5, model_state_path=str(ck),
                         output_path=str(out), mcts_simulations=16, temperature_init=1.0, temperature_final=0.1,
                         temperature_threshold=10, exploration_weight=1.0, dirichlet_alpha=0.3, dirichlet_epsilon=0.25,
                         soft_value_k=2.0, opening_random_moves=2, max_game_plies=72, concurrent_games_per_device=8,
                         chunk_output_dir=str(tmp_path), chunk_file_prefix="w", search_backend="tree", **RESIGN)
    clear_engine_cache()
    man = torch.load(out, weights_only=False)
    settings = {"threshold": -0.001, "min_moves": 0, "consecutive": 1, "playthrough_fraction": 0.25, "streak": "side"}
    assert man["metadata"]["resign"] == settings
    c = man["stats"]["mcts_counters"]
    assert all(k in c for k in COUNTER_KEYS + DERIVED_KEYS)
    assert c["resigned_games"] == c["resigned_black"] + c["resigned_white"] > 0
    assert c["resigned_games"] + c["playthrough_games"] <= 16
    merged = merge_worker_manifests([str(out)], output_path=str(tmp_path / "sp.pt"))
    assert merged["metadata"]["resign"] == {**settings, **{k: int(c[k]) for k in COUNTER_KEYS + DERIVED_KEYS}}
    samples, _, meta = load_self_play_payload(str(tmp_path / "sp.pt"))
    assert meta["resign"] == merged["metadata"]["resign"]
    v = samples.value_targets.float()
    assert v.shape[0] == man["num_samples"] < 16 * 72 and bool(torch.isfinite(v).all())
