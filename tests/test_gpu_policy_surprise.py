"""Policy surprise weighting of the tree backend's self-play (lz_wave_note_surprise, lz_wave_surprise_resample,
WaveTail(policy_surprise_weight), self_play_tree_gpu(policy_surprise_weight)) against the numpy restatement of
tests/policy_surprise.py.

Tolerance of a surprise: |s - numpy float64| <= 1e-6 max(1, s).  The kernel sums its terms in double in another order
than numpy (~1e-16 relative) and rounds once to float32 (<= 6e-8 relative).  The source map src is compared exactly; a game
is left out only where one of its C_j + u lies within 1e-9 of an integer, where the kernel's scan and the sequential sum
may round to different sides -- the synthetic games are seeded so that this never happens."""
import numpy as np
import pytest
import torch

from tests import policy_surprise as PS

DEV = torch.device("cuda:0")
SEED = 7
FIELDS = ("state_tensors", "legal_masks", "policy_targets", "value_targets", "soft_value_targets")
T = 220


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _net():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    torch.manual_seed(20260314)
    return FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tol(want):
    return 1e-6 * max(1.0, float(want))


# ---- 1. lz_wave_note_surprise through the C ABI ------------------------------------------------------------------------
@pytest.mark.gpu
def test_note_kernel_on_a_scripted_wave():
    _need_gpu()
    from liuzhou_amd import _lib as L
    G, TMAX, SENT = 70, 16, -7.5
    rng = np.random.default_rng(20261019)
    done = np.array([g % 7 == 3 for g in range(G)])
    unrec = np.array([g % 5 == 1 for g in range(G)]) & ~done
    over = np.array([g % 11 == 5 for g in range(G)]) & ~done & ~unrec       # a step outside the history
    assert done.sum() > 3 and unrec.sum() > 3 and over.sum() > 2
    legal = np.zeros((G, T), np.uint8)
    pi = np.zeros((G, T), np.float32)
    prior = np.zeros((G, T), np.float32)
    for g in range(G):
        k = (1, 2, 64, 65, 220)[g % 5]
        idx = rng.permutation(T)[:k]
        legal[g, idx] = 1
        t = rng.random(k)
        if k > 1:
            t[rng.random(k) < 0.3] = 0.0                                   # zeros on legal actions
        if t.sum() == 0:
            t[0] = 1.0
        pi[g, idx] = (t / t.sum()).astype(np.float32)
        q = rng.random(k) + 1e-3
        q = q / q.sum()
        if g % 4 == 0:
            q[0] = 0.0                                                      # the clamp: a zero prior ...
            pi[g, idx[0]] = max(pi[g, idx[0]], np.float32(0.125))           # ... under a positive target
        if g % 8 == 2:
            q[:] = 1e-38                                                    # below the clamp everywhere
        prior[g, idx] = q.astype(np.float32)
        # what illegal actions hold must not matter
        off = np.setdiff1d(np.arange(T), idx)
        pi[g, off] = rng.random(len(off)).astype(np.float32) * (g % 2)
        prior[g, off] = rng.random(len(off)).astype(np.float32)
    counts = rng.integers(1, TMAX + 1, G).astype(np.int64)
    counts[over] = np.where(np.arange(G)[over] % 2 == 0, 0, TMAX + 1)
    rows = np.where(done | unrec, -1, np.arange(G) + 100).astype(np.int64)
    full = torch.full((G + 2, TMAX), SENT, dtype=torch.float32, device=DEV)
    w_full = torch.full((G + 2,), 9, dtype=torch.uint8, device=DEV)
    overflow = torch.zeros((1,), dtype=torch.int32, device=DEV)
    dv = [_d(x) for x in (done.astype(np.uint8), rows, counts, legal, pi, prior)]       # kept alive across the launch
    L.check(L.lib().lz_wave_note_surprise(L.ptr(dv[0]), L.i64(G), L.ptr(dv[1]), L.ptr(dv[2]), L.ptr(dv[3]), L.ptr(dv[4]),
                                          L.ptr(dv[5]), L.i64(T), L.ptr(full[1:]), L.ptr(w_full[1:]), L.i64(TMAX),
                                          L.ptr(overflow), L.stream_ptr(DEV)), "wave_note_surprise")
    torch.cuda.synchronize()
    got = full.cpu().numpy()
    assert int(overflow.item()) == int(over.sum())
    assert w_full.cpu().tolist() == [9] + (~done).astype(int).tolist() + [9]
    written = np.zeros((G + 2, TMAX), bool)
    worst = 0.0
    for g in range(G):
        if done[g] or unrec[g] or over[g]:
            continue
        want = PS.surprise(legal[g], pi[g], prior[g])
        s = float(got[g + 1, counts[g] - 1])
        written[g + 1, counts[g] - 1] = True
        worst = max(worst, abs(s - want) / max(1.0, want))
        assert abs(s - want) <= _tol(want), (g, s, want)
        assert s >= 0.0
    assert (got[~written] == np.float32(SENT)).all()                       # guards, unrecorded, finished, overflowing slots
    assert got[written].max() > 60.0                                       # the clamp was exercised: -log 1e-30 = 69
    print(f"note_surprise: worst relative error = {worst:.3e}")


# ---- 2. lz_wave_surprise_resample through the C ABI --------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 128, 129, 200)
TMAX = 512
RUN_SEED = 0xC0FFEE1234
GAME_BASE = 1000


class _Wave:
    """39 slots: 0..31 the 8 lengths x 4 surprise patterns, 32 a 512-row game, 33..35 still live, 36..38 finished on an
    earlier ply (was_live = 0); every arena field of every row holds a value of its own."""

    def __init__(self, addressing):
        rng = np.random.default_rng(20261019)
        self.G = G = 39
        self.n = np.array([LENGTHS[g % 8] for g in range(32)] + [512] + [40, 1, 200] + [64, 3, 130], np.int64)
        self.pat = [PS.PATTERNS[g // 8] for g in range(32)] + ["gamma"] * 7
        self.ends = np.arange(G) < 33
        self.done = np.array([1] * 33 + [0] * 3 + [1] * 3, np.uint8)
        self.was_live = np.array([1] * 36 + [0] * 3, np.uint8)
        self.slot_game = rng.permutation(G).astype(np.int64) + 5
        self.hist = np.full((G, TMAX), 5.0, np.float32)                    # beyond a game's rows: never read
        for g in range(G):
            self.hist[g, :self.n[g]] = PS.pattern(self.pat[g], int(self.n[g]), rng)
        self.steps = TMAX
        if addressing == "matrix":
            self.cap = int(self.n.sum()) + 64
            perm = np.random.default_rng(5).permutation(self.cap)
            self.row_of = np.full((G, TMAX), -1, np.int64)
            k = 0
            for g in range(G):
                self.row_of[g, :self.n[g]] = perm[k:k + self.n[g]]
                k += self.n[g]
        else:
            self.cap = G * TMAX
            self.row_of = np.arange(G * TMAX, dtype=np.int64).reshape(G, TMAX)
        self.matrix = addressing == "matrix"
        r = np.arange(self.cap + 2, dtype=np.int64)                        # one guard row on either side
        self.arena = [
            (r[:, None] * 396 + np.arange(396)[None, :]).astype(np.float32),
            ((r[:, None] * 7 + np.arange(T)[None, :] * 13) % 251).astype(np.uint8),
            (-(r[:, None] * T + np.arange(T)[None, :]) - 0.5).astype(np.float32),
            (r + 0.125).astype(np.float32), (-r - 0.375).astype(np.float32), ((r % 127) - 63).astype(np.int8)]

    def u(self, g):
        return PS.game_u(RUN_SEED, int(self.slot_game[g]) + GAME_BASE)


@pytest.mark.gpu
@pytest.mark.parametrize("addressing", ["matrix", "slot_major"])
def test_resample_kernel_on_synthetic_games(addressing):
    _need_gpu()
    import ctypes as C
    from liuzhou_amd import _lib as L
    w = _Wave(addressing)
    G = w.G
    lib, st = L.lib(), L.stream_ptr(DEV)
    done, hist, counts = _d(w.done), _d(w.hist), _d(w.n)
    slot_game = _d(w.slot_game)
    step_index = _d(w.row_of) if w.matrix else None
    left_out = moved_rows = 0
    for alpha in PS.ALPHAS:
        arena = [_d(a) for a in w.arena]
        views = [a[1:] for a in arena]                                     # row 0 of the kernel = row 1 of the guarded tensor
        src_full = torch.full((G + 2, TMAX), -9, dtype=torch.int32, device=DEV)
        counters = torch.zeros((3,), dtype=torch.int64, device=DEV)
        total = torch.zeros((1,), dtype=torch.float64, device=DEV)
        was_live = _d(w.was_live)

        def launch():
            L.check(lib.lz_wave_surprise_resample(
                L.ptr(done), L.ptr(was_live), L.i64(G), C.c_double(alpha), L.ptr(hist), L.ptr(slot_game), L.i64(GAME_BASE),
                C.c_uint64(RUN_SEED), *(L.ptr(v) for v in views), L.i64(T), L.ptr(step_index), L.ptr(counts),
                L.i64(TMAX), L.ptr(src_full[1:]), L.ptr(counters), L.ptr(total), st), "wave_surprise_resample")
        launch()
        torch.cuda.synchronize()
        got = [a.cpu().numpy() for a in arena]
        src = src_full.cpu().numpy()
        want = [a.copy() for a in w.arena]
        want_src = np.full((G + 2, TMAX), -9, np.int32)
        c_games = c_rows = c_dropped = 0
        c_sum = 0.0
        skip = set()
        for g in np.nonzero(w.ends)[0]:
            n, s, u = int(w.n[g]), w.hist[g, :w.n[g]], w.u(g)
            c_games, c_rows, c_sum = c_games + 1, c_rows + n, c_sum + float(s.astype(np.float64).sum())
            if PS.near_integer(s, alpha, u):
                skip.add(int(g))
                continue
            plan = PS.plan(s, alpha, u)
            want_src[g + 1, :n] = plan
            c_dropped += PS.rows_dropped(plan)
            rows = w.row_of[g, :n] + 1
            for f, a in zip(want, w.arena):
                f[rows] = a[rows[plan]]
            moved_rows += int((plan != np.arange(n)).sum())
        left_out += len(skip)
        assert len(skip) == 0                                              # the seeds were picked so
        for g in range(G):
            assert np.array_equal(src[g + 1], want_src[g + 1]), (alpha, g, w.pat[g], int(w.n[g]))
        assert (src[0] == -9).all() and (src[G + 1] == -9).all()
        for name, a, b in zip(("state", "legal", "policy", "value", "soft", "sign"), got, want):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (alpha, name)    # every row of the arena, guards too
        assert counters.cpu().tolist() == [c_games, c_rows, c_dropped]
        assert abs(float(total.item()) - c_sum) <= 1e-9 * max(1.0, c_sum)
        assert np.array_equal(counts.cpu().numpy(), w.n)
        # a second launch with was_live cleared changes nothing
        was_live.zero_()
        launch()
        torch.cuda.synchronize()
        for a, b in zip(arena, got):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8))
        assert np.array_equal(src_full.cpu().numpy(), src) and counters.cpu().tolist() == [c_games, c_rows, c_dropped]
    assert moved_rows > 100
    print(f"surprise_resample, {addressing}: {moved_rows} rows moved, {left_out} games left out")


@pytest.mark.gpu
def test_resample_refuses_bad_arguments():
    _need_gpu()
    import ctypes as C
    from liuzhou_amd import _lib as L
    z = torch.zeros((64,), dtype=torch.float64, device=DEV)
    p = L.ptr(z)
    call = lambda alpha, t: L.lib().lz_wave_surprise_resample(
        p, p, L.i64(1), C.c_double(alpha), p, None, L.i64(0), C.c_uint64(1), p, p, p, p, p, p, L.i64(t), None, p,
        L.i64(4), p, p, p, L.stream_ptr(DEV))
    assert call(1.5, T) == -1 and call(float("nan"), T) == -1              # LZ_ERR_ARG
    assert call(0.5, 222) == -2 and call(0.5, 260) == -2                   # LZ_ERR_UNSUPPORTED


# ---- 3. end to end -------------------------------------------------------------------------------------------------------
def _selfplay(net, **kw):
    from liuzhou_amd.tree_engine import self_play_tree_gpu, clear_engine_cache
    args = dict(num_games=16, mcts_simulations=16, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                exploration_weight=1.0, device=str(DEV), concurrent_games=8, max_game_plies=48, seed=SEED)
    args.update(kw)
    out = self_play_tree_gpu(net, **args)
    clear_engine_cache()
    return out


def _bytes_equal(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def _stats_key(st):
    return (st.num_games, st.num_positions, st.black_wins, st.white_wins, st.draws, st.avg_game_length,
            dict(st.piece_delta_buckets))


@pytest.mark.gpu
def test_off_is_the_call_without_the_kwarg(monkeypatch):
    _need_gpu()
    from liuzhou_amd import wave_tail
    tails = []
    init = wave_tail.WaveTail.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        tails.append(self)
    monkeypatch.setattr(wave_tail.WaveTail, "__init__", spy)
    net = _net()
    ba, sa = _selfplay(net)
    bb, sb = _selfplay(net, policy_surprise_weight=0.0)
    for f in FIELDS:
        assert _bytes_equal(getattr(ba, f), getattr(bb, f)), f
    assert _stats_key(sa) == _stats_key(sb) and set(sa.mcts_counters) == set(sb.mcts_counters)
    assert not any(k.startswith("surprise") for k in sa.mcts_counters)
    assert len(tails) == 2
    for t in tails:
        assert t.surprise_alpha is None and t.surprise_hist is None and t.surprise_src is None
        assert t.surprise_counters is None and t.surprise_sum is None and t.prior_fn is None and t.was_live is None


@pytest.mark.gpu
def test_tail_without_a_prior_fn_refuses_to_run():
    _need_gpu()
    from liuzhou_amd.trajectory_buffer import TensorTrajectoryBuffer
    from liuzhou_amd.wave_tail import WaveTail
    buf = TensorTrajectoryBuffer(DEV, T, max_steps_hint=8, concurrent_games_hint=4)
    tail = WaveTail(buf, 4, 8, DEV, policy_surprise_weight=ALPHA)
    assert tail.prior_fn is None and tail.surprise_hist is not None
    with pytest.raises(RuntimeError, match="prior_fn"):
        tail.run(None, None, None, None, torch.zeros((4, 8), dtype=torch.int64, device=DEV), None, None, 1.0, 0.1, 10)
    fn = lambda search: None
    assert WaveTail(buf, 4, 8, DEV, policy_surprise_weight=ALPHA, prior_fn=fn).prior_fn is fn
    assert WaveTail(buf, 4, 8, DEV, prior_fn=fn).prior_fn is None                   # off: nothing of the feature is kept


def _logged_selfplay(net, monkeypatch, cap, **kw):
    """Self-play with every search logged -- (live, game id, ply, records a row, current player, model input, policy target,
    root value) -- and, when the feature is on, every call of WaveTail.note_surprise: the slots that recorded, their game
    and step, the kernel's surprise and what it was computed from."""
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    from liuzhou_amd.wave_tail import WaveTail
    log, notes = [], []
    orig = PortableTreeMCTS.search_batch
    note = WaveTail.note_surprise

    def wrapped(self, states, *a, **k):
        if "rng_game_ids" not in k:                                     # not a ply of the runner
            return orig(self, states, *a, **k)
        player, live = states.current_player.clone(), k["active"].clone()
        game, ply = k["rng_game_ids"].clone(), k["rng_plies"].clone()
        out = orig(self, states, *a, **k)
        rec = self.full_search.clone().bool() if cap else torch.ones_like(live)
        log.append((live, game, ply, rec, player, out.model_input.clone(), out.policy_dense.clone(), out.root_value.clone()))
        return out

    def noted(self, done, step_counts, search, prior):
        note(self, done, step_counts, search, prior)
        rec = (self.rows >= 0) & ~done.bool()
        step = (step_counts - 1).clamp(min=0)
        s = self.surprise_hist[torch.arange(self.G, device=step.device), step]
        notes.append(tuple(x.clone().cpu().numpy() for x in (
            rec, self.slot_game + self.game_base, step, s, search.legal_mask, search.policy_dense, search.model_input)))
    with monkeypatch.context() as m:
        m.setattr(PortableTreeMCTS, "search_batch", wrapped)
        m.setattr(WaveTail, "note_surprise", noted)
        batch, stats = _selfplay(net, **kw)
    return batch, stats, [tuple(x.cpu().numpy() for x in e) for e in log], notes


def _rows_of_games(log, off_batch):
    """game -> the rows of its steps in the batch: the arena order is ply after ply, ascending slots (lz_wave_record)."""
    off_state = off_batch.state_tensors.cpu().numpy()
    rows = {}
    r = 0
    for live, game, ply, rec, player, mi, pol, rv in log:
        for s in np.nonzero(live & rec)[0]:
            assert np.array_equal(off_state[r].reshape(-1), mi[s].reshape(-1)), "rows are not in arena order"
            rows.setdefault(int(game[s]), []).append(r)
            r += 1
    assert r == off_state.shape[0]
    return rows


FORMS = {"default": dict(), "one_wave": dict(num_games=8), "reseated_slots": dict(num_games=24),
         "playout_cap": dict(playout_cap_fast_simulations=4, playout_cap_full_prob=0.5),
         "gumbel": dict(gumbel_considered=4), "td_lambda": dict(value_target_lambda=0.8),
         "sequential_waves": dict(continuous_waves=False), "eval_symmetry": dict(eval_symmetry="random"),
         "resign_solver_forced": dict(resign_threshold=-0.001, resign_min_moves=4, resign_consecutive=1, mcts_solver=True,
                                      forced_playouts_k=2.0)}
ALPHA = 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_on_resamples_each_games_rows_and_nothing_else(monkeypatch, form):
    _need_gpu()
    from liuzhou_amd import v0_core
    from liuzhou_amd.mcts_gpu import AUXILIARY_DIM, MOVEMENT_DIM, PLACEMENT_DIM, SELECTION_DIM
    net = _net()
    kw = FORMS[form]
    cap = "playout_cap_fast_simulations" in kw
    b0, s0, log0, notes0 = _logged_selfplay(net, monkeypatch, cap, **kw)
    b1, s1, log1, notes1 = _logged_selfplay(net, monkeypatch, cap, policy_surprise_weight=ALPHA, **kw)
    games = kw.get("num_games", 16)
    # the games are the same games: stats, every search's inputs and outputs
    assert _stats_key(s0) == _stats_key(s1)
    assert len(log0) == len(log1) and all(np.array_equal(a, b) for x, y in zip(log0, log1) for a, b in zip(x, y))
    assert notes0 == [] and len(notes1) == len(log1)
    assert set(s1.mcts_counters) - set(s0.mcts_counters) == {"surprise_games", "surprise_rows", "surprise_rows_replaced",
                                                             "surprise_sum_micro", "surprise_mean"}
    # the note kernel's surprises against numpy, the prior computed here
    surprises = {}                                                      # game -> [s of step 0, 1, ...]
    worst, total = 0.0, 0.0
    for (live, game, ply, rec_l, player, mi_l, pol_l, rv), (rec, gid, step, s, legal, pi, mi) in zip(log1, notes1):
        assert np.array_equal(rec, live & rec_l) and np.array_equal(gid[live], game[live])
        if not rec.any():
            continue
        lp1, lp2, lpm, _ = net(_d(mi))
        prior, _ = v0_core.project_policy_logits_fast(lp1.float(), lp2.float(), lpm.float(), _d(legal).bool(), PLACEMENT_DIM,
                                                      MOVEMENT_DIM, SELECTION_DIM, AUXILIARY_DIM)
        prior = prior.cpu().numpy()
        for g in np.nonzero(rec)[0]:
            want = PS.surprise(legal[g], pi[g], prior[g])
            worst = max(worst, abs(float(s[g]) - want) / max(1.0, want))
            assert abs(float(s[g]) - want) <= _tol(want), (form, int(gid[g]), int(step[g]), float(s[g]), want)
            lst = surprises.setdefault(int(gid[g]), [])
            assert int(step[g]) == len(lst)
            lst.append(np.float32(s[g]))
            total += float(s[g])
    # every game's rows of the on-run = the off-run's rows of that game gathered by the oracle's src
    rows = _rows_of_games(log0, b0)
    assert set(rows) == set(surprises) and sum(len(v) for v in rows.values()) == b0.num_samples == b1.num_samples
    off = [getattr(b0, f).contiguous().cpu().numpy() for f in FIELDS]
    on = [getattr(b1, f).contiguous().cpu().numpy() for f in FIELDS]
    left_out, replaced, moved = [], 0, 0
    for game, rws in rows.items():
        s = np.asarray(surprises[game], np.float32)
        assert len(s) == len(rws)
        u = PS.game_u(SEED, game)
        if PS.near_integer(s, ALPHA, u):
            left_out.append(game)
            continue
        src = PS.plan(s, ALPHA, u)
        replaced += PS.rows_dropped(src)
        r = np.asarray(rws)
        for f, a, b in zip(FIELDS, off, on):
            assert np.array_equal(b[r].view(np.uint8), a[r[src]].view(np.uint8)), (form, game, f)
        moved += int((src != np.arange(len(src))).sum())
    assert len(left_out) <= 1
    assert any(not np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(off, on))     # a row did change
    c = s1.mcts_counters
    assert c["surprise_games"] == len(rows) <= games and c["surprise_rows"] == b1.num_samples
    if not left_out:
        assert c["surprise_rows_replaced"] == replaced
    assert 0 < c["surprise_rows_replaced"] <= c["surprise_rows"]
    assert abs(c["surprise_sum_micro"] - total * 1e6) <= 2.0 + 1e-6 * total * 1e6
    if cap:
        assert s1.mcts_counters["fast_searches"] > 0
    if form == "reseated_slots":
        assert max(rows) == 23
    print(f"policy surprise, {form}: {b1.num_samples} rows, {replaced} replaced, {moved} moved, worst relative error of a "
          f"surprise {worst:.3e}, mean surprise {total / max(1, b1.num_samples):.4f}, left out {left_out}")


@pytest.mark.gpu
def test_streamed_rows_are_the_batch_runs_rows():
    """The same games through a finished-row log: the rows leave the ply their game ends, resampled."""
    _need_gpu()
    from liuzhou_amd.finished_log import FinishedRowLog
    net = _net()
    kw = dict(num_games=8, policy_surprise_weight=ALPHA)
    b, st = _selfplay(net, **kw)
    got = {f: [] for f in FIELDS}

    def take(seg):
        seg.ready.synchronize()
        n = int(seg.arena.counters[0].item())
        a = seg.arena
        for f, t in zip(FIELDS, (a.state, a.legal, a.policy, a.value, a.soft)):
            got[f].append(t[:n].clone())
        seg.release()
    log = FinishedRowLog(DEV, segment_games=2, num_slots=8, max_steps=48, on_segment=take)
    _, sl = _selfplay(net, row_log=log, **kw)
    assert log.segments_cut >= 2                                        # at least one arena switch
    assert _stats_key(sl)[:5] == _stats_key(st)[:5]
    assert all(sl.mcts_counters[k] == st.mcts_counters[k] for k in ("surprise_games", "surprise_rows", "surprise_rows_replaced"))
    assert st.mcts_counters["surprise_rows_replaced"] > 0
    cat = {f: torch.cat(v) for f, v in got.items()}
    assert cat["value_targets"].shape[0] == b.num_samples

    def rows(d):
        a = [d[f].contiguous().cpu().numpy() for f in FIELDS]
        return sorted(b"".join(x[i].tobytes() for x in a) for i in range(a[0].shape[0]))
    assert rows(cat) == rows({f: getattr(b, f) for f in FIELDS})        # the same multiset, bit for bit


@pytest.mark.gpu
def test_two_streams_give_the_rows_of_one_engine():
    _need_gpu()
    net = _net()
    kw = dict(num_games=64, concurrent_games=64, policy_surprise_weight=ALPHA)
    b1, s1 = _selfplay(net, dual_stream=False, **kw)
    b2, s2 = _selfplay(net, dual_stream=True, **kw)
    assert s2.mcts_counters["search_parts"] == 2 and s1.mcts_counters["search_parts"] == 1
    for f in FIELDS:
        assert _bytes_equal(getattr(b1, f), getattr(b2, f)), f
    assert _stats_key(s1) == _stats_key(s2)
    for k in ("surprise_games", "surprise_rows", "surprise_rows_replaced"):
        assert s1.mcts_counters[k] == s2.mcts_counters[k]
    assert s1.mcts_counters["surprise_games"] == 64 and s1.mcts_counters["surprise_rows_replaced"] > 0


@pytest.mark.gpu
def test_module_evaluator_feeds_the_kernel_its_own_prior(monkeypatch):
    """evaluator="module": the root prior comes from the module itself.  The prior the tail was handed is a distribution over
    the legal actions, and the recorded surprise is numpy's of that prior (the bound of test 1)."""
    _need_gpu()
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.wave_tail import WaveTail
    torch.manual_seed(20260314)
    mod = ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV)
    note, seen = WaveTail.note_surprise, []

    def noted(self, done, step_counts, search, prior):
        note(self, done, step_counts, search, prior)
        rec = (self.rows >= 0) & ~done.bool()
        step = (step_counts - 1).clamp(min=0)
        s = self.surprise_hist[torch.arange(self.G, device=step.device), step]
        seen.append(tuple(x.clone().cpu().numpy() for x in (rec, s, search.legal_mask, search.policy_dense, prior)))
    monkeypatch.setattr(WaveTail, "note_surprise", noted)
    b, st = _selfplay(mod, num_games=8, evaluator="module", policy_surprise_weight=ALPHA)
    c = st.mcts_counters
    assert c["surprise_games"] == 8 and c["surprise_rows"] == b.num_samples > 0
    assert 0 < c["surprise_rows_replaced"] <= c["surprise_rows"] and c["surprise_mean"] > 0
    assert seen and sum(int(e[0].sum()) for e in seen) == b.num_samples
    for rec, s, legal, pi, prior in seen:
        for g in np.nonzero(rec)[0]:
            lg = legal[g].astype(bool)
            assert abs(float(prior[g][lg].sum()) - 1.0) < 1e-5 and (prior[g][~lg] == 0).all()
            want = PS.surprise(lg, pi[g], prior[g])
            assert abs(float(s[g]) - want) <= _tol(want)


# ---- 4. a worker run -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_worker_run_reports_the_feature(tmp_path):
    _need_gpu()
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS, stable_resnet_init
    from liuzhou_amd.self_play_stage import load_self_play_payload, merge_worker_manifests
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
                         policy_surprise_weight=ALPHA)
    clear_engine_cache()
    man = torch.load(out, weights_only=False)
    ps = man["metadata"]["policy_surprise"]
    assert set(ps) == {"weight", "games", "rows", "rows_replaced", "mean_surprise"}
    assert ps["weight"] == ALPHA and ps["games"] == 16 and ps["rows"] == man["num_samples"] == 16 * 12
    assert 0 <= ps["rows_replaced"] <= ps["rows"] and ps["mean_surprise"] > 0.0
    merged = merge_worker_manifests([str(out)], output_path=str(tmp_path / "sp.pt"))
    assert merged["metadata"]["policy_surprise"] == ps
    samples, _, meta = load_self_play_payload(str(tmp_path / "sp.pt"))
    assert meta["policy_surprise"] == ps and samples.value_targets.shape[0] == man["num_samples"]
