"""TD(lambda) value targets of the tree backend's self-play (lz_wave_note_value, lz_wave_td_targets, WaveTail(value_target_lambda),
self_play_tree_gpu(value_target_lambda)) against the float64 sequential recurrence of tests/td_targets.py.

Tolerance of the float comparisons: 1e-6 absolute, the project's bar for float outputs.  The kernel evaluates the recurrence
in double as a chunked suffix scan and rounds every y once to float32; the scan's own deviation from the sequential
float64 recurrence is ~1e-16 relative, so what remains is a float32 rounding that can fall on the other side: at most one
ulp of a value in [-1, 1], 6e-8.  lambda = 0 and lambda = 1 are exact in any evaluation order."""
import numpy as np
import pytest
import torch

from tests.td_targets import td_lambda_targets

DEV = torch.device("cuda:0")
SEED = 7
TOL = 1e-6
LAMBDAS = (0.0, 0.5, 0.9, 1.0)
FIELDS = ("state_tensors", "legal_masks", "policy_targets", "value_targets", "soft_value_targets")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _net():
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    torch.manual_seed(20260314)
    return FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))


# ---- 1. the kernels on synthetic games, through the C ABI ---------------------------------------------------------------
G, TMAX = 70, 200
LENGTHS = (1, 2, 63, 64, 65, 128, 129, 200)
PATTERNS = ("all", "third", "last", "none")
SENT_F, SENT_I = -7.5, -77


class _Games:
    """70 slots played ply by ply by hand: slots 0..63 are the 8 lengths x 4 recording patterns, once with alternating
    players and once with random ones, and end at their length; slots 64..69 are still playing after the last ply."""

    def __init__(self):
        rng = np.random.default_rng(20261017)
        self.length = np.array([LENGTHS[g % 8] if g < 64 else TMAX for g in range(G)])
        self.ends = np.arange(G) < 64
        self.z = np.array([(-1.0, 0.0, 1.0)[g % 3] for g in range(G)], np.float32)
        self.pattern = [PATTERNS[(g // 8) % 4] if g < 64 else PATTERNS[g % 2] for g in range(G)]
        t = np.arange(TMAX)
        alt = np.where(t % 2 == 0, 1, -1)
        self.player = np.stack([alt if (g // 32) % 2 == 0 else rng.choice([-1, 1], TMAX) for g in range(G)], 1).astype(np.int64)
        self.rv = rng.uniform(-1.0, 1.0, (TMAX, G)).astype(np.float32)
        self.live = t[:, None] < self.length[None, :]                                  # [T, G]
        rec = np.zeros((TMAX, G), bool)
        for g in range(G):
            n, p = self.length[g], self.pattern[g]
            if p == "all":
                rec[:n, g] = True
            elif p == "third":
                rec[:n:3, g] = True
            elif p == "last":
                rec[n - 1, g] = True
        self.rec = rec & self.live
        self.counts = np.cumsum(self.rec, 0).astype(np.int64)                          # step_counts after the ply's record
        self.q = (self.player * self.rv).astype(np.float32)                            # exact: a product with +-1

    def steps(self, g):
        return np.nonzero(self.rec[:, g])[0]

    def expected(self, g, lam):
        """float32 sign * y of slot g's recorded steps."""
        n = self.length[g]
        y = td_lambda_targets(self.q[:n, g], self.z[g], lam).astype(np.float32)
        s = self.steps(g)
        return self.player[s, g].astype(np.float32) * y[s]


def _guarded(rows, cols, dtype, fill):
    """A [rows, cols] view with one guard row on either side."""
    full = torch.full((rows + 2, cols), fill, dtype=dtype, device=DEV)
    return full, full[1:rows + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("addressing", ["matrix", "slot_major"])
def test_kernels_on_synthetic_games(addressing):
    _need_gpu()
    import ctypes as C
    from liuzhou_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr(DEV)
    gm = _Games()
    steps = TMAX + 3 if addressing == "matrix" else TMAX                # stride of step_index / of the slot-major arena
    cap = G * steps + 64
    row_of = np.full((G, steps), -1, np.int64)                          # arena row of slot g's step j
    if addressing == "matrix":
        perm = np.random.default_rng(5).permutation(cap)
        k = 0
        for g in range(G):
            n = len(gm.steps(g))
            row_of[g, :n] = perm[k:k + n]
            k += n
    else:
        for g in range(G):
            n = len(gm.steps(g))
            row_of[g, :n] = g * steps + np.arange(n)
    step_index = torch.from_numpy(row_of).to(DEV) if addressing == "matrix" else None
    rows_t = np.full((TMAX, G), -1, np.int64)                           # what lz_wave_record leaves in `rows`
    sign = np.zeros(cap, np.int8)
    for g in range(G):
        for j, t in enumerate(gm.steps(g)):
            rows_t[t, g] = row_of[g, j]
            sign[row_of[g, j]] = gm.player[t, g]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    done_before = d((~gm.live).astype(np.uint8))                        # [T, G] at the start of ply t
    ended = gm.live & (np.arange(TMAX)[:, None] == gm.length[None, :] - 1) & gm.ends[None, :]
    done_after = d((~gm.live | ended).astype(np.uint8))                 # ... and after its lz_wave_step_finish
    plies = d(np.where(gm.live, np.arange(TMAX)[:, None], gm.length[None, :]).astype(np.int64))
    rows, counts, rv, player = d(rows_t), d(gm.counts), d(gm.rv), d(gm.player)
    signs = d(sign)
    q_full, q_hist = _guarded(G, TMAX, torch.float32, SENT_F)
    p_full, step_ply = _guarded(G, TMAX, torch.int32, SENT_I)
    h_full = torch.full((G + 2,), SENT_I, dtype=torch.int32, device=DEV)
    w_full = torch.full((G + 2,), 9, dtype=torch.uint8, device=DEV)
    hist_len, was_live = h_full[1:G + 1], w_full[1:G + 1]
    overflow = torch.zeros((1,), dtype=torch.int32, device=DEV)
    nan = float("nan")
    value = {lam: torch.full((cap + 2,), nan, dtype=torch.float32, device=DEV) for lam in LAMBDAS}     # guards: [0], [-1]
    shadow = torch.full((cap + 2,), nan, dtype=torch.float32, device=DEV)      # the step kernel's writes only
    for t in range(TMAX):
        L.check(lib.lz_wave_note_value(L.ptr(done_before[t]), L.i64(G), L.ptr(plies[t]), L.ptr(rows[t]), L.ptr(counts[t]),
                                       L.ptr(rv[t]), L.ptr(player[t]), L.ptr(q_hist), L.ptr(step_ply), L.ptr(hist_len),
                                       L.ptr(was_live), L.i64(TMAX), L.ptr(overflow), st), "wave_note_value")
        fin = np.nonzero(ended[t])[0]
        if fin.size:                                                    # what lz_wave_step_finish writes: sign * z
            idx = np.concatenate([row_of[g, :len(gm.steps(g))] for g in fin])
            val = np.concatenate([gm.player[gm.steps(g), g].astype(np.float32) * gm.z[g] for g in fin])
            if idx.size:
                for a in (*value.values(), shadow):
                    a[1:cap + 1][d(idx)] = d(val)
        for lam, a in value.items():
            L.check(lib.lz_wave_td_targets(L.ptr(done_after[t]), L.ptr(was_live), L.i64(G), C.c_double(lam), L.ptr(q_hist),
                                           L.ptr(step_ply), L.ptr(hist_len), L.i64(TMAX), L.ptr(a[1:]), L.ptr(signs),
                                           L.ptr(step_index), L.ptr(counts[t]), L.i64(steps), st), "wave_td_targets")
    torch.cuda.synchronize()
    assert int(overflow.item()) == 0
    # the note kernel: every searched ply's Q, the ply of every recorded step, nothing else
    want_q = np.full((G + 2, TMAX), SENT_F, np.float32)
    want_p = np.full((G + 2, TMAX), SENT_I, np.int32)
    for g in range(G):
        want_q[g + 1, :gm.length[g]] = gm.q[:gm.length[g], g]
        s = gm.steps(g)
        want_p[g + 1, :len(s)] = s
    assert np.array_equal(q_full.cpu().numpy().view(np.uint32), want_q.view(np.uint32))
    assert np.array_equal(p_full.cpu().numpy(), want_p)
    assert h_full.cpu().tolist() == [SENT_I] + gm.length.tolist() + [SENT_I]
    assert w_full.cpu().tolist() == [9] + gm.live[TMAX - 1].astype(int).tolist() + [9]      # as of the last ply's start
    # the target kernel: the rows of the games that ended, and no other byte of the arena
    base = shadow.cpu().numpy()
    worst = 0.0
    for lam, a in value.items():
        got = a.cpu().numpy()
        mine = np.zeros(cap + 2, bool)
        for g in np.nonzero(gm.ends)[0]:
            r = row_of[g, :len(gm.steps(g))] + 1
            mine[r] = True
            want = gm.expected(g, lam)
            if lam in (0.0, 1.0):
                assert np.array_equal(got[r], want), (lam, g)
            else:
                err = float(np.abs(got[r].astype(np.float64) - want.astype(np.float64)).max()) if r.size else 0.0
                worst = max(worst, err)
                assert err <= TOL, (lam, g, err)
        assert np.array_equal(got[~mine].view(np.uint32), base[~mine].view(np.uint32)), lam
        assert np.isnan(got[~mine]).all()                               # guards, unused rows, games still playing
    print(f"td targets, {addressing}: worst |kernel - float64 sequential| = {worst:.3e}")


@pytest.mark.gpu
def test_a_ply_past_the_history_raises_the_overflow_counter_and_writes_nothing():
    _need_gpu()
    from liuzhou_amd import _lib as L
    t, n = 8, 70                                                        # a history of 8 plies; slots at ply 7, 8 and 9
    q_full, q_hist = _guarded(n, t, torch.float32, SENT_F)
    p_full, step_ply = _guarded(n, t, torch.int32, SENT_I)
    h_full = torch.full((n + 2,), SENT_I, dtype=torch.int32, device=DEV)
    w_full = torch.full((n + 2,), 9, dtype=torch.uint8, device=DEV)
    ply = np.array([t - 1 + g % 3 for g in range(n)], np.int64)
    done = torch.zeros((n,), dtype=torch.uint8, device=DEV)
    plies = torch.from_numpy(ply).to(DEV)
    rows = torch.arange(n, dtype=torch.int64, device=DEV)
    counts = torch.from_numpy(np.minimum(ply + 1, t)).to(DEV)
    rv = torch.full((n,), 0.25, dtype=torch.float32, device=DEV)
    player = torch.ones((n,), dtype=torch.int64, device=DEV)
    overflow = torch.zeros((1,), dtype=torch.int32, device=DEV)
    L.check(L.lib().lz_wave_note_value(L.ptr(done), L.i64(n), L.ptr(plies), L.ptr(rows), L.ptr(counts), L.ptr(rv),
                                       L.ptr(player), L.ptr(q_hist), L.ptr(step_ply), L.ptr(h_full[1:]), L.ptr(w_full[1:]),
                                       L.i64(t), L.ptr(overflow), L.stream_ptr(DEV)), "wave_note_value")
    torch.cuda.synchronize()
    inside = ply < t
    assert int(overflow.item()) == int((~inside).sum()) > 0
    want_q = np.full((n + 2, t), SENT_F, np.float32)
    want_p = np.full((n + 2, t), SENT_I, np.int32)
    want_q[1:n + 1, t - 1][inside] = 0.25
    want_p[1:n + 1, t - 1][inside] = t - 1
    assert np.array_equal(q_full.cpu().numpy(), want_q) and np.array_equal(p_full.cpu().numpy(), want_p)
    assert h_full.cpu().tolist() == [SENT_I] + [t if i else SENT_I for i in inside] + [SENT_I]
    assert w_full.cpu().tolist() == [9] + [1] * n + [9]


# ---- 2..5. self-play ----------------------------------------------------------------------------------------------------
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
    bb, sb = _selfplay(net, value_target_lambda=1.0)
    for f in FIELDS:
        assert _bytes_equal(getattr(ba, f), getattr(bb, f)), f
    assert _stats_key(sa) == _stats_key(sb) and set(sa.mcts_counters) == set(sb.mcts_counters)
    assert len(tails) == 2
    for t in tails:
        assert t.td_lambda is None and t.q_hist is None and t.step_ply is None and t.hist_len is None and t.was_live is None


def _logged_selfplay(net, monkeypatch, cap, **kw):
    """Self-play with every search logged: (root_value, current_player, live, game id, ply, model input, records a row)."""
    from liuzhou_amd.tree_engine import PortableTreeMCTS
    log = []
    orig = PortableTreeMCTS.search_batch

    def wrapped(self, states, *a, **k):
        if "rng_game_ids" not in k:                                     # not a ply of the runner
            return orig(self, states, *a, **k)
        player, live = states.current_player.clone(), k["active"].clone()
        game, ply = k["rng_game_ids"].clone(), k["rng_plies"].clone()
        out = orig(self, states, *a, **k)
        rec = self.full_search.clone().bool() if cap else torch.ones_like(live)
        log.append((out.root_value.clone(), player, live, game, ply, out.model_input.clone(), rec))
        return out
    with monkeypatch.context() as m:
        m.setattr(PortableTreeMCTS, "search_batch", wrapped)
        batch, stats = _selfplay(net, **kw)
    return batch, stats, [tuple(x.cpu().numpy() for x in e) for e in log]


def _expected_values(log, off_batch, lam):
    """The rows of a run in arena order (ply after ply, ascending slots: lz_wave_record) with the checker's target: z of a
    game comes from the same rows of the run without TD targets (sign * value of the game's first row)."""
    off_value = off_batch.value_targets.cpu().numpy()
    off_state = off_batch.state_tensors.cpu().numpy()
    q, rows = {}, {}                                                    # game -> {ply: Q}, game -> [(ply, row, sign)]
    r = 0
    for rv, player, live, game, ply, mi, rec in log:
        for s in np.nonzero(live)[0]:
            gq = q.setdefault(int(game[s]), {})
            assert int(ply[s]) not in gq
            gq[int(ply[s])] = float(np.float32(player[s]) * rv[s])
            if rec[s]:
                assert np.array_equal(off_state[r].reshape(-1), mi[s].reshape(-1)), "rows are not in arena order"
                rows.setdefault(int(game[s]), []).append((int(ply[s]), r, 1.0 if player[s] >= 0 else -1.0))
                r += 1
    assert r == off_value.shape[0]
    want = np.full(r, np.nan, np.float32)
    for game, rws in rows.items():
        plies = sorted(q[game])
        assert plies == list(range(len(plies)))                         # every search of the game, from ply 0
        z = rws[0][2] * float(off_value[rws[0][1]])
        assert z in (-1.0, 0.0, 1.0)
        y = td_lambda_targets([q[game][p] for p in plies], z, lam).astype(np.float32)
        for p, row, sg in rws:
            assert off_value[row] == np.float32(sg * z)
            want[row] = np.float32(sg) * y[p]
    assert not np.isnan(want).any()
    return want, len(q)


def _row_multiset(state, value):
    """(state bytes, value) pairs in a canonical order: opening positions repeat across games, so rows have no key."""
    s = np.ascontiguousarray(state).reshape(state.shape[0], -1)
    pairs = sorted(((s[i].tobytes(), float(value[i])) for i in range(s.shape[0])))
    return [p[0] for p in pairs], np.array([p[1] for p in pairs], np.float64)


FORMS = {"one_wave": dict(num_games=8), "reseated_slots": dict(num_games=24),
         "playout_cap": dict(playout_cap_fast_simulations=4, playout_cap_full_prob=0.5),
         "gumbel": dict(gumbel_considered=4)}


def _on_against_off(net, monkeypatch, form, lam=0.8):
    kw = FORMS[form]
    cap = "playout_cap_fast_simulations" in kw
    b0, s0, log0 = _logged_selfplay(net, monkeypatch, cap, **kw)
    b1, s1, log1 = _logged_selfplay(net, monkeypatch, cap, value_target_lambda=lam, **kw)
    return kw, cap, (b0, s0, log0), (b1, s1, log1)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_on_changes_only_the_value_column(monkeypatch, form):
    _need_gpu()
    lam = 0.8
    kw, cap, (b0, s0, log0), (b1, s1, log1) = _on_against_off(_net(), monkeypatch, form, lam)
    for f in ("state_tensors", "legal_masks", "policy_targets", "soft_value_targets"):
        assert _bytes_equal(getattr(b0, f), getattr(b1, f)), f
    assert _stats_key(s0) == _stats_key(s1)
    assert len(log0) == len(log1) and all(np.array_equal(a, b) for x, y in zip(log0, log1) for a, b in zip(x, y))
    want, games = _expected_values(log1, b0, lam)
    assert games == kw.get("num_games", 16)
    if cap:
        fast = sum(int((live & ~rec).sum()) for _, _, live, _, _, _, rec in log1)
        assert fast > 0 and fast == s1.mcts_counters["fast_searches"]
    if form == "reseated_slots":
        assert max(int(game[live].max()) for _, _, live, game, _, _, _ in log1 if live.any()) == 23
    got = b1.value_targets.cpu().numpy()
    state = b1.state_tensors.cpu().numpy()
    ks, vs = _row_multiset(state, got)
    kw_, vw = _row_multiset(state, want)
    assert ks == kw_
    err = float(np.abs(vs - vw).max())
    print(f"td targets, {form}: {got.shape[0]} rows, worst |value - checker| = {err:.3e}, "
          f"rows that differ from z: {int((got != b0.value_targets.cpu().numpy()).sum())}")
    assert err <= TOL
    assert float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) <= TOL      # row by row as well
    assert (got != b0.value_targets.cpu().numpy()).any()                # the targets did change
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0


@pytest.mark.gpu
def test_streamed_rows_carry_the_same_targets():
    """The same games through a finished-row log: the rows leave the ply their game ends, with their final targets."""
    _need_gpu()
    from liuzhou_amd.finished_log import FinishedRowLog
    net = _net()
    kw = dict(num_games=8, value_target_lambda=0.8)
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
    cat = {f: torch.cat(v) for f, v in got.items()}
    assert cat["value_targets"].shape[0] == b.num_samples
    def rows(d):
        a = [d[f].contiguous().cpu().numpy() for f in FIELDS]
        return sorted(b"".join(x[i].tobytes() for x in a) for i in range(a[0].shape[0]))
    assert rows(cat) == rows({f: getattr(b, f) for f in FIELDS})        # value_targets bit for bit


@pytest.mark.gpu
def test_two_streams_give_the_targets_of_one_engine():
    _need_gpu()
    net = _net()
    kw = dict(num_games=64, concurrent_games=64, value_target_lambda=0.8)
    b1, s1 = _selfplay(net, dual_stream=False, **kw)
    b2, s2 = _selfplay(net, dual_stream=True, **kw)
    assert s2.mcts_counters["search_parts"] == 2 and s1.mcts_counters["search_parts"] == 1
    for f in FIELDS:
        assert _bytes_equal(getattr(b1, f), getattr(b2, f)), f
    assert _stats_key(s1) == _stats_key(s2)
    v = b1.value_targets
    assert bool(((v != 0) & (v.abs() != 1)).any())                      # blended targets, not results


# ---- 6. a worker run ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_worker_run_reports_the_mode(tmp_path):
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
                         value_target_lambda=0.8)
    clear_engine_cache()
    man = torch.load(out, weights_only=False)
    assert man["metadata"]["value_target"] == {"td_lambda": 0.8}
    assert man["num_samples"] == 16 * 12
    # what the stage does with its workers' manifests, then the loader the trainers use
    merged = merge_worker_manifests([str(out)], output_path=str(tmp_path / "sp.pt"))
    assert merged["metadata"]["value_target"] == {"td_lambda": 0.8}
    samples, _, meta = load_self_play_payload(str(tmp_path / "sp.pt"))
    assert meta["value_target"] == {"td_lambda": 0.8}
    v = samples.value_targets.float()
    assert v.shape[0] == man["num_samples"] and bool(torch.isfinite(v).all()) and float(v.abs().max()) <= 1.0
    assert bool(((v != 0) & (v.abs() != 1)).any())
