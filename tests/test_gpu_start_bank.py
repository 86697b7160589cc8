"""GPU: the start bank (game forking) -- lz_start_bank_capture and lz_start_bank_seed (csrc/lz_ops.hip) through the C ABI,
WaveTail's two launch points and self_play_tree_gpu(start_fork_prob, start_capture_prob, start_bank), held to the numpy
restatement tests/start_bank_ref.py (which tests/test_start_bank_cpu.py holds to the host build of the same header and
whose fixed-seed coverage it asserts).  Everything is integers and bytes: every comparison is exact, every output buffer
starts as a sentinel and is compared over its whole length."""
import numpy as np
import pytest
import torch

from tests import start_bank_ref as S
from tests.test_start_bank_cpu import check_argument_refusals

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = ("state_tensors", "legal_masks", "policy_targets", "value_targets", "soft_value_targets")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from liuzhou_amd import _lib
    return _lib


# =========================================================================================================================
# the kernels
# =========================================================================================================================
@pytest.mark.parametrize("capacity", [3, 7, 4096])
@pytest.mark.parametrize("G", S.CAPTURE_G)
def test_capture_equals_the_restatement(L, G, capacity):
    """Mixed done / terminal / invalid-pick / out-of-window slots, every slot a candidate (more candidates than rows for
    the small rings), no candidate, and capture_prob = 0, from a total of 0, capacity - 1 and 5 capacity + 2."""
    lib = L.lib()
    for total in S.capture_totals(capacity):
        S.run_capture(L, lib, DEV, S.capture_case(G, "mixed"), capacity, total)
        assert S.run_capture(L, lib, DEV, S.capture_case(G, "all"), capacity, total) == G
        assert S.run_capture(L, lib, DEV, S.capture_case(G, "none"), capacity, total) == 0
        assert S.run_capture(L, lib, DEV, S.capture_case(G, "all"), capacity, total, capture_prob=0.0) == 0
    S.run_capture(L, lib, DEV, S.capture_case(G, "mixed"), capacity, 0, with_slot_game=False)


@pytest.mark.parametrize("G", S.CAPTURE_G)
def test_seed_equals_the_restatement(L, G):
    lib = L.lib()
    c = S.seed_case(G)
    for filled in (0, 1, 7):
        for prob in (0.0, 0.5, 1.0):
            S.run_seed(L, lib, DEV, c, S.seed_bank(7, filled), prob)
    S.run_seed(L, lib, DEV, c, S.seed_bank(7, 7, total=5 * 7 + 2), 0.5)       # a ring that has wrapped
    base = (1 << 35) + 3                                      # a game_base is a shift of slot_game
    a = S.run_seed(L, lib, DEV, c, S.seed_bank(7, 7), 0.5, game_base=base)
    b = S.run_seed(L, lib, DEV, c, S.seed_bank(7, 7), 0.5, slot_game=c["slot_game"] + base)
    assert np.array_equal(a, b) and (a >= 0).any()
    a = S.run_seed(L, lib, DEV, c, S.seed_bank(7, 7), 0.5, game_base=base, slot_game=None)
    b = S.run_seed(L, lib, DEV, c, S.seed_bank(7, 7), 0.5, slot_game=np.arange(G, dtype=np.int64) + base)
    assert np.array_equal(a, b)


def test_argument_refusals_return_without_a_launch(L):
    check_argument_refusals(L, L.lib(), DEV)


def test_scripted_wave_equals_the_restatement_after_every_ply(L):
    """8 slots, a ring of 3 rows, a dozen plies: record -> capture -> step_finish -> reseat -> seed on the device with the
    inputs of the host's scripted wave; states, bank, cursor and counters after every ply."""
    from tests.test_gpu_wave_tail import dev_arena, dv, lz_record, lz_reseat, lz_step_finish
    lib = L.lib()
    w = S.scripted_bank_tail()
    G, Tmax, T = w.G, w.TMAX, w.T
    ts = S.to_device(w.st, DEV)
    d_arena = dev_arena(w.R, T)
    d_plies, d_done, d_counts, d_index, d_rows = dv(w.plies), dv(w.done), dv(w.counts), dv(w.index), dv(w.rows)
    d_outcome, d_hist, d_lengths = dv(w.outcome), dv(w.hist), dv(w.lengths)
    d_game, d_reseated = dv(w.slot_game), dv(w.reseated)
    d_cursor, d_overflow, d_finished = dv(np.array([w.cursor], np.int64)), dv(np.zeros(1, np.int32)), dv(np.zeros(1, np.int64))
    d_budget, d_next = dv(np.array([w.budget], np.int64)), dv(np.array([w.next_game], np.int64))
    entries, cursor, counters = dv(w.bank.entries), dv(np.zeros(1, np.int64)), dv(np.zeros(3, np.int64))
    for ply in range(w.PLIES):
        x = w.inputs()
        d_term, d_cvalid = dv(x["terminal"]), dv(x["cvalid"])
        d_reseated.zero_()
        L.check(lz_record(L, G, d_done, d_cursor, w.capacity, Tmax, d_index, d_counts, d_rows, d_overflow,
                          dv(x["model_input"]), dv(x["legal"]), dv(x["policy"]), ts[4], T, d_arena, None), "wave_record")
        L.check(S.call_capture(L, lib, DEV, ts, d_done, d_term, d_cvalid, d_plies, d_game, w.GAME_BASE, w.RUN_SEED,
                               w.CAPTURE_PROB, w.MIN_MOVE, w.MAX_MOVE, entries, w.CAPACITY, cursor, counters),
                "start_bank_capture")
        L.check(lz_step_finish(L, ts, G, d_plies, d_done, dv(x["codes"]), d_term, d_cvalid, w.MAX_PLIES, w.K, d_arena[3],
                               d_arena[4], d_arena[5], d_index, d_counts, Tmax, d_outcome, d_hist, d_lengths, d_game,
                               d_finished, None, False, None), "wave_step_finish")
        L.check(lz_reseat(L, ts, G, d_done, d_plies, d_counts, d_budget, d_next, d_game, d_reseated, False), "wave_reseat")
        L.check(S.call_seed(L, lib, DEV, ts, d_reseated, d_game, w.GAME_BASE, w.RUN_SEED, w.FORK_PROB, entries, w.CAPACITY,
                            cursor, counters), "start_bank_seed")
        w.capture(x)
        w.advance(x)
        w.seed()
        where = f"ply {ply}: "
        S.assert_states(ts, w.st, where + "states")
        S.assert_bytes(entries, w.bank.entries, where + "entries")
        assert int(cursor.item()) == w.bank.cursor and counters.tolist() == w.bank.counters.tolist(), where
        for name, got, want in (("plies", d_plies, w.plies), ("done", d_done, w.done), ("step_counts", d_counts, w.counts),
                                ("slot_game", d_game, w.slot_game), ("reseated", d_reseated, w.reseated),
                                ("step_index", d_index, w.index), ("lengths", d_lengths, w.lengths)):
            S.assert_bytes(got, want, where + name)
    w.check_bank_coverage()


# =========================================================================================================================
# end to end
# =========================================================================================================================
@pytest.fixture(scope="module")
def net(L):
    from liuzhou_amd.net import ChessNet, MODEL_CONFIGS
    from liuzhou_amd.net_hip import FusedNet
    torch.manual_seed(20260314)
    return FusedNet(ChessNet(**MODEL_CONFIGS["b6c64"]).eval().to(DEV))


def _selfplay(net, **kw):
    from liuzhou_amd.tree_engine import clear_engine_cache, self_play_tree_gpu
    args = dict(num_games=24, mcts_simulations=8, temperature_init=1.0, temperature_final=0.1, temperature_threshold=10,
                exploration_weight=1.0, device=DEV, concurrent_games=8, max_game_plies=12, seed=S.SEED)
    args.update(kw)
    out = self_play_tree_gpu(net, **args)
    clear_engine_cache()
    return out


def _bank(capacity, packed=None):
    from liuzhou_amd.start_bank import StartBank
    bank = StartBank(capacity, DEV)
    if packed is not None:
        bank.append_packed(torch.from_numpy(packed))
    return bank


def _row_multiset(tensors):
    a = [t.contiguous().cpu().numpy() for t in tensors]
    return sorted(b"".join(x[i].tobytes() for x in a) for i in range(a[0].shape[0]))


def test_off_equals_the_call_without_the_options(net, monkeypatch):
    from liuzhou_amd import wave_tail
    tails = []
    init = wave_tail.WaveTail.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        tails.append(self)
    monkeypatch.setattr(wave_tail.WaveTail, "__init__", spy)
    ba, sa = _selfplay(net)
    bb, sb = _selfplay(net, start_fork_prob=0.0, start_capture_prob=0.0, start_bank_capacity=65536, start_min_move=1,
                       start_max_move=143)
    for f in ROWS:
        x, y = getattr(ba, f), getattr(bb, f)
        assert x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), f
    assert set(sa.mcts_counters) == set(sb.mcts_counters) and not any(k.startswith("start_") for k in sa.mcts_counters)
    key = lambda st: (st.num_positions, st.black_wins, st.white_wins, st.draws)
    assert key(sa) == key(sb)
    assert len(tails) == 2 and all(t.bank is None and t.start is None and t.start_counters is None for t in tails)


def test_forked_games_start_from_the_drawn_entries(net):
    """40 one-ply games on 8 slots from a bank of 7 playout positions: every game records exactly its start position."""
    from liuzhou_amd import v0_core
    st7, packed = S.playout_positions()
    bank = _bank(7, packed)
    before = bank.state_dict()
    batch, stats = _selfplay(net, num_games=40, max_game_plies=1, start_fork_prob=0.5, start_capture_prob=0.0,
                             start_bank_capacity=7, start_bank=bank)
    j = S.fork_entries(S.SEED, np.arange(40), 0.5, 7)
    assert int((j >= 0).sum()) == 19
    starts = S.O.initial_states(40)
    forked = S.unpack_states(packed[j[j >= 0]])
    for f in S.FIELDS:
        starts[f][j >= 0] = forked[f].astype(starts[f].dtype)
    t = S.to_device(starts, DEV)
    want = v0_core.states_to_model_input(*t[:5])
    assert batch.num_samples == 40 and stats.num_positions == 40
    assert _row_multiset([batch.state_tensors]) == _row_multiset([want])
    c = stats.mcts_counters
    assert c["start_forked_games"] == 19 and c["start_captured"] == 0
    assert c["start_fork_move_sum"] == int(st7["move_count"][j[j >= 0]].sum())
    after = bank.state_dict()
    assert torch.equal(after["entries"], before["entries"]) and torch.equal(after["cursor"], before["cursor"])


COMBINED = dict(value_target_lambda=0.9, resign_threshold=-0.9, policy_surprise_weight=0.5, playout_cap_fast_simulations=4,
                playout_cap_full_prob=0.5)


@pytest.mark.parametrize("combined", [False, True], ids=["alone", "with_the_other_tail_rules_and_the_log"])
def test_capture_and_fork_together_are_deterministic(net, combined):
    from liuzhou_amd.finished_log import FinishedRowLog
    runs = []
    for _ in range(2):
        bank, got = _bank(64), []
        kw = dict(start_capture_prob=0.25, start_fork_prob=0.5, start_bank_capacity=64, start_bank=bank)
        if combined:
            def take(seg):
                seg.ready.synchronize()
                n, a = int(seg.arena.counters[0].item()), seg.arena
                got.append([t[:n].clone() for t in (a.state, a.legal, a.policy, a.value, a.soft)])
                seg.release()
            kw.update(COMBINED, row_log=FinishedRowLog(DEV, segment_games=2, num_slots=8, max_steps=12, on_segment=take))
        batch, stats = _selfplay(net, **kw)                   # check_overflow runs inside: a dropped row raises
        rows = [torch.cat(x) for x in zip(*got)] if combined else [getattr(batch, f) for f in ROWS]
        assert rows[0].shape[0] == stats.num_positions > 0 and bool(torch.isfinite(rows[3]).all())
        c = stats.mcts_counters
        assert c["start_captured"] == bank.total() > 0 and c["start_forked_games"] > 0
        assert c["start_fork_move_sum"] >= c["start_forked_games"]               # start_min_move = 1: never the empty board
        runs.append((_row_multiset(rows) if combined else [r.contiguous().view(torch.uint8).cpu() for r in rows],
                     bank.state_dict(), {k: v for k, v in c.items() if k.startswith("start_")},
                     (stats.black_wins, stats.white_wins, stats.draws)))
    a, b = runs
    if combined:
        assert a[0] == b[0]
    else:
        assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    assert torch.equal(a[1]["entries"], b[1]["entries"]) and torch.equal(a[1]["cursor"], b[1]["cursor"])
    assert a[2] == b[2] and a[3] == b[3]


@pytest.mark.parametrize("continuous", [True, False], ids=["continuous_waves", "sequential_waves"])
def test_a_bank_carried_into_a_second_call_seeds_its_first_wave(net, continuous):
    bank = _bank(256)
    _, s1 = _selfplay(net, num_games=8, start_capture_prob=1.0, start_bank_capacity=256, start_bank=bank,
                      continuous_waves=continuous)
    assert s1.mcts_counters["start_forked_games"] == 0 and s1.mcts_counters["start_captured"] == bank.total() > 0
    filled = bank.filled()
    entries = bank.state_dict()["entries"].numpy()
    _, s2 = _selfplay(net, num_games=8, start_fork_prob=0.5, start_bank_capacity=256, start_bank=bank,
                      continuous_waves=continuous)
    j = S.fork_entries(S.SEED, np.arange(8), 0.5, filled)    # num_games <= concurrent_games: only the first wave starts games
    assert s2.mcts_counters["start_forked_games"] == int((j >= 0).sum()) == 5
    assert s2.mcts_counters["start_fork_move_sum"] == int(S.unpack_states(entries[j[j >= 0]])["move_count"].sum())
    assert s2.mcts_counters["start_captured"] == 0 and bank.filled() == filled
