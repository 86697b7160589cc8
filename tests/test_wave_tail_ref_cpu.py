"""CPU: tests/wave_tail_ref.py (the sequential restatement of lz_wave_record / lz_wave_step_finish / lz_wave_reseat that
tests/test_gpu_wave_tail.py holds the kernels to) against the reference's golden vectors (g7_ops.npz: the step and the
trajectory fixtures) and against hand-written miniature cases with literal expected arrays."""
import numpy as np

from oracle import lz_oracle as O
from tests.golden_utils import FIELDS, load, states, states_equal
from tests.wave_tail_cases import (RESEAT_G, SENT_F32, STEP_KINDS, ScriptedTail, copy_states, cut_slot, record_case,
                                   reseat_budgets, reseat_case, sentinel_f32, step_case, step_kinds_of_result)
from tests.wave_tail_ref import ref_finalize_book, ref_record, ref_reseat, ref_step_finish

NAN = np.float32(np.nan)


def _arena(rows, T, fill=0.0):
    return (np.full((rows, 396), fill, np.float32), np.full((rows, T), 0x7F, np.uint8), np.full((rows, T), fill, np.float32),
            np.full(rows, 7.0, np.float32), np.full(rows, 7.0, np.float32), np.full(rows, 0x7F, np.int8))


def _sample(G, T, seed):
    r = np.random.default_rng(seed)
    return (r.random((G, 11, 6, 6), dtype=np.float32), r.integers(0, 256, (G, T), dtype=np.uint8),
            r.random((G, T), dtype=np.float32), r.choice(np.array([-1, 1], np.int64), G))


# ---- the golden vectors -------------------------------------------------------------------------------------------------
def test_step_finish_reproduces_the_step_fixture():
    """g7_ops.npz, 64 slots, max_plies 96, k 2.0: the 55 active slots are the live ones (the fixture's other slots are not
    stepped: here they are `done` on entry and must stay exactly as they were).  Every slot holds 1..4 recorded steps in
    scattered rows."""
    z = load("g7_ops.npz")
    G, Tmax = 64, 4
    work = {f: np.array(z[f"s_{f}"]) for f in FIELDS}
    active = z["step_active"]
    idle = np.setdiff1d(np.arange(G), active)
    plies = z["step_plies_in"].copy()
    done = np.ones(G, np.uint8)
    done[active] = 0
    codes = np.full((G, 4), -1, np.int32); codes[active] = z["step_codes"]
    term = np.zeros(G, np.uint8); term[active] = z["step_term"]
    cvalid = np.zeros(G, np.uint8); cvalid[active] = z["step_valid"]
    r = np.random.default_rng(7)
    counts = r.integers(1, Tmax + 1, G)
    step_index = np.full((G, Tmax), -1, np.int64)
    perm = r.permutation(G * Tmax + 40)
    p = 0
    for g in range(G):
        step_index[g, :counts[g]] = perm[p:p + counts[g]]
        p += counts[g]
    signs = r.choice(np.array([-1, 1], np.int8), perm.size)
    value, soft = np.full(perm.size, NAN), np.full(perm.size, NAN)
    outcome, hist, lengths = np.zeros(3, np.int64), np.zeros(37, np.int64), np.full(G, -1, np.int64)
    step_counts = counts.copy()
    finished = ref_step_finish(work, plies, done, codes, term, cvalid, 96, 2.0, value, soft, signs, step_index,
                               step_counts, Tmax, outcome, hist, lengths)
    ok, field = states_equal(work, {f: z[f"step_after_{f}"] for f in FIELDS})
    assert ok, field
    assert np.array_equal(plies, z["step_plies_out"])
    assert np.array_equal(done[active] != 0, z["step_done_out"][active])
    assert not z["step_done_out"][idle].any() and (done[idle] == 1).all()
    want_v, want_s = np.full(perm.size, NAN), np.full(perm.size, NAN)
    for g, res, sft in zip(z["step_slots"], z["step_result"], z["step_soft"]):
        idx = step_index[g, :counts[g]]
        want_v[idx] = signs[idx].astype(np.float32) * res
        want_s[idx] = signs[idx].astype(np.float32) * sft
    assert np.array_equal(value.view(np.int32), want_v.view(np.int32))           # signed zeros and NaN fills included
    assert np.array_equal(np.isnan(soft), np.isnan(want_s))
    np.testing.assert_allclose(soft, want_s, atol=1e-6, rtol=0, equal_nan=True)
    res = z["step_result"]
    assert finished == res.size == 6
    assert outcome.tolist() == [int((res > 0).sum()), int((res < 0).sum()), int((res == 0).sum())]
    want_len = np.full(G, -1, np.int64); want_len[z["step_slots"]] = counts[z["step_slots"]]
    assert np.array_equal(lengths, want_len) and np.array_equal(step_counts, counts)
    b = z["step_after_board"][z["step_slots"]].reshape(6, -1)
    delta = (b == 1).sum(1) - (b == -1).sum(1)
    assert np.array_equal(hist, np.bincount(np.clip(delta + 18, 0, 36), minlength=37))


def test_record_then_finalise_reproduces_the_trajectory_fixture():
    """g7_ops.npz traj_*: 12 slots record their traj_counts steps ply after ply through ref_record (the sign of a step is
    the fixture's sign of that step; the policy carries the fixture's row number), then the fixture's five games are
    finalised.  ref_record numbers the rows ply-major, the fixture at random: the targets must agree row for row through
    that mapping, and the rows ref_record never handed out stay untouched."""
    z = load("g7_ops.npz")
    fix_index, counts, fsigns = z["traj_step_index"], z["traj_counts"], z["traj_signs"]
    G, Tmax = fix_index.shape
    T, total = 5, int(counts.sum())
    arena = _arena(total + 9, T)
    step_index, step_counts = np.full((G, Tmax), -1, np.int64), np.zeros(G, np.int64)
    rows, cursor, overflow = np.zeros(G, np.int64), 0, 0
    mi, lm, _, _ = _sample(G, T, 3)
    for t in range(Tmax):
        done = (counts <= t).astype(np.uint8)
        src = np.where(done == 0, fix_index[:, t], 0)
        pol = np.repeat(src[:, None], T, 1).astype(np.float32)
        cursor, overflow = ref_record(done, cursor, total + 9, Tmax, step_index, step_counts, rows, overflow, mi, lm,
                                      pol, fsigns[src].astype(np.int64), arena)
    assert cursor == total and overflow == 0 and np.array_equal(step_counts, counts)
    assert np.array_equal(step_index >= 0, fix_index >= 0)
    _, _, a_policy, a_value, a_soft, a_sign = arena
    src_row = a_policy[:total, 0].astype(np.int64)                             # arena row -> the fixture's row
    assert np.array_equal(np.sort(src_row), np.sort(fix_index[fix_index >= 0]))
    assert np.array_equal(a_sign[:total], fsigns[src_row])
    assert np.isnan(a_value[:total]).all() and np.isnan(a_soft[:total]).all()
    outcome = np.zeros(3, np.int64)
    done, plies = np.zeros(G, np.uint8), counts.copy()
    fin = ref_finalize_book(O.initial_states(G), z["traj_slots"], z["traj_result"], z["traj_soft"], plies, done, plies,
                            a_value, a_soft, a_sign, step_index, step_counts, Tmax, outcome)
    assert fin == 5 and np.array_equal(outcome, z["traj_counts_out"])
    assert np.array_equal(a_value[:total].view(np.int32), z["traj_value_out"][src_row].view(np.int32))
    np.testing.assert_allclose(a_soft[:total], z["traj_soft_out"][src_row], atol=1e-7, rtol=0, equal_nan=True)
    assert (a_value[total:] == 7.0).all() and (a_soft[total:] == 7.0).all() and (a_sign[total:] == 0x7F).all()
    assert np.array_equal(np.flatnonzero(done), z["traj_slots"])


# ---- miniature cases, expected arrays written out ----------------------------------------------------------------------
def test_record_capacity_cut_by_hand():
    """G = 5, arena of 3 rows, cursor at 1: slots 0 and 2 get rows 1 and 2; slots 3 and 4 take the numbers 3 and 4, which
    lie outside -> -1 and two overflows, and the cursor still ends at 5."""
    G, T, Tmax = 5, 3, 4
    mi, lm, pol, _ = _sample(G, T, 1)
    player = np.array([0, -1, -1, 1, 1], np.int64)             # a player of 0 gets the sign +1
    done = np.array([0, 1, 0, 0, 0], np.uint8)
    step_index, step_counts = np.full((G, Tmax), -1, np.int64), np.array([0, 2, 1, 0, 3], np.int64)
    rows, arena = np.full(G, 99, np.int64), _arena(8, T)
    cursor, overflow = ref_record(done, 1, 3, Tmax, step_index, step_counts, rows, 0, mi, lm, pol, player, arena)
    assert (cursor, overflow) == (5, 2)
    assert rows.tolist() == [1, -1, 2, -1, -1]
    assert step_counts.tolist() == [1, 2, 2, 0, 3]
    assert step_index.tolist() == [[1, -1, -1, -1], [-1] * 4, [-1, 2, -1, -1], [-1] * 4, [-1] * 4]
    a_state, a_legal, a_policy, a_value, a_soft, a_sign = arena
    assert a_sign.tolist() == [0x7F, 1, -1] + [0x7F] * 5
    assert np.isnan(a_value[1:3]).all() and np.isnan(a_soft[1:3]).all()
    assert (np.delete(a_value, [1, 2]) == 7.0).all() and (np.delete(a_soft, [1, 2]) == 7.0).all()
    assert np.array_equal(a_state[1], mi[0].reshape(-1)) and np.array_equal(a_state[2], mi[2].reshape(-1))
    assert np.array_equal(a_legal[1:3], lm[[0, 2]]) and np.array_equal(a_policy[1:3], pol[[0, 2]])
    assert (np.delete(a_state, [1, 2], 0) == 0).all() and (np.delete(a_legal, [1, 2], 0) == 0x7F).all()


def test_record_full_slot_by_hand():
    """Tmax = 2 with slot 1 already at 2: it takes row number 5 (a hole), gets -1 and one overflow; both layouts."""
    G, T, Tmax = 3, 2, 2
    mi, lm, pol, player = _sample(G, T, 2)
    done = np.zeros(G, np.uint8)
    step_index, step_counts = np.full((G, Tmax), -1, np.int64), np.array([0, 2, 1], np.int64)
    step_index[1] = [0, 1]; step_index[2, 0] = 2
    rows, arena = np.zeros(G, np.int64), _arena(10, T)
    cursor, overflow = ref_record(done, 4, 10, Tmax, step_index, step_counts, rows, 3, mi, lm, pol, player, arena)
    assert (cursor, overflow) == (7, 4)
    assert rows.tolist() == [4, -1, 6] and step_counts.tolist() == [1, 2, 2]
    assert step_index.tolist() == [[4, -1], [0, 1], [2, 6]]
    assert (arena[5] != 0x7F).nonzero()[0].tolist() == [4, 6]
    # slot-major: row = g * Tmax + n, nothing to number
    step_counts, rows, arena = np.array([0, 2, 1], np.int64), np.zeros(G, np.int64), _arena(6, T)
    cursor, overflow = ref_record(done, None, 6, Tmax, None, step_counts, rows, 0, mi, lm, pol, player, arena)
    assert (cursor, overflow) == (None, 1)
    assert rows.tolist() == [0, -1, 5] and step_counts.tolist() == [1, 2, 2]
    assert (arena[5] != 0x7F).nonzero()[0].tolist() == [0, 5]
    assert np.array_equal(arena[2][5], pol[2])


def test_record_mask_by_hand():
    """A live slot whose search records nothing (record == 0) takes no row number and counts no step."""
    G, T, Tmax = 4, 2, 3
    mi, lm, pol, player = _sample(G, T, 4)
    done, record = np.array([0, 0, 1, 0], np.uint8), np.array([1, 0, 1, 1], np.uint8)
    step_index, step_counts = np.full((G, Tmax), -1, np.int64), np.array([1, 1, 1, 0], np.int64)
    rows, arena = np.zeros(G, np.int64), _arena(9, T)
    cursor, overflow = ref_record(done, 2, 9, Tmax, step_index, step_counts, rows, 0, mi, lm, pol, player, arena, record)
    assert (cursor, overflow) == (4, 0)
    assert rows.tolist() == [2, -1, -1, 3] and step_counts.tolist() == [2, 1, 1, 1]
    assert step_index.tolist() == [[-1, 2, -1], [-1] * 3, [-1] * 3, [3, -1, -1]]
    assert (arena[5] != 0x7F).nonzero()[0].tolist() == [2, 3]


def test_reseat_budget_and_logged_only_by_hand():
    """Four finished slots, budget 2.  Plain: slots 0 and 1 restart as games 40 and 41.  logged_only: slot 1 still holds
    rows and waits, so slots 0 and 3 restart and slot 4 is left over with the budget at 0."""
    z = load("g7_ops.npz")
    G = 5
    done0 = np.array([1, 1, 0, 1, 1], np.uint8)
    counts0 = np.array([0, 3, 5, 0, 0], np.int64)
    fresh = O.initial_states(1)
    for logged_only, seated in ((False, [0, 1]), (True, [0, 3])):
        st = {f: np.array(states(z, "s")[f][:G]) for f in FIELDS}
        before = {f: st[f].copy() for f in FIELDS}
        done, plies, counts = done0.copy(), np.array([9, 8, 7, 6, 5], np.int64), counts0.copy()
        slot_game, reseated = np.array([10, 11, 12, 13, 14], np.int64), np.zeros(G, np.uint8)
        budget, next_game = ref_reseat(st, done, plies, counts, 2, 40, slot_game, reseated, logged_only)
        assert (budget, next_game) == (0, 42)
        want_done, want_plies, want_counts, want_game = done0.copy(), [9, 8, 7, 6, 5], counts0.copy(), [10, 11, 12, 13, 14]
        for rank, g in enumerate(seated):
            want_done[g], want_plies[g], want_counts[g], want_game[g] = 0, 0, 0, 40 + rank
        assert done.tolist() == want_done.tolist() and plies.tolist() == want_plies
        assert counts.tolist() == want_counts.tolist() and slot_game.tolist() == want_game
        assert reseated.tolist() == [1 if g in seated else 0 for g in range(G)]
        for g in range(G):
            want = fresh if g in seated else before
            assert all(np.array_equal(st[f][g], want[f][0 if g in seated else g]) for f in FIELDS), g
    # a budget of 0 changes nothing; more budget than finished slots keeps the rest
    st = O.initial_states(G)
    done, plies, counts, slot_game = done0.copy(), np.ones(G, np.int64), counts0.copy(), np.zeros(G, np.int64)
    assert ref_reseat(st, done, plies, counts, 0, 7, slot_game) == (0, 7)
    assert done.tolist() == done0.tolist() and plies.tolist() == [1] * G and slot_game.tolist() == [0] * G
    assert ref_reseat(st, done, plies, counts, 9, (1 << 40) + 7, slot_game) == (5, (1 << 40) + 11)
    assert done.tolist() == [0] * G and slot_game.tolist() == [(1 << 40) + 7, (1 << 40) + 8, 0, (1 << 40) + 9, (1 << 40) + 10]


def test_step_finish_endings_by_hand():
    """Five slots on the empty board, Black to move, max_plies 5, k 2: slot 0 plays on; slot 1 reaches the ply cap with this
    move (draw, one black piece: soft = tanh(2 / 18), histogram bin 19); slot 2 is a terminal root (the side to move,
    Black, has lost); slot 3 has no valid choice (draw); slot 4 is already done.  Slot 3 recorded no row: it counts only
    where game_plies is given."""
    G, Tmax = 5, 2
    mask, meta = O.encode_actions(O.initial_states(1))
    code = meta[0, int(np.flatnonzero(mask[0])[0])]
    soft1 = np.float32(np.tanh(np.float32(2.0) / np.float32(18.0)))
    for with_plies in (False, True):
        st = O.initial_states(G)
        plies, done = np.array([0, 4, 2, 3, 1], np.int64), np.array([0, 0, 0, 0, 1], np.uint8)
        codes = np.repeat(code[None], G, 0)
        term, cvalid = np.array([0, 0, 1, 0, 0], np.uint8), np.array([1, 1, 1, 0, 1], np.uint8)
        step_index = np.array([[0, -1], [5, 1], [2, 4], [-1, -1], [3, -1]], np.int64)
        step_counts = np.array([1, 2, 3, 0, 1], np.int64)                     # slot 2: above Tmax, clamped to 2
        signs = np.array([1, -1, 1, 1, -1, 1], np.int8)
        value, soft = np.full(6, NAN), np.full(6, NAN)
        outcome, hist, lengths = np.zeros(3, np.int64), np.zeros(37, np.int64), np.full(8, -1, np.int64)
        slot_game = np.array([7, 6, 5, 4, 3], np.int64)
        game_plies = np.full(8, -1, np.int64) if with_plies else None
        fin = ref_step_finish(st, plies, done, codes, term, cvalid, 5, 2.0, value, soft, signs, step_index, step_counts,
                              Tmax, outcome, hist, lengths, slot_game, 10, None, False, game_plies)
        assert fin == 13
        assert plies.tolist() == [1, 5, 2, 3, 1] and done.tolist() == [0, 1, 1, 1, 1]
        assert step_counts.tolist() == [1, 2, 3, 0, 1]
        assert np.abs(st["board"]).reshape(G, -1).sum(1).tolist() == [1, 1, 0, 0, 0]
        assert st["current_player"].tolist() == [-1, -1, 1, 1, 1]
        want_v = np.array([np.nan, -0.0, -1.0, np.nan, 1.0, 0.0], np.float32)
        assert np.array_equal(value.view(np.int32), want_v.view(np.int32))
        np.testing.assert_allclose(soft, [np.nan, -soft1, 0.0, np.nan, -0.0, soft1], atol=1e-6, rtol=0)
        assert outcome.tolist() == ([0, 1, 2] if with_plies else [0, 1, 1])
        assert lengths.tolist() == [-1, -1, -1, -1, 0 if with_plies else -1, 2, 2, -1]
        assert hist.tolist() == [0] * 18 + [2, 1] + [0] * 17
        if with_plies:
            assert game_plies.tolist() == [-1, -1, -1, -1, 4, 3, 5, -1]
    # the in-kernel re-seat: the finished slots restart instead of being marked done
    st = O.initial_states(G)
    plies, done = np.array([0, 4, 2, 3, 1], np.int64), np.array([0, 0, 0, 0, 1], np.uint8)
    step_counts, reseated = np.array([1, 2, 3, 0, 1], np.int64), np.zeros(G, np.uint8)
    value, soft, outcome = np.full(6, NAN), np.full(6, NAN), np.zeros(3, np.int64)
    fin = ref_step_finish(st, plies, done, codes, term, cvalid, 5, 2.0, value, soft, signs, step_index, step_counts, Tmax,
                          outcome, reseated=reseated, reseat=True)
    assert fin == 3 and outcome.tolist() == [0, 1, 1]
    assert plies.tolist() == [1, 0, 0, 0, 1] and done.tolist() == [0, 0, 0, 0, 1]
    assert step_counts.tolist() == [1, 0, 0, 0, 1] and reseated.tolist() == [0, 1, 1, 1, 0]
    assert np.abs(st["board"]).reshape(G, -1).sum(1).tolist() == [1, 0, 0, 0, 0]
    assert st["current_player"].tolist() == [-1, 1, 1, 1, 1] and st["phase"].tolist() == [1] * G
    assert np.array_equal(value.view(np.int32), want_v.view(np.int32))


# ---- the inputs of tests/test_gpu_wave_tail.py reach their coverage (host alone) ----------------------------------------
def test_gpu_step_case_meets_every_ending_three_times():
    c = step_case()
    G, Tmax = c["G"], c["Tmax"]
    assert 1300 <= G <= 1700
    st, plies, done, counts = copy_states(c["states"]), c["plies"].copy(), c["done"].copy(), c["step_counts"].copy()
    value, soft = sentinel_f32(c["R"]), sentinel_f32(c["R"])
    outcome, hist, lengths = np.zeros(3, np.int64), np.zeros(37, np.int64), np.full(G, -7, np.int64)
    fin = ref_step_finish(st, plies, done, c["codes"], c["terminal"], c["cvalid"], c["max_plies"], c["k"], value, soft,
                          c["signs"], c["step_index"], counts, Tmax, outcome, hist, lengths, c["slot_game"])
    kinds = step_kinds_of_result(c, st, plies, done)
    assert np.array_equal(kinds, c["kinds"])
    for name in STEP_KINDS:
        assert int((kinds == name).sum()) >= 3, name
    ended = ~np.isin(kinds, ("on", "idle"))
    assert fin == int(ended.sum()) and (outcome > 0).all()
    n_rows = np.minimum(c["step_counts"], Tmax)
    assert {0, 1, 64, 65}.issubset(set(n_rows[ended].tolist())) and (c["step_counts"][ended] > Tmax).any()
    assert hist[0] >= 3 and hist[36] >= 3 and int(hist.sum()) == fin
    written = np.zeros(c["R"], bool)
    for g in np.flatnonzero(ended):
        written[c["step_index"][g, :n_rows[g]]] = True
    assert np.array_equal(value.view(np.int32) != SENT_F32, written)           # exactly the rows of the finished games
    assert not written[-G:].any()                                              # the guard band
    assert np.array_equal(np.sort(c["slot_game"]), np.arange(G))


def test_gpu_record_cases_fire_both_overflow_branches():
    """The closed form of a record case (who overflows, where the cursor ends) agrees with the restatement, the capacity
    cut falls where it was placed, and every (layout, mask != zero) family meets both overflow branches."""
    assert cut_slot(2049) % 3 == 1 and cut_slot(16385) % (17 * 64) == 0
    for G in (1, 65, 1025, 2049):
        for slot_major in (False, True):
            for mask in (None, "half", "zero"):
                caps = steps = 0
                for done_kind, cut in (("random", False), ("live", False), ("done", False), ("random", True), ("live", True)):
                    if slot_major and cut:
                        continue
                    c = record_case(G, slot_major, mask, done_kind, cut, T=5)
                    idx = None if slot_major else np.full((G, c["Tmax"]), -7, np.int64)
                    counts, rows = c["step_counts"].copy(), np.zeros(G, np.int64)
                    cursor, overflow = ref_record(c["done"], c["cursor"], c["capacity"], c["Tmax"], idx, counts, rows,
                                                  c["overflow"], c["model_input"], c["legal"], c["policy"], c["player"],
                                                  _arena(c["rows_total"], 5), c["record"])
                    assert overflow - c["overflow"] == c["over_cap"] + c["over_steps"]
                    assert cursor == (None if slot_major else 37 + c["recorded"])
                    if cut and done_kind == "random" and mask != "zero":      # the cut slot is the first one without a row
                        s = cut_slot(G)
                        assert rows[s] == -1 and counts[s] == c["step_counts"][s] and (s == 0 or rows[s - 1] == c["capacity"] - 1
                                                                                       or c["step_counts"][s - 1] >= c["Tmax"])
                    caps, steps = caps + c["over_cap"], steps + c["over_steps"]
                if mask != "zero" and G >= 64:
                    assert steps > 0 and (slot_major or caps > 0)


def test_gpu_reseat_cases_run_out_of_budget():
    for G in RESEAT_G:
        c = reseat_case(G)
        for logged_only in (0, 1):
            eligible, budgets = reseat_budgets(c, logged_only)
            assert G == 1 or eligible >= 2
            assert any(0 < b < eligible for b in budgets) or eligible < 2
        assert ((c["done"] != 0) & (c["step_counts"] > 0)).any() or G == 1
        assert c["next_game"] > 1 << 32


def test_gpu_scripted_wave_meets_its_cases_on_the_host():
    for slot_major in (False, True):
        w = ScriptedTail(slot_major)
        for _ in range(w.PLIES):
            w.advance(w.inputs())
        w.check_coverage()
