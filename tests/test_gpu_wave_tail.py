"""GPU: the device tail of the wave loop -- lz_wave_record, lz_wave_step_finish, lz_wave_reseat (csrc/lz_ops.hip) -- called
through the C ABI with inputs of the test's own and held to the sequential restatement tests/wave_tail_ref.py (which
tests/test_wave_tail_ref_cpu.py anchors to the reference's golden vectors).

Integer, byte, index and copied float outputs are compared bit for bit over the WHOLE buffer: every output starts as a
sentinel (0x7F bytes, a quiet NaN with a marked payload), every arena carries a guard band of at least num_slots rows
past its capacity, so "wrote nothing" is checked everywhere.  The soft targets are the only computed floats (tanhf):
they get the tolerance test_gpu_ops.py::test_self_play_step_inplace gives `soft` (1e-6 absolute), and all rows of one game
must carry bit-identical |soft|."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lz_oracle as O
from tests.golden_utils import states_equal
from tests.test_gpu_ops import DEV, from_dev, to_dev
from tests.wave_tail_cases import (RECORD_G, RESEAT_G, SENT_F32, SENT_I64, STEP_KINDS, ScriptedTail, copy_states,
                                   record_case, reseat_budgets, reseat_case, sentinel_f32, step_case,
                                   step_kinds_of_result)
from tests.wave_tail_ref import ref_record, ref_reseat, ref_step_finish

pytestmark = pytest.mark.gpu

SOFT_ATOL = 1e-6                                          # test_gpu_ops.py::test_self_play_step_inplace
ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from liuzhou_amd import _lib
    return _lib


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_sentinel(shape, dtype):
    """The device twin of a sentinel-filled host buffer, made on the device."""
    if dtype == np.float32:
        return torch.full(shape, SENT_F32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full(shape, 0x7F, dtype={np.uint8: torch.uint8, np.int8: torch.int8}[dtype], device=DEV)


def assert_bits(got, want, name):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, name
    a, b = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        e = int(bad[0]) // got.dtype.itemsize
        raise AssertionError(f"{name}: {bad.size} bytes differ, first at element {e}: got {got.reshape(-1)[e]!r}, "
                             f"want {want.reshape(-1)[e]!r}")


def assert_soft(got, want, name):
    """Computed soft targets within the tolerance where the restatement wrote one, bit-equal (NaN fill / sentinel) elsewhere."""
    got = got.cpu().numpy()
    fin = np.isfinite(want)
    assert_bits(got[~fin], want[~fin], name + " (unwritten rows)")
    np.testing.assert_allclose(got[fin], want[fin], atol=SOFT_ATOL, rtol=0, err_msg=name)


def host_arena(R, T):
    return (sentinel_f32((R, 396)), np.full((R, T), 0x7F, np.uint8), sentinel_f32((R, T)), sentinel_f32(R),
            sentinel_f32(R), np.full(R, 0x7F, np.int8))


def dev_arena(R, T):
    return [dev_sentinel((R, 396), np.float32), dev_sentinel((R, T), np.uint8), dev_sentinel((R, T), np.float32),
            dev_sentinel((R,), np.float32), dev_sentinel((R,), np.float32), dev_sentinel((R,), np.int8)]


ARENA_NAMES = ("a_state", "a_legal", "a_policy", "a_value", "a_soft", "a_sign")


def lz_record(L, G, done, cursor, capacity, Tmax, step_index, step_counts, rows, overflow, mi, lm, pol, player, T, arena,
              record):
    st = L.lib().lz_wave_record(
        L.ptr(done), L.i64(G), L.ptr(cursor), L.i64(capacity), L.i64(Tmax), L.ptr(step_index), L.ptr(step_counts),
        L.ptr(rows), L.ptr(overflow), L.ptr(mi), L.ptr(lm), L.ptr(pol), L.ptr(player), L.i64(T),
        *(L.ptr(a) for a in arena), L.ptr(record), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return st


def lz_step_finish(L, ts, G, plies, done, codes, term, cvalid, max_plies, k, value, soft, signs, step_index, step_counts,
                   Tmax, outcome, hist, lengths, slot_game, finished, reseated, reseat, game_plies):
    """`lengths`: a tensor, None, or a ready C pointer."""
    lp = lengths if isinstance(lengths, C.c_void_p) else L.ptr(lengths)
    st = L.lib().lz_wave_step_finish(
        C.byref(L.soa(ts)), L.i64(G), L.ptr(plies), L.ptr(done), L.ptr(codes), L.ptr(term), L.ptr(cvalid),
        L.i64(max_plies), C.c_float(k), L.ptr(value), L.ptr(soft), L.ptr(signs), L.ptr(step_index), L.ptr(step_counts),
        L.i64(Tmax), L.ptr(outcome), L.ptr(hist), lp, L.ptr(slot_game), L.ptr(finished), L.ptr(reseated),
        C.c_int(1 if reseat else 0), L.ptr(game_plies), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return st


def lz_reseat(L, ts, G, done, plies, step_counts, budget, next_game, slot_game, reseated, logged_only):
    st = L.lib().lz_wave_reseat(C.byref(L.soa(ts)), L.i64(G), L.ptr(done), L.ptr(plies), L.ptr(step_counts),
                                L.ptr(budget), L.ptr(next_game), L.ptr(slot_game), L.ptr(reseated),
                                C.c_int(1 if logged_only else 0), L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return st


# =========================================================================================================================
# lz_wave_record
# =========================================================================================================================
def run_record(L, c):
    G, T, Tmax, R, slot_major = c["G"], c["T"], c["Tmax"], c["rows_total"], c["cursor"] is None
    assert R >= c["capacity"] + G                            # the guard band
    h_arena = host_arena(R, T)
    h_index = None if slot_major else np.full((G, Tmax), -7, np.int64)
    h_counts, h_rows = c["step_counts"].copy(), np.full(G, SENT_I64, np.int64)
    d_arena = dev_arena(R, T)
    d_index, d_counts, d_rows = dv(h_index), dv(h_counts), dv(h_rows)
    d_cursor = None if slot_major else dv(np.array([c["cursor"]], np.int64))
    d_overflow = dv(np.array([c["overflow"]], np.int32))
    d_in = [dv(c[k]) for k in ("model_input", "legal", "policy", "player")]
    L.check(lz_record(L, G, dv(c["done"]), d_cursor, c["capacity"], Tmax, d_index, d_counts, d_rows, d_overflow, *d_in, T,
                      d_arena, dv(c["record"])), "wave_record")
    cursor, overflow = ref_record(c["done"], c["cursor"], c["capacity"], Tmax, h_index, h_counts, h_rows, c["overflow"],
                                  c["model_input"], c["legal"], c["policy"], c["player"], h_arena, c["record"])
    # the restatement against the closed form of the case: who overflows, and where the cursor ends
    assert overflow - c["overflow"] == c["over_cap"] + c["over_steps"]
    assert int((h_rows >= 0).sum()) == c["recorded"] - c["over_cap"] - c["over_steps"]
    if not slot_major:
        assert cursor == c["cursor"] + c["recorded"]
        assert int(d_cursor.item()) == cursor
        assert_bits(d_index, h_index, "step_index")
    assert int(d_overflow.item()) == overflow
    assert_bits(d_rows, h_rows, "rows")
    assert_bits(d_counts, h_counts, "step_counts")
    for name, got, want in zip(ARENA_NAMES, d_arena, h_arena):
        assert_bits(got, want, name)
    cap = c["capacity"]                                       # the guard band past the capacity is untouched
    for name, want, fresh in zip(ARENA_NAMES, h_arena, host_arena(R - cap, T)):
        assert_bits(want[cap:], fresh, name + " guard band")


@pytest.mark.parametrize("mask", [None, "half", "zero"])
@pytest.mark.parametrize("slot_major", [False, True], ids=["cursor", "slot_major"])
@pytest.mark.parametrize("G", RECORD_G)
def test_record_rows_and_arena_equal_the_restatement(L, G, slot_major, mask):
    """done ~30 % / all live / all done; everything fits, and (cursor layout) the capacity cutting through the wave."""
    runs = [("random", False), ("live", False), ("done", False)]
    if not slot_major:
        runs += [("random", True), ("live", True)]
    over_cap = over_steps = 0
    for done_kind, cut in runs:
        c = record_case(G, slot_major, mask, done_kind, cut)
        run_record(L, c)
        over_cap, over_steps = over_cap + c["over_cap"], over_steps + c["over_steps"]
    if mask != "zero" and G >= 64:                            # both overflow branches fired (slot-major has only one)
        assert over_steps > 0 and (slot_major or over_cap > 0)
    if mask == "zero":
        assert over_cap == over_steps == 0


@pytest.mark.parametrize("slot_major", [False, True], ids=["cursor", "slot_major"])
def test_record_action_width_5(L, slot_major):
    """T = 5: no multiple of 4 or 64."""
    for cut in ([False, True] if not slot_major else [False]):
        run_record(L, record_case(65, slot_major, "half", "random", cut, T=5))


def test_record_refuses_bad_arguments_without_a_launch(L):
    G, T, Tmax = 4, 5, 6
    c = record_case(G, False, None, "live", False, T=T)
    R = c["rows_total"]
    arena = dev_arena(R, T)
    index, counts, rows = dv(np.full((G, Tmax), -7, np.int64)), dv(c["step_counts"]), dv(np.full(G, SENT_I64, np.int64))
    cursor, overflow = dv(np.array([37], np.int64)), dv(np.array([5], np.int32))
    d_in = [dv(c[k]) for k in ("model_input", "legal", "policy", "player")]
    done = dv(c["done"])

    def call(G=G, cursor=cursor, capacity=R, Tmax=Tmax, index=index, T=T):
        return lz_record(L, G, done, cursor, capacity, Tmax, index, counts, rows, overflow, *d_in, T, arena, None)

    assert call(cursor=None) == ERR_ARG                       # exactly one of cursor / step_index
    assert call(index=None) == ERR_ARG
    assert call(cursor=None, index=None, capacity=G * Tmax - 1) == ERR_ARG     # slot-major needs G * Tmax rows
    assert call(Tmax=0) == ERR_ARG and call(Tmax=-1) == ERR_ARG
    assert call(T=0) == ERR_ARG and call(T=-3) == ERR_ARG
    assert call(G=-1) == ERR_ARG and call(capacity=-1) == ERR_ARG
    null = C.c_void_p(None)
    assert L.lib().lz_wave_record(null, L.i64(0), null, L.i64(0), L.i64(1), *([null] * 8), L.i64(1), *([null] * 8)) == 0
    assert cursor.item() == 37 and overflow.item() == 5       # nothing ran
    assert_bits(rows, np.full(G, SENT_I64, np.int64), "rows")
    assert_bits(counts, c["step_counts"], "step_counts")
    assert_bits(index, np.full((G, Tmax), -7, np.int64), "step_index")
    for name, got, want in zip(ARENA_NAMES, arena, host_arena(R, T)):
        assert_bits(got, want, name)


# =========================================================================================================================
# lz_wave_step_finish
# =========================================================================================================================
@pytest.mark.parametrize("variant", ["game_map", "slot_major", "in_kernel_reseat"])
def test_step_finish_every_ending_in_one_launch(L, variant):
    """~1600 slots (tests/wave_tail_cases.py::step_case) under three pointer / flag variants:
    game_map: step_index, slot_game = a permutation + 2^32 (lengths is addressed through the full 64-bit game number: its
              pointer is passed 2^32 elements low), lengths / delta_hist / finished given, game_plies NULL;
    slot_major: step_index NULL (row = g * Tmax + j), slot_game NULL, lengths / game_plies / delta_hist / finished given;
    in_kernel_reseat: step_index, everything optional NULL, reseat = 1 with `reseated`."""
    c = step_case()
    G, Tmax = c["G"], c["Tmax"]
    slot_major, reseat = variant == "slot_major", variant == "in_kernel_reseat"
    h_index = None if slot_major else c["step_index"]
    signs = c["signs_slot"] if slot_major else c["signs"]
    R = signs.shape[0]
    h_st, h_plies, h_done, h_counts = copy_states(c["states"]), c["plies"].copy(), c["done"].copy(), c["step_counts"].copy()
    h_value, h_soft = sentinel_f32(R), sentinel_f32(R)
    h_outcome = np.array([3, 5, 7], np.int64)
    h_hist = None if reseat else np.arange(37, dtype=np.int64)
    h_lengths = None if reseat else np.full(G, -7, np.int64)
    h_plies_out = np.full(G, -7, np.int64) if slot_major else None
    h_game = c["slot_game"] if variant == "game_map" else None
    h_reseated = np.full(G, 0x7F, np.uint8)
    HI = 1 << 32

    ts = to_dev(h_st)
    d_plies, d_done, d_counts = dv(h_plies), dv(h_done), dv(h_counts)
    d_value, d_soft, d_outcome = dv(h_value), dv(h_soft), dv(h_outcome)
    d_hist, d_lengths, d_plies_out, d_reseated = dv(h_hist), dv(h_lengths), dv(h_plies_out), dv(h_reseated)
    d_finished = None if reseat else dv(np.array([11], np.int64))
    d_game = None if h_game is None else dv(h_game + HI)
    lengths_arg = C.c_void_p(d_lengths.data_ptr() - HI * 8) if h_game is not None else d_lengths
    d_index = dv(h_index)

    finished = ref_step_finish(h_st, h_plies, h_done, c["codes"], c["terminal"], c["cvalid"], c["max_plies"], c["k"],
                               h_value, h_soft, signs, h_index, h_counts, Tmax, h_outcome, h_hist, h_lengths, h_game, 11,
                               h_reseated if reseat else None, reseat, h_plies_out)
    # coverage, in the restatement's result, before anything is compared
    if reseat:
        kinds = c["kinds"]
        assert (h_done == c["done"]).all() and int((h_reseated == 1).sum()) == finished - 11
    else:
        kinds = step_kinds_of_result(c, h_st, h_plies, h_done)
        assert np.array_equal(kinds, c["kinds"])
    for name in STEP_KINDS:
        assert int((kinds == name).sum()) >= 3, name
    ended = ~np.isin(kinds, ("on", "idle"))
    assert finished - 11 == int(ended.sum())
    n_rows = np.minimum(c["step_counts"], Tmax)
    assert {0, 1, 64, 65}.issubset(set(n_rows[ended].tolist())) and (c["step_counts"][ended] > Tmax).any()
    if not reseat:
        assert h_hist[0] - 0 >= 3 and h_hist[36] - 36 >= 3        # the clamp of the histogram, both ends

    L.check(lz_step_finish(L, ts, G, d_plies, d_done, dv(c["codes"]), dv(c["terminal"]), dv(c["cvalid"]), c["max_plies"],
                           c["k"], d_value, d_soft, dv(signs), d_index, d_counts, Tmax, d_outcome, d_hist, lengths_arg,
                           d_game, d_finished, d_reseated, reseat, d_plies_out), "wave_step_finish")
    ok, field = states_equal(from_dev(ts), h_st)
    assert ok, field
    assert_bits(d_plies, h_plies, "plies")
    assert_bits(d_done, h_done, "done")
    assert_bits(d_counts, h_counts, "step_counts")
    assert_bits(d_value, h_value, "value column")
    assert_soft(d_soft, h_soft, "soft column")
    assert_bits(d_outcome, h_outcome, "outcome")
    assert_bits(d_reseated, h_reseated, "reseated")
    if not reseat:
        assert_bits(d_hist, h_hist, "delta_hist")
        assert_bits(d_lengths, h_lengths, "lengths")
        assert int(d_finished.item()) == finished
    if slot_major:
        assert_bits(d_plies_out, h_plies_out, "game_plies")
    if d_index is not None:
        assert_bits(d_index, h_index, "step_index")
    # all rows of one game carry the same |soft|, bit for bit
    got_soft = d_soft.cpu().numpy().view(np.int32) & 0x7FFFFFFF
    sim = h_index if h_index is not None else np.arange(G * Tmax, dtype=np.int64).reshape(G, Tmax)
    for g in np.flatnonzero(ended & (n_rows > 0)):
        assert np.unique(got_soft[sim[g, :n_rows[g]]]).size == 1, g


# =========================================================================================================================
# lz_wave_reseat
# =========================================================================================================================
@pytest.mark.parametrize("with_reseated", [True, False], ids=["reseated", "reseated_null"])
@pytest.mark.parametrize("logged_only", [0, 1])
@pytest.mark.parametrize("G", RESEAT_G)
def test_reseat_in_slot_order_while_the_budget_lasts(L, G, logged_only, with_reseated):
    c = reseat_case(G)
    eligible, budgets = reseat_budgets(c, logged_only)
    is_eligible = (c["done"] != 0) & ~((c["step_counts"] > 0) & bool(logged_only))
    ran_dry = False
    for budget in budgets:
        h_st, h_done, h_plies = copy_states(c["states"]), c["done"].copy(), c["plies"].copy()
        h_counts, h_game = c["step_counts"].copy(), c["slot_game"].copy()
        h_reseated = np.full(G, 0x7F, np.uint8) if with_reseated else None
        ts = to_dev(h_st)
        d_done, d_plies, d_counts, d_game, d_reseated = dv(h_done), dv(h_plies), dv(h_counts), dv(h_game), dv(h_reseated)
        d_budget, d_next = dv(np.array([budget], np.int64)), dv(np.array([c["next_game"]], np.int64))
        L.check(lz_reseat(L, ts, G, d_done, d_plies, d_counts, d_budget, d_next, d_game, d_reseated, logged_only),
                "wave_reseat")
        left, next_game = ref_reseat(h_st, h_done, h_plies, h_counts, budget, c["next_game"], h_game, h_reseated,
                                     bool(logged_only))
        used = min(eligible, budget)
        assert (left, next_game) == (budget - used, c["next_game"] + used)
        assert int(d_budget.item()) == left and int(d_next.item()) == next_game
        got = from_dev(ts)
        ok, field = states_equal(got, h_st)
        assert ok, field
        assert_bits(d_done, h_done, "done")
        assert_bits(d_plies, h_plies, "plies")
        assert_bits(d_counts, h_counts, "step_counts")
        assert_bits(d_game, h_game, "slot_game")
        if with_reseated:
            assert_bits(d_reseated, h_reseated, "reseated")
        # slots that were not eligible, and eligible ones past the budget, are exactly as they were
        seated = is_eligible & (np.cumsum(is_eligible) <= used)
        assert int(seated.sum()) == used
        keep = ~seated
        if keep.any():                                        # (G = 1: the only slot may be the one that restarts)
            ok, field = states_equal(O.select_states(got, keep), O.select_states(c["states"], keep))
            assert ok, field
        assert_bits(d_done.cpu().numpy()[keep], c["done"][keep], "done of untouched slots")
        assert_bits(d_game.cpu().numpy()[keep], c["slot_game"][keep], "slot_game of untouched slots")
        assert (d_game.cpu().numpy()[seated] == c["next_game"] + np.arange(used)).all()
        ran_dry |= left == 0 and eligible > used
    if eligible >= 2:
        assert ran_dry                                        # the budget ran out with eligible slots left over


# =========================================================================================================================
# record -> step_finish -> reseat, ply after ply
# =========================================================================================================================
@pytest.mark.parametrize("slot_major", [False, True], ids=["cursor", "slot_major"])
def test_scripted_wave_equals_the_restatement_after_every_ply(L, slot_major):
    """tests/wave_tail_cases.py::ScriptedTail on the host, the three kernels on the device with the same inputs: every
    buffer after every ply, and with it the arena as it is built."""
    w = ScriptedTail(slot_major)
    G, Tmax, T = w.G, w.TMAX, w.T
    ts = to_dev(w.st)
    d_arena = dev_arena(w.R, T)
    d_plies, d_done, d_counts, d_index, d_rows = dv(w.plies), dv(w.done), dv(w.counts), dv(w.index), dv(w.rows)
    d_outcome, d_hist, d_lengths, d_game_plies = dv(w.outcome), dv(w.hist), dv(w.lengths), dv(w.game_plies)
    d_game, d_reseated = dv(w.slot_game), dv(w.reseated)
    d_cursor = None if slot_major else dv(np.array([w.cursor], np.int64))
    d_overflow, d_finished = dv(np.zeros(1, np.int32)), dv(np.zeros(1, np.int64))
    d_budget, d_next = dv(np.array([w.budget], np.int64)), dv(np.array([w.next_game], np.int64))
    for ply in range(w.PLIES):
        x = w.inputs()
        d_reseated.zero_()
        L.check(lz_record(L, G, d_done, d_cursor, w.capacity, Tmax, d_index, d_counts, d_rows, d_overflow,
                          dv(x["model_input"]), dv(x["legal"]), dv(x["policy"]), ts[4], T, d_arena, dv(x["record"])),
                "wave_record")
        L.check(lz_step_finish(L, ts, G, d_plies, d_done, dv(x["codes"]), dv(x["terminal"]), dv(x["cvalid"]), w.MAX_PLIES,
                               w.K, d_arena[3], d_arena[4], d_arena[5], d_index, d_counts, Tmax, d_outcome, d_hist,
                               d_lengths, d_game, d_finished, None, False, d_game_plies), "wave_step_finish")
        if slot_major:
            d_counts[d_done != 0] = 0
        L.check(lz_reseat(L, ts, G, d_done, d_plies, d_counts, d_budget, d_next, d_game, d_reseated, slot_major),
                "wave_reseat")
        w.advance(x)
        where = f"ply {ply}: "
        ok, field = states_equal(from_dev(ts), w.st)
        assert ok, where + field
        for name, got, want in (("plies", d_plies, w.plies), ("done", d_done, w.done), ("step_counts", d_counts, w.counts),
                                ("rows", d_rows, w.rows), ("outcome", d_outcome, w.outcome), ("delta_hist", d_hist, w.hist),
                                ("lengths", d_lengths, w.lengths), ("slot_game", d_game, w.slot_game),
                                ("reseated", d_reseated, w.reseated)):
            assert_bits(got, want, where + name)
        if slot_major:
            assert_bits(d_game_plies, w.game_plies, where + "game_plies")
        else:
            assert_bits(d_index, w.index, where + "step_index")
            assert int(d_cursor.item()) == w.cursor, where
        assert (int(d_overflow.item()), int(d_finished.item())) == (w.overflow, w.finished), where
        assert (int(d_budget.item()), int(d_next.item())) == (w.budget, w.next_game), where
        for name, got, want in zip(ARENA_NAMES, d_arena, w.arena):
            (assert_soft if name == "a_soft" else assert_bits)(got, want, where + name)
    w.check_coverage()
