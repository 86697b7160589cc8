"""Sequential restatement of the device tail of the wave loop (numpy only): `lz_wave_record`, `lz_wave_step_finish` and
`lz_wave_reseat` (csrc/lz_ops.hip), one plain loop over the slots in ascending order each.

Written from the kernels' contracts (include/liuzhou_hip.h) and the reference's runner, v1/python/self_play_gpu_runner.py:
190-256 (`append_steps` -> `step_index_matrix[active, positions] = rows` -> `self_play_step_inplace` -> piece-delta
histogram -> `finalize_games_inplace` -> `game_lengths`).  The move, the endings and the targets are NOT restated here:
they come from oracle.lz_oracle (`self_play_step_inplace`, `finalize_trajectory_inplace`, `initial_states`), which the
golden vectors anchor.  What this file adds is only what the fused kernels add around them: the row numbering, the
overflow rule, the bookkeeping of a finished game, and the start of the next games.

Every function works IN PLACE on the numpy arrays it is given (the counterparts of the device buffers) and returns the
scalars the kernels keep in one-element buffers.

The arena is the tuple the kernels take: (state float32[R, 396], legal uint8[R, T], policy float32[R, T],
value float32[R], soft float32[R], sign int8[R]) with R >= capacity rows; rows nobody writes keep what they held.
"""
import numpy as np

from oracle import lz_oracle as O

FIELDS = O.STATE_FIELDS
DELTA_BINS = 37                                           # piece difference -18 .. +18, clamped (runner: _PIECE_DELTA_*)


def ref_record(done, cursor, capacity, Tmax, step_index, step_counts, rows, overflow, model_input, legal, policy, player,
               arena, record=None):
    """lz_wave_record.  `cursor` int with `step_index` int64[G, Tmax], or both None for the slot-major arena
    (row = g * Tmax + n).  Returns (cursor, overflow).

    A live slot (done == 0) that records (record is None or record[g] != 0) always takes the next row number; the row is
    written only if it lies inside the arena and the slot has a free step, otherwise the slot gets -1, the overflow
    counter rises and the row number stays a hole.  The cursor advances by the number of live recording slots."""
    if (cursor is None) != (step_index is None):
        raise ValueError("ref_record: cursor and step_index go together")
    G = int(done.shape[0])
    if cursor is None and capacity < G * Tmax:
        raise ValueError("ref_record: the slot-major arena needs num_slots * max_steps rows")
    a_state, a_legal, a_policy, a_value, a_soft, a_sign = arena
    overflow = int(overflow)
    for g in range(G):
        if done[g] != 0 or (record is not None and record[g] == 0):
            rows[g] = -1
            continue
        n = int(step_counts[g])
        if cursor is None:
            row, fits = g * Tmax + n, n < Tmax
        else:
            row, fits = cursor, cursor < capacity and n < Tmax
            cursor += 1
        if not fits:
            rows[g] = -1
            overflow += 1
            continue
        rows[g] = row
        if step_index is not None:
            step_index[g, n] = row
        step_counts[g] = n + 1
        a_state[row] = model_input[g].reshape(-1)
        a_legal[row] = legal[g]
        a_policy[row] = policy[g]
        a_value[row] = np.float32(np.nan)
        a_soft[row] = np.float32(np.nan)
        a_sign[row] = 1 if player[g] >= 0 else -1         # v1/python/trajectory_buffer.py:145 (0 counts as +1)
    return cursor, overflow


def ref_finalize_book(states, slots, result, soft, plies_before, done, plies, value_t, soft_t, signs, step_index,
                      step_counts, Tmax, outcome, delta_hist=None, lengths=None, slot_game=None, finished=0,
                      reseated=None, reseat=False, game_plies=None):
    """What lz_wave_step_finish adds to the operator pair of the runner for the games `slots` that have just ended with
    `result` / `soft` (Black's frame): the targets of their rows (finalize_trajectory_inplace over min(step_counts, Tmax)
    steps; step_index None: row = g * Tmax + j), then per game, in ascending slot order, outcome / lengths / game_plies /
    the piece-delta histogram / the finished counter, and `done` or the fresh game.  Returns `finished`."""
    G = int(done.shape[0])
    slots = np.asarray(slots, np.int64).reshape(-1)
    order = np.argsort(slots, kind="stable")
    slots, result, soft = slots[order], np.asarray(result, np.float32)[order], np.asarray(soft, np.float32)[order]
    sim = step_index if step_index is not None else np.arange(G * Tmax, dtype=np.int64).reshape(G, Tmax)
    clamped = np.minimum(np.asarray(step_counts, np.int64), Tmax)
    O.finalize_trajectory_inplace(value_t, soft_t, signs, sim, clamped, slots, result, soft)
    fresh = O.initial_states(1)
    finished = int(finished)
    for g, res in zip(slots.tolist(), result.tolist()):
        n = int(clamped[g])
        gi = int(slot_game[g]) if slot_game is not None else g
        searched = int(plies_before[g]) + 1               # one search per ply, the last one included
        if n > 0 or game_plies is not None:               # a game without rows counts only where its searches are booked
            outcome[0 if res > 0 else (1 if res < 0 else 2)] += 1
            if lengths is not None:
                lengths[gi] = n
        if game_plies is not None:
            game_plies[gi] = searched
        if delta_hist is not None:
            b = np.asarray(states["board"][g]).reshape(-1)
            delta = int((b == 1).sum()) - int((b == -1).sum())
            delta_hist[min(max(delta + 18, 0), DELTA_BINS - 1)] += 1
        finished += 1
        if reseat:
            for f in FIELDS:
                states[f][g] = fresh[f][0]
            plies[g] = 0
            step_counts[g] = 0
            done[g] = 0
            if reseated is not None:
                reseated[g] = 1
        else:
            done[g] = 1
    return finished


def ref_step_finish(states, plies, done, codes, terminal, cvalid, max_plies, k, value_t, soft_t, signs, step_index,
                    step_counts, Tmax, outcome, delta_hist=None, lengths=None, slot_game=None, finished=0, reseated=None,
                    reseat=False, game_plies=None):
    """lz_wave_step_finish.  `states` dict of numpy arrays (oracle layout), `codes` int32[G, 4], `terminal` / `cvalid`
    one byte per slot, all indexed by slot; slots with done != 0 are left alone.  Returns `finished`."""
    live = np.flatnonzero(np.asarray(done) == 0)
    plies_before = np.array(plies, np.int64)
    slots, res, soft = O.self_play_step_inplace(states, plies, done, live, np.asarray(codes, np.int32)[live],
                                                np.asarray(terminal)[live] != 0, np.asarray(cvalid)[live] != 0,
                                                int(max_plies), float(k))
    return ref_finalize_book(states, slots, res, soft, plies_before, done, plies, value_t, soft_t, signs, step_index,
                             step_counts, Tmax, outcome, delta_hist, lengths, slot_game, finished, reseated, reseat,
                             game_plies)


def ref_reseat(states, done, plies, step_counts, budget, next_game, slot_game, reseated=None, logged_only=False):
    """lz_wave_reseat: finished slots, in ascending order while `budget` lasts, start game next_game + rank from the
    empty board; with `logged_only` a finished slot that still holds rows (step_counts > 0) waits.
    Returns (budget, next_game)."""
    budget, next_game = int(budget), int(next_game)
    fresh = O.initial_states(1)
    for g in range(int(done.shape[0])):
        if budget <= 0:
            break
        if done[g] == 0 or (logged_only and step_counts[g] > 0):
            continue
        for f in FIELDS:
            states[f][g] = fresh[f][0]
        plies[g] = 0
        step_counts[g] = 0
        done[g] = 0
        slot_game[g] = next_game
        if reseated is not None:
            reseated[g] = 1
        next_game += 1
        budget -= 1
    return budget, next_game
