"""Device-side tail of one ply of the v1 wave loop for a fixed wave of slots: trajectory rows, the move and the
finalisation of finished games without a host round trip (`lz_wave_record`, `lz_wave_step_finish`), and optionally the
TD(lambda) value targets from the searches' root values (`lz_wave_note_value`, `lz_wave_td_targets`; value_target.py)
and resignation with play-through calibration (`lz_wave_resign`, `lz_wave_resign_book`; resign.py) and policy surprise
weighting of a finished game's rows (`lz_wave_note_surprise`, `lz_wave_surprise_resample`; policy_surprise.py) and the
start bank that games fork from (`lz_start_bank_capture`, `lz_start_bank_seed`; start_bank.py).

It replaces, for whole waves, the sequence `append_steps` -> `step_index[...] = rows` -> `self_play_step_inplace` ->
`finalize_games_inplace` of v1/python/self_play_gpu_runner.py:205-247, whose `nonzero`-shaped outputs force one host
synchronisation per ply; finished slots stay in the batch and are masked by `done`."""
from __future__ import annotations

import ctypes as C
import time
from typing import Optional

import torch

from . import _lib as L
from .mcts_gpu import GpuStateBatch, RootSearchBatchOutput
from .trajectory_buffer import TensorTrajectoryBuffer
from .policy_surprise import policy_surprise_on
from .resign import COUNTER_KEYS, resign_kwargs
from .search_rules import SearchRules, start_bank_on
from .value_target import td_lambda_on

DELTA_BINS = 37


class WaveTail:
    def __init__(self, buffer: TensorTrajectoryBuffer, num_slots: int, max_game_plies: int, device,
                 soft_value_k: float = 2.0, reseat: bool = False, row_log=None, value_target_lambda: float = 1.0,
                 resign_threshold: float = 0.0, resign_min_moves: int = 10, resign_consecutive: int = 3,
                 resign_playthrough_fraction: float = 0.1, resign_streak: str = "side", seed: int = 0,
                 policy_surprise_weight: float = 0.0, prior_fn=None, start_bank=None, start_fork_prob: float = 0.0,
                 start_capture_prob: float = 0.0, start_min_move: int = 1, start_max_move: int = 143) -> None:
        # TD(lambda) value targets (value_target.py; 1 = off: every row gets the game's result, nothing below exists)
        self.td_lambda = float(value_target_lambda) if td_lambda_on(value_target_lambda) else None
        if self.td_lambda is not None and reseat:
            raise ValueError("WaveTail: value_target_lambda < 1 is not supported with the in-kernel re-seat (reseat=True): "
                             "it clears step_counts inside the step kernel, before the targets of the game are formed")
        # resignation (resign.py; threshold 0 = off: nothing below exists and `step_finish` reads the search's terminal mask)
        self.resign = resign_kwargs(resign_threshold, resign_min_moves, resign_consecutive, resign_playthrough_fraction,
                                    resign_streak) or None
        if self.resign is not None and reseat:
            raise ValueError("WaveTail: resignation is not supported with the in-kernel re-seat (reseat=True): `done` is "
                             "never set there, so the games that end are never booked")
        # policy surprise weighting (policy_surprise.py; 0 = off: nothing below exists, every game keeps its own rows)
        self.surprise_alpha = float(policy_surprise_weight) if policy_surprise_on(policy_surprise_weight) else None
        if self.surprise_alpha is not None:
            SearchRules(surprise_weight=self.surprise_alpha).refuse(reseat=reseat)
        # the start bank (start_bank.py; both probabilities 0 = off: nothing below exists and every game starts from the
        # empty board); the bank is the caller's and outlives the tail
        capacity = start_bank.capacity if start_bank is not None else 1
        start = None
        if start_bank_on(start_fork_prob, start_capture_prob, capacity, start_min_move, start_max_move):
            if start_bank is None:
                raise ValueError("WaveTail: the start bank rule is on but no `start_bank` (start_bank.StartBank) was passed")
            start = SearchRules(start=(float(start_fork_prob), float(start_capture_prob), capacity, int(start_min_move),
                                       int(start_max_move)))
            start.refuse(reseat=reseat)
        elif start_bank is not None:
            raise ValueError("WaveTail: a start bank was passed but start_fork_prob and start_capture_prob are both 0")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("WaveTail needs a HIP device (no CPU path)")
        self.buffer, self.G, self.max_plies, self.device = buffer, int(num_slots), int(max_game_plies), dev
        self.soft_k, self.reseat = float(soft_value_k), bool(reseat)
        z = lambda n, dt: torch.zeros((n,), dtype=dt, device=dev)
        self.rows = z(self.G, torch.int64)
        self.overflow = z(1, torch.int32)
        self.outcome = z(3, torch.int64)
        self.delta_hist = z(DELTA_BINS, torch.int64)
        self.finished = z(1, torch.int64)
        self.slot_game = torch.arange(self.G, dtype=torch.int64, device=dev)   # game number played in each slot (run())
        self.collect_timing = False
        self._timing_events = []
        self.live_estimate = self.G                          # run(): live slots two plies ago (host-visible without a wait)
        self.host_wait_ms = self.loop_ms = 0.0              # run(): time the host spent waiting for the device / in the loop
        self.plies_launched = 0
        # playout cap: `record_mask` uint8[G] (the search's full / fast mask, refreshed in place every ply) -- slots whose
        # search was fast record no row; `game_plies` int64 (indexed like `lengths`) -- the searches of every finished
        # game, which also decide that it counts in `outcome` when none of its searches recorded a row
        self.record_mask: Optional[torch.Tensor] = None
        self.game_plies: Optional[torch.Tensor] = None
        # finished_log.FinishedRowLog: the live rows are slot-major (row = slot * max_plies + step, no step_index matrix)
        # and the rows of a game move to the log when the game ends (the streaming worker)
        self.row_log = row_log
        # TD(lambda): the root value of every searched ply from Black's frame, the ply of every recorded step, the searched
        # plies of the game in each slot and the slots that were live when the ply began (8 B per slot and ply + 5 B per slot)
        self.q_hist = self.step_ply = self.hist_len = self.was_live = None
        if self.td_lambda is not None:
            self.q_hist = torch.zeros((self.G, self.max_plies), dtype=torch.float32, device=dev)
            self.step_ply = torch.zeros((self.G, self.max_plies), dtype=torch.int32, device=dev)
            self.hist_len = z(self.G, torch.int32)
            self.was_live = z(self.G, torch.uint8)
        # resignation: the per-slot streak counters (Black's, White's; "ply" mode uses the first), the latched would-be
        # resigner of a play-through game and its ply, the terminal mask the step kernel reads instead of the search's, the
        # slots that resigned this ply and the int64[8] counter block (21 B per slot + 64 B); `seed` keys the play-through
        # draw and `game_base` is the game number of slot_game 0 (sequential waves)
        self.streak = self.would = self.would_ply = self.terminal_out = self.resigned = self.resign_counters = None
        self.seed, self.game_base = int(seed) & 0xFFFFFFFFFFFFFFFF, 0
        if self.resign is not None:
            self.streak = torch.zeros((self.G, 2), dtype=torch.int32, device=dev)
            self.would = z(self.G, torch.int32)
            self.would_ply = z(self.G, torch.int32)
            self.terminal_out = z(self.G, torch.uint8)
            self.resigned = z(self.G, torch.uint8)
            self.resign_counters = z(len(COUNTER_KEYS), torch.int64)
            if self.was_live is None:
                self.was_live = z(self.G, torch.uint8)
        # policy surprise weighting: the surprise of every recorded step, the source row of every row slot of the game
        # that was resampled last (scratch, readable), the int64[3] counter block and the double sum of the surprises
        # (8 B per slot and step + 32 B); `prior_fn(search)` -> the noise-free root priors float32[G, action_dim] of the
        # searched positions (policy_surprise.root_prior; run() calls it once per ply)
        self.surprise_hist = self.surprise_src = self.surprise_counters = self.surprise_sum = None
        self.prior_fn = None
        if self.surprise_alpha is not None:
            self.prior_fn = prior_fn                     # run() refuses to start without one
            self.surprise_hist = torch.zeros((self.G, self.max_plies), dtype=torch.float32, device=dev)
            self.surprise_src = torch.zeros((self.G, self.max_plies), dtype=torch.int32, device=dev)
            self.surprise_counters = z(3, torch.int64)
            self.surprise_sum = z(1, torch.float64)
            if self.was_live is None:
                self.was_live = z(self.G, torch.uint8)
        # the start bank: its parameters and the int64[3] counter block (forked games, the sum of their move counts at
        # the fork, positions captured)
        self.bank = self.start = self.start_counters = None
        if start is not None:
            if start_bank.device != dev:
                raise ValueError(f"WaveTail: the start bank lives on {start_bank.device}, the wave on {dev}")
            self.bank, self.start = start_bank, start.start_kwargs()
            self.start_counters = z(3, torch.int64)
        if row_log is not None:
            if reseat:
                raise ValueError("WaveTail: the finished-row log needs run()'s re-seating (reseat=False)")
            if int(row_log.G) != self.G or int(row_log.Tmax) != self.max_plies:
                raise ValueError("WaveTail: the finished-row log was built for another wave shape")

    def _bracket(self, name: str):
        """HIP-event bracket + roctx range for one tail kernel sequence (bucket names of the reference's runner,
        v1/python/self_play_gpu_runner.py:276-281)."""
        from contextlib import contextmanager

        @contextmanager
        def cm():
            torch.cuda.nvtx.range_push(f"lz.tail.{name}")
            if self.collect_timing:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(torch.cuda.current_stream(self.device))
            try:
                yield
            finally:
                if self.collect_timing:
                    b.record(torch.cuda.current_stream(self.device))
                    self._timing_events.append((name, a, b))
                torch.cuda.nvtx.range_pop()
        return cm()

    def get_timing(self):
        torch.cuda.synchronize(self.device)
        out = {}
        for name, a, b in self._timing_events:
            d = out.setdefault(name, {"ms": 0.0, "calls": 0})
            d["ms"] += float(a.elapsed_time(b)); d["calls"] += 1
        self._timing_events = []
        return out

    def record(self, states: GpuStateBatch, done: torch.Tensor, step_index: torch.Tensor, step_counts: torch.Tensor,
               search: RootSearchBatchOutput) -> None:
        """Append this ply's sample of every live slot to the trajectory arena."""
        G = self.G
        shape = tuple(int(x) for x in search.model_input.shape[1:])
        if self.row_log is not None:
            cursor, steps = None, self.max_plies
            self.buffer.reserve_slot_major(G, steps, shape)
        else:
            cursor, steps = self.buffer.reserve_rows(G, shape), int(step_index.shape[1])
        a_state, a_legal, a_policy, a_value, a_soft, a_sign = self.buffer.arena()
        mi, lm, pol = search.model_input.contiguous(), search.legal_mask.contiguous(), search.policy_dense.contiguous()
        T = int(pol.shape[1])
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_wave_record(
                L.ptr(done), L.i64(G), L.ptr(cursor), L.i64(self.buffer.capacity), L.i64(steps),
                L.ptr(step_index), L.ptr(step_counts), L.ptr(self.rows), L.ptr(self.overflow), L.ptr(mi), L.ptr(lm),
                L.ptr(pol), L.ptr(states.current_player), L.i64(T), L.ptr(a_state), L.ptr(a_legal), L.ptr(a_policy),
                L.ptr(a_value), L.ptr(a_soft), L.ptr(a_sign), L.ptr(self.record_mask), L.stream_ptr(self.device)),
                "wave_record")

    def step_finish(self, states: GpuStateBatch, plies: torch.Tensor, done: torch.Tensor, step_index: torch.Tensor,
                    step_counts: torch.Tensor, search: RootSearchBatchOutput, lengths: Optional[torch.Tensor] = None,
                    reseated: Optional[torch.Tensor] = None, slot_game: Optional[torch.Tensor] = None) -> None:
        """Play the chosen move of every live slot; finalise (and re-seat, if asked) the games that end."""
        _, _, _, a_value, a_soft, a_sign = self.buffer.arena()
        ts = states.tensors()
        if any(not t.is_contiguous() for t in ts):
            raise RuntimeError("WaveTail.step_finish: state tensors must be contiguous (they are updated in place)")
        codes = search.chosen_action_codes.contiguous()
        term = search.terminal_mask.contiguous() if self.resign is None else self.terminal_out
        cvalid = search.chosen_valid_mask.contiguous()
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_wave_step_finish(
                C.byref(L.soa(ts)), L.i64(self.G), L.ptr(plies), L.ptr(done), L.ptr(codes), L.ptr(term), L.ptr(cvalid),
                L.i64(self.max_plies), C.c_float(self.soft_k), L.ptr(a_value), L.ptr(a_soft), L.ptr(a_sign),
                L.ptr(step_index), L.ptr(step_counts),
                L.i64(self.max_plies if step_index is None else int(step_index.shape[1])), L.ptr(self.outcome),
                L.ptr(self.delta_hist), L.ptr(lengths), L.ptr(slot_game), L.ptr(self.finished), L.ptr(reseated),
                C.c_int(1 if self.reseat else 0), L.ptr(self.game_plies), L.stream_ptr(self.device)), "wave_step_finish")

    def note_value(self, states: GpuStateBatch, plies: torch.Tensor, done: torch.Tensor, step_counts: torch.Tensor,
                   search: RootSearchBatchOutput) -> None:
        """TD(lambda): keep this ply's root value of every live slot (between `record` and `step_finish`)."""
        rv = search.root_value.contiguous()
        if rv.dtype != torch.float32 or int(rv.numel()) != self.G:
            raise RuntimeError("WaveTail.note_value: root_value must be float32[num_slots]")
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_wave_note_value(
                L.ptr(done), L.i64(self.G), L.ptr(plies), L.ptr(self.rows), L.ptr(step_counts), L.ptr(rv),
                L.ptr(states.current_player), L.ptr(self.q_hist), L.ptr(self.step_ply), L.ptr(self.hist_len),
                L.ptr(self.was_live), L.i64(self.max_plies), L.ptr(self.overflow), L.stream_ptr(self.device)),
                "wave_note_value")

    def td_targets(self, done: torch.Tensor, step_index: torch.Tensor, step_counts: torch.Tensor) -> None:
        """TD(lambda): rewrite the value targets of the games that ended this ply (after `step_finish`, before their rows
        leave for a finished-row log)."""
        _, _, _, a_value, _, a_sign = self.buffer.arena()
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_wave_td_targets(
                L.ptr(done), L.ptr(self.was_live), L.i64(self.G), C.c_double(self.td_lambda), L.ptr(self.q_hist),
                L.ptr(self.step_ply), L.ptr(self.hist_len), L.i64(self.max_plies), L.ptr(a_value), L.ptr(a_sign),
                L.ptr(step_index), L.ptr(step_counts),
                L.i64(self.max_plies if step_index is None else int(step_index.shape[1])), L.stream_ptr(self.device)),
                "wave_td_targets")

    def resign_step(self, states: GpuStateBatch, plies: torch.Tensor, done: torch.Tensor, search: RootSearchBatchOutput,
                    slot_game: Optional[torch.Tensor] = None) -> None:
        """Resignation: this ply's rule for every live slot (after `record` / `note_value`, before `step_finish`, which then
        reads `terminal_out`)."""
        rv = search.root_value.contiguous()
        term = search.terminal_mask.contiguous()
        if rv.dtype != torch.float32 or int(rv.numel()) != self.G:
            raise RuntimeError("WaveTail.resign_step: root_value must be float32[num_slots]")
        if term.element_size() != 1 or int(term.numel()) != self.G:
            raise RuntimeError("WaveTail.resign_step: terminal_mask must be one byte per slot")
        r = self.resign
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_wave_resign(
                L.ptr(done), L.i64(self.G), L.ptr(plies), L.ptr(states.phase), L.ptr(states.current_player), L.ptr(rv),
                L.ptr(term), L.ptr(slot_game), L.i64(self.game_base), C.c_uint64(self.seed),
                C.c_float(r["resign_threshold"]), L.i64(r["resign_min_moves"]), C.c_int32(r["resign_consecutive"]),
                C.c_float(r["resign_playthrough_fraction"]), C.c_int(1 if r["resign_streak"] == "ply" else 0),
                L.ptr(self.streak), L.ptr(self.would), L.ptr(self.would_ply), L.ptr(self.terminal_out),
                L.ptr(self.was_live), L.ptr(self.resigned), L.stream_ptr(self.device)), "wave_resign")

    def resign_book(self, states: GpuStateBatch, plies: torch.Tensor, done: torch.Tensor, search: RootSearchBatchOutput,
                    slot_game: Optional[torch.Tensor] = None) -> None:
        """Resignation: book the games that ended this ply (after `step_finish`, before `td_targets` and the log)."""
        cvalid = search.chosen_valid_mask.contiguous()
        if cvalid.element_size() != 1 or int(cvalid.numel()) != self.G:
            raise RuntimeError("WaveTail.resign_book: chosen_valid_mask must be one byte per slot")
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_wave_resign_book(
                C.byref(L.soa(states.tensors())), L.i64(self.G), L.ptr(done), L.ptr(self.was_live), L.ptr(plies),
                L.ptr(self.terminal_out), L.ptr(cvalid), L.ptr(self.resigned), L.ptr(self.would), L.ptr(self.would_ply),
                L.ptr(slot_game), L.i64(self.game_base), C.c_uint64(self.seed),
                C.c_float(self.resign["resign_playthrough_fraction"]), L.ptr(self.resign_counters),
                L.stream_ptr(self.device)), "wave_resign_book")

    def note_surprise(self, done: torch.Tensor, step_counts: torch.Tensor, search: RootSearchBatchOutput,
                      prior: torch.Tensor) -> None:
        """Policy surprise: keep KL(policy target || prior) of the row every live slot recorded this ply (after `record` /
        `note_value`, before `resign_step` / `step_finish`).  `prior` float32[num_slots, action_dim]."""
        lm, pol = search.legal_mask.contiguous(), search.policy_dense.contiguous()
        T = int(pol.shape[1])
        if pol.dtype != torch.float32 or lm.element_size() != 1 or tuple(lm.shape) != (self.G, T):
            raise RuntimeError("WaveTail.note_surprise: policy_dense must be float32 and legal_mask one byte per action")
        if prior.dtype != torch.float32 or tuple(prior.shape) != (self.G, T) or not prior.is_contiguous():
            raise RuntimeError("WaveTail.note_surprise: prior must be contiguous float32[num_slots, action_dim]")
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_wave_note_surprise(
                L.ptr(done), L.i64(self.G), L.ptr(self.rows), L.ptr(step_counts), L.ptr(lm), L.ptr(pol), L.ptr(prior),
                L.i64(T), L.ptr(self.surprise_hist), L.ptr(self.was_live), L.i64(self.max_plies), L.ptr(self.overflow),
                L.stream_ptr(self.device)), "wave_note_surprise")

    def surprise_resample(self, done: torch.Tensor, step_index: torch.Tensor, step_counts: torch.Tensor,
                          slot_game: Optional[torch.Tensor] = None) -> None:
        """Policy surprise: resample, in place, the rows of the games that ended this ply (after `step_finish`,
        `resign_book` and `td_targets`, before their rows leave for a finished-row log)."""
        if step_index is not None and int(step_index.shape[1]) != self.max_plies:
            raise RuntimeError("WaveTail.surprise_resample: the step_index matrix must have max_game_plies columns")
        a_state, a_legal, a_policy, a_value, a_soft, a_sign = self.buffer.arena()
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_wave_surprise_resample(
                L.ptr(done), L.ptr(self.was_live), L.i64(self.G), C.c_double(self.surprise_alpha),
                L.ptr(self.surprise_hist), L.ptr(slot_game), L.i64(self.game_base), C.c_uint64(self.seed),
                L.ptr(a_state), L.ptr(a_legal), L.ptr(a_policy), L.ptr(a_value), L.ptr(a_soft), L.ptr(a_sign),
                L.i64(int(a_policy.shape[1])), L.ptr(step_index), L.ptr(step_counts), L.i64(self.max_plies),
                L.ptr(self.surprise_src), L.ptr(self.surprise_counters), L.ptr(self.surprise_sum),
                L.stream_ptr(self.device)), "wave_surprise_resample")

    def start_capture(self, states: GpuStateBatch, plies: torch.Tensor, done: torch.Tensor, search: RootSearchBatchOutput,
                      slot_game: Optional[torch.Tensor] = None) -> None:
        """The start bank: append a seeded share of this ply's searched positions (after `record` / `note_value` /
        `note_surprise`, before `resign_step` / `step_finish`: the state is still the searched root)."""
        term, cvalid = search.terminal_mask.contiguous(), search.chosen_valid_mask.contiguous()
        if term.element_size() != 1 or int(term.numel()) != self.G or cvalid.element_size() != 1 or int(cvalid.numel()) != self.G:
            raise RuntimeError("WaveTail.start_capture: terminal_mask and chosen_valid_mask must be one byte per slot")
        b, p = self.bank, self.start
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_start_bank_capture(
                C.byref(L.soa(states.tensors())), L.i64(self.G), L.ptr(done), L.ptr(term), L.ptr(cvalid), L.ptr(plies),
                L.ptr(slot_game), L.i64(self.game_base), C.c_uint64(self.seed), C.c_float(p["start_capture_prob"]),
                L.i64(p["start_min_move"]), L.i64(p["start_max_move"]), L.ptr(b.entries), L.i64(b.capacity),
                L.ptr(b.cursor), L.ptr(self.start_counters), L.stream_ptr(self.device)), "start_bank_capture")

    def start_seed(self, states: GpuStateBatch, fresh: torch.Tensor, slot_game: Optional[torch.Tensor] = None) -> None:
        """The start bank: a seeded share of the slots `fresh` marks (uint8 / bool per slot: they start a game with this
        ply's search) takes a bank position instead of the empty board."""
        if fresh.element_size() != 1 or int(fresh.numel()) != self.G or not fresh.is_contiguous():
            raise RuntimeError("WaveTail.start_seed: `fresh` must be one contiguous byte per slot")
        ts = states.tensors()
        if any(not t.is_contiguous() for t in ts):
            raise RuntimeError("WaveTail.start_seed: state tensors must be contiguous (they are updated in place)")
        b = self.bank
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_start_bank_seed(
                C.byref(L.soa(ts)), L.i64(self.G), L.ptr(fresh), L.ptr(slot_game), L.i64(self.game_base),
                C.c_uint64(self.seed), C.c_float(self.start["start_fork_prob"]), L.ptr(b.entries), L.i64(b.capacity),
                L.ptr(b.cursor), L.ptr(self.start_counters), L.stream_ptr(self.device)), "start_bank_seed")

    def start_next_games(self, states: GpuStateBatch, plies: torch.Tensor, done: torch.Tensor, step_counts: torch.Tensor,
                         budget: torch.Tensor, next_game: torch.Tensor, slot_game: torch.Tensor,
                         reseated: Optional[torch.Tensor] = None) -> None:
        """Finished slots restart from the empty board (ascending slot order) while `budget` games remain to be started."""
        with torch.cuda.device(self.device):
            L.check(L.lib().lz_wave_reseat(C.byref(L.soa(states.tensors())), L.i64(self.G), L.ptr(done), L.ptr(plies),
                                           L.ptr(step_counts), L.ptr(budget), L.ptr(next_game), L.ptr(slot_game),
                                           L.ptr(reseated), C.c_int(1 if self.row_log is not None else 0),
                                           L.stream_ptr(self.device)), "wave_reseat")

    def run(self, search_fn, states: GpuStateBatch, plies: torch.Tensor, done: torch.Tensor, step_index: torch.Tensor,
            step_counts: torch.Tensor, lengths: torch.Tensor, t_init: float, t_final: float, t_threshold: int,
            games_to_start: int = 0, temperature_table: Optional[torch.Tensor] = None) -> int:
        """The wave loop with nothing per ply on the host: `search_fn(states, temperatures, done, reseated)` ->
        RootSearchBatchOutput for all slots (finished ones are masked by `done`; `reseated` uint8 marks slots that
        have just started a new game), then record / move / finalise on the device.  `games_to_start` > 0: a slot
        whose game has finished starts the next game at once (lz_wave_reseat) instead of idling until the whole wave
        is done; `lengths` is then indexed by game.  The loop ends on the `all done` flag of TWO plies ago (copied to
        pinned memory behind an event), so the host stays one ply ahead of the device; the price is exactly one
        extra, fully masked ply at the end.  Returns the number of plies launched (including that one).
        With a finished-row log (`row_log`) `step_index` is None, the rows of the games that have ended move to the log
        after every ply, and the loop ends when every game has ended AND is in a log (which the caller then closes).
        With TD(lambda) value targets (`value_target_lambda` < 1) the order per ply is record -> note_value -> step_finish
        -> td_targets -> the log: the rows of a game that ends carry their final targets before they leave.
        With resignation (`resign_threshold` < 0) it is record -> note_value -> resign -> step_finish -> resign_book ->
        td_targets -> the log.
        With policy surprise weighting (`policy_surprise_weight` > 0) the full order is record -> note_value ->
        note_surprise -> resign -> step_finish -> resign_book -> td_targets -> surprise_resample -> the log: a game's rows
        carry their final targets before they are resampled, and are resampled before they leave.  `prior_fn(search)` is
        called once per ply, right after the search (one extra network launch).
        With the start bank (`start_fork_prob` / `start_capture_prob` > 0) start_seed follows the re-seat (and precedes the
        first ply's search, for the slots that are live then), and start_capture follows note_surprise.
        `temperature_table` (float32 on the device, move_pick.temperature_table: the half-life schedule): the temperature of
        a slot is table[min(ply, len - 1)] instead of the t_init / t_final step at `t_threshold`."""
        dev, g = self.device, self.G
        log = self.row_log
        if (log is None) == (step_index is None):
            raise ValueError("WaveTail.run: pass a step_index matrix, or build the tail with a finished-row log")
        if self.surprise_alpha is not None and not callable(self.prior_fn):
            raise RuntimeError("WaveTail.run: policy surprise weighting is on but the tail has no `prior_fn` (search -> the "
                               "noise-free root priors float32[num_slots, action_dim]); pass WaveTail(prior_fn=...), e.g. "
                               "a closure over policy_surprise.root_prior")
        flags = [torch.zeros((1,), dtype=torch.bool).pin_memory() for _ in range(2)]
        live = [torch.full((1,), g, dtype=torch.int64).pin_memory() for _ in range(2)]     # live slots, as of two plies ago
        self.live_estimate = g
        events = [torch.cuda.Event() for _ in range(2)]
        budget = torch.full((1,), int(games_to_start), dtype=torch.int64, device=dev)
        next_game = torch.full((1,), g, dtype=torch.int64, device=dev)
        slot_game = self.slot_game
        slot_game.copy_(torch.arange(g, dtype=torch.int64, device=dev))
        reseated = torch.zeros((g,), dtype=torch.uint8, device=dev)
        forks = self.start is not None and self.start["start_fork_prob"] > 0.0
        captures = self.start is not None and self.start["start_capture_prob"] > 0.0
        ply = 0
        t_run = time.perf_counter()
        while True:
            k = ply & 1
            if ply >= 2:
                t_w = time.perf_counter()
                events[k].synchronize()
                self.host_wait_ms += (time.perf_counter() - t_w) * 1e3      # ~0 for a whole run: the HOST is the bottleneck
                if bool(flags[k].item()):
                    break
                self.live_estimate = int(live[k].item())          # a search may size its launches by it (compact lists)
                if log is not None:
                    log.poll(k)                                   # may switch log arenas (a segment leaves)
            if games_to_start > 0 and ply > 0:
                self.start_next_games(states, plies, done, step_counts, budget, next_game, slot_game, reseated)
                if forks:
                    self.start_seed(states, reseated, slot_game=slot_game)
            if forks and ply == 0:                      # a bank filled by an earlier call seeds the first wave too
                self.start_seed(states, ~done if done.dtype == torch.bool else (done == 0), slot_game=slot_game)
            if temperature_table is not None:
                temps = temperature_table.index_select(0, plies.clamp(0, int(temperature_table.numel()) - 1))
            else:
                temps = torch.where(plies < int(t_threshold), float(t_init), float(t_final)).to(torch.float32)
            search = search_fn(states, temps, done, reseated)
            reseated.zero_()
            with self._bracket("finalize_ms"):
                self.record(states, done, step_index, step_counts, search)
                if self.td_lambda is not None:
                    self.note_value(states, plies, done, step_counts, search)
                if self.surprise_alpha is not None:
                    self.note_surprise(done, step_counts, search, self.prior_fn(search))
                if captures:
                    self.start_capture(states, plies, done, search, slot_game=slot_game)
            with self._bracket("self_play_step_ms"):
                if self.resign is not None:
                    self.resign_step(states, plies, done, search, slot_game=slot_game)
                self.step_finish(states, plies, done, step_index, step_counts, search, lengths=lengths, slot_game=slot_game)
                if self.resign is not None:
                    self.resign_book(states, plies, done, search, slot_game=slot_game)
            if self.td_lambda is not None:
                with self._bracket("finalize_ms"):
                    self.td_targets(done, step_index, step_counts)
            if self.surprise_alpha is not None:
                with self._bracket("finalize_ms"):
                    self.surprise_resample(done, step_index, step_counts, slot_game=slot_game)
            # all finished and nothing left to start (a finished slot restarts at the top of the next ply otherwise)
            if log is not None:
                if ply == 0:
                    log.bind(self.buffer.arena())
                log.after_ply(done, step_counts, k)
                flags[k].copy_((done.all() & (budget <= 0).all() & (log.waiting() == 0)).view(1), non_blocking=True)
            else:
                flags[k].copy_((done.all() & (budget <= 0).all()).view(1), non_blocking=True)
            live[k].copy_((~done).sum().view(1), non_blocking=True)
            events[k].record(torch.cuda.current_stream(dev))
            ply += 1
        self.loop_ms += (time.perf_counter() - t_run) * 1e3
        self.plies_launched += ply
        return ply

    def check_overflow(self) -> None:
        n = int(self.overflow.item())
        if n:
            raise RuntimeError(f"WaveTail: {n} trajectory rows were dropped (arena or step-index capacity too small)")
