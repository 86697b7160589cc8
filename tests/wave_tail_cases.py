"""Inputs of tests/test_gpu_wave_tail.py (numpy only, seeded): the waves the kernels lz_wave_record / lz_wave_step_finish /
lz_wave_reseat are given, and the coverage each of them must reach.  tests/test_wave_tail_ref_cpu.py builds the same
inputs on the host alone and checks that coverage there, so that a GPU run never finds its cases missing."""
import functools

import numpy as np

from oracle import lz_oracle as O
from tests.golden_utils import FIELDS, load, states

SCAN_THREADS = 1024                                       # the ordered scans run in one workgroup of this size
SENT_F32 = 0x7FC12345                                     # a quiet NaN with a marked payload: "nobody wrote here"
SENT_I64 = 0x7F7F7F7F7F7F7F7F
RECORD_TMAX = 6
RECORD_G = (1, 64, 65, 1023, 1024, 1025, 2049, 16385)
RESEAT_G = (1, 65, 1024, 1025, 2049, 16385)


def sentinel_f32(shape):
    return np.full(shape, SENT_F32, np.int32).view(np.float32)


def random_f32(r, shape):
    """float32 with random bits (NaNs and denormals included): a copy must keep every bit."""
    return r.integers(-(1 << 31), 1 << 31, shape, dtype=np.int64).astype(np.int32).view(np.float32)


def cut_slot(G):
    """The first slot that the capacity cut leaves without a row.  G = 2049 (3 slots per scan thread): the middle slot of
    thread 341's run; G = 16385 (17 slots per thread): the first slot of scan wave 8, so the cut falls between two waves
    of the scan."""
    per = -(-G // SCAN_THREADS)
    return {2049: 341 * per + 1, 16385: 8 * 64 * per}.get(G, G // 2)


def record_case(G, slot_major, mask, done_kind, cut, T=220, seed=0):
    """One launch of lz_wave_record.  mask: None / "half" / "zero"; done_kind: "random" (~30 % done) / "live" / "done";
    cut: the capacity ends in the middle of the wave (cursor layout only)."""
    r = np.random.default_rng([seed, G, int(slot_major), {None: 0, "half": 1, "zero": 2}[mask], int(cut), T])
    Tmax = RECORD_TMAX
    done = {"random": (r.random(G) < 0.3), "live": np.zeros(G, bool), "done": np.ones(G, bool)}[done_kind].astype(np.uint8)
    record = None if mask is None else ((r.random(G) < 0.5) if mask == "half" else np.zeros(G, bool)).astype(np.uint8)
    s = cut_slot(G)
    if done_kind == "random":                             # the slots around the cut are live and record
        done[max(s - 1, 0):s + 2] = 0
        if mask == "half":
            record[max(s - 1, 0):s + 2] = 1
    step_counts = r.integers(0, Tmax + 1, G).astype(np.int64)            # several slots sit exactly at Tmax
    rec = (done == 0) & (record != 0 if record is not None else True)
    rank = np.cumsum(rec) - rec
    cursor = None if slot_major else 37
    if slot_major:
        capacity = G * Tmax
    elif cut:
        capacity = 37 + int(rank[s])
    else:
        capacity = 37 + int(rec.sum()) + 3
    over_cap = rec & (37 + rank >= capacity) if not slot_major else np.zeros(G, bool)
    over_steps = rec & ~over_cap & (step_counts >= Tmax)
    return dict(G=G, T=T, Tmax=Tmax, done=done, record=record, step_counts=step_counts, cursor=cursor, capacity=capacity,
                rows_total=capacity + max(G, 64), overflow=5, over_cap=int(over_cap.sum()), over_steps=int(over_steps.sum()),
                recorded=int(rec.sum()), model_input=random_f32(r, (G, 11, 6, 6)),
                legal=r.integers(0, 256, (G, T), dtype=np.uint8), policy=random_f32(r, (G, T)),
                player=r.choice(np.array([-1, 1, 1, -1, 0], np.int64), G))   # a stray 0 counts as Black (sign +1)


def seeded_moves(st, r):
    """One legal action per state, drawn uniformly: (codes int32[N, 4], has_move bool[N])."""
    mask, meta = O.encode_actions(st)
    pick = (r.random(mask.shape) * mask).argmax(1)
    return np.ascontiguousarray(meta[np.arange(mask.shape[0]), pick]), mask.any(1)


def ending_kind(nxt, plies_after, max_plies):
    """Why a game ends after its move, when exactly one reason holds: 'black' / 'white' (the winner), 'moves', 'nocapture',
    'cap'; 'on' if it goes on, 'mixed' otherwise."""
    ph = nxt["phase"]
    post = (ph == 4) | (ph == 5) | (ph == 7)
    b = np.asarray(nxt["board"]).reshape(-1, 36)
    white = post & ((b == 1).sum(1) < O.LOSE_PIECE_THRESHOLD)
    black = post & ((b == -1).sum(1) < O.LOSE_PIECE_THRESHOLD)
    moves = nxt["move_count"] >= O.MAX_MOVE_COUNT
    nocap = nxt["moves_since_capture"] >= O.NO_CAPTURE_DRAW_LIMIT
    cap = np.asarray(plies_after) >= max_plies
    n = white.astype(int) + black + moves + nocap + cap
    kind = np.full(ph.shape[0], "mixed", dtype=object)
    kind[n == 0] = "on"
    for name, m in (("white", white), ("black", black), ("moves", moves), ("nocapture", nocap), ("cap", cap)):
        kind[(n == 1) & m] = name
    return kind


STEP_KINDS = ("terminal_black_to_move", "terminal_white_to_move", "no_valid", "black", "white", "moves", "nocapture",
              "cap", "on", "idle")


@functools.lru_cache(maxsize=None)
def step_case():
    """One launch of lz_wave_step_finish over ~1600 slots that meets every ending (see STEP_KINDS) at least three times.
    States: g15_rules_large.npz with a seeded legal move each -- all the moves that win or reach a draw limit among eight
    draws per state, the rest drawn at random -- plus g16_garbage_large.npz boards with every piece turned to one colour
    (g16 itself holds no board beyond +-18) and no valid choice, for the clamp of the piece-delta histogram."""
    r = np.random.default_rng(20)
    max_plies, Tmax = 96, 65
    pool = states(load("g15_rules_large.npz"), "s")
    N = pool["phase"].shape[0]
    src, codes, kinds = [], [], []
    for _ in range(8):
        c, has = seeded_moves(pool, r)
        assert has.all()
        nxt = O.apply_moves(pool, c, np.arange(N))
        k = ending_kind(nxt, np.zeros(N), max_plies)
        for name in ("black", "white", "moves", "nocapture"):
            hit = np.flatnonzero(k == name)[:12]
            src.append(hit); codes.append(c[hit]); kinds += [name] * hit.size
        on = r.permutation(np.flatnonzero(k == "on"))[:165]
        src.append(on); codes.append(c[on]); kinds += ["on"] * on.size
    src, codes, kinds = np.concatenate(src), np.concatenate(codes), np.array(kinds, dtype=object)
    order = r.permutation(src.size)
    src, codes, kinds = src[order], codes[order], kinds[order]
    st = O.select_states(pool, src)
    G0 = src.size
    plies = r.integers(0, max_plies - 1, G0).astype(np.int64)
    terminal, cvalid, done = np.zeros(G0, np.uint8), np.ones(G0, np.uint8), np.zeros(G0, np.uint8)
    on = np.flatnonzero(kinds == "on")
    cap, term, noval, idle = on[:9], on[9:29], on[29:38], on[38:47]
    plies[cap] = max_plies - 1
    kinds[cap] = "cap"
    terminal[term] = 1
    terminal[term[:3]] = 0x80                                 # any non-zero byte counts
    cvalid[term[10:]] = 0                                     # a terminal root wins over a missing choice
    kinds[term] = np.where(st["current_player"][term] > 0, "terminal_black_to_move", "terminal_white_to_move")
    cvalid[noval] = 0
    kinds[noval] = "no_valid"
    done[idle] = 1
    done[idle[:3]] = 0x80
    kinds[idle] = "idle"
    # garbage boards beyond +-18
    gar = states(load("g16_garbage_large.npz"), "s")
    pieces = (np.asarray(gar["board"]).reshape(-1, 36) != 0).sum(1)
    pick = np.flatnonzero(pieces > 18)[:8]
    assert pick.size == 8
    extra = O.select_states(gar, pick)
    extra["board"] = np.where(extra["board"] != 0, np.where(np.arange(8) % 2 == 0, 1, -1)[:, None, None], 0).astype(np.int8)
    st = O.concat_states([st, extra])
    G = G0 + 8
    plies = np.concatenate([plies, r.integers(0, 50, 8)]).astype(np.int64)
    terminal, done = np.concatenate([terminal, np.zeros(8, np.uint8)]), np.concatenate([done, np.zeros(8, np.uint8)])
    cvalid = np.concatenate([cvalid, np.zeros(8, np.uint8)])
    codes = np.concatenate([codes, np.full((8, 4), -1, np.int32)])
    kinds = np.concatenate([kinds, np.array(["no_valid"] * 8, dtype=object)])
    # recorded steps: mostly a few, and the lane-stride edges 0, 1, 64, 65 and one count above Tmax
    step_counts = r.integers(0, 13, G).astype(np.int64)
    for name in STEP_KINDS:                                   # every kind meets every edge count once
        slots = np.flatnonzero(kinds == name)
        step_counts[slots[:5]] = [0, 1, 64, 65, 70][:slots[:5].size]
    rows_needed = int(np.minimum(step_counts, Tmax).sum())
    R = rows_needed + rows_needed // 3 + G
    perm = r.permutation(R - G)                               # the last G rows are the guard band
    step_index = np.full((G, Tmax), -7, np.int64)
    p = 0
    for g in range(G):
        n = min(int(step_counts[g]), Tmax)
        step_index[g, :n] = perm[p:p + n]
        p += n
    return dict(G=G, Tmax=Tmax, max_plies=max_plies, k=2.0, states=st, plies=plies, done=done, codes=codes,
                terminal=terminal, cvalid=cvalid, kinds=kinds, step_counts=step_counts, step_index=step_index, R=R,
                signs=r.choice(np.array([-1, 1], np.int8), R), signs_slot=r.choice(np.array([-1, 1], np.int8), G * Tmax + G),
                slot_game=r.permutation(G).astype(np.int64))


def step_kinds_of_result(case, st_after, plies_after, done_after):
    """The ending of every slot as the restatement's result shows it (the coverage the GPU test asserts before comparing):
    from the state the slot was left in, not from how the case was put together."""
    kind = ending_kind(st_after, plies_after, case["max_plies"])
    live = case["done"] == 0
    term = live & (case["terminal"] != 0)
    noval = live & ~term & (case["cvalid"] == 0)
    kind[term] = np.where(case["states"]["current_player"][term] > 0, "terminal_black_to_move", "terminal_white_to_move")
    kind[noval] = "no_valid"
    kind[~live] = "idle"
    moved = live & ~term & ~noval
    assert np.array_equal(done_after[moved] != 0, kind[moved] != "on")
    return kind


def reseat_case(G, seed=0):
    """Non-empty states, about half the slots finished, rows left (step_counts > 0) on a third of the finished slots."""
    r = np.random.default_rng([seed, G, 77])
    pool = states(load("g15_rules_large.npz"), "s")
    st = O.select_states(pool, r.integers(0, pool["phase"].shape[0], G))
    done = (r.random(G) < 0.5).astype(np.uint8)
    if G == 1:
        done[:] = 1
    done[done != 0] = r.choice(np.array([1, 0x80, 0xFF], np.uint8), int((done != 0).sum()))
    step_counts = np.where(r.random(G) < 1 / 3, r.integers(1, 9, G), 0).astype(np.int64)
    step_counts[done == 0] = r.integers(0, 9, int((done == 0).sum()))
    return dict(G=G, states=st, done=done, step_counts=step_counts, plies=r.integers(1, 90, G).astype(np.int64),
                slot_game=r.integers(0, 1 << 20, G).astype(np.int64), next_game=(3 << 32) + 11)


def reseat_budgets(case, logged_only):
    eligible = int(((case["done"] != 0) & ~((case["step_counts"] > 0) & bool(logged_only))).sum())
    return eligible, (0, 1, eligible // 2, eligible + 5)


def copy_states(st):
    return {f: np.array(st[f]) for f in FIELDS}


class ScriptedTail:
    """record -> step_finish -> reseat for 12 plies on the host (tests/wave_tail_ref.py): 70 slots, 8 steps per slot, ply
    cap 10.  The "search" of a ply (`inputs`) is a seeded legal move per slot with random rows as its sample; `advance`
    plays it.  Slots live longer than 8 plies (the step overflow), the cursor arena is too small for the last plies (the
    capacity overflow), 25 further games start in finished slots.  Slot-major run: a record mask, game_plies, and the
    step_counts of finished slots cleared between plies as the finished-row log does."""
    G, TMAX, PLIES, T, MAX_PLIES, K, EXTRA = 70, 8, 12, 220, 10, 2.0, 25

    def __init__(self, slot_major):
        from tests.wave_tail_ref import ref_record, ref_reseat, ref_step_finish
        self._ref = (ref_record, ref_step_finish, ref_reseat)
        G, Tmax = self.G, self.TMAX
        self.slot_major = bool(slot_major)
        self.r = r = np.random.default_rng(11 + int(slot_major))
        pool = states(load("g15_rules_large.npz"), "s")
        self.st = O.concat_states([O.initial_states(35), O.select_states(pool, r.integers(0, pool["phase"].shape[0], 35))])
        self.plies = np.concatenate([np.zeros(35, np.int64), r.integers(0, 6, 35)]).astype(np.int64)
        self.done, self.counts = np.zeros(G, np.uint8), np.zeros(G, np.int64)
        self.capacity = G * Tmax if slot_major else 600
        self.R = self.capacity + G
        self.arena = (sentinel_f32((self.R, 396)), np.full((self.R, self.T), 0x7F, np.uint8),
                      sentinel_f32((self.R, self.T)), sentinel_f32(self.R), sentinel_f32(self.R),
                      np.full(self.R, 0x7F, np.int8))
        self.index = None if slot_major else np.full((G, Tmax), -7, np.int64)
        self.rows = np.full(G, SENT_I64, np.int64)
        self.games = G + self.EXTRA
        self.outcome, self.hist = np.zeros(3, np.int64), np.zeros(37, np.int64)
        self.lengths = np.full(self.games + G, -7, np.int64)                  # G spare entries past the last game
        self.game_plies = np.full(self.games + G, -7, np.int64) if slot_major else None
        self.slot_game, self.reseated = np.arange(G, dtype=np.int64), np.zeros(G, np.uint8)
        self.cursor = None if slot_major else 0
        self.overflow, self.finished, self.budget, self.next_game = 0, 0, self.EXTRA, G
        self.step_overflows = 0

    def inputs(self):
        G, T, r = self.G, self.T, self.r
        codes, has = seeded_moves(self.st, r)
        return dict(codes=codes, terminal=(~has | (r.random(G) < 0.03)).astype(np.uint8),
                    cvalid=(has & (r.random(G) >= 0.03)).astype(np.uint8), model_input=random_f32(r, (G, 11, 6, 6)),
                    legal=r.integers(0, 256, (G, T), dtype=np.uint8), policy=random_f32(r, (G, T)),
                    record=(r.random(G) < 0.8).astype(np.uint8) if self.slot_major else None)

    def advance(self, x):
        ref_record, ref_step_finish, ref_reseat = self._ref
        rec = (self.done == 0) & (x["record"] != 0 if x["record"] is not None else True)
        self.step_overflows += int((rec & (self.counts >= self.TMAX)).sum())
        self.reseated[:] = 0
        self.cursor, self.overflow = ref_record(
            self.done, self.cursor, self.capacity, self.TMAX, self.index, self.counts, self.rows, self.overflow,
            x["model_input"], x["legal"], x["policy"], self.st["current_player"].copy(), self.arena, x["record"])
        self.finished = ref_step_finish(
            self.st, self.plies, self.done, x["codes"], x["terminal"], x["cvalid"], self.MAX_PLIES, self.K, self.arena[3],
            self.arena[4], self.arena[5], self.index, self.counts, self.TMAX, self.outcome, self.hist, self.lengths,
            self.slot_game, self.finished, None, False, self.game_plies)
        if self.slot_major:
            self.counts[self.done != 0] = 0
        self.budget, self.next_game = ref_reseat(self.st, self.done, self.plies, self.counts, self.budget, self.next_game,
                                                 self.slot_game, self.reseated, self.slot_major)

    def check_coverage(self):
        assert self.step_overflows > 0 and self.overflow >= self.step_overflows
        if not self.slot_major:
            assert self.cursor > self.capacity and self.overflow > self.step_overflows      # the arena ran full as well
        assert self.finished >= self.EXTRA and self.budget == 0 and self.next_game == self.games
        assert (self.outcome > 0).all() and int(self.outcome.sum()) <= self.finished
