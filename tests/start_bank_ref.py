"""Sequential restatement of the start bank (csrc/lz_start_bank.h, lz_start_bank_capture / lz_start_bank_seed) in numpy,
built on oracle/rng_oracle.draw, and the cases the CPU and GPU tests share.  States are the oracle's dicts of arrays
(tests/golden_utils.FIELDS); a packed state is the 32-byte record of csrc/lz_rules.h, four little-endian 64-bit words."""
import functools

import numpy as np

from oracle import lz_oracle as O
from oracle import rng_oracle as R
from tests.golden_utils import FIELDS, load, states

PURPOSE, INDEX_CAPTURE, INDEX_FORK = 3, 1020, 1021
SENT = 0x7F                                                # the byte unwritten bank rows are filled with
CAPTURE_G = (1, 64, 65, 1030, 2500)
SCAN_THREADS = 1024
_BITS = np.uint64(1) << np.arange(36, dtype=np.uint64)


def _bitboard(cells):
    return (np.asarray(cells).reshape(-1, 36).astype(bool) * _BITS).sum(1, dtype=np.uint64)


def pack_states(st):
    """uint8[N, 32]: lz::pack of every state."""
    b = np.asarray(st["board"]).reshape(-1, 36)
    f = lambda name, mask, shift: (np.asarray(st[name]).astype(np.int64).astype(np.uint64) & np.uint64(mask)) << np.uint64(shift)
    w0 = (_bitboard(b == 1) | f("move_count", 0xFF, 36) | f("moves_since_capture", 0x3F, 44) | f("phase", 7, 50) |
          ((np.asarray(st["current_player"]) < 0).astype(np.uint64) << np.uint64(53)) | f("forced_removals_done", 3, 54) |
          f("pending_marks_required", 3, 56) | f("pending_marks_remaining", 3, 58) | f("pending_captures_required", 3, 60) |
          f("pending_captures_remaining", 3, 62))
    words = np.stack([w0, _bitboard(b == -1), _bitboard(np.asarray(st["marks_black"]) != 0),
                      _bitboard(np.asarray(st["marks_white"]) != 0)], axis=1)
    return np.ascontiguousarray(words.astype("<u8")).view(np.uint8).reshape(-1, 32)


def unpack_states(packed):
    """lz::unpack of uint8[N, 32] records -> a state dict."""
    w = np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1, 32).view("<u8").astype(np.uint64)
    n = w.shape[0]
    cells = lambda x: ((x[:, None] >> np.arange(36, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    f = lambda shift, mask: ((w[:, 0] >> np.uint64(shift)) & np.uint64(mask)).astype(np.int64)
    st = O.empty_states(n)
    st["board"] = (cells(w[:, 0]).astype(np.int8) - cells(w[:, 1]).astype(np.int8)).reshape(n, 6, 6)
    st["marks_black"], st["marks_white"] = cells(w[:, 2]).reshape(n, 6, 6), cells(w[:, 3]).reshape(n, 6, 6)
    st["move_count"], st["moves_since_capture"], st["phase"] = f(36, 0xFF), f(44, 0x3F), f(50, 7)
    st["current_player"] = np.where(f(53, 1) != 0, -1, 1).astype(np.int64)
    st["forced_removals_done"], st["pending_marks_required"], st["pending_marks_remaining"] = f(54, 3), f(56, 3), f(58, 3)
    st["pending_captures_required"], st["pending_captures_remaining"] = f(60, 3), f(62, 3)
    return st


def capture_draws(seed, games, plies, capture_prob):
    """bool[N]: u01(draw(seed, game, ply, purpose 3, index 1020, 0).x) < capture_prob (float32 compare)."""
    return R.u01(R.draw(seed, games, plies, PURPOSE, INDEX_CAPTURE, 0)[:, 0]) < np.float32(capture_prob)


def fork_entries(seed, games, fork_prob, filled):
    """int64[N]: the bank entry every game forks from, -1 where it starts from the empty board."""
    games = np.asarray(games, np.int64).reshape(-1)
    if filled <= 0:
        return np.full(games.shape[0], -1, np.int64)
    r = R.draw(seed, games, 0, PURPOSE, INDEX_FORK, 0)
    forks = R.u01(r[:, 0]) < np.float32(fork_prob)
    j = [(int(y) * int(filled)) >> 32 for y in r[:, 1]]      # integers only
    return np.where(forks, np.array(j, np.int64), -1)


class BankRef:
    """entries uint8[capacity, 32] (sentinel-filled), cursor, counters int64[3] = forked games, their move counts, captured."""

    def __init__(self, capacity, total=0, counters=(0, 0, 0)):
        self.capacity, self.cursor = int(capacity), int(total)
        self.entries = np.full((self.capacity, 32), SENT, np.uint8)
        self.counters = np.array(counters, np.int64)

    def filled(self):
        return min(self.cursor, self.capacity)

    def append(self, packed):
        """The ring rule, one record after the other (the last writer of a row stays)."""
        for r, rec in enumerate(packed):
            self.entries[(self.cursor + r) % self.capacity] = rec
        self.cursor += len(packed)

    def capture(self, st, done, terminal, cvalid, plies, slot_game, game_base, seed, capture_prob, min_move, max_move):
        """lz_start_bank_capture: one loop over the slots in ascending order.  Returns the candidate mask."""
        G = len(done)
        if not capture_prob > 0:
            return np.zeros(G, bool)
        games = (np.arange(G, dtype=np.int64) if slot_game is None else np.asarray(slot_game, np.int64)) + int(game_base)
        mc = np.asarray(st["move_count"], np.int64)
        cand = ((np.asarray(done) == 0) & (np.asarray(terminal) == 0) & (np.asarray(cvalid) != 0) & (mc >= min_move) &
                (mc <= max_move) & capture_draws(seed, games, plies, capture_prob))
        idx = np.flatnonzero(cand)
        if idx.size:
            self.append(pack_states(O.select_states(st, idx)))
            self.counters[2] += idx.size
        return cand

    def seed(self, st, fresh, slot_game, game_base, seed, fork_prob):
        """lz_start_bank_seed, in place on `st`.  Returns the entry of every slot (-1: untouched)."""
        G = len(fresh)
        games = (np.arange(G, dtype=np.int64) if slot_game is None else np.asarray(slot_game, np.int64)) + int(game_base)
        j = np.where(np.asarray(fresh) != 0, fork_entries(seed, games, fork_prob, self.filled()), -1)
        idx = np.flatnonzero(j >= 0)
        if idx.size:
            new = unpack_states(self.entries[j[idx]])
            for f in FIELDS:
                st[f][idx] = new[f].astype(st[f].dtype)
            self.counters[0] += idx.size
            self.counters[1] += int(new["move_count"].sum())
        return j


# ---- the shared cases ------------------------------------------------------------------------------------------------------
SEED = 12345


@functools.lru_cache(maxsize=None)
def pool():
    return states(load("g15_rules_large.npz"), "s")


def pool_states(r, n):
    p = pool()
    return O.select_states(p, r.integers(0, p["phase"].shape[0], n))


def capture_case(G, kind="mixed"):
    """One launch of lz_start_bank_capture.  kind: "mixed" (done / terminal / invalid pick / out of the move window, ~60 %
    of the rest drawn), "all" (every slot a candidate: capture_prob = 1, the whole window), "none" (no slot passes)."""
    r = np.random.default_rng([31, G, ("mixed", "all", "none").index(kind)])
    st = pool_states(r, G)
    flag = lambda p: np.where(r.random(G) < p, r.choice(np.array([1, 0x80, 0xFF], np.uint8), G), 0).astype(np.uint8)
    done, terminal = flag(0.15), flag(0.1)
    cvalid = np.where(r.random(G) < 0.1, 0, r.choice(np.array([1, 0x80], np.uint8), G)).astype(np.uint8)
    prob, lo, hi = 0.6, 20, 100
    if kind == "all":
        done[:], terminal[:], cvalid[:], prob, lo, hi = 0, 0, 1, 1.0, 0, 143
    if kind == "none":
        terminal[r.random(G) < 0.5] = 1
        done[terminal == 0] = 1
    return dict(G=G, states=st, done=done, terminal=terminal, cvalid=cvalid, plies=r.integers(0, 140, G).astype(np.int64),
                slot_game=r.integers(0, 1 << 40, G).astype(np.int64), game_base=(1 << 33) + 5, seed=SEED + G,
                capture_prob=prob, min_move=lo, max_move=hi)


def capture_totals(capacity):
    return (0, capacity - 1, 5 * capacity + 2)


def seed_case(G):
    """Slots in the middle of other games, a fresh mask of ~half of them, random plies / step_counts / done."""
    r = np.random.default_rng([37, G])
    fresh = np.where(r.random(G) < 0.5, r.choice(np.array([1, 0x80, 0xFF], np.uint8), G), 0).astype(np.uint8)
    if G == 1:
        fresh[:] = 1
    return dict(G=G, states=pool_states(r, G), fresh=fresh, slot_game=r.integers(0, 1 << 40, G).astype(np.int64),
                plies=r.integers(0, 90, G).astype(np.int64), step_counts=r.integers(0, 9, G).astype(np.int64),
                done=(r.random(G) < 0.3).astype(np.uint8), seed=SEED + G)


@functools.lru_cache(maxsize=None)
def playout_positions():
    """7 distinct reachable positions of one fixed-seed oracle playout: the phases placement, mark selection, removal,
    movement and capture selection are all among them.  Returns (states dict of 7, uint8[7, 32])."""
    r = np.random.default_rng(2024)
    st, seen, want = O.initial_states(1), {}, (1, 1, 2, 3, 4, 4, 5)
    for _ in range(143):
        mask, meta = O.encode_actions(st)
        if not mask.any():
            break
        a = int(r.choice(np.flatnonzero(mask[0])))
        st = O.apply_moves(st, np.ascontiguousarray(meta[:, a]), np.arange(1))
        ph = int(st["phase"][0])
        have = seen.setdefault(ph, [])
        if len(have) < want.count(ph) and (ph != 1 or int(st["move_count"][0]) in (5, 17)):
            have.append(O.select_states(st, [0]))
    picked = [s for ph in (1, 2, 3, 4, 5) for s in seen.get(ph, [])]
    assert len(picked) == 7, {k: len(v) for k, v in seen.items()}
    out = O.concat_states(picked)
    packed = pack_states(out)
    assert len({bytes(p) for p in packed}) == 7
    return out, packed


# ---- one launch through the C ABI (the HIP library on a device, or its host twin on CPU tensors), held to the restatement
def to_device(st, device):
    import torch
    out = []
    for f in FIELDS:
        a = np.ascontiguousarray(st[f])
        a = a.astype(np.int8) if f == "board" else a.astype(bool) if f.startswith("marks") else a.astype(np.int64)
        out.append(torch.from_numpy(a).to(device))
    return out


def from_device(ts):
    return {f: t.cpu().numpy() for f, t in zip(FIELDS, ts)}


def tensor(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _sync(device):
    import torch
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def call_capture(L, lib, device, ts, done, terminal, cvalid, plies, slot_game, game_base, seed, capture_prob, min_move,
                 max_move, entries, capacity, cursor, counters, G=None):
    import ctypes as C
    import torch
    st = lib.lz_start_bank_capture(
        C.byref(L.soa(ts)) if ts is not None else None, L.i64(len(done) if G is None else G), L.ptr(done), L.ptr(terminal),
        L.ptr(cvalid), L.ptr(plies), L.ptr(slot_game), L.i64(game_base), C.c_uint64(seed), C.c_float(capture_prob),
        L.i64(min_move), L.i64(max_move), L.ptr(entries), L.i64(capacity), L.ptr(cursor), L.ptr(counters),
        L.stream_ptr(torch.device(device)))
    _sync(device)
    return st


def call_seed(L, lib, device, ts, fresh, slot_game, game_base, seed, fork_prob, entries, capacity, cursor, counters, G=None):
    import ctypes as C
    import torch
    st = lib.lz_start_bank_seed(
        C.byref(L.soa(ts)) if ts is not None else None, L.i64(len(fresh) if G is None else G), L.ptr(fresh),
        L.ptr(slot_game), L.i64(game_base), C.c_uint64(seed), C.c_float(fork_prob), L.ptr(entries), L.i64(capacity),
        L.ptr(cursor), L.ptr(counters), L.stream_ptr(torch.device(device)))
    _sync(device)
    return st


def assert_bytes(got, want, name):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.ascontiguousarray(got)
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, name
    a, b = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        raise AssertionError(f"{name}: {bad.size} bytes differ, first at byte {int(bad[0])}")


def assert_states(ts, want, name):
    from tests.golden_utils import states_equal
    ok, field = states_equal(from_device(ts), want)
    assert ok, f"{name}: {field}"


def run_capture(L, lib, device, c, capacity, total, capture_prob=None, with_slot_game=True):
    """One capture launch on a sentinel-filled bank against BankRef: entries over their whole length, cursor, counters,
    and the states and masks it must not touch.  Returns the number of candidates."""
    prob = c["capture_prob"] if capture_prob is None else capture_prob
    ref = BankRef(capacity, total, counters=(3, 5, 7))
    slot_game = c["slot_game"] if with_slot_game else None
    ts = to_device(c["states"], device)
    d = {k: tensor(c[k], device) for k in ("done", "terminal", "cvalid", "plies")}
    d_game = tensor(slot_game, device)
    entries, cursor = tensor(ref.entries, device), tensor(np.array([total], np.int64), device)
    counters = tensor(ref.counters, device)
    L.check(call_capture(L, lib, device, ts, d["done"], d["terminal"], d["cvalid"], d["plies"], d_game, c["game_base"],
                         c["seed"], prob, c["min_move"], c["max_move"], entries, capacity, cursor, counters),
            "start_bank_capture")
    cand = ref.capture(c["states"], c["done"], c["terminal"], c["cvalid"], c["plies"], slot_game, c["game_base"], c["seed"],
                       prob, c["min_move"], c["max_move"])
    where = f"G={c['G']} capacity={capacity} total={total}: "
    assert_bytes(entries, ref.entries, where + "entries")
    assert int(cursor.item()) == ref.cursor == total + int(cand.sum()), where + "cursor"
    assert_bytes(counters, ref.counters, where + "counters")
    assert_states(ts, c["states"], where + "states")
    for k in d:
        assert_bytes(d[k], c[k], where + k)
    return int(cand.sum())


def seed_bank(capacity, filled, total=None):
    """A bank whose first `filled` rows hold the playout's positions (cycled), the rest the sentinel."""
    ref = BankRef(capacity, filled if total is None else total)
    packed = playout_positions()[1]
    for i in range(filled):
        ref.entries[i] = packed[i % len(packed)]
    return ref


def run_seed(L, lib, device, c, ref, fork_prob, game_base=0, slot_game="case"):
    """One seed launch against BankRef: all twelve state tensors over their whole length, the counters, and the bank it
    must only read.  Returns the entry of every slot (-1 = untouched)."""
    ref.counters = np.array([3, 5, 7], np.int64)
    slot_game = c["slot_game"] if isinstance(slot_game, str) else slot_game
    want = {f: np.array(c["states"][f]) for f in FIELDS}
    ts = to_device(c["states"], device)
    fresh, d_game = tensor(c["fresh"], device), tensor(slot_game, device)
    entries, cursor = tensor(ref.entries, device), tensor(np.array([ref.cursor], np.int64), device)
    counters = tensor(ref.counters, device)
    L.check(call_seed(L, lib, device, ts, fresh, d_game, game_base, c["seed"], fork_prob, entries, ref.capacity, cursor,
                      counters), "start_bank_seed")
    before = ref.entries.copy()
    j = ref.seed(want, c["fresh"], slot_game, game_base, c["seed"], fork_prob)
    where = f"G={c['G']} filled={ref.filled()} fork_prob={fork_prob}: "
    assert_states(ts, want, where + "states")
    assert_bytes(counters, ref.counters, where + "counters")
    assert_bytes(entries, before, where + "entries")
    assert int(cursor.item()) == ref.cursor, where + "cursor"
    assert_bytes(fresh, c["fresh"], where + "fresh")
    keep = j < 0                                              # slots that do not fork keep their bytes
    if keep.any():
        assert_states([t[torch_index(keep, device)] for t in ts], O.select_states(c["states"], keep), where + "untouched slots")
    return j


def torch_index(mask, device):
    import torch
    return torch.from_numpy(np.flatnonzero(mask)).to(device)


def scripted_bank_tail():
    """tests/wave_tail_cases.ScriptedTail cut down to 8 slots (cursor layout), with a bank of 3 rows beside it: per ply
    record -> capture -> step_finish -> reseat -> seed, which is the tail's order reseat -> seed -> search -> record ->
    capture -> step seen from one ply later.  `capture(x)` before and `seed()` after the tail's own `advance(x)`."""
    from tests.wave_tail_cases import ScriptedTail

    class ScriptedBankTail(ScriptedTail):
        CAPACITY, CAPTURE_PROB, FORK_PROB, MIN_MOVE, MAX_MOVE, RUN_SEED, GAME_BASE = 3, 0.5, 0.6, 1, 143, SEED, 1 << 34

        def __init__(self):
            super().__init__(False)
            G = self.G = 8
            keep = np.r_[0:4, 35:39]                          # four empty boards, four games under way
            self.st = O.select_states(self.st, keep)
            self.plies, self.done, self.counts = self.plies[keep].copy(), self.done[:G].copy(), self.counts[:G].copy()
            self.index, self.rows = self.index[:G].copy(), self.rows[:G].copy()
            self.games = G + self.EXTRA
            self.lengths = self.lengths[:self.games + G].copy()
            self.slot_game, self.reseated, self.next_game = np.arange(G, dtype=np.int64), np.zeros(G, np.uint8), G
            self.bank = BankRef(self.CAPACITY)
            self.captures_per_ply, self.forks = [], 0

        def capture(self, x):
            cand = self.bank.capture(self.st, self.done, x["terminal"], x["cvalid"], self.plies, self.slot_game,
                                     self.GAME_BASE, self.RUN_SEED, self.CAPTURE_PROB, self.MIN_MOVE, self.MAX_MOVE)
            self.captures_per_ply.append(int(cand.sum()))

        def seed(self):
            j = self.bank.seed(self.st, self.reseated, self.slot_game, self.GAME_BASE, self.RUN_SEED, self.FORK_PROB)
            self.forks += int((j >= 0).sum())

        def check_bank_coverage(self):
            assert max(self.captures_per_ply) > self.CAPACITY          # one launch with more candidates than rows
            assert self.bank.cursor > 2 * self.CAPACITY and self.forks >= 3            # the ring wrapped; games forked
            assert self.bank.counters[0] == self.forks and self.bank.counters[1] > 0

    return ScriptedBankTail()
