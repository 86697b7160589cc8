"""Sequential restatement of the opening book (csrc/lz_opening_book.h, lz_opening_book_keys / lz_states_from_packed) in
numpy and Python integers on the host scalar rule engine (include/liuzhou_scalar.h through liuzhou_amd/v0_scalar.py), and
the cases the CPU and GPU tests share.  A record is the 32-byte packed state of csrc/lz_rules.h, four little-endian
64-bit words; here a tuple of four Python integers.  The board symmetries are restated from their (r, c) formulas."""
import ctypes as C
import functools

import numpy as np
import torch

from liuzhou_amd import v0_scalar as VS
from tests import start_bank_ref as S

SENT = 0x7F
FULL = (1 << 36) - 1
NO_KEY = -(1 << 63)
SIZES = (1, 63, 64, 65, 255, 256, 257)
_RC = (lambda r, c: (r, c), lambda r, c: (c, 5 - r), lambda r, c: (5 - r, 5 - c), lambda r, c: (5 - c, r),
       lambda r, c: (r, 5 - c), lambda r, c: (5 - r, c), lambda r, c: (c, r), lambda r, c: (5 - c, 5 - r))
PERM = [[_RC[k](x // 6, x % 6)[0] * 6 + _RC[k](x // 6, x % 6)[1] for x in range(36)] for k in range(8)]


# ---- records ---------------------------------------------------------------------------------------------------------------
def to_bytes(words):
    """uint8[n, 32] of a list of 4-tuples."""
    a = np.array([[w & 0xFFFFFFFFFFFFFFFF for w in rec] for rec in words], dtype=np.uint64).reshape(-1, 4)
    return np.ascontiguousarray(a.astype("<u8")).view(np.uint8).reshape(-1, 32)


def to_words(packed):
    w = np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1, 32).view("<u8")
    return [tuple(int(x) for x in row) for row in w]


def field(w0, shift, mask):
    return (w0 >> shift) & mask


def meta_of(w0):
    return dict(move_count=field(w0, 36, 0xFF), msc=field(w0, 44, 0x3F), phase=field(w0, 50, 7),
                player=-1 if field(w0, 53, 1) else 1, forced=field(w0, 54, 3), pm_req=field(w0, 56, 3),
                pm_rem=field(w0, 58, 3), pc_req=field(w0, 60, 3), pc_rem=field(w0, 62, 3))


def with_fields(rec, **kw):
    """The record with some fields of word 0 replaced (move_count, msc, phase, player, forced, pm_*, pc_*)."""
    m = {**meta_of(rec[0]), **kw}
    w0 = (rec[0] & FULL) | (m["move_count"] & 0xFF) << 36 | (m["msc"] & 0x3F) << 44 | (m["phase"] & 7) << 50 | \
         (1 if m["player"] < 0 else 0) << 53 | (m["forced"] & 3) << 54 | (m["pm_req"] & 3) << 56 | (m["pm_rem"] & 3) << 58 | \
         (m["pc_req"] & 3) << 60 | (m["pc_rem"] & 3) << 62
    return (w0,) + tuple(rec[1:])


def sym_board(k, b):
    out = 0
    for x in range(36):
        if (b >> x) & 1:
            out |= 1 << PERM[k][x]
    return out


def sym_record(k, rec):
    return ((rec[0] & ~FULL) | sym_board(k, rec[0] & FULL),) + tuple(sym_board(k, w & FULL) for w in rec[1:])


# ---- the host scalar engine ----------------------------------------------------------------------------------------------------
def cstate(rec):
    """LzScalarState of a record without overlapping boards."""
    m = meta_of(rec[0])
    cs = VS._CState()
    for x in range(36):
        cs.board[x] = 1 if (rec[0] >> x) & 1 else (-1 if (rec[1] >> x) & 1 else 0)
        cs.marks_black[x] = (rec[2] >> x) & 1
        cs.marks_white[x] = (rec[3] >> x) & 1
    cs.phase, cs.current_player, cs.forced_removals_done, cs.move_count = m["phase"], m["player"], m["forced"], m["move_count"]
    cs.pending_marks_required, cs.pending_marks_remaining = m["pm_req"], m["pm_rem"]
    cs.pending_captures_required, cs.pending_captures_remaining = m["pc_req"], m["pc_rem"]
    cs.moves_since_capture = m["msc"]
    return cs


def record_of(cs):
    bits = lambda arr, want: sum(1 << x for x in range(36) if want(arr[x]))
    rec = (bits(cs.board, lambda v: v == 1), bits(cs.board, lambda v: v == -1), bits(cs.marks_black, lambda v: v != 0),
           bits(cs.marks_white, lambda v: v != 0))
    return with_fields((rec[0],) + rec[1:], move_count=cs.move_count, msc=cs.moves_since_capture, phase=cs.phase,
                       player=cs.current_player, forced=cs.forced_removals_done, pm_req=cs.pending_marks_required,
                       pm_rem=cs.pending_marks_remaining, pc_req=cs.pending_captures_required,
                       pc_rem=cs.pending_captures_remaining)


def status(cs):
    """game_status: 0 running, +1 / -1 the winner, 2 a draw by a limit."""
    winner, over = C.c_int32(0), C.c_int32(0)
    assert VS._host()["lz_scalar_status"](C.byref(cs), C.byref(winner), C.byref(over)) == 0
    return int(winner.value) if winner.value else (2 if over.value else 0)


def legal_moves(cs):
    """GenerateAllLegalMoves: (phase, action type, primary, secondary) tuples; none when the game is over."""
    buf, n = (C.c_int32 * 640)(), C.c_int32(0)
    assert VS._host()["lz_scalar_generate"](C.byref(cs), 7, buf, 640, C.byref(n)) == 0
    v = list(buf[:int(n.value)])
    return [tuple(v[i:i + 4]) for i in range(0, len(v), 4)]


def action_index(move):
    """The 220-d index of a move record (v0/python/move_encoder.py:46-51)."""
    _phase, kind, a, b = move
    if kind == 1:
        return a
    if kind == 2:
        return 36 + 4 * a + {-6: 0, 6: 1, -1: 2, 1: 3}[b - a]
    return 216 if kind == 8 else 180 + a


def apply_move(cs, move):
    out, why = VS._CState(), C.c_int32(0)
    st = VS._host()["lz_scalar_apply_move"](C.byref(cs), C.byref(VS._CMove(*move)), C.byref(out), C.byref(why))
    assert st == 0, (st, why.value, move)
    return out


# ---- the rules -----------------------------------------------------------------------------------------------------------------
def valid_ref(rec, min_move, max_move):
    if any(w >> 36 for w in rec[1:]):                       # canonical: words 1..3 own bits 0..35, word 0 all 64
        return False
    m = meta_of(rec[0])
    if not 1 <= m["phase"] <= 7 or (rec[0] & rec[1] & FULL):
        return False
    cs = cstate(rec)
    if status(cs) != 0 or not legal_moves(cs):
        return False
    return min_move <= m["move_count"] <= max_move


def key_ref(rec, row, min_move, max_move):
    """(valid, key words as signed 64-bit integers, sym)."""
    if not valid_ref(rec, min_move, max_move):
        return 0, [NO_KEY | row, 0, 0, 0], 0
    boards = [w & FULL for w in rec]
    best, img = 0, boards
    for k in range(1, 8):
        cand = [sym_board(k, b) for b in boards]
        if cand < img:                                      # lexicographic, the lowest k among equals
            best, img = k, cand
    return 1, [img[0] | (rec[0] >> 50) << 36, img[1], img[2], img[3]], best


def keys_ref(words, min_move, max_move):
    out = [key_ref(rec, i, min_move, max_move) for i, rec in enumerate(words)]
    return (np.array([o[0] for o in out], np.uint8), np.array([o[1] for o in out], np.int64).reshape(-1, 4),
            np.array([o[2] for o in out], np.int8))


def book_rows_ref(words, min_move=0, max_move=143, max_positions=None):
    """The rows OpeningBook.from_packed keeps, and its counts."""
    seen, rows, invalid, dup = {}, [], 0, 0
    for i, rec in enumerate(words):
        ok, key, _ = key_ref(rec, i, min_move, max_move)
        if not ok:
            invalid += 1
        elif tuple(key) in seen:
            dup += 1
        else:
            seen[tuple(key)] = i
            rows.append(i)
    kept = rows if max_positions is None else rows[:max_positions]
    return kept, dict(seen=len(words), invalid=invalid, duplicate=dup, truncated=len(rows) - len(kept), kept=len(kept))


# ---- positions -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk_positions(seed=20261021, games=6, max_steps=400):
    """Every running position of seeded random legal walks from the empty board with the host scalar engine, as records,
    game by game (a list of lists)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(games):
        cs = VS._CState()
        cs.phase, cs.current_player = 1, 1
        game = []
        for _ in range(max_steps):
            moves = legal_moves(cs)
            if not moves:
                break
            game.append(record_of(cs))
            cs = apply_move(cs, moves[int(rng.integers(len(moves)))])
        out.append(game)
    return out


@functools.lru_cache(maxsize=None)
def pool():
    return [rec for game in walk_positions() for rec in game]


def playable(min_move=6):
    return [r for r in pool() if valid_ref(r, min_move, 143)]


def finished_records():
    """Hand-built finished games on walked boards: black wins (white under four pieces), white wins, a draw by move count
    and a draw by the no-capture limit.  Returns {status: record}."""
    mv = next(r for r in pool() if meta_of(r[0])["phase"] == 4 and bin(r[0] & FULL).count("1") >= 4 and bin(r[1]).count("1") >= 4)
    few = lambda b: sum(1 << x for x in [x for x in range(36) if (b >> x) & 1][:3])
    return {1: (mv[0], few(mv[1]), 0, 0), -1: ((mv[0] & ~FULL) | few(mv[0] & FULL), mv[1], 0, 0),
            2: with_fields(mv, move_count=144), "msc": with_fields(mv, msc=36)}


def no_legal_record():
    """A canonical running position without a legal action: mark selection with no mark left to make."""
    base = next(r for r in pool() if meta_of(r[0])["phase"] == 1 and meta_of(r[0])["move_count"] >= 8)
    return with_fields(base, phase=2, pm_req=1, pm_rem=0)


def mixed_records(m):
    """m records: walked positions, their symmetric images, copies that differ in move_count / msc only, in the player
    only, in the phase only, and every kind of invalid record."""
    p, fin = pool(), finished_records()
    out = []
    for i in range(m):
        base = p[(37 * i + 11) % len(p)]
        kind = i % 12
        if kind == 3:
            rec = sym_record(1 + i % 7, base)
        elif kind == 4:
            rec = with_fields(base, msc=(meta_of(base[0])["msc"] + 1 + i % 5) % 30, move_count=min(143, meta_of(base[0])["move_count"] + i % 3))
        elif kind == 5:
            rec = with_fields(base, player=-meta_of(base[0])["player"])
        elif kind == 6:
            rec = (0, 0, 0, 0)
        elif kind == 7:
            rec = list(base)
            rec[1 + i % 3] |= 1 << (36 + (5 * i) % 28)
            rec = tuple(rec)
        elif kind == 8:
            rec = (base[0], base[1] | (base[0] & FULL & -(base[0] & FULL)), base[2], base[3])      # black's lowest piece is white too
        elif kind == 9:
            rec = (fin[1], fin[-1], fin[2], fin["msc"], no_legal_record(), with_fields(base, phase=0))[(i // 12) % 6]
        elif kind == 10:
            rec = with_fields(base, phase=1 + (meta_of(base[0])["phase"] + i) % 7)
        else:
            rec = base
        out.append(rec)
    return out


# ---- launches through the C ABI (the HIP library on a device, or its host twin on CPU tensors) -------------------------------------
def _sync(device):
    import torch
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def call_keys(L, lib, device, records, m, min_move, max_move, valid, keys, sym):
    import torch
    st = lib.lz_opening_book_keys(L.ptr(records), L.i64(m), L.i64(min_move), L.i64(max_move), L.ptr(valid), L.ptr(keys),
                                  L.ptr(sym), L.stream_ptr(torch.device(device)))
    _sync(device)
    return st


def run_keys(L, lib, device, words, min_move=0, max_move=143):
    """One keys launch on sentinel-filled outputs with a guard row past the end, against keys_ref: every byte."""
    import torch
    m = len(words)
    rec = S.tensor(to_bytes(words), device)
    valid = torch.full((m + 16,), SENT, dtype=torch.uint8, device=device)
    keys = torch.full((m + 4, 4), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device=device)
    sym = torch.full((m + 16,), SENT, dtype=torch.int8, device=device)
    L.check(call_keys(L, lib, device, rec, m, min_move, max_move, valid, keys, sym), "opening_book_keys")
    v, k, s = keys_ref(words, min_move, max_move)
    where = f"m={m} moves {min_move}..{max_move}: "
    S.assert_bytes(valid, np.concatenate([v, np.full(16, SENT, np.uint8)]), where + "valid")
    S.assert_bytes(keys, np.concatenate([k, np.full((4, 4), 0x7F7F7F7F7F7F7F7F, np.int64)]), where + "keys")
    S.assert_bytes(sym, np.concatenate([s, np.full(16, SENT, np.int8)]), where + "sym")
    S.assert_bytes(rec, to_bytes(words), where + "records")
    return v, k, s


def sentinel_states(n, device):
    """Twelve state tensors of n rows filled with the sentinel byte (the marks as bytes)."""
    import torch
    cells = lambda dt: torch.full((n, 36), SENT, dtype=dt, device=device)
    return [cells(torch.int8), cells(torch.uint8), cells(torch.uint8)] + \
           [torch.full((n,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device=device) for _ in range(9)]


def call_from_packed(L, lib, device, records, capacity, index, n, ts):
    import torch
    st = lib.lz_states_from_packed(L.ptr(records), L.i64(capacity), L.ptr(index), L.i64(n),
                                   C.byref(L.soa(ts)) if ts is not None else None, L.stream_ptr(torch.device(device)))
    _sync(device)
    return st


def run_from_packed(L, lib, device, words, index, rows=None):
    """One lz_states_from_packed launch of len(index) rows on sentinel-filled tensors of `rows` rows (default: two more
    than the launch), against the restatement: every byte of all twelve tensors.  Returns the tensors."""
    n = len(index)
    rows = n + 2 if rows is None else rows
    packed = to_bytes(words)
    rec, idx = S.tensor(packed, device), S.tensor(np.asarray(index, np.int64), device)
    ts = sentinel_states(rows, device)
    L.check(call_from_packed(L, lib, device, rec, len(words), idx, n, ts), "states_from_packed")
    want = [t.cpu().numpy().copy() for t in sentinel_states(rows, "cpu")]
    hit = [g for g in range(n) if 0 <= index[g] < len(words)]
    if hit:
        st = S.unpack_states(packed[[index[g] for g in hit]])
        for t, f in zip(want, S.FIELDS):
            a = np.asarray(st[f])
            t[hit] = a.reshape(len(hit), -1).astype(t.dtype) if t.ndim == 2 else a.astype(t.dtype)
    for t, w, f in zip(ts, want, S.FIELDS):
        S.assert_bytes(t, w, f"n={n} capacity={len(words)}: {f}")
    S.assert_bytes(rec, packed, "records")
    S.assert_bytes(idx, np.asarray(index, np.int64), "index")
    return ts, hit


# ---- the refusals of both entry points (CPU and GPU tests) ----------------------------------------------------------------------
ERR_ARG, ERR_ALIGN = -1, -4


def check_argument_refusals(L, lib, device):
    """Range, null and alignment refusals of both entry points return without touching a buffer; a size of 0 is ok."""
    words = playable(0)[:7]
    raw = S.tensor(np.concatenate([to_bytes(words).reshape(-1), np.full(16, SENT, np.uint8)]), device)
    rec = raw[:7 * 32].view(7, 32)
    valid = torch.full((7,), SENT, dtype=torch.uint8, device=device)
    keys_raw = torch.full((7 * 4 + 2,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device=device)
    keys = keys_raw[:28].view(7, 4)
    sym = torch.full((7,), SENT, dtype=torch.int8, device=device)

    def k(rec=rec, m=7, lo=0, hi=143, valid=valid, keys=keys, sym=sym):
        return call_keys(L, lib, device, rec, m, lo, hi, valid, keys, sym)

    assert k(m=-1) == ERR_ARG and k(lo=-1) == ERR_ARG and k(lo=9, hi=8) == ERR_ARG
    assert k(rec=None) == ERR_ARG and k(valid=None) == ERR_ARG and k(keys=None) == ERR_ARG and k(sym=None) == ERR_ARG
    assert k(rec=raw[8:8 + 7 * 32].view(7, 32)) == ERR_ALIGN and k(keys=keys_raw[1:29].view(7, 4)) == ERR_ALIGN
    assert k(m=0, rec=None, valid=None, keys=None, sym=None) == 0

    ts = sentinel_states(7, device)
    index = S.tensor(np.arange(8, dtype=np.int64), device)

    def f(rec=rec, capacity=7, index=index[:7], n=7, ts=ts):
        return call_from_packed(L, lib, device, rec, capacity, index, n, ts)

    assert f(n=-1) == ERR_ARG and f(capacity=-1) == ERR_ARG and f(rec=None) == ERR_ARG and f(index=None) == ERR_ARG
    assert f(ts=None) == ERR_ARG
    assert f(rec=raw[8:8 + 7 * 32].view(7, 32)) == ERR_ALIGN
    odd = [t for t in sentinel_states(8, device)]
    odd[0] = odd[0].view(-1)[1:1 + 7 * 36].view(7, 36)
    assert f(ts=odd) == ERR_ALIGN
    assert f(n=0, rec=None, index=None, ts=None) == 0
    S.assert_bytes(valid, np.full(7, SENT, np.uint8), "valid")                   # nothing ran
    S.assert_bytes(keys_raw, np.full(30, 0x7F7F7F7F7F7F7F7F, np.int64), "keys")
    S.assert_bytes(sym, np.full(7, SENT, np.int8), "sym")
    for t, w in zip(ts, sentinel_states(7, "cpu")):
        S.assert_bytes(t, w.numpy(), "states")
    S.assert_bytes(raw[7 * 32:], np.full(16, SENT, np.uint8), "guard")


# ---- replaying an arena game -------------------------------------------------------------------------------------------------------
def replay(rec, log, max_plies):
    """Play the logged 220-d action indices from the opening `rec` with the host scalar rules: every move must be legal,
    nothing may follow the game's end.  Returns the result from black's side (+1, -1, 0) as the arena's loop decides it."""
    cs, plies = cstate(rec), 0
    log = [int(a) for a in log]
    for t, a in enumerate(log):
        if a < 0:
            assert all(x < 0 for x in log[t:]), "a move after the game's end"
            break
        moves = {action_index(mv): mv for mv in legal_moves(cs)}
        assert a in moves, f"ply {plies}: action {a} is not legal"
        cs = apply_move(cs, moves[a])
        plies += 1
        if status(cs) != 0 or plies >= max_plies:
            assert all(x < 0 for x in log[t + 1:]), "a move after the game's end"
            break
    st = status(cs)
    if st != 0:
        return 0 if st == 2 else st
    if plies >= max_plies:
        return 0
    assert not legal_moves(cs), "the game stopped although it was running and the mover had a move"
    return -int(cs.current_player)
