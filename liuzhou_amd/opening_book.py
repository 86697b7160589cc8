"""The opening book of the evaluation arena: positions real self-play games passed through, distinct up to board symmetry
and checked playable, each played twice with the colours swapped.

A start bank (start_bank.py) holds `lz::Packed` records, uint8[n, 32].  `OpeningBook.from_packed` keys them
(`lz_opening_book_keys`: validity, the symmetric key, csrc/lz_opening_book.h), groups the keys exactly
(`position_dedup.group_rows`) and keeps the lowest row of every group of valid records.  The arena seats the games of a
match from the book with one `lz_states_from_packed` launch (eval_arena.py); `assign_openings` is the assignment of book
entries to game pairs and `paired_statistics` the pentanomial statistics of the colour-swapped pairs.

HIP tensors go to the gfx950 kernels, CPU tensors to the host build of the same C ABI; there is no fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, Optional, Sequence

import torch

from . import _lib as L
from .position_dedup import group_rows

FORMAT = "lz_opening_book_v1"
RECORD_BYTES = 32
MAX_RECORDS = 1 << 24
Z95 = 1.959964


def _records(records: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(records, torch.Tensor) or records.dtype != torch.uint8 or records.dim() != 2 or \
            int(records.shape[1]) != RECORD_BYTES:
        raise ValueError(f"{what}: records must be a uint8[n, 32] tensor")
    return records.contiguous()


def _move_range(min_move, max_move) -> None:
    for name, v in (("min_move", min_move), ("max_move", max_move)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"opening book: {name} must be an integer, got {v!r}")
    if int(min_move) < 0 or int(max_move) < int(min_move):
        raise ValueError(f"opening book: need 0 <= min_move <= max_move, got {min_move!r}, {max_move!r}")


def book_keys(records: torch.Tensor, min_move: int = 0, max_move: int = 143):
    """(valid uint8[m], keys int64[m,4], sym int8[m]) of uint8[m,32] records (include/liuzhou_hip.h:
    lz_opening_book_keys), on the records' device."""
    rec = _records(records, "book_keys")
    _move_range(min_move, max_move)
    m, dev = int(rec.shape[0]), rec.device
    valid = torch.empty((m,), dtype=torch.uint8, device=dev)
    keys = torch.empty((m, 4), dtype=torch.int64, device=dev)
    sym = torch.empty((m,), dtype=torch.int8, device=dev)
    with L.device_ctx(dev):
        st = L.lib_for(rec).lz_opening_book_keys(L.ptr(rec), L.i64(m), L.i64(min_move), L.i64(max_move), L.ptr(valid),
                                                 L.ptr(keys), L.ptr(sym), L.stream_ptr(dev))
    L.check(st, "opening_book.book_keys")
    return valid, keys, sym


def states_from_packed(records: torch.Tensor, index: torch.Tensor, state_tensors: Sequence[torch.Tensor]) -> None:
    """Row g of the twelve state tensors becomes the unpacked records[index[g]], in place; rows whose index is outside
    the records are left as they are (include/liuzhou_hip.h: lz_states_from_packed)."""
    rec = _records(records, "states_from_packed")
    if index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous():
        raise ValueError("states_from_packed: index must be a contiguous int64[n] tensor")
    ts = tuple(state_tensors)
    n, dev = int(index.numel()), rec.device
    if len(ts) != 12 or any(t.device != dev or int(t.shape[0]) < n or not t.is_contiguous() for t in ts) or index.device != dev:
        raise ValueError("states_from_packed: twelve contiguous state tensors of at least n rows, all on the records' device")
    with L.device_ctx(dev):
        st = L.lib_for(rec).lz_states_from_packed(L.ptr(rec), L.i64(int(rec.shape[0])), L.ptr(index), L.i64(n),
                                                  C.byref(L.soa(ts)), L.stream_ptr(dev))
    L.check(st, "opening_book.states_from_packed")


def _move_counts(positions: torch.Tensor) -> torch.Tensor:
    """int64[B]: bits 36..43 of word 0 (little-endian: the high nibble of byte 4, the low nibble of byte 5)."""
    b = positions.to(torch.int64)
    return (b[:, 4] >> 4) | ((b[:, 5] & 0xF) << 4)


class OpeningBook:
    """positions uint8[B, 32] (packed states, on a device), move_counts int64[B] (same device), meta (plain values)."""

    def __init__(self, positions: torch.Tensor, meta: Optional[Dict[str, Any]] = None) -> None:
        self.positions = _records(positions, "OpeningBook")
        self.move_counts = _move_counts(self.positions)
        self.meta: Dict[str, Any] = dict(meta or {})

    def __len__(self) -> int:
        return int(self.positions.shape[0])

    @property
    def device(self) -> torch.device:
        return self.positions.device

    def to(self, device) -> "OpeningBook":
        return OpeningBook(self.positions.to(torch.device(device)), self.meta)

    @staticmethod
    def from_packed(records: torch.Tensor, *, min_move: int = 0, max_move: int = 143,
                    max_positions: Optional[int] = None) -> "OpeningBook":
        """The book of uint8[n, 32] records: of every group of valid records with one key the lowest row, in ascending
        row order, at most `max_positions` of them."""
        rec = _records(records, "OpeningBook.from_packed")
        if int(rec.shape[0]) > MAX_RECORDS:
            raise ValueError(f"OpeningBook.from_packed: at most 2**24 records, got {int(rec.shape[0])}")
        if max_positions is not None and (isinstance(max_positions, bool) or int(max_positions) != max_positions or
                                          int(max_positions) < 1):
            raise ValueError(f"OpeningBook.from_packed: max_positions must be an integer >= 1, got {max_positions!r}")
        valid, keys, _sym = book_keys(rec, min_move, max_move)
        seen = int(rec.shape[0])
        _group, order, begin, _count = group_rows(keys)
        first = order.index_select(0, begin[:-1])                 # every group's lowest row, ascending
        keep = first[valid.index_select(0, first) != 0]
        n_valid, distinct = int((valid != 0).sum()), int(keep.numel())
        if max_positions is not None:
            keep = keep[:int(max_positions)]
        kept = int(keep.numel())
        meta = {"format": FORMAT, "seen": seen, "invalid": seen - n_valid, "duplicate": n_valid - distinct,
                "truncated": distinct - kept, "kept": kept, "min_move": int(min_move), "max_move": int(max_move),
                "max_positions": None if max_positions is None else int(max_positions)}
        return OpeningBook(rec.index_select(0, keep), meta)

    @staticmethod
    def from_bank(start_bank, **kw) -> "OpeningBook":
        """The book of a StartBank's filled entries, the physical rows [0, filled)."""
        return OpeningBook.from_packed(start_bank.entries[:start_bank.filled()], **kw)

    def save(self, path: str) -> None:
        torch.save({"format": FORMAT, "positions": self.positions.detach().cpu().clone(),
                    "move_counts": self.move_counts.detach().cpu().clone(), "meta": dict(self.meta)}, path)

    @staticmethod
    def load(path: str, device="cpu") -> "OpeningBook":
        obj = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(obj, dict) or obj.get("format") != FORMAT:
            raise ValueError(f"OpeningBook.load: {path} is not a {FORMAT} file")
        pos, mc = obj.get("positions"), obj.get("move_counts")
        if not isinstance(pos, torch.Tensor) or pos.dtype != torch.uint8 or pos.dim() != 2 or int(pos.shape[1]) != RECORD_BYTES:
            raise ValueError(f"OpeningBook.load: {path}: positions must be uint8[B, 32]")
        if not isinstance(mc, torch.Tensor) or mc.dtype != torch.int64 or tuple(mc.shape) != (int(pos.shape[0]),) or \
                not torch.equal(mc, _move_counts(pos)):
            raise ValueError(f"OpeningBook.load: {path}: move_counts must be the int64[B] move counts of the positions")
        meta = obj.get("meta")
        if not isinstance(meta, dict):
            raise ValueError(f"OpeningBook.load: {path}: meta must be a dict")
        return OpeningBook(pos.to(torch.device(device)), meta)


def assign_openings(book_size: int, pairs: int, seed: int) -> torch.Tensor:
    """int64[pairs] (CPU): pair p plays book entry perm[p % book_size], perm the permutation of a CPU generator seeded with
    `seed` -- every opening is used before any is repeated.  A pure function of its arguments."""
    if int(book_size) < 1 or int(pairs) < 0:
        raise ValueError(f"assign_openings: need book_size >= 1 and pairs >= 0, got {book_size!r}, {pairs!r}")
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    perm = torch.randperm(int(book_size), generator=g, dtype=torch.int64)
    return perm.index_select(0, torch.arange(int(pairs), dtype=torch.int64) % int(book_size))


def _elo(score: float) -> Optional[float]:
    return None if not 0.0 < score < 1.0 else -400.0 * math.log10(1.0 / score - 1.0)


def paired_statistics(challenger_points_first, challenger_points_second) -> Dict[str, Any]:
    """Pentanomial statistics of P colour-swapped game pairs: the challenger's points (0, 1/2, 1) in the first and in the
    second game of every pair.  Host float64.  `pentanomial` N[5] counts the pair sums 0, 1/2, 1, 3/2, 2; score =
    sum N_k (k/4) / P; score_stderr = sqrt(sum N_k (k/4 - score)^2 / P / P); elo = -400 log10(1/score - 1) (None at 0 or
    1); elo_ci95 the Elo of score -+ 1.959964 stderr, an end outside (0, 1) None; los = (1 + erf((score - 1/2) /
    (stderr sqrt 2))) / 2, at stderr 0: 1, 0 or 1/2 by the sign; trinomial_stderr: the standard error of the same 2P games'
    mean taken as independent."""
    a = [float(x) for x in (challenger_points_first.tolist() if hasattr(challenger_points_first, "tolist") else challenger_points_first)]
    b = [float(x) for x in (challenger_points_second.tolist() if hasattr(challenger_points_second, "tolist") else challenger_points_second)]
    if len(a) != len(b) or not a:
        raise ValueError("paired_statistics: two sequences of the same non-zero length")
    if any(x not in (0.0, 0.5, 1.0) for x in a + b):
        raise ValueError("paired_statistics: points per game are 0, 1/2 or 1")
    P = len(a)
    N = [0] * 5
    for x, y in zip(a, b):
        N[int(round(2.0 * (x + y)))] += 1
    score = sum(N[k] * (k / 4.0) for k in range(5)) / P
    stderr = math.sqrt(sum(N[k] * (k / 4.0 - score) ** 2 for k in range(5)) / P / P)
    games = a + b
    tri = math.sqrt(sum((x - score) ** 2 for x in games) / len(games) / len(games))
    if stderr > 0.0:
        los = 0.5 * (1.0 + math.erf((score - 0.5) / (stderr * math.sqrt(2.0))))
    else:
        los = 1.0 if score > 0.5 else 0.0 if score < 0.5 else 0.5
    return {"pairs": P, "pentanomial": N, "score": score, "score_stderr": stderr, "elo": _elo(score),
            "elo_ci95": [_elo(score - Z95 * stderr), _elo(score + Z95 * stderr)], "los": los, "trinomial_stderr": tri}
