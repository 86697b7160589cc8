"""Replay window of past self-play generations, resident in HBM as exact 360-byte records.

The reference trains every iteration on a sliding window of generations (`v1/train.py:1486-1735`); the file-based stage
has one by re-reading shards (`scripts/train_stage.py --self_play_replay_inputs`).  This is the window of the in-process
loop: one `uint8[capacity_rows, 360]` ring of `trajectory_codec` records (7.5x smaller than the five tensors), a
generation = consecutive slots modulo the capacity, and training batches decoded straight out of the ring by one kernel
(`lz_replay_gather_rows`: unpack + board symmetry in one pass; no expanded copy of the window ever exists).

`GenerationTable` is the bookkeeping alone -- plain Python, no tensors -- and `select_slots` the selection rule on any
device; `ReplayWindow` is HIP only, like the codec.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch

from . import _lib as L
from .trajectory_codec import RECORD_BYTES

_MASK63 = (1 << 63) - 1


class GenerationTable:
    """(generation id, first slot, row count) of the generations a ring of `capacity_rows` slots holds, oldest first.
    A generation occupies `count` consecutive slots modulo the capacity, right behind its predecessor."""

    def __init__(self, max_generations: int, capacity_rows: int) -> None:
        if int(max_generations) < 1 or int(capacity_rows) < 1:
            raise ValueError(f"max_generations and capacity_rows must be positive, got {max_generations}, {capacity_rows}")
        self.max_generations, self.capacity_rows = int(max_generations), int(capacity_rows)
        self.entries: List[Tuple[int, int, int]] = []
        self.head = 0                                     # the slot the next generation starts at
        self.last_id: Optional[int] = None                # the newest id ever added (evicted or not)

    @property
    def num_rows(self) -> int:
        return sum(c for _, _, c in self.entries)

    def add(self, count: int, generation: Optional[int] = None) -> Dict[str, Any]:
        """Make room for `count` rows: evict the oldest generations until `max_generations` and the capacity both hold.
        Every refusal is raised before anything changes."""
        count = int(count)
        if count <= 0:
            raise ValueError("a generation needs at least one row")
        if count > self.capacity_rows:
            raise ValueError(f"a generation of {count} rows does not fit a ring of {self.capacity_rows}")
        gid = (0 if self.last_id is None else self.last_id + 1) if generation is None else int(generation)
        if self.last_id is not None and gid <= self.last_id:
            raise ValueError(f"generation id {gid} is not greater than the newest one ({self.last_id})")
        evicted = []
        while self.entries and (len(self.entries) + 1 > self.max_generations
                                or self.num_rows + count > self.capacity_rows):
            evicted.append(self.entries.pop(0)[0])
        first = self.head
        self.entries.append((gid, first, count))
        self.head = (first + count) % self.capacity_rows
        self.last_id = gid
        return {"generation": gid, "first_slot": first, "rows": count, "evicted": evicted}

    def shares(self, budget_per_old_generation: int) -> List[Tuple[int, int, int, int]]:
        """The selection rule of `scripts/train_stage.py` (`resolve_shard_specs`: replay inputs give at most their budget,
        the primary everything): (id, first slot, count, rows taken), newest first.  A budget <= 0 means
        newest count // number of older generations -- the window weighs as much as the new data."""
        if not self.entries:
            return []
        older = len(self.entries) - 1
        newest = self.entries[-1]
        budget = int(budget_per_old_generation)
        if budget <= 0:
            budget = newest[2] // older if older else 0
        out = [(newest[0], newest[1], newest[2], newest[2])]
        out += [(g, f, c, min(c, budget)) for g, f, c in reversed(self.entries[:-1])]
        return out

    def state(self) -> Dict[str, Any]:
        return {"max_generations": self.max_generations, "capacity_rows": self.capacity_rows,
                "entries": [list(e) for e in self.entries], "head": self.head, "last_id": self.last_id}


def _draw_seed(seed: int, newest: int, generation: int) -> int:
    return ((int(seed) * 1000003 + int(newest)) * 1000003 + int(generation)) & _MASK63


def select_slots(table: GenerationTable, budget_per_old_generation: int, seed: int, device,
                 generator: Optional[torch.Generator] = None, return_ages: bool = False):
    """int64 slots of one training pass: every row of the newest generation in row order, then the older generations
    from newest to oldest, `min(count, budget)` rows each, drawn uniformly without replacement and listed in ascending
    row order.  The draw of a generation is seeded by (seed, newest id, its id) on a generator of its own: the default
    generator's stream is not touched.  `return_ages`: (slots, ages), ages int64 -- for every slot, how many generations
    of the table its generation lies behind the newest (0 for the newest, whether or not the ones between gave rows)."""
    dev = torch.device(device)
    shares = table.shares(budget_per_old_generation)
    if not shares:
        empty = torch.zeros((0,), dtype=torch.int64, device=dev)
        return (empty, empty.clone()) if return_ages else empty
    gen = generator if generator is not None else torch.Generator(device=dev)
    newest = shares[0][0]
    parts, ages = [], []
    for i, (gid, first, count, take) in enumerate(shares):
        if take <= 0:
            continue
        if i == 0 or take == count:
            rows = torch.arange(count, dtype=torch.int64, device=dev)
        else:
            gen.manual_seed(_draw_seed(seed, newest, gid))
            rows = torch.randperm(count, generator=gen, device=dev)[:take].sort().values
        parts.append((rows + first) % table.capacity_rows)
        ages.append(i)
    slots = torch.cat(parts)
    if not return_ages:
        return slots
    return slots, torch.cat([torch.full((int(p.numel()),), a, dtype=torch.int64, device=dev) for p, a in zip(parts, ages)])


class ReplayWindow:
    """The last `max_generations` generations of training rows as records in one device ring of `capacity_rows` slots."""

    def __init__(self, device, *, max_generations: int, capacity_rows: int) -> None:
        self.device = torch.device(device)
        self.table = GenerationTable(max_generations, capacity_rows)
        self.ring = torch.empty((0, RECORD_BYTES), dtype=torch.uint8, device=self.device)
        L.require_hip(self.ring, "ReplayWindow")
        self.ring = torch.zeros((self.table.capacity_rows, RECORD_BYTES), dtype=torch.uint8, device=self.device)
        self._gen = torch.Generator(device=self.device)
        self.last_add: Dict[str, Any] = {"generation": None, "rows": 0, "filtered_non_finite_rows": 0, "evicted": []}

    # ---- properties --------------------------------------------------------------------------------------------------
    @property
    def num_rows(self) -> int:
        return self.table.num_rows

    @property
    def generations(self) -> List[Tuple[int, int, int]]:
        """(id, first slot, rows), oldest first."""
        return list(self.table.entries)

    @property
    def nbytes(self) -> int:
        return int(self.ring.numel())

    def slots_of(self, generation: int) -> torch.Tensor:
        """The slots of a held generation in row order."""
        for gid, first, count in self.table.entries:
            if gid == int(generation):
                return (torch.arange(count, dtype=torch.int64, device=self.device) + first) % self.table.capacity_rows
        raise KeyError(f"generation {generation} is not in the window")

    # ---- writing -----------------------------------------------------------------------------------------------------
    def _records_of(self, rows) -> Tuple[torch.Tensor, int]:
        from .trajectory_buffer import TensorSelfPlayBatch
        if isinstance(rows, TensorSelfPlayBatch):
            from .trajectory_codec import pack_batch
            L.require_hip(rows.state_tensors, "ReplayWindow.add_generation")
            if rows.num_samples <= 0:
                raise ValueError("a generation needs at least one row")
            states = rows.state_tensors.to(self.device, torch.float32)
            policy = rows.policy_targets.to(self.device, torch.float32)
            values = rows.value_targets.to(self.device, torch.float32).view(-1)
            soft = rows.soft_value_targets.to(self.device, torch.float32).view(-1)
            masks = rows.legal_masks.to(self.device)
            # rows with a non-finite target are dropped, as train_network_from_tensors drops them
            finite = torch.isfinite(values) & torch.isfinite(soft) & torch.isfinite(policy).all(dim=1) & \
                torch.isfinite(states.view(states.size(0), -1)).all(dim=1)
            filtered = int(finite.numel() - int(finite.sum().item()))
            if filtered:
                keep = torch.nonzero(finite).view(-1)
                states, masks, policy, values, soft = (t.index_select(0, keep) for t in (states, masks, policy, values, soft))
            if int(states.shape[0]) == 0:
                raise ValueError("a generation needs at least one row (none is left after the non-finite filter)"
                                 if filtered else "a generation needs at least one row")
            rec, bad = pack_batch(TensorSelfPlayBatch(states, masks, policy, values, soft), return_bad=True)
            n_bad = int(bad.item())
            if n_bad:
                raise ValueError(f"{n_bad} rows are not representable as compact records (planes not 0/1, policy mass "
                                 "off the legal set, or more than 72 legal actions); the window is unchanged")
            return rec, filtered
        if not isinstance(rows, torch.Tensor):
            raise TypeError("rows must be a TensorSelfPlayBatch or a uint8[n, 360] tensor of records")
        L.require_hip(rows, "ReplayWindow.add_generation")
        if rows.dtype != torch.uint8 or rows.dim() != 2 or int(rows.shape[1]) != RECORD_BYTES:
            raise ValueError(f"expected uint8[n, {RECORD_BYTES}] records, got {rows.dtype} {tuple(rows.shape)}")
        return rows.to(self.device), 0

    def _write(self, first: int, rec: torch.Tensor) -> None:
        n, cap = int(rec.shape[0]), self.table.capacity_rows
        a = min(n, cap - first)
        self.ring[first:first + a].copy_(rec[:a])
        if a < n:                                         # the generation wraps the end of the ring
            self.ring[:n - a].copy_(rec[a:])

    def add_generation(self, rows, generation: Optional[int] = None) -> Dict[str, Any]:
        """Append a generation (a `TensorSelfPlayBatch` on the HIP device, filtered and packed here, or records taken as
        they are) and evict the oldest ones until `max_generations` and the capacity hold.  ValueError -- window
        untouched -- for rows the record format cannot hold, an empty generation, one larger than the ring, or an id
        that is not greater than the newest.  Returns what was added, filtered and evicted."""
        rec, filtered = self._records_of(rows)
        info = self.table.add(int(rec.shape[0]), generation)
        self._write(info["first_slot"], rec)
        info["filtered_non_finite_rows"] = filtered
        self.last_add = info
        return dict(info)

    # ---- reading -----------------------------------------------------------------------------------------------------
    def select(self, budget_per_old_generation: int = 0, seed: int = 0, return_ages: bool = False):
        return select_slots(self.table, budget_per_old_generation, seed, self.device, self._gen, return_ages)

    def gather(self, slots: torch.Tensor, sym: Optional[torch.Tensor] = None):
        """(planes f32[m,11,6,6], masks bool[m,220], policy f32[m,220], value f32[m], soft f32[m]) of the records at
        `slots`, each under the board symmetry `sym[j]` (int8 / int32 ids; None: as stored).  A slot outside the ring or
        an id outside 0..7 gives an all-zero row."""
        L.require_hip(slots, "ReplayWindow.gather")
        dev = self.device
        if slots.dtype != torch.int64 or slots.device != dev:
            raise ValueError(f"slots must be int64 on {dev}, got {slots.dtype} on {slots.device}")
        slots = slots.reshape(-1).contiguous()
        m = int(slots.numel())
        width = 1
        if sym is not None:
            if sym.dtype not in (torch.int8, torch.int32):
                raise TypeError("sym must be an int8 / int32 tensor")
            if sym.numel() != m or sym.device != dev:
                raise ValueError(f"sym must hold {m} ids on {dev}")
            sym = sym.reshape(-1).contiguous()
            width = 1 if sym.dtype == torch.int8 else 4
        planes = torch.empty((m, 11, 6, 6), dtype=torch.float32, device=dev)
        masks = torch.empty((m, 220), dtype=torch.uint8, device=dev)
        policy = torch.empty((m, 220), dtype=torch.float32, device=dev)
        value = torch.empty((m,), dtype=torch.float32, device=dev)
        soft = torch.empty((m,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().lz_replay_gather_rows(L.ptr(self.ring), L.i64(self.table.capacity_rows), L.ptr(slots),
                                                  L.ptr(sym), width, L.i64(m), L.ptr(planes), L.ptr(masks),
                                                  L.ptr(policy), L.ptr(value), L.ptr(soft), L.stream_ptr(dev)),
                    "replay_gather_rows")
        return planes, masks.view(torch.bool), policy, value, soft

    # ---- restart -----------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        """The held records on the CPU (generation by generation, oldest first) and the table."""
        parts = [self.ring.index_select(0, self.slots_of(g)) for g, _, _ in self.table.entries]
        rec = torch.cat(parts).cpu() if parts else torch.zeros((0, RECORD_BYTES), dtype=torch.uint8)
        return {"records": rec, "table": self.table.state(), "last_add": dict(self.last_add)}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        """Restore into this window.  With the same capacity every generation returns to its slots; another capacity
        lays the generations out again from slot 0 (ValueError when they do not fit this window)."""
        t, rec = state["table"], state["records"]
        entries = [tuple(int(v) for v in e) for e in t["entries"]]
        if rec.dtype != torch.uint8 or rec.dim() != 2 or int(rec.shape[1]) != RECORD_BYTES or \
                int(rec.shape[0]) != sum(c for _, _, c in entries):
            raise ValueError("state_dict records do not match its table")
        if len(entries) > self.table.max_generations or int(rec.shape[0]) > self.table.capacity_rows:
            raise ValueError(f"{len(entries)} generations of {int(rec.shape[0])} rows do not fit a window of "
                             f"{self.table.max_generations} generations and {self.table.capacity_rows} rows")
        fresh = GenerationTable(self.table.max_generations, self.table.capacity_rows)
        if int(t["capacity_rows"]) == fresh.capacity_rows:
            fresh.entries, fresh.head = list(entries), int(t["head"])
        else:
            for gid, _, count in entries:
                fresh.add(count, gid)
        fresh.last_id = None if t["last_id"] is None else int(t["last_id"])
        self.table = fresh
        rec, start = rec.to(self.device), 0
        for _, first, count in fresh.entries:
            self._write(first, rec[start:start + count])
            start += count
        self.last_add = dict(state.get("last_add") or self.last_add)

    def metrics(self, budget_per_old_generation: int) -> Dict[str, Any]:
        """The `replay_window` entry of the trainer's metrics for one selection, newest generation first."""
        shares = self.table.shares(budget_per_old_generation)
        return {"generations": [g for g, _, _, _ in shares], "rows_held": [c for _, _, c, _ in shares],
                "rows_selected": [k for _, _, _, k in shares], "window_rows": self.num_rows,
                "window_bytes": self.nbytes, "evicted": list(self.last_add.get("evicted", [])),
                "filtered_non_finite_rows": int(self.last_add.get("filtered_non_finite_rows", 0))}
