"""Replay window of past self-play generations, resident in HBM as exact 360-byte records.

The reference trains every iteration on a sliding window of generations (`v1/train.py:1486-1735`); the file-based stage
has one by re-reading shards (`scripts/train_stage.py --self_play_replay_inputs`).  This is the window of the in-process
loop: one `uint8[capacity_rows, 360]` ring of `trajectory_codec` records (7.5x smaller than the five tensors), a
generation = consecutive slots modulo the capacity, and training batches decoded straight out of the ring by one kernel
(`lz_replay_gather_rows`: unpack + board symmetry in one pass; no expanded copy of the window ever exists).

Duplicate positions across the window are merged record to record: `record_position_keys`
and `merge_record_groups` read and write records only -- HIP tensors through the kernels of csrc/lz_replay_merge.hip,
CPU tensors through the host build -- and `ReplayWindow.merge_selection` turns a selection into one record per position
with a row weight.

`GenerationTable` is the bookkeeping alone -- plain Python, no tensors -- and `select_slots` the selection rule on any
device; `ReplayWindow` is HIP only, like the codec.
"""
from __future__ import annotations

import math
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


def _records_and_slots(records: torch.Tensor, slots: torch.Tensor, op: str) -> Tuple[torch.Tensor, torch.Tensor]:
    if not isinstance(records, torch.Tensor) or not isinstance(slots, torch.Tensor):
        raise TypeError(f"{op}: records and slots must be tensors")
    if records.dtype != torch.uint8 or records.dim() != 2 or int(records.shape[1]) != RECORD_BYTES:
        raise ValueError(f"{op}: expected uint8[capacity, {RECORD_BYTES}] records, got {records.dtype} {tuple(records.shape)}")
    if slots.dtype != torch.int64 or slots.device != records.device:
        raise ValueError(f"slots must be int64 on {records.device}, got {slots.dtype} on {slots.device}")
    return records.contiguous(), slots.reshape(-1).contiguous()


def gather_records(records: torch.Tensor, slots: torch.Tensor, sym: Optional[torch.Tensor] = None, *,
                   op: str = "replay_window.gather_records"):
    """`ReplayWindow.gather` over any uint8[capacity,360] buffer of records on a HIP device (the ring, or the merged
    records of `merge_selection`): one launch of `lz_replay_gather_rows`."""
    L.require_hip(slots, op)
    records, slots = _records_and_slots(records, slots, op)
    dev = records.device
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
        L.check(L.lib().lz_replay_gather_rows(L.ptr(records), L.i64(int(records.shape[0])), L.ptr(slots),
                                              L.ptr(sym), width, L.i64(m), L.ptr(planes), L.ptr(masks),
                                              L.ptr(policy), L.ptr(value), L.ptr(soft), L.stream_ptr(dev)),
                "replay_gather_rows")
    return planes, masks.view(torch.bool), policy, value, soft


def record_position_keys(records: torch.Tensor, slots: torch.Tensor, *, symmetric: bool):
    """(keys int64[m,8], sym int8[m], not_representable int32[1]) of the records uint8[capacity,360] at `slots` int64[m]
    (include/liuzhou_hip.h: lz_replay_position_keys): byte for byte the keys of the unpacked rows.  A slot outside
    [0, capacity) gets a key of its own and is counted.  HIP tensors go to the kernel, CPU tensors to the host build;
    the counter stays on the records' device, nothing is read back."""
    records, slots = _records_and_slots(records, slots, "replay_window.record_position_keys")
    dev = records.device
    m = int(slots.numel())
    keys = torch.empty((m, 8), dtype=torch.int64, device=dev)
    sym = torch.empty((m,), dtype=torch.int8, device=dev)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    with L.device_ctx(dev):
        st = L.lib_for(records).lz_replay_position_keys(L.ptr(records), L.i64(int(records.shape[0])), L.ptr(slots), L.i64(m),
                                                        1 if symmetric else 0, L.ptr(keys), L.ptr(sym), L.ptr(bad),
                                                        L.stream_ptr(dev))
    L.check(st, "replay_window.record_position_keys")
    return keys, sym, bad


def merge_record_groups(records: torch.Tensor, slots: torch.Tensor, sym: torch.Tensor, order: torch.Tensor,
                        begin: torch.Tensor):
    """(merged uint8[groups,360], count int32[groups], not_representable int32[1]): one record per group of positions
    in `slots` (include/liuzhou_hip.h: lz_replay_merge_records; `sym` int8[m] from `record_position_keys`, `order`
    int64[m] and `begin` int64[groups+1] from `position_dedup.group_rows`).  Byte for byte the packed rows of
    `position_dedup.merge_duplicate_positions` on the unpacked records."""
    records, slots = _records_and_slots(records, slots, "replay_window.merge_record_groups")
    dev = records.device
    m = int(slots.numel())
    if sym.dtype != torch.int8 or int(sym.numel()) != m or sym.device != dev:
        raise ValueError(f"sym must hold {m} int8 ids on {dev}")
    if order.dtype != torch.int64 or begin.dtype != torch.int64 or order.device != dev or begin.device != dev:
        raise ValueError(f"order and begin must be int64 on {dev}")
    if int(order.numel()) != m or int(begin.numel()) < 1:
        raise ValueError(f"order must hold {m} positions and begin at least one boundary")
    sym, order, begin = sym.reshape(-1).contiguous(), order.reshape(-1).contiguous(), begin.reshape(-1).contiguous()
    groups = int(begin.numel()) - 1
    merged = torch.zeros((groups, RECORD_BYTES), dtype=torch.uint8, device=dev)
    count = torch.zeros((groups,), dtype=torch.int32, device=dev)
    over = torch.zeros((1,), dtype=torch.int32, device=dev)
    with L.device_ctx(dev):
        st = L.lib_for(records).lz_replay_merge_records(L.ptr(records), L.i64(int(records.shape[0])), L.ptr(slots), L.i64(m),
                                                        L.ptr(sym), L.ptr(order), L.ptr(begin), L.i64(groups),
                                                        L.ptr(merged), L.ptr(count), L.ptr(over), L.stream_ptr(dev))
    L.check(st, "replay_window.merge_record_groups")
    return merged, count, over


def check_max_weight(max_weight) -> float:
    """`max_weight` as a float: a finite number >= 1; bools, NaN and everything else: ValueError."""
    if isinstance(max_weight, bool) or not isinstance(max_weight, (int, float)) or not math.isfinite(float(max_weight)) \
            or float(max_weight) < 1.0:
        raise ValueError(f"replay_merge_max_weight must be a finite number >= 1, got {max_weight!r}")
    return float(max_weight)


def merge_weights(group_of_row: torch.Tensor, count: torch.Tensor, ages: Optional[torch.Tensor], age_decay: float,
                  max_weight, span: Optional[int] = None) -> torch.Tensor:
    """float64[groups]: w_g = min(sum over the members of age_decay ** age, max_weight), before normalisation.  No
    floating-point scatter: the members are counted per (group, age) with an integer bincount, then count[g, a] *
    age_weights(a) is added in ascending age.  Without ages, or with a decay of 1, this is min(count, max_weight);
    with no duplicates it is `row_weights.age_weights` bit for bit.  `span`: the ages are known to lie in [0, span)
    (the caller has checked, ages outside are clamped); without it the largest age is read from the device."""
    cap = check_max_weight(max_weight)
    groups = int(count.numel())
    if ages is None or groups == 0:
        return count.to(torch.float64).clamp(max=cap)
    from .row_weights import age_weights, check_age_decay
    decay = check_age_decay(age_decay)
    if decay == 1.0:
        return count.to(torch.float64).clamp(max=cap)
    if span is None:
        lo, hi = (int(v) for v in torch.stack([ages.min(), ages.max()]).tolist())
        if lo < 0:
            raise ValueError("ages must not be negative")
        span = hi + 1
    span = max(1, int(span))
    per = torch.bincount(group_of_row * span + ages.clamp(0, span - 1), minlength=groups * span).view(groups, span)
    scale = age_weights(torch.arange(span, dtype=torch.int64, device=count.device), decay)
    total = torch.zeros((groups,), dtype=torch.float64, device=count.device)
    for a in range(span):
        total = total + per[:, a].to(torch.float64) * scale[a]
    return total.clamp(max=cap)


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
        return gather_records(self.ring, slots, sym, op="ReplayWindow.gather")

    # ---- duplicate positions --------------------------------------------------------------------
    def position_keys(self, slots: torch.Tensor, *, symmetric: bool):
        """(keys int64[m,8], sym int8[m], not_representable int32[1]) of the records at `slots`: what
        `position_dedup.position_keys` gives for their unpacked rows, from the 88 header bytes of each record."""
        return record_position_keys(self.ring, slots, symmetric=symmetric)

    def merge_selection(self, slots: torch.Tensor, *, mode: str, ages: Optional[torch.Tensor] = None,
                        age_decay: float = 1.0, max_weight=1, value_target: str = "mean", soft_label_alpha: float = 0.0):
        """(merged uint8[groups,360], weights float64[groups], info): the selection with duplicate positions merged
        record to record -- keys, `position_dedup.group_rows` (exact, groups by ascending first member), merge.  A
        selection lists the newest generation first, so a group keeps its newest member's frame.  A group's targets are
        the plain mean over its members whatever their age; its weight is min(sum of age_decay ** age over the members,
        max_weight) (`merge_weights`; every member counts 1 without `ages`).  `info`: `position_dedup.STAT_KEYS`, mode,
        max_weight, group_of_row int64[m] and count int32[groups]; one host read.  value_target "distribution"
        (DESIGN.md section 31): `info` gains "value_target", "value_dist" float32[merged_groups,101] -- the mean of the
        members' two-hot value distributions at `soft_label_alpha`, computed straight from the ring through `slots` -- and
        "value_dist_row" int32[groups], -1 for a group of one.  The merged records keep the mean value and soft value."""
        from . import position_dedup as dedup
        if not isinstance(mode, str) or mode not in dedup.MODES[1:]:
            raise ValueError(f"merge_selection needs mode 'exact' or 'symmetric', got {mode!r}")
        distribution = dedup.value_target_on(value_target, mode, name="value_target", needs="mode")
        cap = check_max_weight(max_weight)
        keys, sym, bad = self.position_keys(slots, symmetric=mode == "symmetric")
        slots = slots.reshape(-1).contiguous()
        m = int(slots.numel())
        if ages is not None and (ages.dtype != torch.int64 or int(ages.numel()) != m or ages.device != slots.device):
            raise ValueError(f"ages must hold {m} int64 ages on {slots.device}")
        group_of_row, order, begin, count64 = dedup.group_rows(keys)
        merged, count, over = merge_record_groups(self.ring, slots, sym, order, begin)
        groups = int(count64.numel())
        span = max(1, len(self.table.entries))              # an age is a number of generations behind the newest
        zero = torch.zeros((), dtype=torch.int64, device=slots.device)
        off = zero
        if ages is not None:
            ages = ages.reshape(-1)
            off = ((ages < 0) | (ages >= span)).sum()
        weights = merge_weights(group_of_row, count64, ages, age_decay, cap, span=span)
        big = count64 > 1
        stats = torch.stack([big.sum(), (count64 * big).sum(), count64.max() if groups else zero,
                             bad[0].to(torch.int64) + over[0].to(torch.int64), off]).tolist()     # the one host read
        if stats[4]:
            raise ValueError(f"{int(stats[4])} ages lie outside [0, {span}): the window holds {span} generations")
        info: Dict[str, Any] = {"rows_in": m, "rows_out": groups, "groups": groups, "merged_groups": int(stats[0]),
                                "merged_rows": int(stats[1]), "largest_group": int(stats[2]),
                                "not_representable": int(stats[3]), "mode": mode, "max_weight": cap,
                                "group_of_row": group_of_row, "count": count}
        if distribution:                                    # D = merged_groups came with the one read above
            flat = self.ring.view(-1)
            info["value_target"] = "distribution"
            info["value_dist_row"] = dedup.table_rows(count64)
            info["value_dist"] = dedup.merge_value_distributions(
                flat[348:], flat[352:], RECORD_BYTES, int(self.ring.shape[0]), slots, order, begin, info["value_dist_row"],
                max(0.0, min(1.0, float(soft_label_alpha))), int(stats[0]))
        return merged, weights, info

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
