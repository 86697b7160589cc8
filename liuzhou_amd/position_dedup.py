"""Merge duplicate positions among training rows, up to board symmetry.

Every game starts from the empty board, so one iteration's rows hold the same early positions thousands of times, each
copy with its own noised visit distribution and its own single-game outcome.  The mean of those targets is what the
search bought: `merge_duplicate_positions` groups the rows by position (mode "exact") or by position up to the eight
board symmetries (mode "symmetric") and returns one row per group -- the first member's planes and mask, the members'
policy, value and soft value averaged in the first member's frame.  `max_copies` M emits a group min(count, M) times;
with `weighting="weight"` a group leaves once and min(count, M) is its row weight instead.

The keys and the merged rows come from the kernels of csrc/lz_dedup.hip for HIP tensors and from the host build of the
same C ABI for CPU tensors (csrc/lz_dedup_host.cpp); both compile the scalar arithmetic of csrc/lz_dedup.h.  The exact
grouping between the two launches -- sort, boundaries, group order by first member, replication -- is PyTorch.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Tuple

import torch

from . import _lib as L

MODES = ("off", "exact", "symmetric")
WEIGHTINGS = ("copies", "weight")
VALUE_TARGETS = ("mean", "distribution")
VALUE_BINS = 101
NUM_ACTIONS = 220
STAT_KEYS = ("rows_in", "rows_out", "groups", "merged_groups", "merged_rows", "largest_group", "not_representable")


def dedup_on(mode, max_copies=1) -> bool:
    """Validate the two parameters (on or off alike) and say whether the merge runs."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"dedup_positions must be one of {MODES}, got {mode!r}")
    if isinstance(max_copies, bool) or (isinstance(max_copies, float) and not math.isfinite(max_copies)):
        raise ValueError(f"dedup_max_copies must be an integer >= 1, got {max_copies!r}")
    try:
        whole = int(max_copies) == max_copies
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or int(max_copies) < 1:
        raise ValueError(f"dedup_max_copies must be an integer >= 1, got {max_copies!r}")
    return mode != "off"


def weighting_on(weighting, mode="off", max_copies=1) -> bool:
    """Validate `dedup_weighting` (dedup on or off alike) and say whether groups leave once with a row weight."""
    if not isinstance(weighting, str) or weighting not in WEIGHTINGS:
        raise ValueError(f"dedup_weighting must be one of {WEIGHTINGS}, got {weighting!r}")
    if weighting == "weight" and not dedup_on(mode, max_copies):
        raise ValueError("dedup_weighting='weight' needs dedup_positions 'exact' or 'symmetric': with dedup_positions="
                         f"{mode!r} there are no groups to weigh")
    return weighting == "weight"


def value_target_on(value_target, mode="off", max_copies=1, *, name: str = "dedup_value_target",
                    needs: str = "dedup_positions") -> bool:
    """Validate a value-target keyword (merge on or off alike) and say whether merged groups are trained on the
    distribution of their members' value targets."""
    if not isinstance(value_target, str) or value_target not in VALUE_TARGETS:
        raise ValueError(f"{name} must be one of {VALUE_TARGETS}, got {value_target!r}")
    if value_target == "distribution" and not dedup_on(mode, max_copies):
        raise ValueError(f"{name}='distribution' needs {needs} 'exact' or 'symmetric': with {needs}={mode!r} there are "
                         "no groups to describe")
    return value_target == "distribution"


def table_rows(count64: torch.Tensor) -> torch.Tensor:
    """int32[groups]: the row of the value-distribution table of every group -- groups of more than one member are
    numbered in order, a group of one gets -1 (its two-hot is what the loss computes from its value).  No host read."""
    merged = count64 > 1
    return torch.where(merged, torch.cumsum(merged, 0) - 1, torch.full_like(count64, -1)).to(torch.int32)


def merge_value_distributions(value_base: torch.Tensor, soft_base: torch.Tensor, stride_bytes: int, n: int, index,
                              order: torch.Tensor, begin: torch.Tensor, dist_row: torch.Tensor, alpha: float,
                              rows: int) -> torch.Tensor:
    """float32[rows,101]: the table of include/liuzhou_hip.h: lz_merge_value_distributions.  `value_base` / `soft_base`
    are tensors whose first byte is element 0's value / soft value (float32 [n] with stride 4, or views into a ring of
    records with stride 360 and `index` = the selection's slots).  HIP tensors go to the kernel, CPU tensors to the host
    build.  Rows no group points at stay zero."""
    dev = order.device
    dist = torch.zeros((int(rows), VALUE_BINS), dtype=torch.float32, device=dev)
    groups = int(begin.numel()) - 1
    with L.device_ctx(dev):
        st = L.lib_for(order).lz_merge_value_distributions(
            L.ptr(value_base), L.ptr(soft_base), L.i64(stride_bytes), L.i64(n), L.ptr(index), L.i64(int(order.numel())),
            L.ptr(order), L.ptr(begin), L.i64(groups), L.ptr(dist_row), float(alpha), L.ptr(dist), L.i64(int(rows)),
            L.stream_ptr(dev))
    L.check(st, "position_dedup.merge_value_distributions")
    return dist


def group_weights(count: torch.Tensor, max_copies: int = 1) -> torch.Tensor:
    """float64[groups]: the row weight of each merged group before normalisation, min(count, max_copies) -- what
    `max_copies` copies of the group's row weigh together.  `count` is `info["count"]`."""
    if isinstance(max_copies, bool) or int(max_copies) != max_copies or int(max_copies) < 1:
        raise ValueError(f"dedup_max_copies must be an integer >= 1, got {max_copies!r}")
    return count.to(torch.int64).clamp(max=int(max_copies)).to(torch.float64)


def dedup_refusal(mode, max_copies=1, *, policy_draw_weight: float = 1.0, anti_draw_penalty: float = 0.0) -> None:
    """The trainer's refusals: both options key on |value| < 1e-8 meaning "this game was drawn", which a mean of
    results no longer means."""
    if not dedup_on(mode, max_copies):
        return
    if float(policy_draw_weight) != 1.0:
        raise ValueError(f"dedup_positions={mode!r} cannot be combined with policy_draw_weight={policy_draw_weight!r}: "
                         "a merged row's value is a mean of results, |value| < 1e-8 no longer marks a drawn game")
    if abs(float(anti_draw_penalty)) > 1e-9:
        raise ValueError(f"dedup_positions={mode!r} cannot be combined with anti_draw_penalty={anti_draw_penalty!r}: "
                         "a merged row's value is a mean of results, |value| < 1e-8 no longer marks a drawn game")


def _rows(planes: torch.Tensor, masks: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, int]:
    if not isinstance(planes, torch.Tensor) or not isinstance(masks, torch.Tensor):
        raise TypeError("planes and masks must be tensors")
    if planes.dtype != torch.float32:
        raise TypeError("planes must be float32")
    if masks.dtype not in (torch.bool, torch.uint8):
        raise TypeError("masks must be bool or uint8")
    n = int(planes.shape[0]) if planes.dim() else -1
    if n < 0 or planes.numel() != n * 396:
        raise ValueError(f"planes must be [n,11,6,6] or [n,11,36], got {tuple(planes.shape)}")
    if masks.numel() != n * NUM_ACTIONS or (masks.dim() and int(masks.shape[0]) != n):
        raise ValueError(f"masks must be [{n},220], got {tuple(masks.shape)}")
    if masks.device != planes.device:
        raise ValueError(f"all tensors must live on {planes.device}")
    return planes.reshape(n, 396).contiguous(), masks.reshape(n, NUM_ACTIONS).contiguous(), n


def position_keys(planes: torch.Tensor, masks: torch.Tensor, *, symmetric: bool):
    """(keys int64[n,8], sym int8[n], not_representable int32[1]) of planes float32[n,11,6,6] and masks bool / uint8
    [n,220]: the key words and the symmetry k* of every row (include/liuzhou_hip.h: lz_dedup_position_keys).  The
    counter stays on the rows' device; nothing is read back."""
    pl, mk, n = _rows(planes, masks)
    dev = pl.device
    keys = torch.empty((n, 8), dtype=torch.int64, device=dev)
    sym = torch.empty((n,), dtype=torch.int8, device=dev)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    with L.device_ctx(dev):
        st = L.lib_for(pl).lz_dedup_position_keys(L.ptr(pl), L.ptr(mk), L.i64(n), 1 if symmetric else 0, L.ptr(keys),
                                                  L.ptr(sym), L.ptr(bad), L.stream_ptr(dev))
    L.check(st, "position_dedup.position_keys")
    return keys, sym, bad


def group_rows(keys: torch.Tensor):
    """Exact grouping of int64[n,8] keys: (group_of_row int64[n], order int64[n], group_begin int64[groups+1],
    count int64[groups]).  Groups are numbered by ascending first member; `order` lists the rows group by group,
    ascending inside a group."""
    n = int(keys.shape[0])
    dev = keys.device
    if n == 0:
        empty = torch.zeros((0,), dtype=torch.int64, device=dev)
        return empty, empty.clone(), torch.zeros((1,), dtype=torch.int64, device=dev), empty.clone()
    uniq, inverse = torch.unique(keys, dim=0, return_inverse=True)    # all eight words decide, no hash
    inverse = inverse.view(-1)
    groups = int(uniq.shape[0])
    rows = torch.arange(n, dtype=torch.int64, device=dev)
    first = torch.full((groups,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, inverse, rows, "amin")
    rank = torch.empty((groups,), dtype=torch.int64, device=dev)
    rank[torch.argsort(first)] = torch.arange(groups, dtype=torch.int64, device=dev)
    group_of_row = rank.index_select(0, inverse)
    order = torch.argsort(group_of_row, stable=True)
    count = torch.bincount(group_of_row, minlength=groups)
    begin = torch.zeros((groups + 1,), dtype=torch.int64, device=dev)
    begin[1:] = torch.cumsum(count, 0)
    return group_of_row, order, begin, count


def merge_duplicate_positions(planes: torch.Tensor, masks: torch.Tensor, policy: torch.Tensor, values: torch.Tensor,
                              soft: torch.Tensor, *, mode: str, max_copies: int = 1, weighting: str = "copies",
                              value_target: str = "mean", soft_label_alpha: float = 0.0):
    """((planes, masks, policy, values, soft), info): the rows with duplicate positions merged.

    planes float32[n,11,6,6] (or [n,11,36]); masks bool / uint8 [n,220]; policy float32[n,220]; values and soft
    float32[n].  mode "exact" or "symmetric".  Groups leave in the order of their first members, each min(count,
    max_copies) times.  `info` holds the stats (`STAT_KEYS`, "mode", "max_copies"; one host read), `group_of_row`
    int64[n] and `count` int32[groups].  weighting "weight": each group leaves once, and `info` gains "weighting" and
    "weights" = `group_weights(count, max_copies)`, one per row that leaves.  value_target "distribution" (DESIGN.md
    section 31): `info` gains "value_target", "value_dist" float32[merged_groups,101] -- per group of more than one member
    the mean of its members' two-hot value distributions at `soft_label_alpha` (clamped to [0, 1] as the trainers clamp it)
    -- and "value_dist_row" int32, one per row that leaves: its row of the table, -1 for a group of one.  The rows keep
    their mean value and soft value."""
    if not dedup_on(mode, max_copies):
        raise ValueError("merge_duplicate_positions needs mode 'exact' or 'symmetric'")
    weighted = weighting_on(weighting, mode, max_copies)
    distribution = value_target_on(value_target, mode, max_copies, name="value_target", needs="mode")
    copies = int(max_copies)
    pl, mk, n = _rows(planes, masks)
    dev = pl.device
    for name, t in (("policy", policy), ("values", values), ("soft", soft)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor")
        if t.device != dev:
            raise ValueError(f"all tensors must live on {dev}")
    if policy.numel() != n * NUM_ACTIONS or values.numel() != n or soft.numel() != n:
        raise ValueError(f"policy must be [{n},220], values and soft [{n}]")
    pol, val, sof = policy.reshape(n, NUM_ACTIONS).contiguous(), values.reshape(n).contiguous(), soft.reshape(n).contiguous()
    keys, sym, bad = position_keys(pl, mk, symmetric=mode == "symmetric")
    group_of_row, order, begin, count64 = group_rows(keys)
    groups = int(count64.numel())
    out_planes = torch.empty((groups,) + tuple(planes.shape[1:]), dtype=torch.float32, device=dev)
    out_masks = torch.empty((groups, NUM_ACTIONS), dtype=mk.dtype, device=dev)
    out_policy = torch.empty((groups, NUM_ACTIONS), dtype=torch.float32, device=dev)
    out_values = torch.empty((groups,), dtype=torch.float32, device=dev)
    out_soft = torch.empty((groups,), dtype=torch.float32, device=dev)
    count = torch.zeros((groups,), dtype=torch.int32, device=dev)
    with L.device_ctx(dev):
        st = L.lib_for(pl).lz_dedup_merge_groups(
            L.ptr(pl), L.ptr(mk), L.ptr(pol), L.ptr(val), L.ptr(sof), L.i64(n), L.ptr(sym), L.ptr(order), L.ptr(begin),
            L.i64(groups), L.ptr(out_planes), L.ptr(out_masks), L.ptr(out_policy), L.ptr(out_values), L.ptr(out_soft),
            L.ptr(count), L.stream_ptr(dev))
    L.check(st, "position_dedup.merge_duplicate_positions")
    reps = count64.clamp(max=1 if weighted else copies)
    merged = count64 > 1
    zero = torch.zeros((), dtype=torch.int64, device=dev)
    stats = torch.stack([reps.sum(), merged.sum(), (count64 * merged).sum(), count64.max() if groups else zero,
                         bad[0].to(torch.int64)]).tolist()             # the one host read of the stats
    outs = (out_planes, out_masks, out_policy, out_values, out_soft)
    dist = dist_row = None
    if distribution:                                                  # D = merged_groups came with the one read above
        dist_row = table_rows(count64)
        dist = merge_value_distributions(val, sof, 4, n, None, order, begin, dist_row,
                                         max(0.0, min(1.0, float(soft_label_alpha))), int(stats[1]))
    if stats[0] != groups:                                            # some group leaves more than once
        take = torch.repeat_interleave(torch.arange(groups, dtype=torch.int64, device=dev), reps, output_size=int(stats[0]))
        outs = tuple(t.index_select(0, take) for t in outs)
        if distribution:
            dist_row = dist_row.index_select(0, take)                 # every copy of a group points at the group's row
    info: Dict[str, Any] = {"rows_in": n, "rows_out": int(stats[0]), "groups": groups, "merged_groups": int(stats[1]),
                            "merged_rows": int(stats[2]), "largest_group": int(stats[3]),
                            "not_representable": int(stats[4]), "mode": mode, "max_copies": copies,
                            "group_of_row": group_of_row, "count": count}
    if weighted:
        info["weighting"] = "weight"
        info["weights"] = group_weights(count, copies)
    if distribution:
        info["value_target"] = "distribution"
        info["value_dist"], info["value_dist_row"] = dist, dist_row
    return outs, info


def stats_of(info: Dict[str, Any]) -> Dict[str, Any]:
    """The plain-number part of `info` (what the trainer's metrics carry)."""
    return {k: info[k] for k in STAT_KEYS + ("mode", "max_copies") + (("weighting",) if "weighting" in info else ())
            + (("value_target",) if "value_target" in info else ())}
