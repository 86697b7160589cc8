"""Gumbel root search with Sequential Halving (Danihelka, Guez, Schrittwieser, Silver: "Policy improvement by planning
with Gumbel", ICLR 2022): parameter validation and the visit schedule of the tree backend's Gumbel mode.

The rule itself runs on the device (csrc/lz_tree_dev.h: the depth-0 block of tree_select, the root-step snapshot, the
Gumbel finish; formulas in include/liuzhou_hip.h at LzTreeDesc.gumbel_*).  What lives here is pure Python and needs no
GPU: `gumbel_on` (validation, next to playout_cap_on / forced_playouts_on of tree_engine) and the schedule that tells the
selection how many visits of this search a considered child has when simulation s starts.
"""
from __future__ import annotations

import math
from typing import List

import numpy as np

MAX_CONSIDERED = 72            # kMaxChildren of csrc/lz_tree_dev.h: a root never has more children


def gumbel_on(considered, c_visit=50.0, c_scale=1.0) -> bool:
    """Validate the Gumbel parameters: `considered` = m, 0 = off, 1..72 = on; `c_visit` and `c_scale` finite and >= 0.
    Anything else is a ValueError."""
    if isinstance(considered, bool) or int(considered) != considered:
        raise ValueError(f"gumbel_considered must be an integer in 0..{MAX_CONSIDERED} (0 = off), got {considered!r}")
    m = int(considered)
    if not 0 <= m <= MAX_CONSIDERED:
        raise ValueError(f"gumbel_considered must lie in 0..{MAX_CONSIDERED} (0 = off), got {m}")
    for name, v in (("gumbel_c_visit", c_visit), ("gumbel_c_scale", c_scale)):
        v = float(v)
        if not math.isfinite(v) or v < 0.0:
            raise ValueError(f"{name} must be a finite number >= 0, got {v}")
    return m > 0


def considered_visits(m: int, n: int) -> List[int]:
    """The visit count (of this search) of the children under consideration when simulation s = 0..n-1 starts, for a root
    of which `m` children are considered and a budget of `n` simulations.

    m <= 1: 0, 1, .., n-1 (every simulation goes to the one child).  Otherwise Sequential Halving: phases over
    c = m, max(2, m // 2), max(2, m // 4), .. considered children; a phase repeats max(1, n // (ceil(log2 m) * c)) rounds,
    each of which appends the current per-child visit count c times and then adds one to it; the last phase (c = 2)
    goes on until n entries exist.  This is the schedule of the paper's published implementation, restated from its
    description."""
    m, n = int(m), int(n)
    if n <= 0:
        return []
    if m <= 1:
        return list(range(n))
    log2m = int(math.ceil(math.log2(m)))
    out: List[int] = []
    visits = 0
    c = m
    while len(out) < n:
        rounds = max(1, n // (log2m * c))
        for _ in range(rounds):
            out.extend([visits] * c)
            visits += 1
            if len(out) >= n:
                break
        c = max(2, c // 2)
    return out[:n]


def considered_table(m: int, n: int) -> np.ndarray:
    """int32[m + 1, n]: row j = considered_visits(j, n), the schedule of a root with j = min(m, children) considered
    children.  Uploaded once per engine (LzTreeDesc.gumbel_table)."""
    m, n = int(m), int(n)
    tab = np.zeros((m + 1, max(n, 0)), dtype=np.int32)
    for j in range(m + 1):
        tab[j, :] = considered_visits(j, n)
    return tab
