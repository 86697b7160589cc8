"""Visit-offset / value-cutoff move selection and the temperature half-life of the tree backend's self-play: parameter
validation, the temperature table and the counters.

The rule (per searched game whose move the finish sampled from the visits; N_k the root children's raw visits, q_k their
mean values in the root mover's frame, k* the most visited child, T the game's move temperature, u the pick uniform the
finish consumed): n'_k = N_k - move_visit_offset; a child is eligible if it is k*, or if n'_k > 0 and q_k >= q_k* -
move_value_cutoff (no value test at cutoff 0); the move is drawn with u from the weights (n'_k / n'_k*)^(1/T) over the
eligible children in edge order.  Leela Chess Zero's TempVisitOffset / TempValueCutoff and KataGo's chosenMoveSubtract /
chosenMovePrune are the same idea.  The training targets are never touched.

The rule itself runs on the device (csrc/lz_engine.hip: tree_move_pick_kernel; PortableTreeMCTS.complete_search launches it
between the finish and the solver pick).  What lives here is pure Python and needs no GPU, next to resign.py and
kld_stop.py.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Mapping

import numpy as np

from .kld_stop import _number

# the int64[4] block of lz_tree_move_pick, in its order; all of them add up over parts, chunks, workers and ranks
COUNTER_KEYS = ("move_pick_applied", "move_pick_cut_visits", "move_pick_cut_value", "move_pick_changed")
PARAM_KEYS = ("move_visit_offset", "move_value_cutoff", "temperature_halflife")
VALUE_CUTOFF_MAX = 2.0          # values live in [-1, 1]: a cutoff of 2 cuts nothing


def move_pick_on(move_visit_offset=0.0, move_value_cutoff=0.0) -> bool:
    """Validate the two parameters of the re-pick; True when it is on (either above 0).  move_visit_offset: a finite number
    >= 0; move_value_cutoff: a finite number in [0, 2].  Anything else is a ValueError (whether on or off)."""
    o = _number("move_visit_offset", move_visit_offset, "a number >= 0 (0 = off)")
    if o < 0.0:
        raise ValueError(f"move_visit_offset must be a number >= 0 (0 = off), got {o}")
    c = _number("move_value_cutoff", move_value_cutoff, "a number in [0, 2] (0 = off)")
    if c < 0.0 or c > VALUE_CUTOFF_MAX:
        raise ValueError(f"move_value_cutoff must be a number in [0, 2] (0 = off; values live in [-1, 1]), got {c}")
    return o > 0.0 or c > 0.0


def halflife_on(temperature_halflife=0.0) -> bool:
    """Validate the half-life (a finite number >= 0); True when it is on (above 0)."""
    h = _number("temperature_halflife", temperature_halflife, "a number >= 0 (0 = off)")
    if h < 0.0:
        raise ValueError(f"temperature_halflife must be a number >= 0 (0 = off), got {h}")
    return h > 0.0


def move_pick_kwargs(move_visit_offset=0.0, move_value_cutoff=0.0, temperature_halflife=0.0) -> Dict[str, Any]:
    """The keyword arguments as the next layer down takes them: the two of the re-pick when it is on, the half-life when
    it is on -- {} when everything is off."""
    out: Dict[str, Any] = {}
    if move_pick_on(move_visit_offset, move_value_cutoff):
        out.update(move_visit_offset=float(move_visit_offset), move_value_cutoff=float(move_value_cutoff))
    if halflife_on(temperature_halflife):
        out["temperature_halflife"] = float(temperature_halflife)
    return out


def move_pick_meta(kwargs: Mapping[str, Any]) -> Dict[str, Any]:
    """metadata["move_pick"] of the manifests: the three settings under short names."""
    return {"visit_offset": float(kwargs.get("move_visit_offset", 0.0)),
            "value_cutoff": float(kwargs.get("move_value_cutoff", 0.0)),
            "temperature_halflife": float(kwargs.get("temperature_halflife", 0.0))}


def temperature_table(temperature_init: float, temperature_final: float, temperature_threshold: int,
                      temperature_halflife: float, max_game_plies: int) -> np.ndarray:
    """float32[max_game_plies + 1]: the move temperature of every ply, computed in double and rounded once.
    T(p) = t_final + (t_init - t_final) * 0.5^(p / h) for p < temperature_threshold, t_final from the threshold on;
    h = 0 gives the step (t_init below the threshold).  Indexed on the device by min(ply, max_game_plies)."""
    t0 = _number("temperature_init", temperature_init, "a number")
    t1 = _number("temperature_final", temperature_final, "a number")
    h = float(temperature_halflife) if halflife_on(temperature_halflife) else 0.0
    thr, n = int(temperature_threshold), int(max_game_plies)
    if n < 0:
        raise ValueError(f"max_game_plies must be >= 0, got {max_game_plies!r}")
    table: List[float] = []
    for p in range(n + 1):
        if p >= thr:
            table.append(t1)
        elif h > 0.0:
            table.append(t1 + (t0 - t1) * math.pow(0.5, p / h))
        else:
            table.append(t0)
    return np.asarray(table, dtype=np.float64).astype(np.float32)


def counters_from_block(block) -> Dict[str, int]:
    """The device's int64[4] block -> mcts_counters entries."""
    return {k: int(v) for k, v in zip(COUNTER_KEYS, block)}
