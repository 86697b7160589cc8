"""TD(lambda) value targets of the tree backend's self-play: parameter validation.

The rule: for the searched plies t = 0..L-1 of a game, Q_t = current_player_t * root_value_t (the search's root value
from Black's frame), y_L = z (the game's result), y_t = (1 - lambda) Q_t + lambda y_{t+1}; the row recorded at ply t
gets value_target = sign * y_t.  lambda = 1 is the reference's target (the final result for every row) and means off.

The rule itself runs on the device (csrc/lz_ops.hip: wave_note_value_kernel, wave_td_targets_kernel; wave_tail.WaveTail
launches them).  What lives here is pure Python and needs no GPU, next to gumbel.gumbel_on.
"""
from __future__ import annotations

import math


def td_lambda_on(lam) -> bool:
    """Validate `value_target_lambda`: a finite number in [0, 1]; 1 = off (False), anything below = on (True).  Anything
    else is a ValueError."""
    if isinstance(lam, bool):
        raise ValueError(f"value_target_lambda must be a number in [0, 1] (1 = off), got {lam!r}")
    try:
        v = float(lam)
    except (TypeError, ValueError):
        raise ValueError(f"value_target_lambda must be a number in [0, 1] (1 = off), got {lam!r}") from None
    if not math.isfinite(v) or v < 0.0 or v > 1.0:
        raise ValueError(f"value_target_lambda must be a finite number in [0, 1] (1 = off), got {v}")
    return v < 1.0
