"""Sequential restatement of the resignation rule for ONE game (numpy only; the checker of the resignation tests).

`plies`: the game's searched plies in order, each (mover +1 / -1, phase, root value as np.float32 in the mover's frame,
root is terminal).  Returns (resign ply or None, would, would_ply): the ply at which the game resigns (its mover loses),
and for a play-through game the side and ply of the first time it wanted to resign (0, -1 when it never did)."""
import numpy as np

PHASE_PLACEMENT, PHASE_MOVEMENT, PHASE_CAPTURE_SELECTION, PHASE_COUNTER_REMOVAL = 1, 4, 5, 7
MOVEMENT_PHASES = (PHASE_MOVEMENT, PHASE_CAPTURE_SELECTION, PHASE_COUNTER_REMOVAL)


def resign_rule(plies, threshold, min_moves=10, consecutive=3, streak="side", playthrough=False):
    thr = np.float32(threshold)
    count = {1: 0, -1: 0, "ply": 0}
    would, would_ply = 0, -1
    for p, (mover, phase, value, terminal) in enumerate(plies):
        mover = 1 if mover >= 0 else -1
        eligible = phase in MOVEMENT_PHASES and p >= min_moves and not terminal
        low = bool(eligible and np.float32(value) <= thr)              # a NaN compares false
        if streak == "ply":
            count["ply"] = count["ply"] + 1 if low else 0
            c = count["ply"]
        elif not eligible:
            count[1] = count[-1] = c = 0
        else:
            count[mover] = c = count[mover] + 1 if low else 0
        if low and c >= consecutive:
            if not playthrough:
                return p, would, would_ply
            if would == 0:
                would, would_ply = mover, p
    return None, would, would_ply
