"""Checker of the TD(lambda) value targets: the float64 sequential recurrence, nothing else."""
import numpy as np


def td_lambda_targets(q, z, lam):
    """y[t] = (1 - lam) * q[t] + lam * y[t + 1] for t = L-1 .. 0 with y[L] = z, in float64, one step after the other.
    `q`: the root values of the game's searched plies from Black's frame; `z`: the result from Black's frame."""
    q = np.asarray(q, dtype=np.float64)
    lam = float(lam)
    y = np.empty(q.shape[0], dtype=np.float64)
    nxt = float(z)
    for t in range(q.shape[0] - 1, -1, -1):
        nxt = (1.0 - lam) * q[t] + lam * nxt
        y[t] = nxt
    return y
