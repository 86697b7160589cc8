"""Restatements of the per-row weights, for the tests only (numpy on the CPU).

`ref_loss_weighted`: lz_policy_value_loss_weighted_fwd_bwd in float64.  The row weight rw enters every gradient of its
row linearly and no term but the weight column, so it is tests/train_loss_ref.py::ref_loss with the rows of g1, g2, g3
and gv multiplied by float64(rw) and terms[:, 1] = float32(draw weight * rw).  tests/test_row_weights_cpu.py anchors this
without the linearity argument: integer weights against ref_loss on a batch that repeats the rows.

`ref_normalise`: the trainers' one normalisation rule.  `ref_ages` / `ref_age_weights`: the age of every row a replay
window selects, from the generation table alone, and decay ** age."""
import math

import numpy as np

from tests import train_loss_cases as K
from tests.train_loss_ref import ref_loss

WEIGHT_CYCLE = (1.0, 0.0, 0.5, 2.0, 3.0, 0.1, 1e-3, 255.0, 1e4)


def cycle_weights(B):
    return np.array([WEIGHT_CYCLE[i % len(WEIGHT_CYCLE)] for i in range(B)], np.float32)


def ref_loss_weighted(c, row_weight, setting, weight_sum, grad_scale=1.0):
    """c: a case dict of tests/train_loss_cases.py; row_weight float32 [B] -> the keys of ref_loss, float64."""
    r = dict(ref_loss(*(c[k] for k in K.INPUT_KEYS), alpha=setting[0], anti_draw=setting[1], draw_weight=setting[2],
                      weight_sum=weight_sum, grad_scale=grad_scale))
    rw32 = np.asarray(row_weight, np.float32).reshape(-1)
    rw = rw32.astype(np.float64)
    for name in ("g1", "g2", "g3", "gv"):
        r[name] = r[name] * rw[:, None]
    terms = r["terms"].copy()
    terms[:, 1] = (terms[:, 1].astype(np.float32) * rw32).astype(np.float64)       # the float32 product the kernel stores
    r["terms"] = terms
    return r


def repeat_rows(c, counts):
    """The case with row i repeated counts[i] times (copies adjacent) -> (case, owner of every new row)."""
    owner = np.repeat(np.arange(len(counts)), counts)
    return {k: np.ascontiguousarray(np.asarray(c[k])[owner]) for k in K.INPUT_KEYS}, owner


def ref_normalise(w):
    """float32 weights with mean one: (w * (n / sum(w))) in float64, rounded once.  ValueError as the trainers raise it."""
    w = np.asarray(w, np.float64).reshape(-1)
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights are negative or not finite")
    s = math.fsum(w.tolist())
    if not s > 0.0:
        raise ValueError("the weights sum to zero")
    return (w * (len(w) / s)).astype(np.float32)


def ref_ages(entries, budget):
    """entries: [(id, first slot, count)] oldest first, as GenerationTable.entries -> [(age, rows taken)] in selection order
    (newest first): every row of the newest generation, min(count, budget) of each older one, budget <= 0 meaning
    newest count // number of older generations; generations that give no row are left out but still count as an age."""
    if not entries:
        return []
    newest = entries[-1]
    older = len(entries) - 1
    if budget <= 0:
        budget = newest[2] // older if older else 0
    out = [(0, newest[2])]
    for age, (_, _, count) in enumerate(reversed(entries[:-1]), start=1):
        take = min(count, budget)
        if take > 0:
            out.append((age, take))
    return out


def ref_age_weights(entries, budget, decay):
    """float64 decay ** age of every selected row, before normalisation."""
    parts = [np.full(take, float(decay) ** age, np.float64) for age, take in ref_ages(entries, budget)]
    return np.concatenate(parts) if parts else np.zeros(0, np.float64)
