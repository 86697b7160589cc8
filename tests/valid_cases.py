"""Inputs of the validation-metric tests (tests/test_valid_ref_cpu.py, tests/test_gpu_validation.py): hand-built row
classes for the row kernel and batches of rows for the reduction.  Deterministic; numpy only."""
import functools

import numpy as np

from tests import valid_ref as VR
from tests.train_loss_ref import BINS, TOTAL

INPUT_KEYS = ("lp1", "lp2", "lpm", "vlogits", "mask", "target", "value", "soft")      # the order of the loss kernel
ROW_B = (1, 3, 4, 5, 257)
ROW_OFFSET = {1: 0, 3: 1, 4: 4, 5: 6, 257: 0}            # where a small batch starts inside the 257 rows
ALPHAS = (0.0, 0.3, 1.0)
REDUCE_B = (1, 63, 64, 65, 130)
Z_VALUES = (-1.0, 0.0, 1.0, -0.74, 0.54, 0.27, 0.29, 0.37, -0.37, 5e-9, -0.0, 0.999)
MARGIN = 1e-3
FORCED = ("none", "single", "n72", "last219", "four_ranges", "zero_target", "neginf", "tie_pp", "tie_ps", "tie_target",
          "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "all_neginf", "wide", "onehot_target")


def _log_softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def _margin_ok(comb, legal, target):
    """>= MARGIN between the best and the second-best legal logit, and the two best targets differ."""
    idx = np.flatnonzero(legal)
    if idx.size < 2:
        return True
    c = np.sort(comb[idx])[::-1]
    t = np.sort(target[idx].astype(np.float64))[::-1]
    return bool(c[0] - c[1] >= MARGIN or not np.isfinite(c[0])) and bool(t[0] - t[1] >= 1e-4 or t[0] == 0)


def _row(kind, rng, i):
    heads = _log_softmax(rng.standard_normal((3, 36)) * (25.0 if kind == "wide" else 1.0))
    mask = np.zeros(TOTAL, np.uint8)
    if kind == "none":
        pass
    elif kind == "single":
        mask[int(rng.integers(0, TOTAL))] = 1
    elif kind == "n72":
        mask[rng.choice(VR_ON_BOARD, 72, replace=False)] = 1
    elif kind == "last219":
        mask[[3, 100, 219]] = 1
    elif kind == "four_ranges":
        mask[[0, 35, 37, 178, 180, 215, 219]] = 1
    elif kind in ("tie_pp", "tie_ps", "all_neginf"):
        mask[rng.choice(36, 6, replace=False)] = 1
        mask[180 + rng.choice(36, 6, replace=False)] = 1
    else:
        mask[rng.choice(VR_ON_BOARD, int(rng.integers(3, 40)), replace=False)] = 1
    legal = np.flatnonzero(mask)
    tie = None
    if kind == "neginf" and legal.size:                   # -inf head cells under legal actions, at least one stays finite
        for a in legal[: max(1, legal.size // 2)]:
            if a < 36:
                heads[0, a] = -np.inf
            elif a < 180:
                heads[1, (a - 36) >> 2] = -np.inf
            elif a < 216:
                heads[2, a - 180] = -np.inf
        mask[216] = 1                                     # the auxiliary logit 0 is always finite
        legal = np.flatnonzero(mask)
    if kind == "all_neginf":
        heads[0, legal[legal < 36]] = -np.inf
        heads[2, legal[legal >= 180] - 180] = -np.inf
    if kind == "tie_pp":
        a, b = legal[legal < 36][:2]
        heads[0, a] = heads[0, b] = np.float32(0.75)      # above every log-probability
        tie = (int(a), int(b))
    if kind == "tie_ps":
        a, b = legal[legal < 36][-1], legal[legal >= 180][0]
        heads[0, a] = heads[2, b - 180] = np.float32(0.5)
        tie = (int(a), int(b))
    target = np.zeros(TOTAL, np.float32)
    if legal.size and kind != "zero_target":
        if kind in ("single", "last219", "onehot_target"):
            target[legal[-1]] = 1.0
        elif kind == "tie_target" and legal.size >= 3:
            w = rng.random(legal.size).astype(np.float32) * 0.1
            target[legal] = w * np.float32(0.4 / w.sum())
            target[legal[1]] = target[legal[-1]] = np.float32(0.3)
        else:
            w = rng.random(legal.size) ** 3 + 1e-3
            target[legal] = (w / w.sum()).astype(np.float32)
    vlogits = (2.0 * rng.standard_normal(BINS)).astype(np.float32)
    if kind[0] == "v" and kind[1:].isdigit():             # v_hat well inside calibration bin k
        vlogits = np.zeros(BINS, np.float32)
        vlogits[5 + 10 * int(kind[1:])] = 12.0
    phase = i % 8 - 1                                     # -1: no phase plane
    planes = np.zeros((11, 36), np.float32)
    planes[:4] = rng.random((4, 36)) < 0.3
    if phase >= 0:
        planes[4 + phase] = 1.0
    return dict(lp1=heads[0], lp2=heads[1], lpm=heads[2], vlogits=vlogits, mask=mask, target=target,
                value=np.float32(Z_VALUES[i % len(Z_VALUES)]), soft=np.float32(rng.uniform(-1, 1)),
                planes=planes.reshape(11, 6, 6), kind=kind, tie=tie)


VR_ON_BOARD = None


@functools.lru_cache(maxsize=None)
def row_batch_full(seed=20261020):
    """257 rows: the forced classes first, random ones after.  Every row without a built-in tie keeps MARGIN between its
    two best legal logits and a gap between its two best targets."""
    global VR_ON_BOARD
    from tests.train_loss_cases import ON_BOARD_ACTIONS
    VR_ON_BOARD = np.array(ON_BOARD_ACTIONS)
    rows = []
    for i in range(257):
        kind = FORCED[i] if i < len(FORCED) else ("wide" if i % 5 == 0 else "neginf" if i % 7 == 0 else "random")
        for attempt in range(100):
            r = _row(kind, np.random.default_rng([seed, i, attempt]), i)
            comb = VR.combined(r["lp1"][None], r["lp2"][None], r["lpm"][None])[0]
            if kind in ("tie_pp", "tie_ps", "tie_target", "all_neginf") or _margin_ok(comb, r["mask"], r["target"]):
                break
        else:
            raise AssertionError(f"no row of kind {kind} with the margin")
        rows.append(r)
    c = {k: np.stack([r[k] for r in rows]) for k in INPUT_KEYS + ("planes",)}
    c["kind"] = np.array([r["kind"] for r in rows])
    c["tie"] = [r["tie"] for r in rows]
    return c


def row_batch(B):
    full, o = row_batch_full(), ROW_OFFSET[B]
    return {k: (v[o:o + B].copy() if isinstance(v, np.ndarray) else v[o:o + B]) for k, v in full.items()}


def policy_class(c):
    return np.where(c["kind"] == "wide", "wide", "base")


def value_class(c):
    return np.full(len(c["kind"]), "base")


# ---- batches for the reduction ---------------------------------------------------------------------------------------------
def reduce_batch(B, seed, mode="mixed"):
    """rows f32[B,12] over many magnitudes (so that the association shows), cls consistent with the rules, value, planes.
    mode: "mixed", "one_group" (every row phase 3, bin 4), "all_skipped", ("bad", column, value)."""
    rng = np.random.default_rng([seed, B])
    rows = (rng.standard_normal((B, 12)) * 10.0 ** rng.integers(-6, 7, (B, 12))).astype(np.float32)
    rows[:, VR.V_HAT] = rng.uniform(-1.3, 1.3, B).astype(np.float32)
    rows[:, [VR.TOP1, VR.SIGN_OK, VR.DECISIVE, VR.POLICY_VALID]] = rng.integers(0, 2, (B, 4))
    phase = rng.integers(-1, 7, B).astype(np.int32)
    if mode == "one_group":
        phase[:] = 3
        rows[:, VR.V_HAT] = np.float32(-0.1)
    planes = np.zeros((B, 11, 36), np.float32)
    for i in range(B):
        if phase[i] >= 0:
            planes[i, 4 + phase[i]] = 1.0
    if mode == "all_skipped":
        rows[np.arange(B), rng.integers(0, 12, B)] = np.nan
        rows[:, VR.V_HAT] = np.where(np.isnan(rows[:, VR.V_HAT]), np.nan, rows[:, VR.V_HAT])
    elif isinstance(mode, tuple):
        _, col, bad = mode
        rows[::3, col] = bad
    cls = np.zeros((B, 4), np.int32)
    cls[:, 0] = phase
    cls[:, 1] = VR.calib_bin(rows[:, VR.V_HAT])
    cls[:, 2:] = rng.integers(-1, 220, (B, 2))
    value = rng.choice(np.array([-1.0, 0.0, 1.0, 0.3], np.float32), B)
    return rows, cls, value, planes.reshape(B, 11, 6, 6)
