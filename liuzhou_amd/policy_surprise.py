"""Policy surprise weighting of training rows in the tree backend's self-play (KataGo's policySurpriseDataWeight; Wu,
"Accelerating Self-Play Learning in Go", and the later methods notes): parameter validation, the root-prior
helper and the counters.

The rule (tests/policy_surprise.py restates it in numpy):

1. Root prior of a recorded ply.  After a ply's search the runner evaluates the searched positions once more with the
   plain network, under the identity symmetry whatever `eval_symmetry` says, and projects the three head rows onto the
   220 actions under the search's legal mask (`project_policy_logits_fast`): `prior float32[G, 220]`, noise-free.  That is
   one extra network launch of G positions per ply beside a search of `mcts_simulations + 1` launches.  The tree's own
   edge priors are not used: fresh roots hold the Dirichlet mix and kept roots a re-normalised re-mix whose denominator is
   not stored, so the raw prior cannot be recovered exactly from them.
2. Surprise of a row: s = max(0, sum over legal actions with pi_a > 0 of pi_a (log pi_a - log max(p_a, 1e-30))) with pi
   the row's recorded policy target (visits, pruned visits, Gumbel's improved policy) and p the prior above; evaluated in
   double, stored as float32.
3. Weights of a finished game with N >= 1 recorded rows and S = sum s_j (double): w_j = (1 - alpha) + alpha N s_j / S if
   S > 1e-12 N, otherwise w_j = 1; sum w_j = N.  With the playout cap only the recorded (full-search) rows take part.
4. Systematic resampling keeps the row count: u = u01 of one Philox draw (csrc/lz_rng.h: purpose 3, ply 0, index 1022),
   a pure function of (seed, game id); with C_0 = 0, C_j = sum_{i<=j} w_i in double and C_N := N exactly, row j is written
   c_j = floor(C_j + u) - floor(C_(j-1) + u) times.  Then sum c_j = N, |c_j - w_j| < 1 and E_u[c_j] = w_j.  Output row k
   is source row src[k], the j whose cumulative count first exceeds k; src is non-decreasing.  All six arena tensors of
   a row move together (state, legal mask, policy, value, soft value, sign).
5. In place: the game's rows are rewritten where they lie, one ascending pass over the slots with src[k] > k, then one
   descending pass over those with src[k] < k (the proof is next to the kernel).

Two deviations from KataGo, both on purpose: only recorded rows take part (KataGo also lets surprising fast-search rows
in, which needs provisional rows), and the counts come from systematic resampling with one uniform per game instead of
an independent rounding per row (so a game keeps exactly its N row slots and no row field is added).

The rule itself runs on the device (csrc/lz_ops.hip: wave_note_surprise_kernel, wave_surprise_resample_kernel, scalar
arithmetic in csrc/lz_surprise.h; wave_tail.WaveTail launches them).  What lives here needs no GPU except `root_prior`.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Sequence

# the int64[3] block of lz_wave_surprise_resample, in its order, then the sum of the surprises in micro-nats; all of them
# add up over chunks, workers and ranks
COUNTER_KEYS = ("surprise_games", "surprise_rows", "surprise_rows_replaced", "surprise_sum_micro")
# derived (does NOT add up: derive_counters() recomputes it after every merge): the mean surprise of a row in micro-nats
# (mcts_counters are integers)
DERIVED_KEYS = ("surprise_mean",)


def policy_surprise_on(alpha) -> bool:
    """Validate `policy_surprise_weight`: a number in [0, 1]; 0 = off (False), anything above = on (True).  Anything
    else, NaN included, is a ValueError."""
    if isinstance(alpha, bool):
        raise ValueError(f"policy_surprise_weight must be a number in [0, 1] (0 = off), got {alpha!r}")
    try:
        v = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"policy_surprise_weight must be a number in [0, 1] (0 = off), got {alpha!r}") from None
    if math.isnan(v) or v < 0.0 or v > 1.0:
        raise ValueError(f"policy_surprise_weight must be a number in [0, 1] (0 = off; KataGo uses 0.5), got {v}")
    return v > 0.0


def root_prior(net, search, fused: bool):
    """`prior float32[G, 220]` of the searched positions: the plain network on `search.model_input` (FusedNet.__call__,
    or the module itself when `fused` is False), identity symmetry, projected under `search.legal_mask`.
    All G slots are evaluated on every ply, finished ones and the fully masked last ply of a wave included (their rows
    are never read): the launch keeps one shape, but late in a draining wave, where the search sizes its own launches by
    the live slots, it is a larger share of the ply than 1 / (simulations + 1).  Every call allocates its outputs (three
    head rows, the value, the two projection outputs).  `FusedNet.__call__` leaves its value output in `net.last_value`;
    that attribute is put back, so a caller that reads it after an evaluation of its own still finds that one."""
    import torch

    from . import v0_core
    from .mcts_gpu import AUXILIARY_DIM, MOVEMENT_DIM, PLACEMENT_DIM, SELECTION_DIM
    x = search.model_input
    if fused:
        kept = getattr(net, "last_value", None)
        lp1, lp2, lpm, _ = net(x, want_logits=False)
        net.last_value = kept
    else:
        where = next(net.parameters()).device
        with torch.inference_mode():
            lp1, lp2, lpm = (t.float().to(x.device).contiguous() for t in net(x.to(where))[:3])
    legal = search.legal_mask if search.legal_mask.dtype == torch.bool else search.legal_mask.bool()
    probs, _ = v0_core.project_policy_logits_fast(lp1.float(), lp2.float(), lpm.float(), legal, PLACEMENT_DIM,
                                                  MOVEMENT_DIM, SELECTION_DIM, AUXILIARY_DIM)
    return probs


def derive_counters(counters: Dict[str, Any]) -> Dict[str, Any]:
    """(Re)compute surprise_mean, in place, from the sums -- after a run and after every merge of runs."""
    if "surprise_rows" not in counters:
        return counters
    rows = int(counters.get("surprise_rows", 0))
    counters["surprise_mean"] = int(round(int(counters.get("surprise_sum_micro", 0)) / rows)) if rows else 0
    return counters


def counters_from_block(block: Sequence[int], surprise_sum: float) -> Dict[str, int]:
    """The device's int64[3] block and its double sum of surprises -> mcts_counters entries (sums and derived)."""
    d = {k: int(v) for k, v in zip(COUNTER_KEYS, block)}
    d["surprise_sum_micro"] = int(round(float(surprise_sum) * 1e6))
    return derive_counters(d)


def surprise_meta(alpha: float, counters: Dict[str, Any]) -> Dict[str, Any]:
    """metadata["policy_surprise"] of the manifests."""
    rows = int(counters.get("surprise_rows", 0))
    return {"weight": float(alpha), "games": int(counters.get("surprise_games", 0)), "rows": rows,
            "rows_replaced": int(counters.get("surprise_rows_replaced", 0)),
            "mean_surprise": (int(counters.get("surprise_sum_micro", 0)) / 1e6 / rows) if rows else 0.0}
