"""Per-row sample weights of the trainers: validation, the one normalisation rule, age weights.

The fused loss takes a weight per row as an absolute multiplier (`train_loss.fused_policy_value_loss(row_weights=...)`);
the trainers decide what the numbers mean.  Every consumer -- the caller's own `row_weights`, the merged groups of
`dedup_weighting="weight"`, the generations of `replay_age_decay` -- sends its weights through `normalise_row_weights`
once per call: mean one over the rows actually trained on, so the loss and the step size keep their scale and uniform
weights of any value are no weights at all.  Imported only when a weighting is on.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Tuple

import torch
import torch.distributed as dist


def normalise_row_weights(weights: torch.Tensor, *, source: str = "row_weights", ddp: bool = False
                          ) -> Tuple[torch.Tensor, Dict[str, Any]]:
    """(float32[n] with mean one, info) of weights [n]: `(w.double() * (n / w.double().sum())).float()`.  Under DDP n and
    the sum are all-reduced (SUM), so the mean is one over the rows of all ranks.  The single host read validates:
    every weight finite and >= 0, the sum > 0, else ValueError (on every rank alike).  `info`: the `row_weights` entry
    of the trainer's metrics -- source, min and max before normalisation and the number of zero weights (of this rank)."""
    if not isinstance(weights, torch.Tensor):
        weights = torch.as_tensor(weights)
    if weights.dim() != 1 or weights.is_complex() or weights.dtype == torch.bool:
        raise ValueError(f"{source}: expected one real weight per row, got {weights.dtype} {tuple(weights.shape)}")
    w = weights.double()
    n = int(w.numel())
    ok = torch.isfinite(w) & (w >= 0)
    clean = torch.where(ok, w, torch.zeros_like(w))
    inf = torch.full((), float("inf"), dtype=torch.float64, device=w.device)
    total = torch.stack([clean.sum(), torch.full((), float(n), dtype=torch.float64, device=w.device),
                         (~ok).sum().double()])
    if ddp:
        dist.all_reduce(total, op=dist.ReduceOp.SUM)
    local = torch.stack([clean.min() if n else inf, clean.max() if n else -inf, (clean == 0).sum().double()])
    s, rows, bad, lo, hi, zeros = torch.cat([total, local]).tolist()          # the one host read
    if bad > 0:
        raise ValueError(f"{source}: {int(bad)} weights are negative or not finite")
    if not s > 0.0:
        raise ValueError(f"{source}: the weights sum to {s!r}, nothing would be trained on")
    w32 = (w * (rows / s)).float()
    return w32, {"source": source, "min": float(lo), "max": float(hi), "zero_weight_rows": int(zeros)}


def check_age_decay(decay) -> float:
    """`replay_age_decay` as a float in (0, 1]; bools, NaN and everything else: ValueError."""
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or math.isnan(float(decay)) or \
            not 0.0 < float(decay) <= 1.0:
        raise ValueError(f"replay_age_decay must be a number in (0, 1], got {decay!r}")
    return float(decay)


def age_weights(ages: torch.Tensor, decay: float) -> torch.Tensor:
    """float64 decay ** age for int64 ages (`ReplayWindow.select(..., return_ages=True)`), before normalisation."""
    return torch.pow(torch.full((), check_age_decay(decay), dtype=torch.float64, device=ages.device), ages.double())
