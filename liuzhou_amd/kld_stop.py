"""KLD-gain early stopping of the tree backend's searches: parameter validation.

The rule (Leela Chess Zero's, per game at the root): every `kld_stop_interval` simulations the root's visit distribution
is compared with the one `kld_stop_interval` simulations earlier.  With o_k the visits of child k in the game's snapshot,
n_k the visits now, O = sum o_k and N = sum n_k, the information gained is
    gain = sum_{k: o_k > 0} (o_k / O) * ln((o_k * N) / (n_k * O)),
the Kullback-Leibler divergence of the old distribution from the new one, and the search stops when gain / (N - O) falls
below `kld_stop_threshold` -- not before `kld_stop_min_simulations` simulations.  A stopped game keeps the leaf it has
already selected: its budget becomes the check's simulation + 1, which the playout cap's kernels already understand.

The rule itself runs on the device (csrc/lz_engine.hip: tree_kld_check_kernel, enqueued by lz_tree_search between the
launches of a captured search).  What lives here is pure Python and needs no GPU, next to resign.py, gumbel.py and
puct_shape.py.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Mapping, NamedTuple

INTERVAL_DEFAULT = 100
PARAM_KEYS = ("kld_stop_threshold", "kld_stop_interval", "kld_stop_min_simulations")
COUNTER_KEYS = ("kld_stopped_searches", "kld_simulations_saved")


class KldStop(NamedTuple):
    """Parsed parameters: `threshold` > 0 = on."""
    threshold: float
    interval: int
    min_simulations: int

    @property
    def on(self) -> bool:
        return self.threshold > 0.0

    def kwargs(self) -> Dict[str, Any]:
        """The three keyword arguments as the next layer down takes them -- {} when the rule is off."""
        if not self.on:
            return {}
        return {"kld_stop_threshold": self.threshold, "kld_stop_interval": self.interval,
                "kld_stop_min_simulations": self.min_simulations}

    def meta(self) -> Dict[str, Any]:
        """metadata["kld_stop"] of the manifests."""
        return {"threshold": self.threshold, "interval": self.interval, "min_simulations": self.min_simulations}


def _number(name: str, value, what: str) -> float:
    if isinstance(value, bool):
        raise ValueError(f"{name} must be {what}, got {value!r}")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be {what}, got {value!r}") from None
    if not math.isfinite(v):
        raise ValueError(f"{name} must be {what} (finite), got {v}")
    return v


def _integer(name: str, value, lo: int, what: str) -> int:
    v = _number(name, value, what)
    if v != int(v) or int(v) < lo:
        raise ValueError(f"{name} must be {what}, got {value!r}")
    return int(v)


def parse_kld_stop(kld_stop_threshold=0.0, kld_stop_interval=INTERVAL_DEFAULT, kld_stop_min_simulations=None) -> KldStop:
    """Validate the three parameters (whether on or off).  kld_stop_threshold: a finite number >= 0, 0 = off;
    kld_stop_interval: an integer >= 1; kld_stop_min_simulations: an integer >= 0 (None: the interval).  Anything else
    is a ValueError."""
    thr = _number("kld_stop_threshold", kld_stop_threshold, "a finite number >= 0 (0 = off)")
    if thr < 0.0:
        raise ValueError(f"kld_stop_threshold must be a finite number >= 0 (0 = off), got {thr}")
    interval = _integer("kld_stop_interval", kld_stop_interval, 1, "an integer >= 1")
    if interval >= 1 << 30:
        raise ValueError(f"kld_stop_interval must be an integer >= 1 (below 2^30), got {kld_stop_interval!r}")
    m = interval if kld_stop_min_simulations is None else \
        _integer("kld_stop_min_simulations", kld_stop_min_simulations, 0, "an integer >= 0")
    if m >= 1 << 30:
        raise ValueError(f"kld_stop_min_simulations must be an integer >= 0 (below 2^30), got {kld_stop_min_simulations!r}")
    return KldStop(thr, interval, m)


def kld_stop_kwargs(kld_stop_threshold=0.0, kld_stop_interval=INTERVAL_DEFAULT, kld_stop_min_simulations=None
                    ) -> Dict[str, Any]:
    """parse_kld_stop(...).kwargs(): {} when the rule is off."""
    return parse_kld_stop(kld_stop_threshold, kld_stop_interval, kld_stop_min_simulations).kwargs()


def kld_stop_meta(kwargs: Mapping[str, Any]) -> Dict[str, Any]:
    """metadata["kld_stop"] from the keyword arguments of an `on` configuration."""
    return parse_kld_stop(**{k: kwargs[k] for k in PARAM_KEYS}).meta()
