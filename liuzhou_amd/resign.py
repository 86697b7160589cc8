"""Resignation with play-through calibration in the tree backend's self-play: parameter validation and the counters.

The rule (per live slot and searched ply; p = the game's ply, c = the side to move, v = the search's root value in the
mover's frame): the ply is eligible when the phase is movement, capture selection or counter removal, p >=
resign_min_moves and the root is not terminal; it is low when it is eligible and v <= float32(resign_threshold).  With
resign_streak = "side" the mover's own counter goes up on a low ply and back to 0 on any other of its plies, and an
ineligible ply clears both sides' counters; with "ply" there is one counter per game that every searched ply raises or
clears, whoever moves (the reference's literal counter, v0/python/self_play_runner.py:359-374).  A game whose counter
reaches resign_consecutive is lost by the side to move -- unless it is one of the seeded share of games
(resign_playthrough_fraction) that never resign: those play on, and from them the run counts how often the side that
would have resigned went on to draw or win.

The rule itself runs on the device (csrc/lz_ops.hip: wave_resign_kernel, wave_resign_book_kernel; wave_tail.WaveTail
launches them).  What lives here is pure Python and needs no GPU, next to value_target.td_lambda_on.
"""
from __future__ import annotations

from typing import Any, Dict, Mapping, Sequence

from .kld_stop import _integer, _number

STREAKS = ("side", "ply")
# the int64[8] block of lz_wave_resign_book, in its order; all of them add up over chunks, workers and ranks
COUNTER_KEYS = ("resigned_games", "resigned_black", "resigned_white", "playthrough_games", "playthrough_would_resign",
                "playthrough_false_positive", "resign_ply_sum", "playthrough_plies_after_would")
# derived from the sums above (they do NOT add up: derive_counters() recomputes them after every merge)
DERIVED_KEYS = ("resign_avg_ply", "resign_plies_saved_estimate")
PARAM_KEYS = ("resign_threshold", "resign_min_moves", "resign_consecutive", "resign_playthrough_fraction", "resign_streak")


def resign_on(resign_threshold=0.0, resign_min_moves=10, resign_consecutive=3, resign_playthrough_fraction=0.1,
              resign_streak="side") -> bool:
    """Validate the five parameters; True when resignation is on (resign_threshold < 0).  resign_threshold: a finite number
    in [-1, 0], 0 = off; resign_min_moves: an integer >= 0; resign_consecutive: an integer >= 1;
    resign_playthrough_fraction: a finite number in [0, 1]; resign_streak: "side" or "ply".  Anything else is a
    ValueError (whether on or off)."""
    thr = _number("resign_threshold", resign_threshold, "a number in [-1, 0] (0 = off)")
    if thr > 0.0 or thr < -1.0:
        raise ValueError(f"resign_threshold must be a number in [-1, 0] (0 = off; root values live in [-1, 1]), got {thr}")
    _integer("resign_min_moves", resign_min_moves, 0, "an integer >= 0")
    _integer("resign_consecutive", resign_consecutive, 1, "an integer >= 1")
    frac = _number("resign_playthrough_fraction", resign_playthrough_fraction, "a number in [0, 1]")
    if frac < 0.0 or frac > 1.0:
        raise ValueError(f"resign_playthrough_fraction must be a number in [0, 1], got {frac}")
    if resign_streak not in STREAKS:
        raise ValueError(f"resign_streak must be 'side' or 'ply', got {resign_streak!r}")
    return thr < 0.0


def resign_kwargs(resign_threshold=0.0, resign_min_moves=10, resign_consecutive=3, resign_playthrough_fraction=0.1,
                  resign_streak="side") -> Dict[str, Any]:
    """The five keyword arguments as the next layer down takes them -- {} when the feature is off."""
    if not resign_on(resign_threshold, resign_min_moves, resign_consecutive, resign_playthrough_fraction, resign_streak):
        return {}
    return {"resign_threshold": float(resign_threshold), "resign_min_moves": int(resign_min_moves),
            "resign_consecutive": int(resign_consecutive),
            "resign_playthrough_fraction": float(resign_playthrough_fraction), "resign_streak": str(resign_streak)}


def resign_meta(kwargs: Mapping[str, Any]) -> Dict[str, Any]:
    """metadata["resign"] of the manifests: the settings under the issue's short names."""
    return {"threshold": float(kwargs["resign_threshold"]), "min_moves": int(kwargs["resign_min_moves"]),
            "consecutive": int(kwargs["resign_consecutive"]),
            "playthrough_fraction": float(kwargs["resign_playthrough_fraction"]), "streak": str(kwargs["resign_streak"])}


def derive_counters(counters: Dict[str, Any]) -> Dict[str, Any]:
    """(Re)compute the two derived counters, in place, from the sums -- after a run and after every merge of runs.
    resign_avg_ply: mean ply at which the resigned games ended (rounded; mcts_counters are integers).
    resign_plies_saved_estimate: resigned games x the mean number of plies a play-through game went on after it first
    wanted to resign."""
    if "resigned_games" not in counters:
        return counters
    n = int(counters.get("resigned_games", 0))
    w = int(counters.get("playthrough_would_resign", 0))
    counters["resign_avg_ply"] = int(round(int(counters.get("resign_ply_sum", 0)) / n)) if n else 0
    counters["resign_plies_saved_estimate"] = (
        int(round(n * int(counters.get("playthrough_plies_after_would", 0)) / w)) if w else 0)
    return counters


def counters_from_block(block: Sequence[int]) -> Dict[str, int]:
    """The device's int64[8] block -> mcts_counters entries (sums and derived)."""
    return derive_counters({k: int(v) for k, v in zip(COUNTER_KEYS, block)})
