"""The optional rules of the tree backend's self-play search: parsed once into one `SearchRules`, refused from one table.

Every layer -- scripts/selfplay_stage.py -> run_self_play_stage -> run_self_play_worker -> self_play_tree_gpu ->
DualStreamTreeMCTS -> PortableTreeMCTS -- takes the flat keyword names below, parses them with `SearchRules.parse`
(every value is validated whether its rule is on or off, on any backend), asks `rules.refuse(**what_it_knows)` and
hands `rules.kwargs()` (across a process boundary) or the object itself (`rules=`) to the next layer.  No torch here.
All rules need the tree backend ("tree" / "portable"); off, a rule allocates and launches nothing and every output is
byte-identical.  "The engine conditions" below: fused network search, batch_k = 1, one network, not the persistent
kernel (LZ_TREE_PERSISTENT).

`eval_symmetry` ("none", "random" or an id 0..7; env LZ_EVAL_SYMMETRY overrides): every leaf is evaluated as
    sigma_k(leaf) and the heads are mapped back (symmetry.py).  Not with batch_k > 1 or several networks.
`playout_cap_fast_simulations` F, `playout_cap_full_prob` p (on when 0 < F < mcts_simulations): the
    search of game g at ply t is full (mcts_simulations, root noise, records a training row) when uniform(seed, g, t,
    purpose 3) < p, else fast (F simulations, no root noise, only advances the game).  `num_positions` counts recorded
    rows, `avg_game_length` plies.  Searches always use the compact lists.  Counters: full_searches, fast_searches,
    recorded_positions.  Engine conditions.
`forced_playouts_k` k (0 = off; Wu 2019 section 3.2): in the searches whose root noise is on a root
    child with N > 0 and N^2 < k P n is visited before PUCT is asked, and the training target is formed from the
    pruned visits; the move pick and the kept subtree use the raw visits.  Counters: forced_playouts, pruned_visits.
    Engine conditions.
`gumbel_considered` m (0 = off, at most 72; the paper uses 16), `gumbel_c_visit`, `gumbel_c_scale` (Danihelka et al.
    2022; gumbel.py): in the searches whose root noise is on, the root samples m children without
    replacement by g + log P, spends the simulations on them by Sequential Halving with g + log P + sigma(completed
    Q), plays the winner and trains on softmax(log P + sigma(completed Q)).  Such a search never mixes Dirichlet noise
    into the root priors, whatever `add_dirichlet_noise` says; temperatures, `sample_moves` and the pick uniform do not
    apply to it (opening random moves keep precedence).  Counter: gumbel_searches.  Engine conditions; not with forced
    playouts, `policy_target_temperature`, `policy_target_prior_pseudocount` > 0, the PUCT shape, the KLD-gain stop or
    the move re-pick.
`mcts_solver`: exact results -- eliminations, draws by the move or no-capture limit -- are marked on
    the edges and carried up as far as they decide the parent; decided children stop being searched, and the played
    move never throws a proven win away.  The outputs gain `root_proven`.  Counters: solver_proofs,
    solver_roots_decided, solver_pick_overrides.  Engine conditions.
`fpu_reduction` (None = off, 0.0 = on without a reduction), `fpu_root_reduction` (None = fpu_reduction), `cpuct_log`
    (0 = off), `cpuct_base` (puct_shape.py): first-play urgency and the visit-scaled exploration
    constant on every level that PUCT decides; either half works without the other.  Such a search runs the one-wave
    tree step at every launch size.  Fused search (several networks in one launch included), batch_k = 1, not the
    persistent kernel, not with Gumbel.
`kld_stop_threshold` (0 = off), `kld_stop_interval` (100), `kld_stop_min_simulations` (None = the interval)
    (kld_stop.py): every `interval` simulations a game's root visit distribution is compared with
    the one `interval` simulations earlier, and from `min_simulations` on the search ends once the gain per simulation
    is below the threshold: its budget becomes the check's simulation + 1, and its tree is bit for bit the one a
    search of that many simulations builds.  With the playout cap the cap's draw sets the budget and the rule may
    only lower it.  Searches always use the compact lists.  Counters: kld_stopped_searches, kld_simulations_saved.
    Engine conditions; not with Gumbel.
`move_visit_offset` o (>= 0), `move_value_cutoff` c (in [0, 2]; both 0 = off) (move_pick.py): where
    the finish sampled a game's move from the visits, the move is drawn again with the same uniform from the children
    that keep more than o visits and whose mean value is within c of the most visited child's; the solver pick still
    has the last word.  Rows, targets and RNG streams are untouched.  Counters: move_pick_applied /
    move_pick_cut_visits / move_pick_cut_value / move_pick_changed.  Not with Gumbel or `sample_moves=False`.
`temperature_halflife` h (0 = off): the move temperature of ply p below `temperature_threshold` is temperature_final +
    (temperature_init - temperature_final) * 0.5^(p / h), from a float32 table built once on the host
    (move_pick.temperature_table); a policy target that follows the move temperature follows it too.
`value_target_lambda` (1 = off; value_target.py): with Q_t the root value of the game's t-th search
    from Black's frame (every search counts) and y_L the result, y_t = (1 - lambda) Q_t + lambda y_{t+1}, and the row of
    ply t gets value_target = sign * y_t; `soft_value_targets` stay.  Needs `device_tail`.
`resign_threshold` (0 = off; on in [-1, 0)), `resign_min_moves`, `resign_consecutive`, `resign_playthrough_fraction`,
    `resign_streak` ("side" / "ply") (resign.py): a game whose searches' root values have been <=
    the threshold `resign_consecutive` times in a row in the movement phases, from ply `resign_min_moves` on, ends as
    a loss of the side to move; a seeded share of the games never resigns and measures the false positives.  Counters:
    resign.COUNTER_KEYS + DERIVED_KEYS.  Needs `device_tail`.
`policy_surprise_weight` alpha (0 = off; in [0, 1]; KataGo uses 0.5) (policy_surprise.py): a share
    alpha of a finished game's total row weight is handed out in proportion to KL(the row's policy target || the
    network's noise-free root prior), and systematic resampling with one seeded uniform per game turns the weights
    into copy counts inside the game's own row slots.  One extra network launch of the wave per ply; with the playout
    cap only recorded rows take part.  Counters: policy_surprise.COUNTER_KEYS + DERIVED_KEYS.  Needs `device_tail`,
    not with a `PriorEvaluator` or the tail's in-kernel re-seat.
`start_fork_prob` (0 = off), `start_capture_prob` (0 = off), `start_bank_capacity` (65536), `start_min_move` (1: the
    empty board is never stored), `start_max_move` (143) (start_bank.py): game forking.  Once per
    ply a seeded share `start_capture_prob` of the searched, non-terminal positions whose move count lies in
    [start_min_move, start_max_move] is appended to a device-resident ring of `start_bank_capacity` packed states, and
    a seeded share `start_fork_prob` of the games that start takes a uniformly drawn bank position instead of the
    empty board (none while the bank is empty).  A forked game counts its plies from the fork: the temperature
    schedule and `opening_random_moves` restart there, the game's own limits travel in the state.  The rule is on
    when either probability is > 0 (capture alone fills a bank for later); `self_play_tree_gpu(start_bank=...)` takes
    a `StartBank` that survives the call.  Counters: start_captured, start_forked_games, start_fork_move_sum.  Needs
    `device_tail`, not with the tail's in-kernel re-seat.

Adding a rule: a field (with its one "off" value) and its flat names in `parse`, its group in `kwargs` and `meta`, its
rows in `REFUSALS`, a `RuleSpec` in `RULE_SPECS`, and its paragraph above.
"""
from __future__ import annotations

import math
import os
from typing import Any, Callable, Dict, Mapping, NamedTuple, Optional, Tuple

from . import kld_stop as _kld, move_pick as _pick, policy_surprise as _surprise, resign as _resign
from .gumbel import gumbel_on
from .kld_stop import KldStop, parse_kld_stop
from .puct_shape import CPUCT_BASE_DEFAULT, PuctShape, parse_puct_shape
from .value_target import td_lambda_on


def playout_cap_on(fast_simulations: int, full_prob: float, sims: int) -> bool:
    """Validate the playout cap's parameters against the search's `sims`: on when 0 < fast_simulations < sims, off for
    fast_simulations == 0; anything else (and full_prob outside [0, 1]) is a ValueError."""
    F, p = int(fast_simulations), float(full_prob)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"playout_cap_full_prob must lie in [0, 1], got {full_prob}")
    if F == 0:
        return False
    if not 0 < F < int(sims):
        raise ValueError(f"playout_cap_fast_simulations must be 0 (off) or in (0, mcts_simulations={int(sims)}), got {F}")
    return True


def parse_eval_symmetry(value) -> "str | int":
    """`eval_symmetry` of the tree search: "none", "random" or a fixed element id 0..7 (liuzhou_amd/symmetry.py).  Env
    LZ_EVAL_SYMMETRY=random / none / 0..7 overrides the argument (A/B runs)."""
    env = os.environ.get("LZ_EVAL_SYMMETRY", "").strip().lower()
    if env:
        value = env
    if isinstance(value, str):
        v = value.strip().lower()
        if v in ("none", "random"):
            return v
        if v.isdigit():
            value = int(v)
        else:
            raise ValueError(f"eval_symmetry must be 'none', 'random' or an id 0..7, got {value!r}")
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value < 8:
        raise ValueError(f"eval_symmetry must be 'none', 'random' or an id 0..7, got {value!r}")
    return int(value)


def search_simulations(num_simulations) -> int:
    """Validate the simulations of a search: an integer >= 1.  A root expanded and never searched has no visited child, and
    the read-out (lz_tree_finish) has no policy for it at a temperature above 1e-6 -- the reference raises "no policy mass"
    there; every smaller budget the searches can end with (playout cap, KLD-gain early stopping) is >= 1 too."""
    if isinstance(num_simulations, bool) or int(num_simulations) != num_simulations or int(num_simulations) < 1:
        raise ValueError(f"num_simulations must be an integer >= 1 (a root without a visit has no policy), got {num_simulations!r}")
    return int(num_simulations)


def forced_playouts_on(k) -> bool:
    """Validate `forced_playouts_k`: 0 = off, a positive finite number = on; negative or non-finite is a ValueError."""
    k = float(k)
    if not math.isfinite(k) or k < 0.0:
        raise ValueError(f"forced_playouts_k must be a finite number >= 0 (0 = off), got {k}")
    return k > 0.0


START_KEYS = ("start_fork_prob", "start_capture_prob", "start_bank_capacity", "start_min_move", "start_max_move")
START_DEFAULTS = (0.0, 0.0, 65536, 1, 143)
START_MAX_CAPACITY = 1 << 24
START_COUNTER_KEYS = ("start_forked_games", "start_fork_move_sum", "start_captured")      # the order of the device block


def start_bank_on(fork_prob, capture_prob, capacity, min_move, max_move) -> bool:
    """Validate the start bank's parameters: both probabilities in [0, 1], 1 <= capacity <= 2**24 and 0 <= min_move <=
    max_move <= 143 (integers); on when either probability is > 0."""
    for name, p in (("start_fork_prob", fork_prob), ("start_capture_prob", capture_prob)):
        if isinstance(p, bool) or not 0.0 <= float(p) <= 1.0:                  # a NaN compares false
            raise ValueError(f"{name} must lie in [0, 1] (0 = off), got {p!r}")
    for name, v in (("start_bank_capacity", capacity), ("start_min_move", min_move), ("start_max_move", max_move)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not 1 <= int(capacity) <= START_MAX_CAPACITY:
        raise ValueError(f"start_bank_capacity must lie in [1, 2**24], got {capacity!r}")
    if not 0 <= int(min_move) <= int(max_move) <= 143:
        raise ValueError(f"start_min_move / start_max_move must satisfy 0 <= min <= max <= 143, got {min_move!r} / "
                         f"{max_move!r}")
    return float(fork_prob) > 0.0 or float(capture_prob) > 0.0


def start_meta(settings: Mapping[str, Any], counters: Mapping[str, Any]) -> Dict[str, Any]:
    """The manifest entry of the start bank: its settings, its three counters and the mean move count at the fork."""
    c = {k: int(counters.get(k, 0)) for k in START_COUNTER_KEYS}
    forks = c["start_forked_games"]
    return {**settings, "start_captured": c["start_captured"], "start_forked_games": forks,
            "start_fork_move_sum": c["start_fork_move_sum"],
            "fork_avg_move": (c["start_fork_move_sum"] / forks) if forks else 0.0}


def persistent_default() -> bool:
    """Is the persistent search kernel asked for (env LZ_TREE_PERSISTENT)?  What callers hand `refuse(persistent=...)`."""
    return os.environ.get("LZ_TREE_PERSISTENT", "0").strip().lower() in ("1", "on", "true")


# the engines' constructor names of the same options (PortableTreeMCTS / DualStreamTreeMCTS; `kld_stop` is a KldStop)
ENGINE_ALIASES = {"fast_simulations": "playout_cap_fast_simulations", "full_prob": "playout_cap_full_prob",
                  "solver": "mcts_solver"}


class SearchRules(NamedTuple):
    """The parsed state of every rule; each rule has ONE off value (the defaults), so equal searches compare equal."""
    eval_symmetry: Any = "none"
    cap_fast_simulations: int = 0
    cap_full_prob: float = 1.0
    forced_k: float = 0.0
    gumbel_considered: int = 0
    gumbel_c_visit: float = 50.0
    gumbel_c_scale: float = 1.0
    td_lambda: float = 1.0
    solver: bool = False
    shape: PuctShape = parse_puct_shape()
    resign: Tuple = ()                       # the five values in resign.PARAM_KEYS order, () = off
    kld: KldStop = parse_kld_stop()
    move_visit_offset: float = 0.0
    move_value_cutoff: float = 0.0
    temperature_halflife: float = 0.0
    surprise_weight: float = 0.0
    start: Tuple = ()                        # the five values in START_KEYS order, () = off

    @classmethod
    def parse(cls, mcts_simulations, *, eval_symmetry="none", playout_cap_fast_simulations=0, playout_cap_full_prob=1.0,
              forced_playouts_k=0.0, gumbel_considered=0, gumbel_c_visit=50.0, gumbel_c_scale=1.0,
              value_target_lambda=1.0, mcts_solver=False, fpu_reduction=None, fpu_root_reduction=None, cpuct_log=0.0,
              cpuct_base=CPUCT_BASE_DEFAULT, resign_threshold=0.0, resign_min_moves=10, resign_consecutive=3,
              resign_playthrough_fraction=0.1, resign_streak="side", kld_stop_threshold=0.0,
              kld_stop_interval=_kld.INTERVAL_DEFAULT, kld_stop_min_simulations=None, move_visit_offset=0.0,
              move_value_cutoff=0.0, temperature_halflife=0.0, policy_surprise_weight=0.0, start_fork_prob=0.0,
              start_capture_prob=0.0, start_bank_capacity=65536, start_min_move=1, start_max_move=143) -> "SearchRules":
        """From the public flat keyword names (an unknown one is a TypeError).  Every value is validated, on or off."""
        start = start_bank_on(start_fork_prob, start_capture_prob, start_bank_capacity, start_min_move, start_max_move)
        surprise = _surprise.policy_surprise_on(policy_surprise_weight)
        repick = _pick.move_pick_on(move_visit_offset, move_value_cutoff)
        halflife = _pick.halflife_on(temperature_halflife)
        kld = parse_kld_stop(kld_stop_threshold, kld_stop_interval, kld_stop_min_simulations)
        resign = _resign.resign_kwargs(resign_threshold, resign_min_moves, resign_consecutive,
                                       resign_playthrough_fraction, resign_streak)
        shape = parse_puct_shape(fpu_reduction, fpu_root_reduction, cpuct_log, cpuct_base)
        td = td_lambda_on(value_target_lambda)
        gumbel = gumbel_on(gumbel_considered, gumbel_c_visit, gumbel_c_scale)
        forced = forced_playouts_on(forced_playouts_k)
        cap = playout_cap_on(playout_cap_fast_simulations, playout_cap_full_prob, mcts_simulations)
        off = cls()
        return cls(
            eval_symmetry=parse_eval_symmetry(eval_symmetry),
            cap_fast_simulations=int(playout_cap_fast_simulations) if cap else 0,
            cap_full_prob=float(playout_cap_full_prob) if cap else 1.0,
            forced_k=float(forced_playouts_k) if forced else 0.0,
            gumbel_considered=int(gumbel_considered) if gumbel else 0,
            gumbel_c_visit=float(gumbel_c_visit) if gumbel else off.gumbel_c_visit,
            gumbel_c_scale=float(gumbel_c_scale) if gumbel else off.gumbel_c_scale,
            td_lambda=float(value_target_lambda) if td else 1.0, solver=bool(mcts_solver),
            shape=parse_puct_shape(**shape.kwargs()),        # the half that is off forgets its parameters
            resign=tuple(resign[k] for k in _resign.PARAM_KEYS) if resign else (), kld=kld if kld.on else off.kld,
            move_visit_offset=float(move_visit_offset) if repick else 0.0,
            move_value_cutoff=float(move_value_cutoff) if repick else 0.0,
            temperature_halflife=float(temperature_halflife) if halflife else 0.0,
            surprise_weight=float(policy_surprise_weight) if surprise else 0.0,
            start=(float(start_fork_prob), float(start_capture_prob), int(start_bank_capacity), int(start_min_move),
                   int(start_max_move)) if start else ())

    @classmethod
    def parse_engine(cls, num_simulations, *, kld_stop: Optional[KldStop] = None, **options) -> "SearchRules":
        """`parse` for the engines' constructor names (ENGINE_ALIASES; `kld_stop` a KldStop or None)."""
        flat = {ENGINE_ALIASES.get(k, k): v for k, v in options.items()}
        if kld_stop is not None:
            flat.update(zip(_kld.PARAM_KEYS, kld_stop))
        rules = cls.parse(num_simulations, **flat)
        if rules != rules.engine():
            raise TypeError(f"the per-ply tail's rules are not options of a search engine: {sorted(options)}")
        return rules

    # ---- which rules are on ----
    cap = property(lambda self: self.cap_fast_simulations > 0)
    forced = property(lambda self: self.forced_k > 0.0)
    gumbel = property(lambda self: self.gumbel_considered > 0)
    td = property(lambda self: self.td_lambda < 1.0)
    repick = property(lambda self: self.move_visit_offset > 0.0 or self.move_value_cutoff > 0.0)
    halflife = property(lambda self: self.temperature_halflife > 0.0)
    move_options = property(lambda self: self.repick or self.halflife)
    surprise = property(lambda self: self.surprise_weight > 0.0)
    symmetric = property(lambda self: self.eval_symmetry != "none")
    shaped = property(lambda self: self.shape.on)
    kld_on = property(lambda self: self.kld.on)

    def resign_kwargs(self) -> Dict[str, Any]:
        return dict(zip(_resign.PARAM_KEYS, self.resign))

    def start_kwargs(self) -> Dict[str, Any]:
        return dict(zip(START_KEYS, self.start))

    def kwargs(self) -> Dict[str, Any]:
        """The flat keyword arguments of the groups that are on ({} with everything off):
        `SearchRules.parse(sims, **rules.kwargs()) == rules`."""
        return {**({"eval_symmetry": self.eval_symmetry} if self.symmetric else {}),
                **({"playout_cap_fast_simulations": self.cap_fast_simulations,
                    "playout_cap_full_prob": self.cap_full_prob} if self.cap else {}),
                **({"forced_playouts_k": self.forced_k} if self.forced else {}),
                **({"gumbel_considered": self.gumbel_considered, "gumbel_c_visit": self.gumbel_c_visit,
                    "gumbel_c_scale": self.gumbel_c_scale} if self.gumbel else {}),
                **({"value_target_lambda": self.td_lambda} if self.td else {}),
                **({"mcts_solver": True} if self.solver else {}), **self.shape.kwargs(), **self.resign_kwargs(),
                **self.kld.kwargs(),
                **({"move_visit_offset": self.move_visit_offset, "move_value_cutoff": self.move_value_cutoff}
                   if self.repick else {}),
                **({"temperature_halflife": self.temperature_halflife} if self.halflife else {}),
                **({"policy_surprise_weight": self.surprise_weight} if self.surprise else {}), **self.start_kwargs()}

    def meta(self) -> Dict[str, Any]:
        """What a worker records in its manifest's metadata: one entry (RuleSpec.key) per rule that is on."""
        pick = {"move_visit_offset": self.move_visit_offset, "move_value_cutoff": self.move_value_cutoff,
                "temperature_halflife": self.temperature_halflife}
        return {**({"eval_symmetry": self.eval_symmetry} if self.symmetric else {}),
                **({"playout_cap": {"fast_simulations": self.cap_fast_simulations, "full_prob": self.cap_full_prob}}
                   if self.cap else {}),
                **({"forced_playouts": {"k": self.forced_k}} if self.forced else {}),
                **({"gumbel": {"considered": self.gumbel_considered, "c_visit": self.gumbel_c_visit,
                               "c_scale": self.gumbel_c_scale}} if self.gumbel else {}),
                **({"value_target": {"td_lambda": self.td_lambda}} if self.td else {}),
                **({"mcts_solver": True} if self.solver else {}),
                **({"puct_shape": self.shape.meta()} if self.shaped else {}),
                **({"resign": _resign.resign_meta(self.resign_kwargs())} if self.resign else {}),
                **({"kld_stop": self.kld.meta()} if self.kld_on else {}),
                **({"move_pick": _pick.move_pick_meta(pick)} if self.move_options else {}),
                **({"policy_surprise": {"weight": self.surprise_weight}} if self.surprise else {}),
                **({"start_bank": dict(zip(("fork_prob", "capture_prob", "capacity", "min_move", "max_move"), self.start))}
                   if self.start else {})}

    def engine(self) -> "SearchRules":
        """The rules a search engine sees: those of the per-ply tail (TD(lambda), resignation, policy surprise, the
        temperature half-life, the start bank) are off, so engines that differ only in them are one engine (the engine cache's key)."""
        return self._replace(td_lambda=1.0, resign=(), temperature_halflife=0.0, surprise_weight=0.0, start=())

    def refusal(self, **context) -> Optional[str]:
        """The message of the first row of REFUSALS whose rule is on and whose condition holds in `context`
        (CONTEXT_KEYS), or None.  A key the caller does not pass is not checked: every layer says what it knows."""
        unknown = sorted(set(context) - set(CONTEXT_KEYS))
        if unknown:
            raise TypeError(f"unknown context keys {unknown}; known: {CONTEXT_KEYS}")
        for on, key, bad, text in REFUSALS:
            if getattr(self, on) and (key is None or key in context) and bad(context.get(key), self):
                return text.format(v=context.get(key), r=self)
        return None

    def refuse(self, **context) -> None:
        """ValueError(refusal(**context)) if there is one."""
        why = self.refusal(**context)
        if why is not None:
            raise ValueError(why)


CONTEXT_KEYS = ("search_backend", "batch_k", "fused", "several_networks", "persistent", "sample_moves", "device_tail",
                "prior_evaluator", "reseat", "policy_target_temperature", "policy_target_prior_pseudocount")

_ROOT = ("search_backend", lambda v, r: str(v).strip().lower() not in ("portable", "tree"))
_WAVES = ("batch_k", lambda v, r: int(v) > 1, "batch_k > 1 (legacy waves)")
_SEVERAL = ("several_networks", lambda v, r: bool(v), "several networks in one search")
_EXTERNAL = ("fused", lambda v, r: not v, "an external evaluator (split-phase path)")
_PERSISTENT = ("persistent", lambda v, r: bool(v), "the persistent search kernel (LZ_TREE_PERSISTENT)")
_ENGINE = (_WAVES, _SEVERAL, _EXTERNAL, _PERSISTENT)
_NO_TAIL = ("device_tail", lambda v, r: not v)


def _with(on: str, subject: str, *causes) -> list:
    """Rows "`subject` not supported with <cause>" of the rule `on`, one per (context key, condition, cause)."""
    return [(on, key, bad, f"{subject} not supported with {why}") for key, bad, why in causes]


# (rule's on-property, context key or None, condition(context value, rules), message) -- walked top to bottom, the first
# hit is raised.  First every rule against the root-PUCT backend, then rule by rule what else is in its way.
REFUSALS = [
    ("start", *_ROOT, "the start bank needs the tree backend, not the root-PUCT search ({v!r}): its capture and seed "
                      "kernels run in the tree backend's per-ply device tail"),
    ("surprise", *_ROOT, "policy surprise weighting needs the tree backend, not the root-PUCT search ({v!r}): it compares "
                         "the tree search's policy target with the network prior"),
    ("move_options", *_ROOT, "move_visit_offset / move_value_cutoff / temperature_halflife need the tree backend, not the "
                             "root-PUCT search ({v!r}): they act on the tree search's root children and its per-ply move "
                             "temperature"),
    ("kld_on", *_ROOT, "KLD-gain early stopping needs the tree backend, not the root-PUCT search ({v!r}): the rule lowers "
                       "the per-game budget of the tree search"),
    ("resign", *_ROOT, "resignation needs the tree backend, not the root-PUCT search ({v!r}): it reads the tree search's "
                       "root values in the per-ply device tail"),
    ("shaped", *_ROOT, "first-play urgency / the visit-scaled cpuct are not supported with the root-PUCT search (it needs "
                       "the tree backend)"),
    ("solver", *_ROOT, "the MCTS-Solver needs the tree backend, not the root-PUCT search ({v!r}): it marks proven results "
                       "in the search tree"),
    ("td", *_ROOT, "TD(lambda) value targets need the tree backend, not the root-PUCT search ({v!r}): they blend the tree "
                   "search's root values"),
    ("gumbel", *_ROOT, "the Gumbel root search needs the tree backend, not the root-PUCT search ({v!r})"),
    ("forced", *_ROOT, "forced playouts need the tree backend, not the root-PUCT search ({v!r})"),
    ("cap", *_ROOT, "playout cap randomization needs the tree backend, not the root-PUCT search ({v!r})"),
    ("symmetric", *_ROOT, "eval_symmetry={r.eval_symmetry!r} needs the tree backend: the root-PUCT search ({v!r}) "
                          "evaluates children without the symmetry hook"),
    *_with("surprise", "policy surprise weighting is",
           (*_NO_TAIL, "the host loop (device_tail=False): the surprises and the resampling live in the per-ply device tail"),
           ("reseat", lambda v, r: bool(v), "the in-kernel re-seat (reseat=True): it clears step_counts inside the step "
                                            "kernel, before the rows of the game are weighed"),
           ("prior_evaluator", lambda v, r: bool(v), "a PriorEvaluator: it returns priors of its own making, there is no "
                                                     "plain network to evaluate the root with")),
    *_with("start", "the start bank is",
           (*_NO_TAIL, "the host loop (device_tail=False): the bank is filled and read by the per-ply device tail"),
           ("reseat", lambda v, r: bool(v), "the in-kernel re-seat (reseat=True): the step kernel starts the next game "
                                            "there, and no kernel runs between its fresh state and the search")),
    ("resign", *_NO_TAIL, "resignation needs device_tail: the rule runs in the per-ply device tail, the host loop has none"),
    ("td", *_NO_TAIL, "value_target_lambda < 1 needs device_tail: the host loop keeps the reference's finalisation (every "
                      "row gets the final result)"),
    ("symmetric", _WAVES[0], _WAVES[1], "eval_symmetry is not supported by the legacy waves (batch_k > 1): their wave "
                                        "kernels evaluate leaves without the symmetry hook"),
    *_with("solver", "the MCTS-Solver is", *_ENGINE),
    *_with("shaped", "first-play urgency / the visit-scaled cpuct are",
           (None, lambda v, r: r.gumbel, "the Gumbel root search (its root level has a rule of its own)"),
           _WAVES, _EXTERNAL, _PERSISTENT),
    *_with("repick", "visit-offset / value-cutoff move selection is",
           (None, lambda v, r: r.gumbel, "the Gumbel root search (its pick is the Sequential Halving winner and ignores "
                                         "temperatures by definition)"),
           ("sample_moves", lambda v, r: not v, "sample_moves=False (the most visited move is played already; there is no "
                                                "sampled move to re-pick)")),
    *_with("kld_on", "KLD-gain early stopping is", *_ENGINE,
           (None, lambda v, r: r.gumbel, "the Gumbel root search (its Sequential Halving schedule is a function of a fixed "
                                         "budget)")),
    *_with("gumbel", "the Gumbel root search is", *_ENGINE,
           (None, lambda v, r: r.forced, "forced playouts (two rules for the same root level)"),
           ("policy_target_temperature", lambda v, r: v is not None,
            "policy_target_temperature (the training target is not made of visit counts)"),
           ("policy_target_prior_pseudocount", lambda v, r: float(v) > 0.0,
            "policy_target_prior_pseudocount > 0 (the training target is not made of visit counts)")),
    *_with("forced", "forced playouts are", *_ENGINE),
    *_with("cap", "playout cap randomization is", *_ENGINE),
]


class RuleSpec(NamedTuple):
    """How a rule travels in the manifests: `key` of metadata, its `settings` (name, default; a default's type casts the
    worker's value, None takes it as it is; () = the entry is the flag True), the mcts_counters that are copied beside
    the settings (`present_only`: those the run has), `on` / `source`: the SearchRules property under which the engine
    attribute `source` holds the counters' block, `summary(settings, counters)`: the entry, where it is not the plain
    union."""
    key: str
    settings: Tuple = ()
    counters: Tuple = ()
    present_only: bool = False
    on: Optional[str] = None
    source: Optional[str] = None
    summary: Optional[Callable[[Mapping[str, Any], Mapping[str, Any]], Dict[str, Any]]] = None


_AS_IS = lambda *names: tuple((n, None) for n in names)
RULE_SPECS = (
    RuleSpec("playout_cap", (("fast_simulations", 0), ("full_prob", 1.0)), ("full_searches", "fast_searches"),
             on="cap", source="cap_counts"),
    RuleSpec("forced_playouts", (("k", 0.0),), ("forced_playouts", "pruned_visits"), on="forced", source="forced_counts"),
    RuleSpec("gumbel", (("considered", 0), ("c_visit", 50.0), ("c_scale", 1.0)), ("gumbel_searches",),
             on="gumbel", source="gumbel_searches"),
    RuleSpec("value_target", (("td_lambda", 1.0),)),
    RuleSpec("mcts_solver", on="solver", source="solver_counts"),        # its counters travel in mcts_counters only
    RuleSpec("puct_shape", _AS_IS("fpu_reduction", "fpu_root_reduction", "cpuct_log", "cpuct_base")),
    RuleSpec("resign", _AS_IS("threshold", "min_moves", "consecutive", "playthrough_fraction", "streak"),
             _resign.COUNTER_KEYS + _resign.DERIVED_KEYS),
    RuleSpec("kld_stop", _AS_IS("threshold", "interval", "min_simulations"), _kld.COUNTER_KEYS,
             on="kld_on", source="kld_counts"),
    RuleSpec("move_pick", _AS_IS("visit_offset", "value_cutoff", "temperature_halflife"), _pick.COUNTER_KEYS,
             present_only=True, on="repick", source="move_pick_counts"),
    RuleSpec("policy_surprise", (("weight", 0.0),), summary=lambda s, c: _surprise.surprise_meta(s["weight"], c)),
    RuleSpec("start_bank", (("fork_prob", 0.0), ("capture_prob", 0.0), ("capacity", 65536), ("min_move", 1),
                            ("max_move", 143)), START_COUNTER_KEYS + ("fork_avg_move",), summary=start_meta),
)
SOLVER_COUNTER_KEYS = ("solver_proofs", "solver_roots_decided", "solver_pick_overrides")


def read_meta(found: Dict[str, Any], worker_meta: Mapping[str, Any]) -> None:
    """Fold one worker's metadata into `found`: per RuleSpec the first worker's settings (a flag: any worker's)."""
    for spec in RULE_SPECS:
        w = worker_meta.get(spec.key)
        if not spec.settings:
            if w:
                found[spec.key] = True
        elif isinstance(w, dict) and spec.key not in found:
            found[spec.key] = {n: w.get(n) if d is None else type(d)(w.get(n, d)) for n, d in spec.settings}


def merged_meta(found: Mapping[str, Any], counters: Mapping[str, Any]) -> Dict[str, Any]:
    """The stage manifest's entries of the rules in `found` (read_meta), with their counters over all workers."""
    out: Dict[str, Any] = {}
    for spec in RULE_SPECS:
        if spec.key not in found:
            continue
        s = found[spec.key]
        out[spec.key] = (True if not spec.settings else spec.summary(s, counters) if spec.summary else
                         {**s, **{k: int(counters.get(k, 0)) for k in spec.counters
                                  if not spec.present_only or k in counters}})
    return out


def engine_counters(rules: SearchRules, mcts) -> Dict[str, int]:
    """mcts_counters entries of the engine-side rules that are on, read from the engine's counter blocks."""
    out: Dict[str, int] = {}
    for spec in RULE_SPECS:
        if spec.source and getattr(rules, spec.on):
            out.update(zip(spec.counters or SOLVER_COUNTER_KEYS, (int(x) for x in getattr(mcts, spec.source).tolist())))
    return out
