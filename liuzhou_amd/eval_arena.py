"""Evaluation arena on the self-play engine.

The reference arena (`scripts/eval_checkpoint.py:262-655`) keeps one Python `GameState` per game and rebuilds a GPU
batch for every move; here the games live on the device for their whole life: one `GpuStateBatch`, legal masks /
transitions / termination through the HIP operators, the two agents searching only the games in which they are to
move.  Semantics kept from the reference worker (`_eval_worker_v1`, :448-654):
  * the challenger plays black in the first half of the games and white in the second,
  * a side that has no legal move loses, the move limits give a draw, `opening_random_moves` plies (by `move_count`)
    are played uniformly at random by whoever is to move,
  * the opponent is another checkpoint (same search settings) or `RandomAgent` (uniform over the legal moves),
  * result payload = wins / losses / draws / rates from the challenger's side (+ per-colour breakdown).
Two search backends: `RootSearchAgent` (the reference's `--backend v1`, root PUCT) and `TreeSearchAgent` (its
`--backend portable`, `_PortableEvalAgent`, eval_checkpoint.py:324-445: the full-tree search, a fresh tree every move, no
root noise).  When both sides are tree agents the games are searched JOINTLY: one engine with a segment of slots per
network (slot g of segment k = game g, active when network k is to move there), so one search per ply covers every game
and each simulation is one network launch for both networks.  `play_matches(joint=False)` searches each agent's games
with its own engine instead -- the same moves (each game's tree depends on its position and its network only; the RNG
is keyed by game and ply).  In the tree backend the opening random moves of a ply are drawn in one call over all games.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import torch

from . import v0_core
from .mcts_gpu import GpuStateBatch, V1RootMCTS, V1RootMCTSConfig, encode_actions_fast
from .net_hip import FusedNet


@dataclass
class EvaluationStats:
    wins: int
    losses: int
    draws: int
    total_games: int
    color_breakdown: Dict[str, Dict[str, int]] = field(default_factory=dict)
    move_log: Optional[torch.Tensor] = None      # int32[games, plies] 220-d action indices (-1 pad), if recorded
    openings: Optional[torch.Tensor] = None      # int64[games] opening-book entry of every game (CPU), with a book
    paired: Optional[Dict[str, Any]] = None      # opening_book.paired_statistics + book_size / openings_used / opening_move_mean

    def _rate(self, v: int) -> float:
        return 0.0 if self.total_games == 0 else v / self.total_games

    @property
    def win_rate(self) -> float:
        return self._rate(self.wins)

    @property
    def loss_rate(self) -> float:
        return self._rate(self.losses)

    @property
    def draw_rate(self) -> float:
        return self._rate(self.draws)

    def to_payload(self, name: str) -> Dict[str, Any]:
        out = {"name": str(name), "wins": int(self.wins), "losses": int(self.losses), "draws": int(self.draws),
               "total_games": int(self.total_games), "win_rate": float(self.win_rate),
               "loss_rate": float(self.loss_rate), "draw_rate": float(self.draw_rate),
               "color_breakdown": {k: dict(v) for k, v in self.color_breakdown.items()}}
        if self.paired is not None:                          # only when an opening book was used
            out["paired"] = dict(self.paired)
        return out


def _uniform_legal_codes(state: GpuStateBatch):
    """Uniform random legal action per state -> (codes int32[B,4], valid bool[B], no_legal bool[B])."""
    mask, meta = encode_actions_fast(state)
    n = mask.sum(dim=1)
    valid = n > 0
    probs = mask.to(torch.float32)
    probs[~valid, 0] = 1.0                                  # keep multinomial well-defined; the row is flagged invalid
    idx = torch.multinomial(probs, 1).view(-1)
    codes = meta[torch.arange(mask.shape[0], device=mask.device), idx].to(torch.int32)
    codes[~valid] = -1
    return codes, valid, ~valid


def codes_to_indices(codes: torch.Tensor) -> torch.Tensor:
    """Action codes int32[N,4] (kind, primary, secondary, extra) -> 220-d action indices (v0/python/move_encoder.py:46-51:
    placement = cell, movement = 36 + 4*from + dir, selections = 180 + cell, process-removal = 216; invalid: -1)."""
    kind, a, b = codes[:, 0].to(torch.int64), codes[:, 1].to(torch.int64), codes[:, 2].to(torch.int64)
    idx = torch.full_like(kind, -1)
    idx = torch.where(kind == 1, a, idx)
    idx = torch.where(kind == 2, 36 + 4 * a + b, idx)
    idx = torch.where((kind >= 3) & (kind <= 7), 180 + a, idx)
    idx = torch.where(kind == 8, torch.full_like(kind, 216), idx)
    return idx.to(torch.int32)


class RandomAgent:
    """Uniform over the legal moves (the reference's vs-random opponent)."""

    def select(self, state: GpuStateBatch, force_uniform: Optional[torch.Tensor] = None):
        return _uniform_legal_codes(state)


class RootSearchAgent:
    """Checkpoint + the reference's evaluation search (V1RootMCTS, no root noise; eval_checkpoint.py:262-322)."""

    def __init__(self, model, device, mcts_simulations: int, temperature: float = 0.1, sample_moves: bool = False) -> None:
        dev = torch.device(device)
        from .net_hip import fused_supported
        net = FusedNet(model.to(dev).eval(), dev) if fused_supported(model) else model.to(dev).eval()
        self.evaluator = "fused_f16" if isinstance(net, FusedNet) else "torch"
        cfg = V1RootMCTSConfig(num_simulations=max(1, int(mcts_simulations)), exploration_weight=1.0,
                               temperature=float(temperature), add_dirichlet_noise=False, sample_moves=bool(sample_moves))
        self.mcts = V1RootMCTS(model=net, config=cfg, device=dev)
        self.temperature = float(temperature)

    def select(self, state: GpuStateBatch, force_uniform: Optional[torch.Tensor] = None):
        temps = torch.full((state.batch_size,), self.temperature, dtype=torch.float32, device=state.device)
        out = self.mcts.search_batch(state, temperatures=temps, add_dirichlet_noise=False,
                                     force_uniform_random_mask=force_uniform)
        return out.chosen_action_codes, out.chosen_valid_mask, out.terminal_mask


def _pad16(n: int) -> int:
    return max(16, -(-int(n) // 16) * 16)


class TreeSearchAgent:
    """Checkpoint + the full-tree search (`PortableTreeMCTS`), as the reference's `_PortableEvalAgent`
    (eval_checkpoint.py:324-445): a fresh tree for every move (no subtree reuse), no Dirichlet noise, and the pick by
    `sample_moves` (visit counts ^ 1/temperature) or the N -> Q -> P -> index order of the deterministic pick.
    `fpu_reduction` / `fpu_root_reduction` / `cpuct_log` / `cpuct_base`: first-play urgency and the visit-scaled
    exploration constant of its searches (tree_engine.PortableTreeMCTS; off by default), so that the arena searches the way
    self-play does.  Agents share one multi-network engine only when these are equal."""

    def __init__(self, model, device, mcts_simulations: int, temperature: float = 0.1, sample_moves: bool = False,
                 seed: int = 0, fpu_reduction: Optional[float] = None, fpu_root_reduction: Optional[float] = None,
                 cpuct_log: float = 0.0, cpuct_base: float = 19652.0) -> None:
        from .puct_shape import parse_puct_shape
        self.puct_shape = parse_puct_shape(fpu_reduction, fpu_root_reduction, cpuct_log, cpuct_base)
        dev = torch.device(device)
        from .net_hip import fused_supported
        self.net = FusedNet(model.to(dev).eval(), dev) if fused_supported(model) else model.to(dev).eval()
        self.evaluator = "fused_f16" if isinstance(self.net, FusedNet) else "torch"
        self.device = dev
        self.sims = max(1, int(mcts_simulations))
        self.temperature = float(temperature)
        self.sample_moves = bool(sample_moves)
        self.seed = int(seed)
        self._engines: Dict[int, Any] = {}

    def engine(self, slots: int):
        """This agent's own engine of `slots` slots (per-agent searches), built once per size."""
        e = self._engines.get(int(slots))
        if e is None:
            e = _tree_engine([self], int(slots))
            self._engines[int(slots)] = e
        return e


def _tree_engine(agents: Sequence[TreeSearchAgent], slots: int):
    """One engine over `agents` (one segment of `slots` slots each when several)."""
    from .tree_engine import PortableTreeMCTS
    a = agents[0]
    nets = [x.net for x in agents]
    kw = dict(add_dirichlet_noise=False, sample_moves=a.sample_moves, reuse_tree=False, compact_evals=True, seed=a.seed,
              **a.puct_shape.kwargs())
    if len(agents) == 1:
        return PortableTreeMCTS(nets[0], slots, a.sims, a.device, **kw)
    return PortableTreeMCTS(nets, slots * len(agents), a.sims, a.device, segment_games=slots, **kw)


def _joint_engine(group: Sequence[TreeSearchAgent], slots: int):
    """The engine that searches `group` together, kept on the first agent for the next match against the same networks.
    Keyed by the networks themselves (the cached engine holds them, so no other object can take their ids while it is
    kept) and the search settings; one joint engine per agent: another group replaces it."""
    a = group[0]
    key = ("joint", tuple(id(x.net) for x in group), int(slots), a.sims, a.sample_moves, a.seed, a.puct_shape.key())
    eng = a._engines.get(key)
    if eng is None or any(x is not y for x, y in zip(eng.nets, [x.net for x in group])):
        for k in [k for k in a._engines if isinstance(k, tuple) and k[0] == "joint"]:
            del a._engines[k]
        eng = a._engines[key] = _tree_engine(group, slots)
    return eng


def _joinable(agents: Sequence[TreeSearchAgent]) -> bool:
    """Tree agents one engine can search together: the same search settings (the networks may differ in anything)."""
    a = agents[0]
    return 2 <= len(agents) <= 8 and all(x.sims == a.sims and x.sample_moves == a.sample_moves and x.seed == a.seed and
                                         x.device == a.device and x.puct_shape.key() == a.puct_shape.key()
                                         for x in agents)


def _check_book(opening_book, games: int, opening_random_moves: int, what: str) -> None:
    """The refusals of a match of `games` games from a book: what a book cannot be combined with is a ValueError."""
    from .opening_book import OpeningBook
    if not isinstance(opening_book, OpeningBook) or len(opening_book) < 1:
        raise ValueError("opening_book must be an OpeningBook with at least one position")
    if int(opening_random_moves) > 0:
        raise ValueError("an opening book cannot be combined with opening_random_moves > 0: the book's positions are the "
                         "openings")
    if int(games) < 2 or int(games) % 2 != 0:
        raise ValueError(f"with an opening book {what} must be even (every opening is played twice, colours swapped), "
                         f"got {games}")


def _book_openings(opening_book, opening_seed: int, games: int, opening_random_moves: int, what: str) -> torch.Tensor:
    """int64[games] (CPU): the book entry of every game of a match of `games` games -- game p and game p + games/2 share
    the opening of pair p (opening_book.assign_openings)."""
    from .opening_book import assign_openings
    _check_book(opening_book, games, opening_random_moves, what)
    return assign_openings(len(opening_book), int(games) // 2, int(opening_seed)).repeat(2)


def _seat_openings(states: GpuStateBatch, opening_book, openings: torch.Tensor) -> None:
    """One lz_states_from_packed launch: game g starts from book entry openings[g]."""
    from .opening_book import states_from_packed
    book = opening_book if opening_book.device == states.device else opening_book.to(states.device)
    states_from_packed(book.positions, openings.to(states.device).contiguous(), states.tensors())


def _paired(res: torch.Tensor, opening_book, openings: torch.Tensor) -> Dict[str, Any]:
    """The pair statistics of one match: `res` the challenger's results (+1 / 0 / -1) of its games, first half then
    second half, `openings` their book entries."""
    from .opening_book import paired_statistics
    points = ((res.to(torch.float64) + 1.0) / 2.0).cpu()
    half = int(points.numel()) // 2
    out = paired_statistics(points[:half], points[half:])
    used = openings[:half]
    out["book_size"] = len(opening_book)
    out["openings_used"] = int(torch.unique(used).numel())
    out["opening_move_mean"] = float(opening_book.move_counts.cpu().index_select(0, used).to(torch.float64).mean())
    return out


def _play_games(agents: Sequence[Any], player_a: torch.Tensor, player_b: torch.Tensor, a_black: torch.Tensor, device, *,
                joint: bool = True, opening_random_moves: int = 0, max_game_plies: int = 512,
                record_moves: bool = False, opening_book=None, openings: Optional[torch.Tensor] = None):
    """Tree-backend game loop: game g between agents player_a[g] (black iff a_black[g]) and player_b[g], from the empty
    board or, with a book, from its entry openings[g].  Returns (result from black's side float32[n], move log
    int32[n, plies] or None)."""
    dev = torch.device(device)
    n = int(player_a.numel())
    G = _pad16(n)
    states = GpuStateBatch.initial(dev, n)
    if opening_book is not None:
        _seat_openings(states, opening_book, openings)
    plies = torch.zeros((n,), dtype=torch.int64, device=dev)
    done = torch.zeros((n,), dtype=torch.bool, device=dev)
    result_black = torch.zeros((n,), dtype=torch.float32, device=dev)
    pad_idx = torch.clamp(torch.arange(G, device=dev), max=n - 1)
    game_ids = torch.arange(G, dtype=torch.int64, device=dev)
    tree_ids = [k for k, a in enumerate(agents) if isinstance(a, TreeSearchAgent)]
    joint_engine = None
    if joint and len(tree_ids) >= 2 and _joinable([agents[k] for k in tree_ids]):
        joint_engine = _joint_engine([agents[k] for k in tree_ids], G)
    log = []
    while True:
        live = ~done
        if not bool(live.any()):
            break
        mover = torch.where((states.current_player > 0) == a_black, player_a, player_b)
        codes = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
        valid = torch.zeros((n,), dtype=torch.bool, device=dev)
        term = torch.zeros((n,), dtype=torch.bool, device=dev)
        opening = states.move_count < int(opening_random_moves)

        def put(rows, c, v, t):
            codes.index_copy_(0, rows, c.to(torch.int32))
            valid.index_copy_(0, rows, v.to(torch.bool))
            term.index_copy_(0, rows, t.to(torch.bool))

        rows = torch.nonzero(live & opening).view(-1)
        if int(rows.numel()) > 0:
            put(rows, *_uniform_legal_codes(states.select(rows)))
        search = live & ~opening
        for k, agent in enumerate(agents):
            if k in tree_ids:
                continue
            rows = torch.nonzero(search & (mover == k)).view(-1)
            if int(rows.numel()) > 0:
                put(rows, *agent.select(states.select(rows), None))
        if tree_ids and bool(search.any()):
            groups = [tree_ids] if joint_engine is not None else [[k] for k in tree_ids]
            padded = states.select(pad_idx)
            ply_pad = plies.index_select(0, pad_idx)
            for group in groups:
                want = [torch.zeros((G,), dtype=torch.bool, device=dev) for _ in group]
                for w, k in zip(want, group):
                    w[:n] = search & (mover == k)
                if not any(bool(w.any()) for w in want):
                    continue
                eng = joint_engine if len(group) > 1 else agents[group[0]].engine(G)
                K = len(group)
                st = padded if K == 1 else padded.select(torch.arange(K * G, device=dev) % G)
                temps = torch.cat([torch.full((G,), agents[k].temperature, dtype=torch.float32, device=dev) for k in group])
                out = eng.search_batch(st, temperatures=temps, active=torch.cat(want), add_dirichlet_noise=False,
                                       rng_game_ids=game_ids.repeat(K), rng_plies=ply_pad.repeat(K))
                for j, w in enumerate(want):
                    rows = torch.nonzero(w[:n]).view(-1)
                    if int(rows.numel()) > 0:
                        src = rows + j * G
                        put(rows, out.chosen_action_codes.index_select(0, src), out.chosen_valid_mask.index_select(0, src),
                            out.terminal_mask.index_select(0, src))
        active = torch.nonzero(live).view(-1)
        c, v, t = codes.index_select(0, active), valid.index_select(0, active), term.index_select(0, active)
        if record_moves:
            row = torch.full((n,), -1, dtype=torch.int32, device=dev)
            row.index_copy_(0, active, torch.where(v & ~t, codes_to_indices(c), torch.full_like(c[:, 0], -1)))
            log.append(row)
        fin, res, _soft = v0_core.self_play_step_inplace(*states.tensors(), plies, done, active, c, t, v,
                                                         int(max_game_plies), 2.0)
        if int(fin.numel()) > 0:
            result_black.index_copy_(0, fin, res)
    return result_black, (torch.stack(log, dim=1) if (record_moves and log) else None)


def _stats(result_black: torch.Tensor, challenger_black: torch.Tensor, move_log, opening_book=None,
           openings: Optional[torch.Tensor] = None) -> EvaluationStats:
    n = int(result_black.numel())
    res = torch.where(challenger_black, result_black, -result_black)
    win, loss, draw = res > 0, res < 0, res == 0
    cb = {}
    for name, sel in (("black", challenger_black), ("white", ~challenger_black)):
        cb[name] = {"wins": int((win & sel).sum()), "losses": int((loss & sel).sum()), "draws": int((draw & sel).sum()),
                    "games": int(sel.sum())}
    stats = EvaluationStats(wins=int(win.sum()), losses=int(loss.sum()), draws=int(draw.sum()), total_games=n,
                            color_breakdown=cb, move_log=move_log)
    if opening_book is not None:
        stats.openings, stats.paired = openings, _paired(res, opening_book, openings)
    return stats


def play_matches(challenger, opponent, num_games: int, device, *, opening_random_moves: int = 0,
                 max_game_plies: int = 512, seed: Optional[int] = None, record_moves: bool = False,
                 joint: bool = True, opening_book=None, opening_seed: int = 0) -> EvaluationStats:
    """All `num_games` games at once on `device`; returns the challenger's W/L/D (`record_moves`: plus every game's
    sequence of 220-d action indices in `move_log`).  With a `TreeSearchAgent` on either side the tree backend's loop
    runs; `joint` (two tree agents): one search per ply over both sides' games, else one per agent.
    `opening_book` (an `OpeningBook`; `num_games` even): game p and game p + num_games/2 start from the book entry of pair
    p (`assign_openings(len(book), num_games/2, opening_seed)`), the challenger black in the first and white in the second;
    the stats gain `openings` and `paired`.  The states' own move_count / moves_since_capture carry the game limits."""
    openings = None
    if opening_book is not None:
        openings = _book_openings(opening_book, opening_seed, num_games, opening_random_moves, "num_games")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("eval arena needs a HIP device (no CPU path)")
    if seed is not None:
        torch.manual_seed(int(seed))
        torch.cuda.manual_seed(int(seed))
    n = int(num_games)
    if isinstance(challenger, TreeSearchAgent) or isinstance(opponent, TreeSearchAgent):
        challenger_black = torch.arange(n, device=dev) < (n / 2)
        res, log = _play_games([challenger, opponent], torch.zeros((n,), dtype=torch.int64, device=dev),
                               torch.ones((n,), dtype=torch.int64, device=dev), challenger_black, dev, joint=joint,
                               opening_random_moves=opening_random_moves, max_game_plies=max_game_plies,
                               record_moves=record_moves, opening_book=opening_book, openings=openings)
        return _stats(res, challenger_black, log, opening_book, openings)
    states = GpuStateBatch.initial(dev, n)
    if opening_book is not None:
        _seat_openings(states, opening_book, openings)
    plies = torch.zeros((n,), dtype=torch.int64, device=dev)
    done = torch.zeros((n,), dtype=torch.bool, device=dev)
    challenger_black = torch.arange(n, device=dev) < (n / 2)          # eval_checkpoint.py:487-495
    result_black = torch.zeros((n,), dtype=torch.float32, device=dev)
    finished = torch.zeros((n,), dtype=torch.bool, device=dev)
    log = []
    while True:
        active = torch.nonzero(~done).view(-1)
        if int(active.numel()) == 0:
            break
        sub = states.select(active)
        black_to_move = sub.current_player > 0
        chall_to_move = black_to_move == challenger_black.index_select(0, active)
        codes = torch.full((int(active.numel()), 4), -1, dtype=torch.int32, device=dev)
        valid = torch.zeros((int(active.numel()),), dtype=torch.bool, device=dev)
        term = torch.zeros_like(valid)
        opening = sub.move_count < int(opening_random_moves)
        for agent, who in ((challenger, chall_to_move), (opponent, ~chall_to_move)):
            rows = torch.nonzero(who).view(-1)
            if int(rows.numel()) == 0:
                continue
            part = sub.select(rows)
            force = opening.index_select(0, rows)
            if bool(force.all()):
                c, v, t = _uniform_legal_codes(part)
            else:
                c, v, t = agent.select(part, force if bool(force.any()) else None)
            codes.index_copy_(0, rows, c.to(torch.int32))
            valid.index_copy_(0, rows, v.to(torch.bool))
            term.index_copy_(0, rows, t.to(torch.bool))
        if record_moves:
            row = torch.full((n,), -1, dtype=torch.int32, device=dev)
            row.index_copy_(0, active, torch.where(valid & ~term, codes_to_indices(codes), torch.full_like(codes[:, 0], -1)))
            log.append(row)
        fin, res, _soft = v0_core.self_play_step_inplace(*states.tensors(), plies, done, active, codes, term, valid,
                                                         int(max_game_plies), 2.0)
        if int(fin.numel()) > 0:
            result_black.index_copy_(0, fin, res)
            finished.index_fill_(0, fin, True)
    res = torch.where(challenger_black, result_black, -result_black)
    win, loss, draw = res > 0, res < 0, res == 0
    cb = {}
    for name, sel in (("black", challenger_black), ("white", ~challenger_black)):
        cb[name] = {"wins": int((win & sel).sum()), "losses": int((loss & sel).sum()), "draws": int((draw & sel).sum()),
                    "games": int(sel.sum())}
    stats = EvaluationStats(wins=int(win.sum()), losses=int(loss.sum()), draws=int(draw.sum()), total_games=n,
                            color_breakdown=cb, move_log=torch.stack(log, dim=1) if (record_moves and log) else None)
    if opening_book is not None:
        stats.openings, stats.paired = openings, _paired(res, opening_book, openings)
    return stats


def load_checkpoint_model(path: str):
    """Checkpoint (raw state_dict or {"model_state_dict": ...}) -> ChessNet of the matching architecture."""
    from .self_play_worker import _infer_model
    obj = torch.load(path, map_location="cpu", weights_only=False)
    state = obj["model_state_dict"] if isinstance(obj, dict) and "model_state_dict" in obj else obj
    model = _infer_model(state)
    model.load_state_dict(state, strict=True)
    return model.eval()


SEARCH_BACKENDS = ("v1", "portable")


def make_agent(model, search_backend: str, device, mcts_simulations: int, temperature: float, sample_moves: bool,
               seed: int = 0, fpu_reduction: Optional[float] = None, fpu_root_reduction: Optional[float] = None,
               cpuct_log: float = 0.0, cpuct_base: float = 19652.0):
    """`search_backend` "v1" (root PUCT, RootSearchAgent) or "portable" (the tree search, TreeSearchAgent).  The PUCT
    shape parameters (first-play urgency, visit-scaled cpuct) need the tree search (ValueError with "v1")."""
    from .puct_shape import parse_puct_shape
    shape = parse_puct_shape(fpu_reduction, fpu_root_reduction, cpuct_log, cpuct_base)
    if search_backend == "v1":
        if shape.on:
            raise ValueError("first-play urgency / the visit-scaled cpuct need the tree backend (search_backend "
                             "'portable'), not the root-PUCT search")
        return RootSearchAgent(model, device, mcts_simulations, temperature, sample_moves)
    if search_backend == "portable":
        return TreeSearchAgent(model, device, mcts_simulations, temperature, sample_moves, seed=seed, **shape.kwargs())
    raise ValueError(f"search_backend must be one of {SEARCH_BACKENDS}, got {search_backend!r}")


def evaluate_checkpoint(challenger_checkpoint: str, opponent_checkpoint: Optional[str] = None, *, num_games: int = 200,
                        device: str = "cuda:0", mcts_simulations: int = 64, temperature: float = 0.1,
                        sample_moves: bool = False, opening_random_moves: int = 0, max_game_plies: int = 512,
                        seed: int = 0, search_backend: str = "v1", fpu_reduction: Optional[float] = None,
                        fpu_root_reduction: Optional[float] = None, cpuct_log: float = 0.0,
                        cpuct_base: float = 19652.0, opening_book=None, opening_seed: int = 0) -> Dict[str, Any]:
    """vs-previous (two checkpoints) or vs-random (opponent None) probe; payload as eval_checkpoint.py:139-154.
    `search_backend`: "v1" (root PUCT) or "portable" (the tree search, both sides in one engine).  `opening_book`: the
    games are colour-swapped pairs from the book (play_matches) and the payload gains the key "paired"."""
    games = int(num_games) if int(num_games) % 2 == 0 else max(2, (int(num_games) // 2) * 2)   # even (:48-54)
    if opening_book is not None:                              # refusals before a checkpoint is read
        _check_book(opening_book, games, opening_random_moves, "num_games")
    if search_backend not in SEARCH_BACKENDS:
        raise ValueError(f"search_backend must be one of {SEARCH_BACKENDS}, got {search_backend!r}")
    shape = dict(fpu_reduction=fpu_reduction, fpu_root_reduction=fpu_root_reduction, cpuct_log=cpuct_log,
                 cpuct_base=cpuct_base)
    chall = make_agent(load_checkpoint_model(challenger_checkpoint), search_backend, device, mcts_simulations,
                       temperature, sample_moves, seed, **shape)
    opp = RandomAgent() if not opponent_checkpoint else make_agent(
        load_checkpoint_model(opponent_checkpoint), search_backend, device, mcts_simulations, temperature, sample_moves,
        seed, **shape)
    book = {} if opening_book is None else dict(opening_book=opening_book, opening_seed=opening_seed)
    stats = play_matches(chall, opp, games, device, opening_random_moves=opening_random_moves,
                         max_game_plies=max_game_plies, seed=seed, **book)
    payload = stats.to_payload("vs_previous" if opponent_checkpoint else "vs_random")
    payload["seed"] = int(seed)
    return payload


@dataclass
class RoundRobinResult:
    wdl: torch.Tensor                         # int64[K, K, 3]: wins / draws / losses of model i against model j
    points: List[int]                         # 3 per win, 1 per draw (tournament_v1_eval.py:28-30)
    pairs: List[tuple]                        # (i, j) in the order their games were laid out
    pair_stats: Dict[tuple, EvaluationStats]  # model i's W/L/D against j (i < j), move logs if recorded

    def to_payload(self, names: Optional[Sequence[str]] = None) -> Dict[str, Any]:
        K = int(self.wdl.shape[0])
        names = list(names) if names is not None else [str(i) for i in range(K)]
        return {"models": names, "points": [int(p) for p in self.points],
                "wdl": [[[int(x) for x in self.wdl[i, j]] for j in range(K)] for i in range(K)],
                "pairs": [{"a": names[i], "b": names[j], **self.pair_stats[(i, j)].to_payload(f"{names[i]}_vs_{names[j]}")}
                          for (i, j) in self.pairs]}


def play_round_robin(models: Sequence[Any], games_per_pair: int, device, *, joint: bool = True,
                     opening_random_moves: int = 0, max_game_plies: int = 512, seed: Optional[int] = None,
                     record_moves: bool = False, opening_book=None, opening_seed: int = 0) -> RoundRobinResult:
    """Every pair (i < j) of up to 8 agents (TreeSearchAgents in one engine, one segment each, when `joint`) plays
    `games_per_pair` games, i black in the first half of them; all games at once.  Pair (i, j)'s games are what
    play_matches(models[i], models[j], games_per_pair) plays when no random moves are drawn.  `opening_book`
    (`games_per_pair` even): every model pair plays the same assignment of openings, the one play_matches makes."""
    openings = None
    if opening_book is not None:
        openings = _book_openings(opening_book, opening_seed, games_per_pair, opening_random_moves, "games_per_pair")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("eval arena needs a HIP device (no CPU path)")
    K, m = len(models), int(games_per_pair)
    if not 2 <= K <= 8 or m < 1:
        raise ValueError("a round robin takes 2..8 models and at least one game per pair")
    if seed is not None:
        torch.manual_seed(int(seed))
        torch.cuda.manual_seed(int(seed))
    pairs = [(i, j) for i in range(K) for j in range(i + 1, K)]
    first = torch.arange(m, device=dev) < (m / 2)
    pa = torch.cat([torch.full((m,), i, dtype=torch.int64, device=dev) for i, _ in pairs])
    pb = torch.cat([torch.full((m,), j, dtype=torch.int64, device=dev) for _, j in pairs])
    a_black = first.repeat(len(pairs))
    res, log = _play_games(list(models), pa, pb, a_black, dev, joint=joint, opening_random_moves=opening_random_moves,
                           max_game_plies=max_game_plies, record_moves=record_moves, opening_book=opening_book,
                           openings=None if openings is None else openings.repeat(len(pairs)))
    wdl = torch.zeros((K, K, 3), dtype=torch.int64)
    points = [0] * K
    pair_stats = {}
    for p, (i, j) in enumerate(pairs):
        sl = slice(p * m, (p + 1) * m)
        st = _stats(res[sl], first, None if log is None else log[sl], opening_book, openings)
        pair_stats[(i, j)] = st
        wdl[i, j] = torch.tensor([st.wins, st.draws, st.losses])
        wdl[j, i] = torch.tensor([st.losses, st.draws, st.wins])
        points[i] += 3 * st.wins + st.draws
        points[j] += 3 * st.losses + st.draws
    return RoundRobinResult(wdl=wdl, points=points, pairs=pairs, pair_stats=pair_stats)
